"""GPU WAIC and pointwise fit (csrc/sr_waic.hip): every output equal, as uint64 bit patterns, to the numpy definition
in tests/waic_ref.py at the shapes where the kernels can go wrong -- one cell, the tile edges (64 taxa x 16 sites),
the chunk tails (32 samples staged with shared rates, 8 with per-taxon rates) and the order of the chain sums, the
batch boundaries of the bounded scratch, any int16 in the rows, constant and mixed X, rates at the domain's edges --
the closed form for identical samples, the reflection identity, Jensen's inequality on a real session, the optional
outputs, the session form (records in HBM) equal to the host-record form and leaving the session untouched, and
the command line's three files."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import seriation_amd as sa
import waic_ref
from seriation_amd import _lib as L
from seriation_amd import analysis, launcher

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DS = os.path.join(ROOT, "tests", "golden", "datasets")
PKG = os.path.join(ROOT, "seriation-in-paleontological-data-using-mcmc_amd")
TILE, S, CH_SHARED, CH_MANY = 64, 16, 32, 8   # csrc/sr_waic.hip: SRW_TILE, SRW_S, SRW_CH_SHARED, SRW_CH_MANY
POINTWISE = ("lppd", "ll_mean", "pwaic", "elpd")
SCALARS = ("elpd_waic", "se", "p_waic", "lppd_sum", "waic")
LO, HI = -700.0, -2.0 ** -50
_DBLP = ctypes.POINTER(ctypes.c_double)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def matrix(xkind, N, M):
    rng = np.random.RandomState(7 * N + M)
    X = {"zeros": np.zeros((N, M), np.uint8), "ones": np.ones((N, M), np.uint8),
         "mixed": rng.randint(0, 2, (N, M)).astype(np.uint8)}[xkind]
    return X


def records(kind, N, M, n_sel, count):
    """[n_sel][count][2M+N] int16.  real: pi a permutation of the positions, 0 <= a <= b <= N, drifting slowly from
    row to row; full: any int16, a good part of the entries drawn near [0, N] so that alive cells exist (a > b rows,
    limits and positions outside [0, N]), and the int16 extremes placed in a, in b and in pi."""
    rng = np.random.RandomState(1000 * N + 10 * M + count + n_sel)
    W = 2 * M + N
    out = np.empty((n_sel, count, W), np.int64)
    if kind == "full":
        x = rng.randint(-32768, 32768, (n_sel, count, W))
        near = rng.randint(-2, N + 3, (n_sel, count, W))
        take = rng.randint(0, 4, (n_sel, count, W)) > 0
        x[take] = near[take]
        x[0, 0, 0], x[0, 1, M], x[0, 1, 2 * M] = -32768, 32767, 32767
        x[-1, -1, M - 1], x[-1, -1, 2 * M - 1], x[-1, -1, W - 1] = 32767, -32768, -32768
        x[0, 0, M], x[0, 0, 2 * M] = 32767, 32766   # a = -32768 <= pi = 32766 < b = 32767: alive at the extremes
        return x.astype(np.int16)
    for k in range(n_sel):
        pi = rng.permutation(N)
        a = rng.randint(0, N + 1, M)
        b = a + rng.randint(0, N + 1, M) % (N + 1 - a)
        for r in range(count):
            if N > 1 and r:
                i, j = rng.randint(0, N, 2)
                pi[i], pi[j] = pi[j], pi[i]
                m = rng.randint(0, M)
                a[m] = rng.randint(0, N + 1)
                b[m] = a[m] + rng.randint(0, N + 1) % (N + 1 - a[m])
            out[k, r, :M], out[k, r, M:2 * M], out[k, r, 2 * M:] = a, b, pi
    return out.astype(np.int16)


def rates(N, M, n_sel, count, manycd, edges=False):
    """log-scale c in [log 0.001, log 0.1], d in [log 0.2, log 0.8], as the sampler's; the shared form carries a
    loglik entry that is never read (NaN here).  edges: both ends of the domain mixed in."""
    rng = np.random.RandomState(31 * N + M + count + 2 * manycd)
    Mt = M if manycd else 1
    c = rng.uniform(np.log(0.001), np.log(0.1), (n_sel, count, Mt))
    d = rng.uniform(np.log(0.2), np.log(0.8), (n_sel, count, Mt))
    if edges:
        for v, at in ((LO, 0), (HI, 1), (HI, 2), (LO, 3)):
            c.reshape(-1)[at::7] = v
            d.reshape(-1)[(at + 2) % 4::5] = v
    tail = [] if manycd else [np.full((n_sel, count, 1), np.nan)]
    return np.concatenate([c, d] + tail, axis=2)


_IN, _REF = {}, {}


def inputs(kind, xkind, N, M, n_sel, count, manycd, edges=False):
    key = (kind, xkind, N, M, n_sel, count, manycd, edges)
    if key not in _IN:
        X, rec, cd = matrix(xkind, N, M), records(kind, N, M, n_sel, count), rates(N, M, n_sel, count, manycd, edges)
        for a in (X, rec, cd):
            a.setflags(write=False)
        _IN[key] = (sa.Dataset(X, np.zeros(N, bool)), X, rec, cd)
    return _IN[key]


def ref_of(*key):
    if key not in _REF:
        _, X, rec, cd = inputs(*key)
        _REF[key] = waic_ref.waic(X, rec, cd, key[6])
    return _REF[key]


def check(res, want, N, M, T):
    assert set(res) == set(POINTWISE) | set(SCALARS) | {"n_high", "site_elpd", "taxon_elpd", "total", "kernel_ms"}
    for k in POINTWISE:
        assert res[k].dtype == np.float64 and res[k].shape == (N, M), k
        assert np.array_equal(bits(res[k]), bits(want[k])), k
    assert np.array_equal(bits(res["site_elpd"]), bits(want["site_elpd"])) and res["site_elpd"].shape == (N,)
    assert np.array_equal(bits(res["taxon_elpd"]), bits(want["taxon_elpd"])) and res["taxon_elpd"].shape == (M,)
    for k in SCALARS:
        assert np.array_equal(bits(res[k]), bits(want[k])), k   # se is NaN for one cell: compared as bits
    assert res["n_high"] == want["n_high"] and res["total"] == T and res["kernel_ms"] > 0
    assert np.isfinite(res["lppd"]).all() and np.isfinite(res["ll_mean"]).all() and np.isfinite(res["pwaic"]).all()


def run_case(kind, xkind, N, M, n_sel, count, manycd, edges=False):
    ds, X, rec, cd = inputs(kind, xkind, N, M, n_sel, count, manycd, edges)
    res = analysis.waic_from_records(ds, rec, cd, manycd=manycd)
    check(res, ref_of(kind, xkind, N, M, n_sel, count, manycd, edges), N, M, n_sel * count)
    return res


# kind, X, N, M, n_sel, count
SHAPES = [
    pytest.param("real", "mixed", 1, 1, 1, 2, id="smallest"),
    pytest.param("real", "mixed", S, TILE, 2, 5, id="exactly-one-tile"),
    pytest.param("real", "mixed", S + 1, TILE + 1, 2, 5, id="one-over"),
    pytest.param("real", "mixed", 40, 200, 2, 5, id="ragged-tiles"),
    pytest.param("full", "mixed", 6, 5, 2, 9, id="full-int16"),
    pytest.param("real", "zeros", 5, 7, 2, 6, id="x-zeros"),
    pytest.param("real", "ones", 5, 7, 2, 6, id="x-ones"),
    pytest.param("real", "mixed", 124, 139, 3, 100, id="g10s10-shape"),
]


@pytest.mark.parametrize("manycd", [False, True], ids=["shared", "manycd"])
@pytest.mark.parametrize("kind,xkind,N,M,n_sel,count", SHAPES)
def test_waic_equals_definition(kind, xkind, N, M, n_sel, count, manycd):
    res = run_case(kind, xkind, N, M, n_sel, count, manycd)
    if kind == "full":   # the case does hold what it is for
        _, X, rec, _ = inputs(kind, xkind, N, M, n_sel, count, manycd)
        a, b, pi = rec[..., :M], rec[..., M:2 * M], rec[..., 2 * M:]
        assert (a > b).any() and a.min() == -32768 and b.max() == 32767 and pi.max() == 32767 and pi.min() == -32768
        idx = waic_ref.index(X, rec[0, 0], N, M)
        assert idx[0, 0] in (1, 2)   # alive between the extremes
    if N * M == 1:
        assert np.isnan(res["se"])


@pytest.mark.parametrize("manycd", [False, True], ids=["shared", "manycd"])
@pytest.mark.parametrize("count", sorted({CH_MANY, CH_MANY + 1, 2 * CH_MANY + 3, CH_SHARED, CH_SHARED + 1,
                                          2 * CH_SHARED + 3}))
def test_chunk_tails_and_chain_order(count, manycd):
    """three chains: ((S0 + S1) + S2) differs from any other order of the chain sums in some cell"""
    N, M, n_sel = 5, 7, 3
    res = run_case("real", "mixed", N, M, n_sel, count, manycd)
    if count == 2 * CH_SHARED + 3:
        _, X, rec, cd = inputs("real", "mixed", N, M, n_sel, count, manycd)
        other = waic_ref.waic(X, rec[[2, 1, 0]], cd[[2, 1, 0]], manycd)
        assert not np.array_equal(bits(other["ll_mean"]), bits(res["ll_mean"]))   # the order is observable here


@pytest.mark.parametrize("manycd", [False, True], ids=["shared", "manycd"])
def test_rates_at_the_domain_edges(manycd):
    N, M, n_sel, count = 5, 7, 2, 11
    res = run_case("real", "mixed", N, M, n_sel, count, manycd, edges=True)
    _, _, _, cd = inputs("real", "mixed", N, M, n_sel, count, manycd, True)
    used = cd[..., :2 * (M if manycd else 1)]
    assert (used == LO).any() and (used == HI).any() and (res["pwaic"] > 0.4).any()


def test_manycd_three_taxa_tiles():
    run_case("real", "mixed", 3, 130, 2, 2 * CH_MANY + 1, True)


@pytest.mark.parametrize("scratch", [40000, 1500])
@pytest.mark.parametrize("manycd", [False, True], ids=["shared", "manycd"])
def test_scratch_batches(monkeypatch, manycd, scratch):
    """SR_WAIC_SCRATCH bounds the per-chain partial sums and the table: at 17 x 65 cells (17680 bytes of partials per
    chain) 40000 bytes take the three chains as 2 + 1 and, per-taxon rates (4160 bytes a row and chain), the rows 4
    at a time; 1500 bytes take the chains one by one and the rows 23 at a time (shared rates, 64 bytes a row) or one
    by one.  The sums are carried across the batches in HBM: the result is the unbatched one."""
    N, M, n_sel, count = S + 1, TILE + 1, 3, (2 * CH_MANY + 3 if manycd else 2 * CH_SHARED + 3)
    plain = run_case("real", "mixed", N, M, n_sel, count, manycd)
    monkeypatch.setenv("SR_WAIC_SCRATCH", str(scratch))
    res = run_case("real", "mixed", N, M, n_sel, count, manycd)
    for k in POINTWISE:
        assert np.array_equal(bits(res[k]), bits(plain[k]))


@pytest.mark.parametrize("n_sel,count", [(1, 2), (2, 2)])
@pytest.mark.parametrize("manycd", [False, True], ids=["shared", "manycd"])
def test_closed_form_identical_samples(n_sel, count, manycd):
    """Every sample the same row and the same rates: p + p and (p + p) + (p + p) are exact, so ll_mean is the
    table's l, lppd is log(p) and pwaic is +0.0 in every cell.  (Not so for longer runs: 3 p is not representable.)"""
    N, M = 5, 7
    ds, X, rec, cd = inputs("real", "mixed", N, M, 1, 1, manycd)
    rec, cd = np.repeat(np.repeat(rec, n_sel, 0), count, 1), np.repeat(np.repeat(cd, n_sel, 0), count, 1)
    res = analysis.waic_from_records(ds, rec, cd, manycd=manycd)
    p, l = waic_ref.table(cd[:1, :1], M, manycd)
    idx = waic_ref.index(X, rec[0, 0], N, M)
    cols = np.arange(M) if manycd else np.zeros(M, int)
    lw, pw = l[0, 0][idx, cols[None, :]], p[0, 0][idx, cols[None, :]]
    assert np.array_equal(bits(res["ll_mean"]), bits(lw))
    assert np.array_equal(bits(res["lppd"]), bits(waic_ref._LOG(pw).astype(np.float64)))
    assert not bits(res["pwaic"]).any() and res["n_high"] == 0   # +0.0, not -0.0
    assert len(set(idx.reshape(-1).tolist())) == 4   # every kind of cell is there


@pytest.mark.parametrize("manycd", [False, True], ids=["shared", "manycd"])
def test_reflection_identity(manycd):
    """GPU against GPU: a' = N - b, b' = N - a, pi' = N - 1 - pi in some chains changes no alive bit and no output."""
    N, M, n_sel, count = 40, 200, 3, 9
    ds, X, rec, cd = inputs("real", "mixed", N, M, n_sel, count, manycd)
    plain = analysis.waic_from_records(ds, rec, cd, manycd=manycd)
    refl = rec.astype(np.int64)
    for k in (0, 2):
        refl[k, :, :M], refl[k, :, M:2 * M] = N - rec[k, :, M:2 * M].astype(np.int64), N - rec[k, :, :M].astype(np.int64)
        refl[k, :, 2 * M:] = N - 1 - rec[k, :, 2 * M:].astype(np.int64)
    assert not np.array_equal(refl, rec)
    other = analysis.waic_from_records(ds, refl.astype(np.int16), cd, manycd=manycd)
    for k in POINTWISE + SCALARS + ("site_elpd", "taxon_elpd"):
        assert np.array_equal(bits(other[k]), bits(plain[k])), k
    assert other["n_high"] == plain["n_high"]


def test_optional_outputs():
    """each output pointer alone gives its entry of the full call; the scalars are always written"""
    N, M, n_sel, count = 40, 200, 2, 5
    ds, X, rec, cd = inputs("real", "mixed", N, M, n_sel, count, False)
    full = analysis.waic_from_records(ds, rec, cd)
    shapes = {"lppd": (N, M), "ll_mean": (N, M), "pwaic": (N, M), "site_elpd": (N,), "taxon_elpd": (M,)}
    for only in (None,) + tuple(shapes):
        out = L.sr_waic_out()
        buf = np.zeros(shapes[only]) if only else None
        if only:
            setattr(out, only, buf.ctypes.data_as(_DBLP))
        rc = sa.lib().sr_waic(ctypes.byref(ds.c), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)),
                              cd.ctypes.data_as(_DBLP), 0, n_sel, count, 0, ctypes.byref(out))
        assert rc == L.SR_OK and out.kernel_ms > 0
        if only:
            assert np.array_equal(bits(buf), bits(full[only])), only
        for k, v in (("elpd_waic", out.elpd), ("se", out.se), ("p_waic", out.p_waic), ("lppd_sum", out.lppd_sum),
                     ("waic", out.waic)):
            assert bits(v) == bits(full[k]), k
        assert out.n_high == full["n_high"]
    light = analysis.waic_from_records(ds, rec, cd, pointwise=False)
    assert not set(light) & set(POINTWISE) and bits(light["elpd_waic"]) == bits(full["elpd_waic"])
    assert np.array_equal(bits(light["site_elpd"]), bits(full["site_elpd"]))


@pytest.mark.parametrize("manycd", [0, 1], ids=["shared", "manycd"])
def test_session_form(manycd):
    ds = sa.Dataset.parse(open(os.path.join(DS, "g10s10.txt"), "rb").read())
    seeds, sel = [5, 9, 13, 21], [2, 0, 3]

    def sampled(s):
        s.run(5)
        s.reset_records()
        s.run(40, save=True)

    kw = dict(calls_per_launch=40, manycd=manycd)
    with sa.Session(ds, seeds, **kw) as s, sa.Session(ds, seeds, **kw) as plain:
        sampled(s)
        sampled(plain)
        ab0, cdl0 = s.fetch_records()
        cd0 = s.fetch_cd_vectors() if manycd else cdl0
        res = analysis.waic_from_session(s, sel, first=4, count=36)
        ab1, cdl1 = s.fetch_records()
        assert np.array_equal(ab0, ab1) and np.array_equal(bits(cdl0), bits(cdl1))
        if manycd:
            assert np.array_equal(bits(cd0), bits(s.fetch_cd_vectors()))
        host = analysis.waic_from_records(ds, ab0[sel, 4:40], cd0[sel, 4:40], manycd=bool(manycd))
        X = np.ctypeslib.as_array(ds.c.X, (ds.N * ds.M,)).reshape(ds.N, ds.M)
        want = waic_ref.waic(X, ab0[sel, 4:40], cd0[sel, 4:40], bool(manycd))
        check(res, want, ds.N, ds.M, 3 * 36)
        check(host, want, ds.N, ds.M, 3 * 36)
        # Jensen: log of the mean >= mean of the logs; the sequential sums carry a relative error of at most T 2^-53
        assert (res["lppd"] >= res["ll_mean"] - 1e-9).all() and (res["pwaic"] >= 0).all()
        # errors: rows beyond the buffered records, a chain index out of range, no rows, fewer than two samples
        for bad in (dict(chains=sel, first=5, count=36), dict(chains=[0, 4], first=0, count=40),
                    dict(chains=[-1], first=0, count=40), dict(chains=sel, first=0, count=0),
                    dict(chains=sel, first=-1, count=4), dict(chains=[], first=0, count=4),
                    dict(chains=[1], first=0, count=1)):
            with pytest.raises(sa.SrError) as e:
                analysis.waic_from_session(s, **bad)
            assert e.value.code == L.SR_EINVAL
        s.run(3, save=False)
        plain.run(3, save=False)
        for c in range(len(seeds)):
            x, y = s.state(c), plain.state(c)
            for k in ("a", "b", "pi", "counts"):
                assert np.array_equal(x[k], y[k])
            assert np.array_equal(bits([x["c"], x["d"], x["loglik"]]), bits([y["c"], y["d"], y["loglik"]]))


@pytest.mark.parametrize("name,extra", [("g2s2", []), ("g10s10", ["--manycd"])], ids=["shared", "manycd"])
def test_cli_waic(tmp_path, name, extra):
    """python -m seriation_amd --select 2 --waic: the three files hold the definition's numbers for the chosen
    chains' chain_data.csv rows."""
    path = os.path.join(DS, name + ".txt")
    r = subprocess.run([sys.executable, "-m", "seriation_amd", path, "--chains", "4", "--burnin", "5", "--samples", "20",
                        "--seed-base", "1", "--root", str(tmp_path), "--select", "2", "--waic"] + extra, cwd=PKG,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ds = sa.Dataset.load(path)
    chosen = launcher.choose_chains(2, str(tmp_path))
    assert ("selected: " + " ".join(str(k) for k in chosen)) in r.stdout and 1 <= len(chosen) <= 2
    rec = analysis.read_chain_rows(str(tmp_path), chosen, ds.N, ds.M)
    cd = analysis.read_chain_cd(str(tmp_path), chosen, ds.M, manycd=bool(extra))
    assert rec.shape == (len(chosen), 20, 2 * ds.M + ds.N) and cd.shape == (len(chosen), 20, 2 * ds.M if extra else 3)
    X = np.ctypeslib.as_array(ds.c.X, (ds.N * ds.M,)).reshape(ds.N, ds.M)
    want = waic_ref.waic(X, rec, cd, bool(extra))
    lines = (tmp_path / "Chains" / "waic.csv").read_text().splitlines()
    assert lines[0] == "elpd_waic,se,p_waic,lppd,waic,n_high,samples,cells" and len(lines) == 2
    assert lines[1] == "%r,%r,%r,%r,%r,%d,%d,%d" % (float(want["elpd_waic"]), float(want["se"]), float(want["p_waic"]),
                                                    float(want["lppd_sum"]), float(want["waic"]), want["n_high"],
                                                    len(chosen) * 20, ds.N * ds.M)
    for fname, key, n in (("waic_sites.csv", "site", ds.N), ("waic_taxa.csv", "taxon", ds.M)):
        lines = (tmp_path / "Chains" / fname).read_text().splitlines()
        assert lines[0] == key + ",elpd" and len(lines) == 1 + n
        assert lines[1:] == ["%d,%r" % (i, float(want[key + "_elpd"][i])) for i in range(n)]
