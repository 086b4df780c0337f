"""GPU placement of query rows (csrc/sr_place.hip): every output equal, as uint64 bit patterns, to the numpy definition
in tests/place_ref.py at the shapes where the kernels can go wrong -- one position, the 64-stride walk of Z with
empty lanes and with several trips, one wave against several and a second position tile, the taxa chunk and the
query tile and their edges, the order of the chain sums and the row batches of the bounded scratch, any int16 in
the rows, constant, mixed and partly unassessed queries, rates at the domain's edges, profiles that underflow --
identical rows, the all-unassessed row's closed form, the reflection of flagged chains, a real session (rows that
sum to 1, the session form equal to the host-record form, the session untouched), the optional outputs and the
command line's three files."""
import ctypes
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import place_ref
import seriation_amd as sa
from seriation_amd import _lib as L
from seriation_amd import analysis, launcher
from seriation_amd import __main__ as cli

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DS = os.path.join(ROOT, "tests", "golden", "datasets")
PKG = os.path.join(ROOT, "seriation-in-paleontological-data-using-mcmc_amd")
QT, MC, PT = 8, 128, 256   # csrc/sr_place.hip: SRX_QT, SRX_MC, SRX_PT
OUTS = ("pos", "site", "lse", "lpd")
LO, HI = -700.0, -2.0 ** -50
_DBLP = ctypes.POINTER(ctypes.c_double)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def queries(ykind, Q, M):
    """[Q][M] uint8.  twos: a mixed matrix with a third of the cells not assessed and its last row all 2."""
    rng = np.random.RandomState(7 * Q + M)
    if ykind == "zeros":
        return np.zeros((Q, M), np.uint8)
    if ykind == "ones":
        return np.ones((Q, M), np.uint8)
    if ykind == "mixed":
        return rng.randint(0, 2, (Q, M)).astype(np.uint8)
    Y = rng.randint(0, 3, (Q, M)).astype(np.uint8)
    Y[-1] = 2
    return Y


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
        x[0, 0, M] = 32767   # a = -32768 <= p < b = 32767: alive at every position
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


def dataset(N, M):
    return sa.Dataset(np.zeros((N, M), np.uint8), np.zeros(N, bool))


def inputs(kind, ykind, N, M, n_sel, count, Q, manycd, edges=False):
    key = (kind, ykind, N, M, n_sel, count, Q, manycd, edges)
    if key not in _IN:
        Y, rec, cd = queries(ykind, Q, M), records(kind, N, M, n_sel, count), rates(N, M, n_sel, count, manycd, edges)
        for a in (Y, rec, cd):
            a.setflags(write=False)
        _IN[key] = (dataset(N, M), Y, rec, cd)
    return _IN[key]


def ref_of(*key):
    if key not in _REF:
        _, Y, rec, cd = inputs(*key)
        _REF[key] = place_ref.placement(key[2], rec, cd, Y, key[7])
    return _REF[key]


def check(res, want, N, Q, n_sel, count):
    assert set(res) == set(OUTS) | {"total", "kernel_ms"}
    shapes = {"pos": (Q, N), "site": (Q, N), "lse": (n_sel, count, Q), "lpd": (Q,)}
    for k in OUTS:
        assert res[k].dtype == np.float64 and res[k].shape == shapes[k], k
        assert np.array_equal(bits(res[k]), bits(want[k])), k
        assert np.isfinite(res[k]).all(), k
    assert res["total"] == n_sel * count and res["kernel_ms"] > 0


def run_case(kind, ykind, N, M, n_sel, count, Q, manycd, edges=False):
    ds, Y, rec, cd = inputs(kind, ykind, N, M, n_sel, count, Q, manycd, edges)
    res = analysis.placement_from_records(ds, rec, cd, Y, manycd=manycd, lse=True)
    check(res, ref_of(kind, ykind, N, M, n_sel, count, Q, manycd, edges), N, Q, n_sel, count)
    return res


# kind, Y, N, M, n_sel, count, Q
SHAPES = [
    pytest.param("real", "mixed", 1, 1, 1, 1, 1, id="smallest"),
    pytest.param("real", "mixed", 2, 63, 3, 2, QT - 1, id="two-positions"),
    pytest.param("real", "twos", 63, 64, 1, 33, QT, id="one-lane-empty-one-query-tile"),
    pytest.param("real", "mixed", 64, 65, 3, 2, QT + 1, id="one-wave-exactly"),
    pytest.param("real", "mixed", 65, MC - 1, 1, 2, 1, id="second-trip-of-one-lane"),
    pytest.param("full", "twos", 129, MC, 3, 2, QT + 1, id="full-int16-one-taxa-chunk"),
    pytest.param("real", "twos", 200, MC + 1, 3, 33, 3, id="ragged-everything"),
    pytest.param("real", "mixed", PT + 44, 5, 1, 2, 2, id="second-position-tile"),
    pytest.param("full", "mixed", 6, 5, 2, 9, 3, id="full-int16-small"),
    pytest.param("real", "zeros", 5, 7, 2, 6, 2, id="y-zeros"),
    pytest.param("real", "ones", 5, 7, 2, 6, 2, id="y-ones"),
]


@pytest.mark.parametrize("manycd", [False, True], ids=["shared", "manycd"])
@pytest.mark.parametrize("kind,ykind,N,M,n_sel,count,Q", SHAPES)
def test_placement_equals_definition(kind, ykind, N, M, n_sel, count, Q, manycd):
    res = run_case(kind, ykind, N, M, n_sel, count, Q, manycd)
    _, Y, rec, _ = inputs(kind, ykind, N, M, n_sel, count, Q, manycd)
    if kind == "full":   # the case does hold what it is for
        a, b, pi = rec[..., :M], rec[..., M:2 * M], rec[..., 2 * M:]
        assert (a > b).any() and a.min() == -32768 and b.max() == 32767 and pi.max() == 32767 and pi.min() == -32768
    if kind == "real":   # pi is a permutation: site is pos read through it, both sum to 1
        assert np.allclose(res["pos"].sum(axis=1), 1.0, atol=1e-12) and np.allclose(res["site"].sum(axis=1), 1.0, atol=1e-12)
    if ykind == "twos":  # the all-unassessed row: L = 0 everywhere, Z = N exactly
        assert np.array_equal(bits(res["lse"][:, :, -1]), bits(np.full((n_sel, count), math.log(float(N)))))
        assert (Y[-1] == 2).all()


@pytest.mark.parametrize("manycd", [False, True], ids=["shared", "manycd"])
def test_chain_order_is_observable(manycd):
    """three chains: ((S0 + S1) + S2) differs from any other order of the chain sums in some entry"""
    N, M, n_sel, count, Q = 5, 7, 3, 33, 2
    res = run_case("real", "mixed", N, M, n_sel, count, Q, manycd)
    _, Y, rec, cd = inputs("real", "mixed", N, M, n_sel, count, Q, manycd)
    other = place_ref.placement(N, rec[[2, 1, 0]], cd[[2, 1, 0]], Y, manycd)
    assert not np.array_equal(bits(other["pos"]), bits(res["pos"]))


def test_identical_rows_identical_bits():
    N, M, n_sel, count = 65, 9, 2, 3
    ds, Y, rec, cd = inputs("real", "twos", N, M, n_sel, count, 3, False)
    Y = Y.copy()
    Y[2] = Y[0]
    res = analysis.placement_from_records(ds, rec, cd, Y, lse=True)
    check(res, place_ref.placement(N, rec, cd, Y), N, 3, n_sel, count)
    for k in ("pos", "site", "lpd"):
        assert np.array_equal(bits(res[k][0]), bits(res[k][2])) and not np.array_equal(bits(res[k][0]), bits(res[k][1]))
    assert np.array_equal(bits(res["lse"][:, :, 0]), bits(res["lse"][:, :, 2]))


@pytest.mark.parametrize("manycd", [False, True], ids=["shared", "manycd"])
def test_rates_at_the_domain_edges(manycd):
    N, M, n_sel, count, Q = 5, 7, 2, 11, 3
    run_case("real", "twos", N, M, n_sel, count, Q, manycd, edges=True)
    _, _, _, cd = inputs("real", "twos", N, M, n_sel, count, Q, manycd, True)
    used = cd[..., :2 * (M if manycd else 1)]
    assert (used == LO).any() and (used == HI).any()


def test_underflowing_profiles():
    """e subnormal and e == 0.0 (tests/test_place_host.py checks that the case holds both), as the C library's"""
    N, rec, cd, Y = place_ref.underflow_case()
    res = analysis.placement_from_records(dataset(N, Y.shape[1]), rec, cd, Y, lse=True)
    check(res, place_ref.placement(N, rec, cd, Y), N, 2, 1, 2)
    assert res["pos"][0, 3] >= 0.0 and res["pos"][0, 0] > 0.4


@pytest.mark.parametrize("scratch", [1, 25000])
@pytest.mark.parametrize("manycd", [False, True], ids=["shared", "manycd"])
def test_scratch_batches(monkeypatch, manycd, scratch):
    """SR_PLACE_SCRATCH bounds the per-chain partial sums and the slab of profiles: at Q N = 9 x 65 (4680 bytes a
    plane) one byte takes one chain and one row per batch; 25000 bytes take the three chains as 2 + 1 (two planes a
    chain) and the rows two at a time.  The sums are carried across the batches in HBM: the result is the unbatched
    one."""
    N, M, n_sel, count, Q = 65, MC + 1, 3, 5, QT + 1
    plain = run_case("real", "twos", N, M, n_sel, count, Q, manycd)
    monkeypatch.setenv("SR_PLACE_SCRATCH", str(scratch))
    res = run_case("real", "twos", N, M, n_sel, count, Q, manycd)
    for k in OUTS:
        assert np.array_equal(bits(res[k]), bits(plain[k]))


def reflected(rec, N, M, which):
    out = rec.astype(np.int64)
    for k in which:
        out[k, :, :M], out[k, :, M:2 * M] = N - rec[k, :, M:2 * M].astype(np.int64), N - rec[k, :, :M].astype(np.int64)
        out[k, :, 2 * M:] = N - 1 - rec[k, :, 2 * M:].astype(np.int64)
    assert np.abs(out).max() < 32768
    return out.astype(np.int16)


@pytest.mark.parametrize("manycd", [False, True], ids=["shared", "manycd"])
def test_flips(manycd):
    """A flagged chain equals the same call on rows reflected beforehand with no flag, every output; all flags set
    and none set both equal the definition (site differs between the two only through the rounding of Z)."""
    N, M, n_sel, count, Q = 70, 40, 3, 4, 3
    ds, Y, rec, cd = inputs("real", "twos", N, M, n_sel, count, Q, manycd)
    flags = np.array([1, 0, 1], np.uint8)
    got = analysis.placement_from_records(ds, rec, cd, Y, manycd=manycd, flips=flags, lse=True)
    pre = analysis.placement_from_records(ds, reflected(rec, N, M, (0, 2)), cd, Y, manycd=manycd, lse=True)
    check(got, place_ref.placement(N, rec, cd, Y, manycd, flags), N, Q, n_sel, count)
    for k in OUTS:
        assert np.array_equal(bits(got[k]), bits(pre[k])), k
    none = analysis.placement_from_records(ds, rec, cd, Y, manycd=manycd, flips=np.zeros(3, np.uint8), lse=True)
    check(none, ref_of("real", "twos", N, M, n_sel, count, Q, manycd), N, Q, n_sel, count)
    every = analysis.placement_from_records(ds, rec, cd, Y, manycd=manycd, flips=np.ones(3, np.uint8), lse=True)
    check(every, place_ref.placement(N, rec, cd, Y, manycd, [1, 1, 1]), N, Q, n_sel, count)
    assert not np.array_equal(bits(every["pos"]), bits(none["pos"]))
    assert np.allclose(every["pos"], none["pos"][:, ::-1], rtol=1e-12, atol=0) and np.allclose(every["site"], none["site"], rtol=1e-12, atol=0)
    # flags on rows of any int16: the reflection is made in int32
    fds, fY, frec, fcd = inputs("full", "mixed", 6, 5, 2, 9, 3, manycd)
    full = analysis.placement_from_records(fds, frec, fcd, fY, manycd=manycd, flips=[0, 1], lse=True)
    check(full, place_ref.placement(6, frec, fcd, fY, manycd, [0, 1]), 6, 3, 2, 9)


def test_optional_outputs():
    """every combination of the four output pointers gives the full call's arrays; one that asks for nothing succeeds"""
    N, M, n_sel, count, Q = 65, 9, 2, 3, 3
    ds, Y, rec, cd = inputs("real", "twos", N, M, n_sel, count, Q, False)
    full = analysis.placement_from_records(ds, rec, cd, Y, lse=True)
    shapes = {"pos": (Q, N), "site": (Q, N), "lse": (n_sel, count, Q), "lpd": (Q,)}
    for want in itertools.product((False, True), repeat=4):
        out = L.sr_place_out()
        bufs = {k: np.full(shapes[k], -7.0) for k, w in zip(OUTS, want) if w}
        for k, b in bufs.items():
            setattr(out, k, b.ctypes.data_as(_DBLP))
        rc = sa.lib().sr_placement(ctypes.byref(ds.c), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)),
                                   cd.ctypes.data_as(_DBLP), 0, n_sel, count,
                                   Y.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), Q, 0, ctypes.byref(out))
        assert rc == L.SR_OK and (out.kernel_ms > 0) == any(want)
        for k, b in bufs.items():
            assert np.array_equal(bits(b), bits(full[k])), (k, want)
    light = analysis.placement_from_records(ds, rec, cd, Y)
    assert "lse" not in light and np.array_equal(bits(light["lpd"]), bits(full["lpd"]))
    one = analysis.placement_from_records(ds, rec, cd, Y[1])   # one row as [M]
    assert one["pos"].shape == (1, N) and np.array_equal(bits(one["pos"][0]), bits(full["pos"][1]))


@pytest.mark.parametrize("manycd", [0, 1], ids=["shared", "manycd"])
def test_session_form(manycd):
    ds = sa.Dataset.parse(open(os.path.join(DS, "g10s10.txt"), "rb").read())
    seeds, sel = [5, 9, 13, 21], [2, 0, 3]
    X = np.ctypeslib.as_array(ds.c.X, (ds.N * ds.M,)).reshape(ds.N, ds.M)
    Y = X[:4].astype(np.uint8).copy()   # three of the run's own rows (in-sample) and a fragment of the fourth
    Y[3, ::2] = 2

    def sampled(s):
        s.run(5)
        s.reset_records()
        s.run(12, save=True)

    kw = dict(calls_per_launch=12, manycd=manycd)
    with sa.Session(ds, seeds, **kw) as s, sa.Session(ds, seeds, **kw) as plain:
        sampled(s)
        sampled(plain)
        ab0, cdl0 = s.fetch_records()
        cd0 = s.fetch_cd_vectors() if manycd else cdl0
        flags = [0, 1, 0]
        res = analysis.placement_from_session(s, sel, Y, first=2, count=10, flips=flags, lse=True)
        ab1, cdl1 = s.fetch_records()
        assert np.array_equal(ab0, ab1) and np.array_equal(bits(cdl0), bits(cdl1))
        if manycd:
            assert np.array_equal(bits(cd0), bits(s.fetch_cd_vectors()))
        host = analysis.placement_from_records(ds, ab0[sel, 2:12], cd0[sel, 2:12], Y, manycd=bool(manycd), flips=flags,
                                               lse=True)
        want = place_ref.placement(ds.N, ab0[sel, 2:12], cd0[sel, 2:12], Y, bool(manycd), flags)
        check(res, want, ds.N, 4, 3, 10)
        check(host, want, ds.N, 4, 3, 10)
        assert (np.abs(res["pos"].sum(axis=1) - 1.0) < 1e-12).all() and (np.abs(res["site"].sum(axis=1) - 1.0) < 1e-12).all()
        assert (res["pos"] >= 0).all() and (res["lpd"] < 0).all()
        # errors: rows beyond the buffered records, a chain index out of range, no rows, no chains
        for bad in (dict(chains=sel, first=3, count=10), dict(chains=[0, 4], first=0, count=12),
                    dict(chains=[-1], first=0, count=12), dict(chains=sel, first=0, count=0),
                    dict(chains=sel, first=-1, count=4), dict(chains=[], first=0, count=4)):
            with pytest.raises(sa.SrError) as e:
                analysis.placement_from_session(s, queries=Y, **bad)
            assert e.value.code == L.SR_EINVAL
        single = analysis.placement_from_session(s, [1], Y, first=0, count=1)   # one sample is enough
        assert np.allclose(single["pos"].sum(axis=1), 1.0, atol=1e-12)
        s.run(3, save=False)
        plain.run(3, save=False)
        for c in range(len(seeds)):
            x, y = s.state(c), plain.state(c)
            for k in ("a", "b", "pi", "counts"):
                assert np.array_equal(x[k], y[k])
            assert np.array_equal(bits([x["c"], x["d"], x["loglik"]]), bits([y["c"], y["d"], y["loglik"]]))


@pytest.mark.parametrize("name,extra", [("g10s10", []), ("g10s10", ["--manycd"])], ids=["shared", "manycd"])
def test_cli_place(tmp_path, name, extra):
    """python -m seriation_amd --select 2 --place FILE: the three files hold the Python call's numbers for the chosen
    chains' chain_data.csv rows, oriented as the command line orients them."""
    path = os.path.join(DS, name + ".txt")
    ds = sa.Dataset.load(path)
    X = np.ctypeslib.as_array(ds.c.X, (ds.N * ds.M,)).reshape(ds.N, ds.M)
    Y = X[[0, ds.N // 2, ds.N - 1]].astype(np.uint8).copy()
    Y[1, 1::3] = 2
    qfile = tmp_path / "queries.txt"
    qfile.write_text("3 %d\n" % ds.M + "".join(" ".join("01?"[v] for v in row) + "\n" for row in Y))
    r = subprocess.run([sys.executable, "-m", "seriation_amd", path, "--chains", "4", "--burnin", "5", "--samples", "12",
                        "--seed-base", "1", "--root", str(tmp_path), "--select", "2", "--place", str(qfile)] + extra,
                       cwd=PKG, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    chosen = launcher.choose_chains(2, str(tmp_path))
    rec = analysis.read_chain_rows(str(tmp_path), chosen, ds.N, ds.M)
    cd = analysis.read_chain_cd(str(tmp_path), chosen, ds.M, manycd=bool(extra))
    assert np.array_equal(analysis.read_queries(str(qfile), ds.M), Y)
    flips = cli._oriented(ds, rec, 0)
    res = analysis.placement_from_records(ds, rec, cd, Y, manycd=bool(extra), flips=flips)
    want = place_ref.placement(ds.N, rec, cd, Y, bool(extra), flips)
    for k in ("pos", "site", "lpd"):
        assert np.array_equal(bits(res[k]), bits(want[k])), k
    s = analysis.placement_summary(res["pos"], res["site"], analysis.PROBS)
    lines = (tmp_path / "Chains" / "placement.csv").read_text().splitlines()
    assert lines[0] == "query,lpd,mean,mode,q0.025,q0.5,q0.975,best_site,p_best_site" and len(lines) == 4
    assert lines[1:] == ["%d,%r,%r,%d,%s,%d,%r" % (q, float(res["lpd"][q]), float(s["mean"][q]), s["mode"][q],
                                                  ",".join(str(v) for v in s["quant"][:, q]), s["best_site"][q],
                                                  float(s["p_best_site"][q])) for q in range(3)]
    for fname, key, col in (("placement_positions.csv", "pos", "position"), ("placement_sites.csv", "site", "site")):
        lines = (tmp_path / "Chains" / fname).read_text().splitlines()
        assert lines[0] == "query,%s,p" % col and len(lines) == 1 + 3 * ds.N
        assert lines[1:] == ["%d,%d,%r" % (q, j, float(res[key][q, j])) for q in range(3) for j in range(ds.N)]
