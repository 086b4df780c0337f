"""GPU posterior predictive checks (csrc/sr_ppc.hip): every output array equal, as integers, to the numpy definition
in tests/ppc_ref.py at the shapes where the kernels can go wrong -- one cell, the tail of the quad of taxa, one site,
the taxon tile (256 taxa to a workgroup) and the pieces of the sample stream (4 samples at least), ragged shapes, the
batch boundaries of the bounded scratch, any int16 in the rows, constant X, rates at the domain's edges -- the closed
form where the replicate is the alive matrix, determinism with the atomics, the seed and the sample index in the
counter, the reflection identity, the optional outputs, the session form (records in HBM) equal to the host-record
form and leaving the session untouched, and the command line's three files."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import ppc_ref
import seriation_amd as sa
from seriation_amd import _lib as L
from seriation_amd import analysis, launcher

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DS = os.path.join(ROOT, "tests", "golden", "datasets")
PKG = os.path.join(ROOT, "seriation-in-paleontological-data-using-mcmc_amd")
TILE, MIN_ROWS = 256, 4   # csrc/sr_ppc.hip: SRQ_TILE (4 * SRQ_QUADS), SRQ_MIN_ROWS
ARRAYS = ("taxon_gt", "taxon_eq", "taxon_sum_obs", "taxon_sum_rep", "site_gt", "site_eq", "site_sum_rep", "total_obs",
          "total_rep", "total_gt", "total_eq")
LO, HI = -700.0, -2.0 ** -50
_DBLP = ctypes.POINTER(ctypes.c_double)
_U32P = ctypes.POINTER(ctypes.c_uint32)
_I64P = ctypes.POINTER(ctypes.c_int64)


def test_constants_are_the_kernels():
    with open(os.path.join(PKG, "csrc", "sr_ppc.hip")) as fh:
        text = fh.read()
    assert "#define SRQ_QUADS %d " % (TILE // 4) in text and "#define SRQ_TILE (4 * SRQ_QUADS)" in text
    assert "#define SRQ_MIN_ROWS %d " % MIN_ROWS in text


def matrix(xkind, N, M):
    rng = np.random.RandomState(7 * N + M)
    return {"zeros": np.zeros((N, M), np.uint8), "ones": np.ones((N, M), np.uint8),
            "mixed": rng.randint(0, 2, (N, M)).astype(np.uint8)}[xkind]


def records(kind, N, M, n_sel, count):
    """[n_sel][count][2M+N] int16.  real: pi a permutation of the positions, 0 <= a <= b <= N, drifting slowly from
    row to row; full: any int16, a good part of the entries drawn near [0, N] so that alive cells exist (a > b rows,
    limits and positions outside [0, N]), and the int16 extremes placed in a, in b and in pi.  (The generators of
    tests/test_gpu_waic.py.)"""
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


def rates(N, M, n_sel, count, manycd, edges=None):
    """log-scale c in [log 0.001, log 0.1], d in [log 0.2, log 0.8], as the sampler's; the shared form carries a
    loglik entry that is never read (NaN here).  edges: "mixed" both ends of the domain mixed in, "lo" c = d = -700
    everywhere, "hi" c = d = -2^-50 everywhere."""
    rng = np.random.RandomState(31 * N + M + count + 2 * manycd)
    Mt = M if manycd else 1
    c = rng.uniform(np.log(0.001), np.log(0.1), (n_sel, count, Mt))
    d = rng.uniform(np.log(0.2), np.log(0.8), (n_sel, count, Mt))
    if edges == "mixed":
        for v, at in ((LO, 0), (HI, 1), (HI, 2), (LO, 3)):
            c.reshape(-1)[at::7] = v
            d.reshape(-1)[(at + 2) % 4::5] = v
    elif edges in ("lo", "hi"):
        c[:] = d[:] = LO if edges == "lo" else HI
    tail = [] if manycd else [np.full((n_sel, count, 1), np.nan)]
    return np.concatenate([c, d] + tail, axis=2)


_IN, _REF = {}, {}


def inputs(kind, xkind, N, M, n_sel, count, manycd, edges=None):
    key = (kind, xkind, N, M, n_sel, count, manycd, edges)
    if key not in _IN:
        X, rec, cd = matrix(xkind, N, M), records(kind, N, M, n_sel, count), rates(N, M, n_sel, count, manycd, edges)
        for a in (X, rec, cd):
            a.setflags(write=False)
        _IN[key] = (sa.Dataset(X, np.zeros(N, bool)), X, rec, cd)
    return _IN[key]


def ref_of(key, seed, reps):
    if (key, seed, reps) not in _REF:
        _, X, rec, cd = inputs(*key)
        _REF[(key, seed, reps)] = ppc_ref.ppc(X, rec, cd, key[6], seed, reps)
    return _REF[(key, seed, reps)]


def check(res, want, N, M, n_sel, count, reps):
    assert set(res) == set(ARRAYS) | {"pairs", "kernel_ms", "p_taxon", "p_site", "p_total"}
    shapes = {"taxon_gt": (5, M), "taxon_eq": (5, M), "taxon_sum_obs": (5, M), "taxon_sum_rep": (5, M), "site_gt": (N,),
              "site_eq": (N,), "site_sum_rep": (N,), "total_obs": (n_sel, count, 5), "total_rep": (n_sel, count, reps, 5),
              "total_gt": (5,), "total_eq": (5,)}
    for k in ARRAYS:
        assert res[k].shape == shapes[k], k
        assert res[k].dtype == (np.uint32 if k in ("taxon_gt", "taxon_eq", "site_gt", "site_eq") else np.int64), k
        assert np.array_equal(res[k].astype(np.int64), want[k]), k
    assert res["pairs"] == want["pairs"] == n_sel * count * reps and res["kernel_ms"] > 0
    assert np.array_equal(res["p_taxon"], ppc_ref.pvalue(want["taxon_gt"], want["taxon_eq"], want["pairs"]))
    assert np.array_equal(res["p_site"], ppc_ref.pvalue(want["site_gt"], want["site_eq"], want["pairs"]))
    assert np.array_equal(res["p_total"], ppc_ref.pvalue(want["total_gt"], want["total_eq"], want["pairs"]))


def run_case(kind, xkind, N, M, n_sel, count, manycd, edges=None, seed=12345, reps=1):
    key = (kind, xkind, N, M, n_sel, count, manycd, edges)
    ds, X, rec, cd = inputs(*key)
    res = analysis.ppc_from_records(ds, rec, cd, manycd=manycd, seed=seed, reps=reps, totals=True)
    check(res, ref_of(key, seed, reps), N, M, n_sel, count, reps)
    return res


# kind, X, N, M, n_sel, count
SHAPES = [
    pytest.param("real", "mixed", 1, 1, 1, 1, id="smallest"),
    pytest.param("real", "mixed", 5, 3, 2, 3, id="quad-tail-3"),
    pytest.param("real", "mixed", 5, 4, 2, 3, id="quad-exact-4"),
    pytest.param("real", "mixed", 5, 5, 2, 3, id="quad-tail-5"),
    pytest.param("real", "mixed", 1, 9, 2, 3, id="one-site"),
    pytest.param("real", "mixed", 3, TILE, 1, MIN_ROWS, id="exactly-one-tile-one-piece"),
    pytest.param("real", "mixed", 3, TILE + 1, 1, MIN_ROWS + 1, id="one-over"),
    pytest.param("real", "mixed", 3, TILE + 1, 3, 3, id="two-tiles-uneven-pieces"),   # 9 samples: 5 + 4
    pytest.param("real", "mixed", 40, 200, 2, 5, id="ragged"),
    pytest.param("full", "mixed", 6, 5, 2, 9, id="full-int16"),
    pytest.param("real", "zeros", 5, 7, 2, 6, id="x-zeros"),
    pytest.param("real", "ones", 5, 7, 2, 6, id="x-ones"),
    pytest.param("real", "mixed", 124, 139, 3, 100, id="g10s10-shape"),
]


@pytest.mark.parametrize("reps", [1, 3])
@pytest.mark.parametrize("manycd", [False, True], ids=["shared", "manycd"])
@pytest.mark.parametrize("kind,xkind,N,M,n_sel,count", SHAPES)
def test_ppc_equals_definition(kind, xkind, N, M, n_sel, count, manycd, reps):
    res = run_case(kind, xkind, N, M, n_sel, count, manycd, reps=reps)
    if kind == "full":   # the case does hold what it is for
        _, X, rec, _ = inputs(kind, xkind, N, M, n_sel, count, manycd)
        a, b, pi = rec[..., :M], rec[..., M:2 * M], rec[..., 2 * M:]
        assert (a > b).any() and a.min() == -32768 and b.max() == 32767 and pi.max() == 32767 and pi.min() == -32768
        assert ppc_ref.alive_of(rec[0, 0], N, M)[0][0, 0]   # alive between the extremes
        assert res["taxon_sum_rep"][1].max() > 2 * N         # spans beyond the number of sites
    if xkind == "zeros":
        assert not res["taxon_sum_obs"][[0, 1, 2, 4]].any() and res["taxon_sum_obs"][3].any()
    if xkind == "ones":
        assert (res["taxon_sum_obs"][0] == N * res["pairs"]).all() and not res["taxon_sum_obs"][3].any()


@pytest.mark.parametrize("manycd", [False, True], ids=["shared", "manycd"])
def test_rates_at_the_domain_edges(manycd):
    N, M, n_sel, count = 5, 7, 2, 11
    run_case("real", "mixed", N, M, n_sel, count, manycd, edges="mixed", reps=2)
    _, _, _, cd = inputs("real", "mixed", N, M, n_sel, count, manycd, "mixed")
    used = cd[..., :2 * (M if manycd else 1)]
    assert (used == LO).any() and (used == HI).any()
    # c = d = -700: thr_alive = 2^32, thr_dead = 0, the replicate is the alive matrix: no false zero, no false one,
    # and -- the alive sites of a taxon are consecutive positions of a permutation -- no gap, whatever the words
    res = run_case("real", "mixed", N, M, n_sel, count, manycd, edges="lo", reps=2)
    assert not res["taxon_sum_rep"][2:].any() and not res["total_rep"][..., 2:].any()
    _, X, rec, _ = inputs("real", "mixed", N, M, n_sel, count, manycd, "lo")
    alive = sum(int(ppc_ref.alive_of(rec[k, r], N, M)[0].sum()) for k in range(n_sel) for r in range(count))
    assert res["taxon_sum_rep"][0].sum() == 2 * alive and (res["taxon_sum_rep"][0] == res["taxon_sum_rep"][1]).all()
    # c = d = -2^-50, the other end: thr_alive = 0, thr_dead = 2^32 - 1
    res = run_case("real", "mixed", N, M, n_sel, count, manycd, edges="hi", reps=2)
    assert res["taxon_sum_rep"][3].sum() == 2 * alive and res["taxon_sum_rep"][4].any()   # every alive cell a false zero


def test_streams():
    N, M, n_sel, count = 40, 200, 3, 5
    key = ("real", "mixed", N, M, n_sel, count, False, None)
    ds, X, rec, cd = inputs(*key)
    one = run_case(*key, seed=12345, reps=2)
    two = analysis.ppc_from_records(ds, rec, cd, seed=12345, reps=2, totals=True)
    for k in ARRAYS:   # run to run, with the atomics
        assert np.array_equal(one[k], two[k]), k
    for seed in (0, 12346, 12345 + (1 << 32), 2 ** 64 - 1):   # 0 is a seed like any other; the high word counts
        other = analysis.ppc_from_records(ds, rec, cd, seed=seed, reps=2, totals=True)
        assert not np.array_equal(other["total_rep"], one["total_rep"]), seed
        check(other, ppc_ref.ppc(X, rec, cd, False, seed, 2), N, M, n_sel, count, 2)
    # chains in another order: t is part of the counter, so a chain's replicates change with its place
    perm = [2, 0, 1]
    moved = analysis.ppc_from_records(ds, rec[perm], cd[perm], seed=12345, reps=2, totals=True)
    check(moved, ppc_ref.ppc(X, rec[perm], cd[perm], False, 12345, 2), N, M, n_sel, count, 2)
    assert np.array_equal(moved["total_obs"], one["total_obs"][perm])
    assert not np.array_equal(moved["total_rep"], one["total_rep"][perm])


@pytest.mark.parametrize("manycd", [False, True], ids=["shared", "manycd"])
def test_reflection_identity(manycd):
    """GPU against GPU: a' = N - b, b' = N - a, pi' = N - 1 - pi in some chains changes no alive bit, no span, no
    random word and so no output."""
    N, M, n_sel, count = 40, 200, 3, 9
    ds, X, rec, cd = inputs("real", "mixed", N, M, n_sel, count, manycd)
    plain = analysis.ppc_from_records(ds, rec, cd, manycd=manycd, seed=3, reps=2, totals=True)
    refl = rec.astype(np.int64)
    for k in (0, 2):
        refl[k, :, :M], refl[k, :, M:2 * M] = N - rec[k, :, M:2 * M].astype(np.int64), N - rec[k, :, :M].astype(np.int64)
        refl[k, :, 2 * M:] = N - 1 - rec[k, :, 2 * M:].astype(np.int64)
    assert not np.array_equal(refl, rec)
    other = analysis.ppc_from_records(ds, refl.astype(np.int16), cd, manycd=manycd, seed=3, reps=2, totals=True)
    for k in ARRAYS:
        assert np.array_equal(other[k], plain[k]), k
    assert plain["taxon_sum_rep"][1].any() and plain["pairs"] == other["pairs"]


@pytest.mark.parametrize("scratch", [20000, 1])
@pytest.mark.parametrize("manycd", [False, True], ids=["shared", "manycd"])
def test_scratch_batches(monkeypatch, manycd, scratch):
    """SR_PPC_SCRATCH bounds a batch's row sums, totals, thresholds and rates: at N = 5, reps = 3 a sample takes
    60 + 288 + 16 + 24 = 388 bytes with shared rates (20000 bytes: batches of 51 of the 3 x 23 = 69 samples, which cut
    chains in the middle) and 60 + 288 + 4112 + 4112 = 8572 bytes with per-taxon rates at M = 257 (batches of 2); one
    byte takes the samples one by one.  The tallies are carried across the batches in HBM: the result is the
    unbatched one."""
    N, M, n_sel, count = 5, TILE + 1, 3, 23
    plain = run_case("real", "mixed", N, M, n_sel, count, manycd, reps=3)
    monkeypatch.setenv("SR_PPC_SCRATCH", str(scratch))
    res = run_case("real", "mixed", N, M, n_sel, count, manycd, reps=3)
    for k in ARRAYS:
        assert np.array_equal(res[k], plain[k]), k


def test_optional_outputs():
    """each output pointer alone gives its entry of the full call; the scalars are always written"""
    N, M, n_sel, count, reps = 40, 200, 2, 5, 2
    ds, X, rec, cd = inputs("real", "mixed", N, M, n_sel, count, False)
    full = analysis.ppc_from_records(ds, rec, cd, seed=9, reps=reps, totals=True)
    shapes = {"taxon_gt": (5, M), "taxon_eq": (5, M), "taxon_sum_obs": (5, M), "taxon_sum_rep": (5, M), "site_gt": (N,),
              "site_eq": (N,), "site_sum_rep": (N,), "total_obs": (n_sel, count, 5), "total_rep": (n_sel, count, reps, 5)}
    for only in (None,) + tuple(shapes):
        out = L.sr_ppc_out()
        buf = None
        if only:
            u32 = only in ("taxon_gt", "taxon_eq", "site_gt", "site_eq")
            buf = np.full(shapes[only], 77, np.uint32 if u32 else np.int64)
            setattr(out, only, buf.ctypes.data_as(_U32P if u32 else _I64P))
        rc = sa.lib().sr_ppc(ctypes.byref(ds.c), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)),
                             cd.ctypes.data_as(_DBLP), 0, n_sel, count, 9, reps, 0, ctypes.byref(out))
        assert rc == L.SR_OK and out.kernel_ms > 0 and out.pairs == n_sel * count * reps
        if only:
            assert np.array_equal(buf, full[only]), only
        assert list(out.total_gt) == full["total_gt"].tolist() and list(out.total_eq) == full["total_eq"].tolist()
    light = analysis.ppc_from_records(ds, rec, cd, seed=9, reps=reps)
    assert "total_obs" not in light and "total_rep" not in light
    assert np.array_equal(light["taxon_gt"], full["taxon_gt"]) and np.array_equal(light["p_total"], full["p_total"])


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


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
        res = analysis.ppc_from_session(s, sel, first=4, count=36, seed=77, reps=2, totals=True)
        ab1, cdl1 = s.fetch_records()
        assert np.array_equal(ab0, ab1) and np.array_equal(bits(cdl0), bits(cdl1))
        if manycd:
            assert np.array_equal(bits(cd0), bits(s.fetch_cd_vectors()))
        host = analysis.ppc_from_records(ds, ab0[sel, 4:40], cd0[sel, 4:40], manycd=bool(manycd), seed=77, reps=2,
                                         totals=True)
        X = np.ctypeslib.as_array(ds.c.X, (ds.N * ds.M,)).reshape(ds.N, ds.M)
        want = ppc_ref.ppc(X, ab0[sel, 4:40], cd0[sel, 4:40], bool(manycd), 77, 2)
        check(res, want, ds.N, ds.M, 3, 36, 2)
        check(host, want, ds.N, ds.M, 3, 36, 2)
        one = analysis.ppc_from_session(s, [1], first=0, count=1)   # a single sample is legal here
        assert one["pairs"] == 1
        # errors: rows beyond the buffered records, a chain index out of range, no rows, no chains
        for bad in (dict(chains=sel, first=5, count=36), dict(chains=[0, 4], first=0, count=40),
                    dict(chains=[-1], first=0, count=40), dict(chains=sel, first=0, count=0),
                    dict(chains=sel, first=-1, count=4), dict(chains=[], first=0, count=4),
                    dict(chains=sel, first=0, count=4, reps=0), dict(chains=sel, first=0, count=4, reps=65)):
            with pytest.raises(sa.SrError) as e:
                analysis.ppc_from_session(s, **bad)
            assert e.value.code == L.SR_EINVAL
        s.run(3, save=False)
        plain.run(3, save=False)
        for c in range(len(seeds)):
            x, y = s.state(c), plain.state(c)
            for k in ("a", "b", "pi", "counts"):
                assert np.array_equal(x[k], y[k])
            assert np.array_equal(bits([x["c"], x["d"], x["loglik"]]), bits([y["c"], y["d"], y["loglik"]]))


@pytest.mark.parametrize("name,extra", [("g2s2", []), ("g10s10", ["--manycd"])], ids=["shared", "manycd"])
def test_cli_ppc(tmp_path, name, extra):
    """python -m seriation_amd --select 2 --ppc --ppc-seed 7 --ppc-reps 2: the three files hold the definition's
    numbers for the chosen chains' chain_data.csv rows."""
    path = os.path.join(DS, name + ".txt")
    r = subprocess.run([sys.executable, "-m", "seriation_amd", path, "--chains", "4", "--burnin", "5", "--samples", "20",
                        "--seed-base", "1", "--root", str(tmp_path), "--select", "2", "--ppc", "--ppc-seed", "7",
                        "--ppc-reps", "2"] + extra, cwd=PKG, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ds = sa.Dataset.load(path)
    chosen = launcher.choose_chains(2, str(tmp_path))
    assert ("selected: " + " ".join(str(k) for k in chosen)) in r.stdout and 1 <= len(chosen) <= 2
    rec = analysis.read_chain_rows(str(tmp_path), chosen, ds.N, ds.M)
    cd = analysis.read_chain_cd(str(tmp_path), chosen, ds.M, manycd=bool(extra))
    assert rec.shape == (len(chosen), 20, 2 * ds.M + ds.N)
    X = np.ctypeslib.as_array(ds.c.X, (ds.N * ds.M,)).reshape(ds.N, ds.M)
    want = ppc_ref.ppc(X, rec, cd, bool(extra), 7, 2)
    pairs = len(chosen) * 20 * 2
    assert want["pairs"] == pairs
    pt = ppc_ref.pvalue(want["total_gt"], want["total_eq"], pairs)
    ptax = ppc_ref.pvalue(want["taxon_gt"], want["taxon_eq"], pairs)
    psite = ppc_ref.pvalue(want["site_gt"], want["site_eq"], pairs)
    lines = (tmp_path / "Chains" / "ppc.csv").read_text().splitlines()
    assert lines[0] == "stat,obs_mean,rep_mean,p,gt,eq,pairs" and len(lines) == 6
    for i, name_ in enumerate(ppc_ref.STATS):
        assert lines[1 + i] == "%s,%r,%r,%r,%d,%d,%d" % (
            name_, float(int(want["total_obs"][..., i].sum()) * 2) / float(pairs),
            float(int(want["total_rep"][..., i].sum())) / float(pairs), float(pt[i]), want["total_gt"][i],
            want["total_eq"][i], pairs)
    lines = (tmp_path / "Chains" / "ppc_taxa.csv").read_text().splitlines()
    assert lines[0] == "taxon,stat,obs_mean,rep_mean,p" and len(lines) == 1 + 5 * ds.M
    assert lines[1:] == ["%d,%s,%r,%r,%r" % (m, ppc_ref.STATS[i], float(want["taxon_sum_obs"][i, m]) / float(pairs),
                                             float(want["taxon_sum_rep"][i, m]) / float(pairs), float(ptax[i, m]))
                         for m in range(ds.M) for i in range(5)]
    lines = (tmp_path / "Chains" / "ppc_sites.csv").read_text().splitlines()
    assert lines[0] == "site,obs,rep_mean,p" and len(lines) == 1 + ds.N
    assert lines[1:] == ["%d,%d,%r,%r" % (n, int(X[n].astype(bool).sum()), float(want["site_sum_rep"][n]) / float(pairs),
                                          float(psite[n])) for n in range(ds.N)]
