"""GPU central sampled state (csrc/sr_central.hip): pooled pair counts, order loss, limit loss, the central row and its
state equal to the numpy definition in tests/central_ref.py (np.array_equal) at the shapes where the kernels can go
wrong, the invariants of permutation rows, the reflection identity, ties in the argmin, the 64-bit sums, the scratch
bands and column batches, the optional outputs, the session form (records in HBM) equal to the host-record form and
leaving the session untouched, and the command line's three files."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import central_ref
import seriation_amd as sa
from seriation_amd import _lib as L
from seriation_amd import analysis

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DS = os.path.join(ROOT, "tests", "golden", "datasets")
PKG = os.path.join(ROOT, "seriation-in-paleontological-data-using-mcmc_amd")
I64P = ctypes.POINTER(ctypes.c_int64)
I32P = ctypes.POINTER(ctypes.c_int32)
U32P = ctypes.POINTER(ctypes.c_uint32)


def dataset(N, M):
    return sa.Dataset(np.zeros((N, M), np.uint8), np.zeros(N, bool))


def records(kind, N, M, n_sel, count):
    """[n_sel][count][2M+N] int16, the generators of tests/test_gpu_agreement.py with limits that are read here: drawn in
    [0, N] for perm and from all of int16 for full.
    perm: every row a permutation, pi[site] = position; a chain starts from a base order (chain 1's the reverse of
    chain 0's, the others' their own) and every row applies a few more swaps of neighbours to the order of the row
    before it.  full: any int16, half of the entries from a narrow range (ties), the extremes placed."""
    rng = np.random.RandomState(1000 * N + 10 * n_sel + count)
    out = np.empty((n_sel, count, 2 * M + N), np.int64)
    if kind == "full":
        out[:, :, :2 * M] = rng.randint(-32768, 32768, (n_sel, count, 2 * M))
        near = rng.randint(-2, N + 3, (n_sel, count, 2 * M))
        pick = rng.randint(0, 2, (n_sel, count, 2 * M)) > 0
        out[:, :, :2 * M][pick] = near[pick]
        out[0, 0, 0], out[0, 0, M], out[1, 1, 0], out[1, 1, M] = -32768, 32767, 32767, -32768
        x = rng.randint(-32768, 32768, (n_sel, count, N))
        narrow = rng.randint(-2, 3, (n_sel, count, N))
        take = rng.randint(0, 2, (n_sel, count, N)) > 0
        x[take] = narrow[take]
        x[0, 0, 0], x[0, 0, N - 1], x[1, 2, 1], x[1, 2, 2] = -32768, 32767, 32767, 32767
        x[2, 1, :] = -32768
        out[:, :, 2 * M:] = x
        return out.astype(np.int16)
    out[:, :, :2 * M] = rng.randint(0, N + 1, (n_sel, count, 2 * M))
    base0 = rng.permutation(N)
    for k in range(n_sel):
        order = base0.copy() if k == 0 else (base0[::-1].copy() if k == 1 else rng.permutation(N))   # order[pos] = site
        for t in range(count):
            for p in (rng.randint(0, N - 1, 1 + N // 16) if N > 1 else ()):
                order[p], order[p + 1] = order[p + 1], order[p]
            out[k, t, 2 * M + order] = np.arange(N)
    return out.astype(np.int16)


def flips_of(n_sel):
    """chain 1 flagged where there is one"""
    return None if n_sel < 2 else [int(k == 1) for k in range(n_sel)]


_REC, _REF = {}, {}


def rec_of(kind, N, M, n_sel, count):
    key = (kind, N, M, n_sel, count)
    if key not in _REC:
        _REC[key] = records(kind, N, M, n_sel, count)
        _REC[key].setflags(write=False)
    return _REC[key]


def ref_of(kind, N, M, n_sel, count):
    key = (kind, N, M, n_sel, count)
    if key not in _REF:
        _REF[key] = central_ref.central(rec_of(kind, N, M, n_sel, count), N, M, flips_of(n_sel))
    return _REF[key]


def check(res, want, N, M, n_sel, count, pair_counts=True):
    assert set(res) == {"order_loss", "limit_loss", "best", "central", "state", "scale", "kernel_ms"} | (
        {"pair_counts"} if pair_counts else set())
    if pair_counts:
        assert res["pair_counts"].dtype == np.uint32 and res["pair_counts"].shape == (N, N)
        assert np.array_equal(res["pair_counts"], want["pair_counts"])
    for k in ("order_loss", "limit_loss"):
        assert res[k].dtype == np.int64 and res[k].shape == (n_sel, count), k
        assert np.array_equal(res[k], want[k]), k
    assert res["best"].dtype == np.int32 and np.array_equal(res["best"], want["best"])
    assert res["central"] == want["central"]
    for k, n in (("a", M), ("b", M), ("pi", N)):
        assert res["state"][k].dtype == np.int32 and res["state"][k].shape == (n,), k
        assert np.array_equal(res["state"][k], want["state"][k]), k
    assert res["scale"] == want["scale"] and res["kernel_ms"] > 0


# kind, N, M, n_sel, count
CASES = [
    pytest.param("perm", 1, 1, 2, 3, id="no-pairs"),
    pytest.param("perm", 2, 1, 1, 1, id="smallest"),
    pytest.param("full", 5, 2, 3, 17, id="full-int16"),
    pytest.param("perm", 64, 1, 2, 65, id="one-tile-one-row-over-a-group"),
    pytest.param("perm", 65, 1, 2, 65, id="one-column-over"),
    pytest.param("perm", 200, 3, 3, 33, id="ragged-tiles"),
    pytest.param("perm", 124, 139, 9, 100, id="g10s10-shape"),
    pytest.param("perm", 8, 1, 17, 1100, id="many-chains-many-rows"),
    pytest.param("perm", 1030, 1, 2, 20, id="many-tile-rows"),
]


@pytest.mark.parametrize("kind,N,M,n_sel,count", CASES)
def test_central_equals_definition(kind, N, M, n_sel, count):
    rec = rec_of(kind, N, M, n_sel, count)
    res = analysis.central_from_records(dataset(N, M), rec, flips=flips_of(n_sel), pair_counts=True)
    want = ref_of(kind, N, M, n_sel, count)
    check(res, want, N, M, n_sel, count)
    T = n_sel * count
    assert res["scale"] == T * (N * (N - 1) // 2)
    C = res["pair_counts"].astype(np.int64)
    off = ~np.eye(N, dtype=bool)
    assert not np.diag(C).any()
    if N == 1:   # no pairs: the limit loss alone decides
        assert not res["order_loss"].any() and res["scale"] == 0
        ck, ct = res["central"]
        assert res["limit_loss"][ck, ct] == res["limit_loss"].min()
    if kind == "perm":
        assert ((C + C.T)[off] == T).all()
        assert int(res["order_loss"].sum()) == 2 * int(np.triu(C * C.T, 1).sum())
        ck, ct = res["central"]
        assert sorted(res["state"]["pi"].tolist()) == list(range(N))
        assert res["order_loss"][ck, ct] == res["order_loss"].min()
    else:   # the case does hold what it is for
        assert ((C + C.T)[off] < T).any()
        assert rec.min() == -32768 and rec.max() == 32767
        assert rec[:, :, :2 * M].min() < 0 and rec[:, :, :2 * M].max() > N


def test_reflection_identity():
    """GPU against GPU: one chain's rows reflected and the chain flagged leaves every output equal; reflected and not
    flagged does not."""
    N, M, n_sel, count, l = 124, 139, 9, 100, 3
    ds, rec = dataset(N, M), rec_of("perm", N, M, n_sel, count)
    flips = flips_of(n_sel)
    plain = analysis.central_from_records(ds, rec, flips=flips, pair_counts=True)
    refl = rec.copy()
    refl[l, :, :M], refl[l, :, M:2 * M] = N - rec[l, :, M:2 * M], N - rec[l, :, :M]
    refl[l, :, 2 * M:] = N - 1 - rec[l, :, 2 * M:]
    f2 = list(flips)
    f2[l] ^= 1
    got = analysis.central_from_records(ds, refl, flips=f2, pair_counts=True)
    check(got, plain, N, M, n_sel, count)
    unflagged = analysis.central_from_records(ds, refl, flips=flips, pair_counts=True)
    assert not np.array_equal(unflagged["order_loss"], plain["order_loss"])
    assert not np.array_equal(unflagged["limit_loss"], plain["limit_loss"])
    assert not np.array_equal(unflagged["pair_counts"], plain["pair_counts"])


def test_ties_in_the_argmin():
    """Chain 1 a byte copy of chain 0: the central chain is 0; two equal rows in a chain: the lower t."""
    N, M, count = 65, 2, 40
    one = rec_of("perm", N, M, 1, count)
    ds = dataset(N, M)
    rec = np.concatenate([one, one]).copy()
    res = analysis.central_from_records(ds, rec)
    assert res["central"][0] == 0 and np.array_equal(res["order_loss"][0], res["order_loss"][1])
    assert res["best"][0] == res["best"][1] == res["central"][1]
    # the best row again, earlier and later in both chains: the earliest wins
    tb = res["central"][1]
    lo, hi = (0, count - 1) if tb not in (0, count - 1) else (1, count - 2)
    rec[:, lo], rec[:, hi] = rec[:, tb], rec[:, tb]
    res = analysis.central_from_records(ds, rec)
    want = central_ref.central(rec, N, M)
    assert want["central"] == (0, lo) and res["central"] == (0, lo) and list(res["best"]) == [lo, lo]
    assert res["order_loss"][0, lo] == res["order_loss"][0, hi] == res["order_loss"][1, tb]


def test_order_loss_needs_64_bits():
    """The identity row at N = 64 against counts all 2^31 - 1: 2016 pairs, each adds 2^31 - 1."""
    N, M = 64, 1
    rec = np.zeros((1, 1, 2 * M + N), np.int16)
    rec[0, 0, 2 * M:] = np.arange(N)
    ag = np.full((N, N), 2 ** 31 - 1, np.uint32)
    r = analysis.order_loss(dataset(N, M), rec, ag)
    assert r["order_loss"].tolist() == [[2016 * (2 ** 31 - 1)]] and 2016 * (2 ** 31 - 1) > 2 ** 32 and r["kernel_ms"] > 0


@pytest.mark.parametrize("hi", [2 ** 32, 2 ** 22], ids=["any-uint32", "narrow-sums"])
def test_order_loss_against_any_counts(hi):
    """Random counts at N = 70 with 17 x 3 rows, one chain flagged: below 2^22 (a wave's share of a tile summed in 32
    bits) and over all of uint32 (every add 64-bit)."""
    N, M, n_sel, count = 70, 2, 17, 3
    rng = np.random.RandomState(70)
    ag = rng.randint(0, hi, (N, N), dtype=np.uint64).astype(np.uint32)
    rec = rec_of("perm", N, M, n_sel, count)
    flips = flips_of(n_sel)
    r = analysis.order_loss(dataset(N, M), rec, ag, flips=flips)
    _a, _b, pi = central_ref.oriented(rec, N, M, flips)
    want = central_ref.order_loss(pi, ag).reshape(n_sel, count)
    assert r["order_loss"].dtype == np.int64 and np.array_equal(r["order_loss"], want)
    # either way a row's total over the 2415 pairs passes 2^32; only the counts differ in width
    assert (want > 2 ** 32).any() and (int(ag.max()) < 2 ** 22) == (hi == 2 ** 22)
    full = rec_of("full", 5, 2, 3, 17)   # ties and extremes
    ag5 = rng.randint(0, hi, (5, 5), dtype=np.uint64).astype(np.uint32)
    r = analysis.order_loss(dataset(5, 2), full, ag5, flips=[0, 1, 0])
    _a, _b, pi = central_ref.oriented(full, 5, 2, [0, 1, 0])
    assert np.array_equal(r["order_loss"], central_ref.order_loss(pi, ag5).reshape(3, 17))


@pytest.mark.parametrize("N,M,n_sel,count", [(200, 3, 3, 33), (124, 139, 9, 100)])
def test_order_loss_against_the_pooled_counts(N, M, n_sel, count):
    ds, rec, flips = dataset(N, M), rec_of("perm", N, M, n_sel, count), flips_of(n_sel)
    res = analysis.central_from_records(ds, rec, flips=flips, pair_counts=True)
    alone = analysis.order_loss(ds, rec, res["pair_counts"], flips=flips)
    assert np.array_equal(alone["order_loss"], res["order_loss"])


@pytest.mark.parametrize("N,M,n_sel,count", [(200, 3, 3, 33), (124, 139, 9, 100), (1030, 1, 2, 20)])
def test_scratch_bound_does_not_change_the_result(monkeypatch, N, M, n_sel, count):
    """A scratch bound below one tile row and below a handful of limit columns: one band per tile row, several column
    batches, the same outputs."""
    ds, rec, flips = dataset(N, M), rec_of("perm", N, M, n_sel, count), flips_of(n_sel)
    want = ref_of("perm", N, M, n_sel, count)
    monkeypatch.setenv("SR_CENTRAL_SCRATCH", "65536")
    banded = analysis.central_from_records(ds, rec, flips=flips, pair_counts=True)
    check(banded, want, N, M, n_sel, count)
    alone = analysis.order_loss(ds, rec, want["pair_counts"], flips=flips)
    assert np.array_equal(alone["order_loss"], want["order_loss"])


def test_optional_outputs():
    N, M, n_sel, count = 200, 3, 3, 33
    ds, rec = dataset(N, M), rec_of("perm", N, M, n_sel, count)
    want = ref_of("perm", N, M, n_sel, count)
    flips = np.array(flips_of(n_sel), np.uint8)
    recp = rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))
    shapes = {"order_loss": ((n_sel, count), np.int64, I64P), "limit_loss": ((n_sel, count), np.int64, I64P),
              "pair_counts": ((N, N), np.uint32, U32P), "best": ((n_sel,), np.int32, I32P),
              "state": ((2 * M + N,), np.int32, I32P)}
    state = np.concatenate([want["state"][k] for k in ("a", "b", "pi")])
    for only in (None,) + tuple(shapes):
        out = L.sr_central_out()
        out.flip = flips.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        if only:
            shape, dtype, ptr = shapes[only]
            buf = np.zeros(shape, dtype)
            setattr(out, only, buf.ctypes.data_as(ptr))
        assert sa.lib().sr_central(ctypes.byref(ds.c), recp, n_sel, count, 0, ctypes.byref(out)) == L.SR_OK
        if only:
            assert np.array_equal(buf, state if only == "state" else want[only]), only
        assert (out.central_chain, out.central_row) == want["central"]
        assert out.scale == want["scale"] and out.kernel_ms > 0
    loss = np.zeros((n_sel, count), np.int64)   # sr_order_loss without kernel_ms
    pc = np.ascontiguousarray(want["pair_counts"])
    assert sa.lib().sr_order_loss(ctypes.byref(ds.c), recp, n_sel, count, flips.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                  pc.ctypes.data_as(U32P), 0, loss.ctypes.data_as(I64P), None) == L.SR_OK
    assert np.array_equal(loss, want["order_loss"])


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def sampled(s):
    s.run(300)
    s.reset_records()
    s.run(200, save=True)


def test_session_form():
    ds = sa.Dataset.parse(open(os.path.join(DS, "g10s10.txt"), "rb").read())
    seeds, sel, flips = list(range(1, 9)), [2, 0, 5, 3], [0, 1, 0, 0]
    with sa.Session(ds, seeds, calls_per_launch=200) as s, sa.Session(ds, seeds, calls_per_launch=200) as plain:
        sampled(s)
        sampled(plain)
        ab0, cdl0 = s.fetch_records()
        res = analysis.central_from_session(s, sel, first=4, count=196, flips=flips, pair_counts=True)
        whole = analysis.central_from_session(s, [3, 4])
        ab1, cdl1 = s.fetch_records()
        assert np.array_equal(ab0, ab1) and np.array_equal(bits(cdl0), bits(cdl1))
        host = analysis.central_from_records(ds, ab0[sel, 4:200], flips=flips, pair_counts=True)
        want = central_ref.central(ab0[sel, 4:200], ds.N, ds.M, flips)
        check(res, want, ds.N, ds.M, 4, 196)
        check(host, want, ds.N, ds.M, 4, 196)
        check(whole, central_ref.central(ab0[[3, 4]], ds.N, ds.M), ds.N, ds.M, 2, 200, pair_counts=False)
        # two chains of one mode: the central row is a state the sampler produced
        st = whole["state"]
        assert sorted(st["pi"].tolist()) == list(range(ds.N)) and (st["a"] <= st["b"]).all()
        assert 0 < whole["order_loss"].min() / whole["scale"] < 0.5   # 0.5: a row unrelated to the others
        # errors: rows beyond the buffered records, a chain index out of range, no rows
        for bad in (dict(chains=sel, first=5, count=196), dict(chains=[0, 8], first=0, count=200),
                    dict(chains=[-1], first=0, count=200), dict(chains=sel, first=0, count=0),
                    dict(chains=sel, first=-1, count=4), dict(chains=[], first=0, count=4)):
            with pytest.raises(sa.SrError) as e:
                analysis.central_from_session(s, **bad)
            assert e.value.code == L.SR_EINVAL
        s.run(3, save=False)
        plain.run(3, save=False)
        for c in range(len(seeds)):
            x, y = s.state(c), plain.state(c)
            for k in ("a", "b", "pi", "counts"):
                assert np.array_equal(x[k], y[k])
            assert np.array_equal(bits([x["c"], x["d"], x["loglik"]]), bits([y["c"], y["d"], y["loglik"]]))


def test_cli_central(tmp_path):
    """python -m seriation_amd --select 2 --central: the three files hold the definition's numbers for the chosen
    chains' chain_data.csv rows."""
    path = os.path.join(DS, "g2s2.txt")
    r = subprocess.run([sys.executable, "-m", "seriation_amd", path, "--chains", "4", "--burnin", "5", "--samples", "20",
                        "--seed-base", "1", "--root", str(tmp_path), "--select", "2", "--central"], cwd=PKG,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    chosen = [int(v) for v in [ln for ln in out if ln.startswith("selected:")][0].split()[1:]]
    assert len(chosen) == 2
    ds = sa.Dataset.load(path)
    rec = analysis.read_chain_rows(str(tmp_path), chosen, ds.N, ds.M)
    assert rec.shape == (2, 20, 2 * ds.M + ds.N)
    # the orientation the command line uses, by its own definition: the sign of the covariance of the pi sums
    pi_sum = rec[:, :, 2 * ds.M:].astype(np.int64).sum(axis=1)
    flips = [int(ds.N * int((pi_sum[0] * y).sum()) - int(pi_sum[0].sum()) * int(y.sum()) < 0) for y in pi_sum]
    want = central_ref.central(rec, ds.N, ds.M, flips)
    ck, ct = want["central"]
    assert ("central: chain %d row %d" % (chosen[ck], ct)) in out
    lines = (tmp_path / "Chains" / "central_order.csv").read_text().splitlines()
    assert lines[0] == "site,position" and len(lines) == 1 + ds.N
    assert [[int(v) for v in ln.split(",")] for ln in lines[1:]] == [[n, int(want["state"]["pi"][n])] for n in range(ds.N)]
    lines = (tmp_path / "Chains" / "central_taxa.csv").read_text().splitlines()
    assert lines[0] == "taxon,a,b" and len(lines) == 1 + ds.M
    assert [[int(v) for v in ln.split(",")] for ln in lines[1:]] == [
        [m, int(want["state"]["a"][m]), int(want["state"]["b"][m])] for m in range(ds.M)]
    lines = (tmp_path / "Chains" / "central_loss.csv").read_text().splitlines()
    assert lines[0] == "chain,flip,best_row,order_loss,limit_loss,order_loss_sum,is_central" and len(lines) == 3
    for k, line in enumerate(lines[1:]):
        t = int(want["best"][k])
        assert [int(v) for v in line.split(",")] == [chosen[k], flips[k], t, int(want["order_loss"][k, t]),
                                                     int(want["limit_loss"][k, t]), int(want["order_loss"][k].sum()),
                                                     int(k == ck)]
