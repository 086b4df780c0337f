"""GPU convergence diagnostics (csrc/sr_diag.hip): the raw lagged moments bit-equal to numpy int64, split-R-hat /
ESS / cut_lag against the definition in tests/diag_ref.py, the session form (records in HBM) equal to the host-record
form and leaving the session untouched, and the argument errors."""
import math
import os

import numpy as np
import pytest

import diag_ref
import seriation_amd as sa
from seriation_amd import _lib as L
from seriation_amd import analysis
from diag_ref import TOL, ar1

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DS = os.path.join(ROOT, "tests", "golden", "datasets")


def dataset(N, M):
    return sa.Dataset(np.zeros((N, M), np.uint8), np.zeros(N, bool))


def records(kind, N, M, n_sel, count):
    """[n_sel][count][2M+N] int16.  full: any int16; mid: |x| <= 5000 (32-bit runs shorter than a sequence);
    small: |x| <= 40; real: autocorrelated limits in [0, N] and slowly moving permutations."""
    rng = np.random.RandomState(1000 * N + 10 * M + count)
    W = 2 * M + N
    if kind == "full":
        x = rng.randint(-32768, 32768, (n_sel, count, W))
        x[0, 0, 0], x[0, 1, W - 1] = -32768, 32767
        return x.astype(np.int16)
    if kind == "mid":
        return rng.randint(-5000, 5001, (n_sel, count, W)).astype(np.int16)
    if kind == "small":
        return rng.randint(-40, 41, (n_sel, count, W)).astype(np.int16)
    out = np.empty((n_sel, count, W), np.int64)
    for m in range(2 * M):
        out[:, :, m] = np.clip(np.rint(ar1(rng, 0.8, n_sel, count, N / 8.0) + N / 2.0), 0, N)
    score = np.stack([ar1(rng, 0.9, n_sel, count, 6.0) + i for i in range(N)], axis=2)
    out[:, :, 2 * M:] = np.argsort(np.argsort(score, axis=2), axis=2)   # pi[site] = position
    return out.astype(np.int16)


_CACHE = {}


def run_case(kind, N, M, n_sel, count, max_lag, scalars=False):
    """One GPU call and one numpy reference per case, shared by the tests."""
    key = (kind, N, M, n_sel, count, max_lag, scalars)
    if key not in _CACHE:
        rec = records(kind, N, M, n_sel, count)
        cdl = None
        if scalars:
            rng = np.random.RandomState(count)
            cdl = np.stack([ar1(rng, 0.6, n_sel, count, 0.05) - 3.0, ar1(rng, 0.3, n_sel, count, 0.02) - 1.5,
                            ar1(rng, 0.8, n_sel, count, 9.0) - 4000.0], axis=2)
        res = analysis.diagnostics_from_records(dataset(N, M), rec, cdl, max_lag=max_lag, moments=True)
        _CACHE[key] = (rec, cdl, res, diag_ref.moments(rec, max_lag))
    return _CACHE[key]


MOMENT_CASES = [
    ("full", 5, 3, 1, 4, 0),         # h = 2, L = 1: the smallest legal input
    ("full", 5, 3, 2, 17, 0),        # odd count: the middle row is dropped
    ("real", 124, 139, 3, 100, 0),   # W = 402: the last tile is partly filled
    ("real", 300, 70, 2, 250, 31),   # truncated lags
    ("full", 5, 3, 1, 2500, 0),      # h = 1250: a half-chain longer than an LDS-resident tile (64-bit sums)
    ("small", 5, 3, 1, 2500, 0),     # the same through the 32-bit runs
    ("full", 124, 139, 3, 100, 0),   # several lag passes per wave, 64-bit sums, LDS tile
    ("mid", 5, 3, 1, 600, 0),        # 32-bit runs of 80 rows: flushed several times per pass
    ("full", 5, 3, 1, 2494, 0),      # h = 1247: the longest half-chain staged in LDS (163728 of a workgroup's 163840 bytes)
    ("full", 5, 3, 1, 2496, 0),      # h = 1248: the shortest that reads global memory
]


@pytest.mark.parametrize("kind,N,M,n_sel,count,max_lag", MOMENT_CASES)
def test_moments_bit_equal_numpy(kind, N, M, n_sel, count, max_lag):
    rec, _, res, (P, F, B, S1) = run_case(kind, N, M, n_sel, count, max_lag)
    h, lags = diag_ref.lags_of(count, max_lag)
    assert res["P"].shape == (2 * n_sel, lags + 1, 2 * M + N) and res["P"].dtype == np.int64
    assert np.array_equal(res["S1"], S1)
    assert np.array_equal(res["F"], F)
    assert np.array_equal(res["B"], B)
    assert np.array_equal(res["P"], P)
    assert res["kernel_ms"] > 0


@pytest.mark.parametrize("value", [32767, -32768])
def test_moments_int16_extremes(value):
    N, M, count = 5, 3, 2400
    h = count // 2
    rec = np.full((1, count, 2 * M + N), value, np.int16)
    res = analysis.diagnostics_from_records(dataset(N, M), rec, None, moments=True)
    assert (res["P"][:, 0, :] == h * value * value).all()
    k = np.arange(h)[None, :, None]
    assert np.array_equal(res["P"], np.broadcast_to((h - k) * value * value, res["P"].shape))
    assert (res["S1"] == h * value).all()
    for name in ("a", "b", "pi"):
        assert np.isnan(res["rhat"][name]).all() and np.isnan(res["ess"][name]).all() and (res["cut_lag"][name] == -1).all()
    assert math.isnan(res["rhat"]["loglik"]) and res["cut_lag"]["c"] == -1   # no cdl supplied


def flat(res, key):
    v = res[key]
    return np.concatenate([v["a"], v["b"], v["pi"], [v["c"], v["d"], v["loglik"]]])


@pytest.mark.parametrize("N,M,n_sel,count,max_lag", [(124, 139, 3, 100, 0), (300, 70, 2, 250, 31)])
def test_rhat_ess_match_definition(N, M, n_sel, count, max_lag):
    rec, cdl, res, _ = run_case("real", N, M, n_sel, count, max_lag, scalars=True)
    P, F, B, S1 = diag_ref.moments(rec, max_lag)
    rhat, ess, cut = diag_ref.reduce(P, F, B, S1, count, max_lag, cdl)   # asserts the margin condition
    print("rel diff rhat %.3e ess %.3e" % (diag_ref.rel_diff(flat(res, "rhat"), rhat), diag_ref.rel_diff(flat(res, "ess"), ess)))
    assert np.array_equal(flat(res, "cut_lag"), cut)
    assert diag_ref.rel_diff(flat(res, "rhat"), rhat) <= TOL
    assert diag_ref.rel_diff(flat(res, "ess"), ess) <= TOL
    assert np.isfinite(rhat[-3:]).all() and np.isfinite(rhat[:2 * M + N]).any()


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def test_session_form():
    ds = sa.Dataset.parse(open(os.path.join(DS, "g10s10.txt"), "rb").read())
    seeds, sel = [5, 9, 13, 21], [2, 0, 3]

    def sampled(s):
        s.run(5)
        s.reset_records()
        s.run(40, save=True)

    with sa.Session(ds, seeds, calls_per_launch=40) as s, sa.Session(ds, seeds, calls_per_launch=40) as plain:
        sampled(s)
        sampled(plain)
        ab0, cdl0 = s.fetch_records()
        res = analysis.diagnostics_from_session(s, sel, first=4, count=36, moments=True)
        ab1, cdl1 = s.fetch_records()
        assert np.array_equal(ab0, ab1) and np.array_equal(bits(cdl0), bits(cdl1))
        want = analysis.diagnostics_from_records(ds, ab0[sel, 4:40], cdl0[sel, 4:40], moments=True)
        for k in ("P", "F", "B", "S1"):
            assert np.array_equal(res[k], want[k])
        for k in ("rhat", "ess"):
            assert np.array_equal(bits(flat(res, k)), bits(flat(want, k)))
        assert np.array_equal(flat(res, "cut_lag"), flat(want, "cut_lag"))
        assert np.isfinite(flat(res, "rhat")).any()
        # errors: rows beyond the buffered records, a chain index out of range
        for bad in (dict(chains=sel, first=5, count=36), dict(chains=[0, 4], first=0, count=40),
                    dict(chains=[-1], first=0, count=40)):
            with pytest.raises(sa.SrError) as e:
                analysis.diagnostics_from_session(s, **bad)
            assert e.value.code == L.SR_EINVAL
        s.run(3, save=False)
        plain.run(3, save=False)
        for c in range(len(seeds)):
            x, y = s.state(c), plain.state(c)
            for k in ("a", "b", "pi", "counts"):
                assert np.array_equal(x[k], y[k])
            assert np.array_equal(bits([x["c"], x["d"], x["loglik"]]), bits([y["c"], y["d"], y["loglik"]]))
