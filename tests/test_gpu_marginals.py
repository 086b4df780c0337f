"""GPU posterior marginals (csrc/sr_marg.hip): every output equal to the numpy definition in tests/marg_ref.py
(integers with np.array_equal, the mean on its bits), the session form (records in HBM) equal to the host-record
form and leaving the session untouched, the orientation of a mirrored chain end to end, the argument errors of
the session form and the command line's marginals.csv."""
import os
import subprocess
import sys

import numpy as np
import pytest

import marg_ref
import seriation_amd as sa
from seriation_amd import _lib as L
from seriation_amd import analysis, launcher
from diag_ref import ar1

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DS = os.path.join(ROOT, "tests", "golden", "datasets")
PKG = os.path.join(ROOT, "seriation-in-paleontological-data-using-mcmc_amd")


def dataset(N, M):
    return sa.Dataset(np.zeros((N, M), np.uint8), np.zeros(N, bool))


def records(kind, N, M, n_sel, count):
    """[n_sel][count][2M+N] int16.  real: autocorrelated limits in [0, N] and slowly moving permutations (as in
    tests/test_gpu_diag.py); full: any int16 with, from column to column, none, a third, two thirds or all of the
    entries drawn from [0, N] instead, so the in-range totals differ per column and some are 0."""
    rng = np.random.RandomState(1000 * N + 10 * M + count)
    W = 2 * M + N
    if kind == "full":
        x = rng.randint(-32768, 32768, (n_sel, count, W))
        x[(x >= 0) & (x <= N)] = -1   # in-range values only where they are put
        inr = rng.randint(0, N + 1, (n_sel, count, W))
        take = rng.randint(0, 3, (n_sel, count, W)) < (np.arange(W) % 4)[None, None, :]
        x[take] = inr[take]
        if count > 1:
            x[0, 0, 1], x[0, 1, W - 1] = -32768, 32767
        return x.astype(np.int16)
    out = np.empty((n_sel, count, W), np.int64)
    for m in range(2 * M):
        out[:, :, m] = np.clip(np.rint(ar1(rng, 0.8, n_sel, count, N / 8.0) + N / 2.0), 0, N)
    score = np.stack([ar1(rng, 0.9, n_sel, count, 6.0) + i for i in range(N)], axis=2)
    out[:, :, 2 * M:] = np.argsort(np.argsort(score, axis=2), axis=2)   # pi[site] = position
    return out.astype(np.int16)


_REC = {}


def rec_of(kind, N, M, n_sel, count):
    key = (kind, N, M, n_sel, count)
    if key not in _REC:
        _REC[key] = records(kind, N, M, n_sel, count)
        _REC[key].setflags(write=False)
    return _REC[key]


def check(res, want, N, M, hist):
    assert np.array_equal(marg_ref.flat(res, "outside"), want["outside"])
    assert np.array_equal(res["pi_sum"], want["pi_sum"]) and res["pi_sum"].dtype == np.int64
    if hist:
        assert res["hist"].shape == (2 * M + N, N + 1) and res["hist"].dtype == np.uint32
        assert np.array_equal(res["hist"], want["hist"])
    else:
        assert "hist" not in res
    assert np.array_equal(marg_ref.flat(res, "mode"), want["mode"])
    assert np.array_equal(marg_ref.flat(res, "quant"), want["quant"])
    assert marg_ref.same_mean(marg_ref.flat(res, "mean"), want["mean"])
    assert res["kernel_ms"] > 0


# kind, N, M, n_sel, count, flips, probs, hist
CASES = [
    pytest.param("real", 5, 3, 1, 1, None, analysis.PROBS, True, id="smallest"),
    pytest.param("full", 5, 3, 2, 17, None, analysis.PROBS, True, id="full-int16"),
    pytest.param("full", 5, 3, 2, 17, [1, 0], analysis.PROBS, True, id="full-int16-flipped"),
    pytest.param("real", 124, 139, 3, 100, None, analysis.PROBS, True, id="g10s10-shape"),
    pytest.param("real", 64, 64, 2, 65, None, analysis.PROBS, True, id="boundaries-at-64"),
    pytest.param("real", 3000, 4, 2, 50, None, analysis.PROBS, True, id="narrow-tile-47-chunks"),
    pytest.param("real", 20000, 2, 1, 8, None, analysis.PROBS, False, id="column-batches"),
    pytest.param("real", 124, 139, 3, 100, [0, 1, 0], analysis.PROBS, True, id="flipped-middle-chain"),
    pytest.param("real", 5, 3, 1, 40, None, (0.0, 1.0, 0.5), True, id="p-0-1-lower-median"),
]


@pytest.mark.parametrize("kind,N,M,n_sel,count,flips,probs,hist", CASES)
def test_marginals_equal_definition(kind, N, M, n_sel, count, flips, probs, hist):
    rec = rec_of(kind, N, M, n_sel, count)
    res = analysis.marginals_from_records(dataset(N, M), rec, probs=probs, flips=flips, hist=hist)
    want = marg_ref.marginals(rec, N, M, probs, flips, hist=hist)
    check(res, want, N, M, hist)
    if kind == "full":   # the case does hold what it is for
        T = want["hist"].sum(axis=1)
        assert (T == 0).any() and len(set(T.tolist())) > 3 and (want["outside"] > 0).any()
        assert (want["mode"][T == 0] == -1).all() and np.isnan(want["mean"][T == 0]).all()
    if probs[0] == 0.0:   # p = 0 the smallest, p = 1 the largest value of each column
        x = rec.reshape(-1, 2 * M + N)
        assert np.array_equal(marg_ref.flat(res, "quant")[0], x.min(axis=0))
        assert np.array_equal(marg_ref.flat(res, "quant")[1], x.max(axis=0))
        assert np.array_equal(marg_ref.flat(res, "quant")[2], np.sort(x, axis=0)[19])


def test_int16_extremes_reflected():
    """N - (-32768) and N - 1 - 32767 leave the int16 range: counted outside, nothing wraps."""
    N, M = 5, 3
    rec = np.full((2, 9, 2 * M + N), -32768, np.int16)
    rec[1] = 32767
    for flips in ([0, 0], [1, 1], [0, 1]):
        res = analysis.marginals_from_records(dataset(N, M), rec, flips=flips, hist=True)
        assert (marg_ref.flat(res, "outside") == 18).all() and not res["hist"].any()
        assert (marg_ref.flat(res, "mode") == -1).all() and (marg_ref.flat(res, "quant") == -1).all()
        assert np.isnan(marg_ref.flat(res, "mean")).all()
        assert np.array_equal(res["pi_sum"], np.array([[-32768 * 9] * N, [32767 * 9] * N]))


def reflected(rec, N, M, chain):
    x = rec.copy()
    x[chain, :, :M] = N - rec[chain, :, M:2 * M]
    x[chain, :, M:2 * M] = N - rec[chain, :, :M]
    x[chain, :, 2 * M:] = N - 1 - rec[chain, :, 2 * M:]
    return x


def test_orientation_end_to_end():
    N, M, n_sel, count = 124, 139, 3, 100
    rec = rec_of("real", N, M, n_sel, count)
    mirrored = reflected(rec, N, M, 1)
    ds = dataset(N, M)
    first = analysis.marginals_from_records(ds, mirrored, probs=())
    assert marg_ref.flat(first, "quant").shape == (0, 2 * M + N)
    flips = analysis.chain_orientation(first["pi_sum"])
    assert flips.tolist() == [0, 1, 0]
    got = analysis.marginals_from_records(ds, mirrored, flips=flips, hist=True)
    want = analysis.marginals_from_records(ds, rec, hist=True)
    for k in ("quant", "mode", "outside"):
        assert np.array_equal(marg_ref.flat(got, k), marg_ref.flat(want, k))
    assert marg_ref.same_mean(marg_ref.flat(got, "mean"), marg_ref.flat(want, "mean"))
    assert np.array_equal(got["hist"], want["hist"])
    # pi_sum stays raw: the mirrored chain's sums are the reflected ones
    assert np.array_equal(got["pi_sum"][[0, 2]], want["pi_sum"][[0, 2]])
    assert np.array_equal(got["pi_sum"][1], count * (N - 1) - want["pi_sum"][1])
    # unoriented, the pooled medians of the sites differ
    assert not np.array_equal(first["mode"]["pi"], want["mode"]["pi"])


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
        res = analysis.marginals_from_session(s, sel, first=4, count=36, flips=[0, 0, 1], hist=True)
        ab1, cdl1 = s.fetch_records()
        assert np.array_equal(ab0, ab1) and np.array_equal(bits(cdl0), bits(cdl1))
        want = analysis.marginals_from_records(ds, ab0[sel, 4:40], flips=[0, 0, 1], hist=True)
        for k in ("quant", "mode", "outside"):
            assert np.array_equal(marg_ref.flat(res, k), marg_ref.flat(want, k))
        assert marg_ref.same_mean(marg_ref.flat(res, "mean"), marg_ref.flat(want, "mean"))
        assert np.array_equal(res["hist"], want["hist"]) and np.array_equal(res["pi_sum"], want["pi_sum"])
        check(res, marg_ref.marginals(ab0[sel, 4:40], ds.N, ds.M, analysis.PROBS, [0, 0, 1], hist=True), ds.N, ds.M, True)
        assert (res["hist"].sum(axis=1) == 3 * 36).all() and not marg_ref.flat(res, "outside").any()
        # errors: rows beyond the buffered records, a chain index out of range, a bad probability, no rows
        for bad in (dict(chains=sel, first=5, count=36), dict(chains=[0, 4], first=0, count=40),
                    dict(chains=[-1], first=0, count=40), dict(chains=sel, first=0, count=40, probs=(0.5, 1.5)),
                    dict(chains=sel, first=0, count=0), dict(chains=sel, first=-1, count=4),
                    dict(chains=sel, first=0, count=40, probs=[0.5] * 17)):
            with pytest.raises(sa.SrError) as e:
                analysis.marginals_from_session(s, **bad)
            assert e.value.code == L.SR_EINVAL
        s.run(3, save=False)
        plain.run(3, save=False)
        for c in range(len(seeds)):
            x, y = s.state(c), plain.state(c)
            for k in ("a", "b", "pi", "counts"):
                assert np.array_equal(x[k], y[k])
            assert np.array_equal(bits([x["c"], x["d"], x["loglik"]]), bits([y["c"], y["d"], y["loglik"]]))


def test_cli_marginals(tmp_path):
    """python -m seriation_amd --select 2 --marginals: Chains/marginals.csv holds the definition's numbers for the
    chosen chains' chain_data.csv rows."""
    path = os.path.join(DS, "g2s2.txt")
    r = subprocess.run([sys.executable, "-m", "seriation_amd", path, "--chains", "4", "--burnin", "5", "--samples", "20",
                        "--seed-base", "1", "--root", str(tmp_path), "--select", "2", "--marginals"], cwd=PKG,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ds = sa.Dataset.load(path)
    chosen = launcher.choose_chains(2, str(tmp_path))
    assert ("selected: " + " ".join(str(k) for k in chosen)) in r.stdout and 1 <= len(chosen) <= 2
    rec = analysis.read_chain_rows(str(tmp_path), chosen, ds.N, ds.M)
    assert rec.shape == (len(chosen), 20, 2 * ds.M + ds.N)
    raw = marg_ref.marginals(rec, ds.N, ds.M, ())
    want = marg_ref.marginals(rec, ds.N, ds.M, analysis.PROBS, analysis.chain_orientation(raw["pi_sum"]))
    lines = (tmp_path / "Chains" / "marginals.csv").read_text().splitlines()
    assert lines[0] == "kind,index,mean,mode,q0.025,q0.5,q0.975,outside"
    assert len(lines) == 1 + 2 * ds.M + ds.N
    kinds = ["a"] * ds.M + ["b"] * ds.M + ["pi"] * ds.N
    index = list(range(ds.M)) * 2 + list(range(ds.N))
    for j, line in enumerate(lines[1:]):
        f = line.split(",")
        assert f[0] == kinds[j] and int(f[1]) == index[j]
        assert marg_ref.same_mean([float(f[2])], [want["mean"][j]])
        assert [int(v) for v in f[3:]] == [want["mode"][j]] + want["quant"][:, j].tolist() + [want["outside"][j]]
