"""The definition of the posterior marginals (include/seriation.h) in numpy, without histograms on the way to the
order statistics: per column the in-range values are sorted and element k - 1 taken, the mean is the Python-int sum
divided once, and only the mode and `hist` itself come from np.bincount.  Test infrastructure: the reference of
tests/test_marg_host.py and tests/test_gpu_marginals.py."""
import math

import numpy as np


def reflect(rec, N, M, flips):
    """rec [n_sel][count][2M+N] -> int64 copy with the flagged chains' rows reflected: a <- N - b, b <- N - a,
    pi <- N - 1 - pi."""
    x = np.asarray(rec).astype(np.int64)
    if flips is None:
        return x
    for k, f in enumerate(flips):
        if f:
            a, b = x[k, :, :M].copy(), x[k, :, M:2 * M].copy()
            x[k, :, :M] = N - b
            x[k, :, M:2 * M] = N - a
            x[k, :, 2 * M:] = N - 1 - x[k, :, 2 * M:]
    return x


def rank(p, T):
    """k = clamp(ceil(p * (double)T), 1, T)"""
    return min(max(int(math.ceil(float(p) * float(T))), 1), T)


def marginals(rec, N, M, probs=(0.025, 0.5, 0.975), flips=None, hist=False):
    """-> {"quant" [Q][W] int32, "mode" [W] int32, "mean" [W] f64, "outside" [W] uint32, "pi_sum" [n_sel][N] int64
    [, "hist" [W][N+1] uint32]}"""
    raw = np.asarray(rec).astype(np.int64)
    W = 2 * M + N
    assert raw.ndim == 3 and raw.shape[2] == W
    x = reflect(raw, N, M, flips).reshape(-1, W)
    Q = len(probs)
    res = {"quant": np.zeros((Q, W), np.int32), "mode": np.zeros(W, np.int32), "mean": np.zeros(W),
           "outside": np.zeros(W, np.uint32), "pi_sum": raw[:, :, 2 * M:].sum(axis=1)}
    if hist:
        res["hist"] = np.zeros((W, N + 1), np.uint32)
    for j in range(W):
        col = x[:, j]
        ok = np.sort(col[(col >= 0) & (col <= N)])
        T = len(ok)
        res["outside"][j] = len(col) - T
        counts = np.bincount(ok, minlength=N + 1)
        if hist:
            res["hist"][j] = counts
        if T == 0:
            res["quant"][:, j], res["mode"][j], res["mean"][j] = -1, -1, np.nan
            continue
        for q, p in enumerate(probs):
            res["quant"][q, j] = ok[rank(p, T) - 1]
        res["mode"][j] = int(np.argmax(counts))   # the first of equal maxima
        res["mean"][j] = int(ok.sum()) / T   # Python ints: exact numerator, one correctly rounded division
    return res


def flat(res, key, axis=-1):
    """a result of analysis.marginals_from_* (views per kind) back to [..., 2M+N]"""
    v = res[key]
    return np.concatenate([v["a"], v["b"], v["pi"]], axis=axis)


def same_mean(got, want):
    """bit equality of the means; NaN (a column without in-range values) only has to be NaN on both sides"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64)))
