"""The definition of WAIC and the pointwise fit (include/seriation.h "WAIC") in numpy, to the bit: the term table
through Python's math.exp / math.log (bit for bit the C library's, as the library's own exp and log are; np.exp is
not), an explicit loop over the rows inside a loop over the chains adding whole [N][M] arrays, so the order of
every sum over samples is the interface's, and np.cumsum for the sequential reductions.  Test infrastructure."""
import math

import numpy as np

_EXP = np.frompyfunc(math.exp, 1, 1)
_LOG = np.frompyfunc(math.log, 1, 1)


def table(cd, M, manycd):
    """cd [n_sel][count][3] or, manycd, [n_sel][count][2M] -> (p, l), each [n_sel][count][4][Mt], Mt = M or 1"""
    cd = np.asarray(cd, np.float64)
    Mt = M if manycd else 1
    c, d = cd[:, :, :Mt], cd[:, :, Mt:2 * Mt]
    ec, ed = _EXP(c).astype(np.float64), _EXP(d).astype(np.float64)
    p = np.stack([1.0 - ec, ed, 1.0 - ed, ec], axis=2)
    l = np.stack([_LOG(1.0 - ec).astype(np.float64), d, _LOG(1.0 - ed).astype(np.float64), c], axis=2)
    return p, l


def index(X, row, N, M):
    """one record row -> [N][M] term indices: 0 true zero, 1 false zero, 2 true one, 3 false one"""
    r = np.asarray(row).astype(np.int32)
    a, b, pi = r[:M], r[M:2 * M], r[2 * M:2 * M + N]
    alive = (a[None, :] <= pi[:, None]) & (pi[:, None] < b[None, :])
    x = np.asarray(X).reshape(N, M) != 0
    return np.where(x, np.where(alive, 2, 3), np.where(alive, 1, 0))


def _seq(a):
    return np.cumsum(np.asarray(a, np.float64).reshape(-1))[-1]


def reduce(lppd, pwaic):
    """sr_waic_reduce: the scalars, site_elpd and taxon_elpd from the pointwise arrays"""
    lppd, pwaic = np.asarray(lppd, np.float64), np.asarray(pwaic, np.float64)
    N, M = lppd.shape
    e = lppd - pwaic
    elpd = _seq(e)
    nm = np.float64(N * M)
    dev = e.reshape(-1) - elpd / nm
    Q = _seq(dev * dev)
    with np.errstate(invalid="ignore", divide="ignore"):
        se = np.sqrt(nm * (Q / np.float64(N * M - 1)))
    return {"elpd_waic": elpd, "se": se, "p_waic": _seq(pwaic), "lppd_sum": _seq(lppd), "waic": -2.0 * elpd,
            "n_high": int((pwaic > 0.4).sum()),
            "site_elpd": np.cumsum(e, axis=1)[:, -1], "taxon_elpd": np.cumsum(e, axis=0)[-1, :]}


def waic(X, ab_pi, cd, manycd=False):
    """X [N][M], ab_pi [n_sel][count][2M+N] int16, cd as table() takes it -> the dict analysis.waic_from_records
    returns with pointwise=True (without kernel_ms)"""
    X = np.asarray(X)
    N, M = X.shape
    rec = np.asarray(ab_pi)
    n_sel, count = rec.shape[:2]
    T = np.float64(n_sel * count)
    p, l = table(cd, M, manycd)
    x = X != 0

    def pick(k, r, *tabs):
        """sample (k, r)'s [4][Mt] terms of each table -> each cell's own, [N][M] (nothing is kept per sample: T
        can be large)"""
        row = rec[k, r].astype(np.int32)
        a, b, pi = row[:M], row[M:2 * M], row[2 * M:2 * M + N]
        alive = (a[None, :] <= pi[:, None]) & (pi[:, None] < b[None, :])
        return tuple(np.where(x, np.where(alive, t[k, r, 2], t[k, r, 3]), np.where(alive, t[k, r, 1], t[k, r, 0]))
                     for t in tabs)

    def total(terms):
        """terms(k, r) -> a tuple of [N][M] arrays; each summed over r within chain k from +0.0, then over k"""
        tot = None
        for k in range(n_sel):
            s = None
            for r in range(count):
                v = terms(k, r)
                s = [np.zeros((N, M)) + e for e in v] if s is None else [e0 + e for e0, e in zip(s, v)]
            tot = [np.zeros((N, M)) + e for e in s] if tot is None else [e0 + e for e0, e in zip(tot, s)]
        return tot

    Sp, Sl = total(lambda k, r: pick(k, r, p, l))
    mu = Sl / T

    def sq(k, r):
        dl = pick(k, r, l)[0] - mu
        return (dl * dl,)

    V, = total(sq)
    lppd = _LOG(Sp / T).astype(np.float64)
    pwaic = V / np.float64(n_sel * count - 1)
    res = reduce(lppd, pwaic)
    res.update({"lppd": lppd, "ll_mean": mu, "pwaic": pwaic, "elpd": lppd - pwaic, "total": n_sel * count})
    return res


def compare(a, b):
    """analysis.waic_compare by explicit loops"""
    d = (np.asarray(a["elpd"], np.float64) - np.asarray(b["elpd"], np.float64)).reshape(-1).tolist()
    tot = 0.0
    for v in d:
        tot += v
    me, q = tot / float(len(d)), 0.0
    for v in d:
        q += (v - me) * (v - me)
    n = float(len(d))
    return {"elpd_diff": tot, "se_diff": math.sqrt(n * (q / (n - 1.0))) if len(d) > 1 else float("nan")}
