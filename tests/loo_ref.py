"""The definition of PSIS-LOO and the Pareto shape per cell (include/seriation.h "PSIS-LOO") in numpy, to the bit: exp
and log through Python's math.exp / math.log (bit for bit the C library's, as the library's own are; np.exp is not),
the host tables through math.sqrt / math.log, the sums over samples by waic_ref's explicit loops over rows inside
loops over chains, the selection by a full sort of every cell's T ratios, and the fit vectorised over cells with
every sum over the tail or over the grid an explicit loop adding whole arrays, so the order of every sum is the
interface's.  Test infrastructure."""
import math

import numpy as np

import waic_ref

INF, NAN = float("inf"), float("nan")


def _log1(x):
    """the C library's log on every input: NaN for a negative or NaN argument, -inf at zero, +inf at +inf"""
    if x != x or x < 0.0:
        return NAN
    if x == 0.0:
        return -INF
    return INF if x == INF else math.log(x)


def _exp1(x):
    if x != x:
        return NAN
    try:
        return math.exp(x)
    except OverflowError:
        return INF


_LOGF, _EXPF = np.frompyfunc(_log1, 1, 1), np.frompyfunc(_exp1, 1, 1)


def LOG(a):
    return _LOGF(np.asarray(a, np.float64)).astype(np.float64)


def EXP(a):
    return _EXPF(np.asarray(a, np.float64)).astype(np.float64)


def tail_len(T):
    """n = min(T / 5, s), s the smallest integer with s * s >= 9 T"""
    s = math.isqrt(9 * T)
    if s * s < 9 * T:
        s += 1
    return min(T // 5, s)


def tables(n):
    """m, G [m], L [n]: the host tables of the fit"""
    m = 30 + math.isqrt(n)
    G = [(1.0 - math.sqrt(float(m) / (float(j) - 0.5))) / 3.0 for j in range(1, m + 1)]
    L = [math.log(1.0 - (float(j) - 0.5) / float(n)) for j in range(1, n + 1)]
    return m, G, L


def tails(T, Y, r_cut, Sr):
    """Y [n][C] ascending along axis 0, r_cut [C], Sr [C]: C cells at once -> (k [C], elpd [C])"""
    Y = np.asarray(Y, np.float64)
    r_cut, Sr = np.asarray(r_cut, np.float64).reshape(-1), np.asarray(Sr, np.float64).reshape(-1)
    C = Sr.shape[0]
    n = Y.shape[0]
    Y = Y.reshape(n, C)
    with np.errstate(all="ignore"):
        plain = LOG(np.float64(T) / Sr)
        if n < 5:
            return np.full(C, INF), plain
        nd = np.float64(n)
        m, G, L = tables(n)
        x = Y - r_cut[None, :]
        xs, xn = x[(n + 2) // 4 - 1], x[n - 1]
        ok = xs > 0.0
        theta, l = [], []
        for j in range(m):
            th_j = 1.0 / xn + np.float64(G[j]) / xs
            s = np.zeros(C)
            for i in range(n):
                s = s + LOG(1.0 - th_j * x[i])
            kj = s / nd
            lj = nd * ((LOG(-th_j / kj) - kj) - 1.0)
            ok = ok & np.isfinite(lj)
            theta.append(th_j)
            l.append(lj)
        lmax = np.full(C, -INF)
        for lj in l:
            lmax = np.where(lj > lmax, lj, lmax)
        z = np.zeros(C)
        for lj in l:
            z = z + EXP(lj - lmax)
        th = np.zeros(C)
        for th_j, lj in zip(theta, l):
            th = th + th_j * (EXP(lj - lmax) / z)
        s = np.zeros(C)
        for i in range(n):
            s = s + LOG(1.0 - th * x[i])
        k0 = s / nd
        sigma = -k0 / th
        k = (k0 * nd + 5.0) / (nd + 10.0)
        ok = ok & np.isfinite(th) & np.isfinite(k0) & np.isfinite(sigma) & np.isfinite(k)
        yn = Y[n - 1]
        St, Sw, Nn = np.zeros(C), np.zeros(C), np.zeros(C)
        for j in range(n):
            Lj = np.float64(L[j])
            sj = np.where(k == 0.0, r_cut - sigma * Lj, r_cut + (sigma * (EXP(-k * Lj) - 1.0)) / k)
            wt = np.where(sj < yn, sj, yn)
            St = St + Y[j]
            Sw = Sw + wt
            Nn = Nn + wt / Y[j]
        D = (Sr - St) + Sw
        smooth = LOG((np.float64(T - n) + Nn) / D)
        return np.where(ok, k, INF), np.where(ok, smooth, plain)


def tail(T, y, r_cut, Sr):
    """sr_loo_tail: one cell's tail y [n] ascending, its cutoff and the sum of all T ratios -> (k, elpd) floats"""
    y = np.asarray(y, np.float64).reshape(-1, 1)
    k, e = tails(T, y, [r_cut], [Sr])
    return float(k[0]), float(e[0])


def _seq(a):
    return np.cumsum(np.asarray(a, np.float64).reshape(-1))[-1]


def reduce(lppd, elpd, pareto_k):
    """sr_loo_reduce: the scalars, n_k, site_elpd and taxon_elpd from the pointwise arrays"""
    lppd, e, k = (np.asarray(a, np.float64) for a in (lppd, elpd, pareto_k))
    N, M = lppd.shape
    tot = _seq(e)
    nm = np.float64(N * M)
    dev = e.reshape(-1) - tot / nm
    Q = _seq(dev * dev)
    with np.errstate(invalid="ignore", divide="ignore"):
        se = np.sqrt(nm * (Q / np.float64(N * M - 1)))
    n_k = [int((k <= 0.5).sum()), int(((k > 0.5) & (k <= 0.7)).sum()), int(((k > 0.7) & (k <= 1.0)).sum()),
           int((~(k <= 1.0)).sum())]
    return {"elpd_loo": tot, "se": se, "p_loo": _seq(lppd - e), "lppd_sum": _seq(lppd), "looic": -2.0 * tot,
            "n_k": n_k, "site_elpd": np.cumsum(e, axis=1)[:, -1], "taxon_elpd": np.cumsum(e, axis=0)[-1, :]}


def ratios(X, ab_pi, cd, manycd=False):
    """(P, R), each [n_sel][count][N][M]: every cell's likelihood and importance ratio in every sample"""
    X = np.asarray(X)
    N, M = X.shape
    rec = np.asarray(ab_pi)
    n_sel, count = rec.shape[:2]
    p, _ = waic_ref.table(cd, M, manycd)
    r = 1.0 / p
    cols = np.arange(M) if manycd else np.zeros(M, int)
    P, R = np.empty((n_sel, count, N, M)), np.empty((n_sel, count, N, M))
    for k in range(n_sel):
        for t in range(count):
            idx = waic_ref.index(X, rec[k, t], N, M)
            P[k, t], R[k, t] = p[k, t][idx, cols[None, :]], r[k, t][idx, cols[None, :]]
    return P, R


def loo(X, ab_pi, cd, manycd=False):
    """X [N][M], ab_pi [n_sel][count][2M+N] int16, cd as waic_ref.table takes it -> the dict
    analysis.loo_from_records returns with pointwise=True (without kernel_ms)"""
    X = np.asarray(X)
    N, M = X.shape
    P, R = ratios(X, ab_pi, cd, manycd)
    n_sel, count = P.shape[:2]
    T = n_sel * count

    def total(A):
        tot = np.zeros((N, M))
        for k in range(n_sel):
            s = np.zeros((N, M))
            for t in range(count):
                s = s + A[k, t]
            tot = tot + s
        return tot

    Sp, Sr = total(P), total(R)
    lppd = LOG(Sp / np.float64(T))
    n = tail_len(T)
    S = np.sort(R.reshape(T, N * M), axis=0)   # the multiset: which of several equal samples is taken does not matter
    k, e = tails(T, S[T - n:], S[T - n - 1], Sr)
    k, e = k.reshape(N, M), e.reshape(N, M)
    res = reduce(lppd, e, k)
    res.update({"elpd": e, "pareto_k": k, "lppd": lppd, "p_loo_cell": lppd - e, "tail_len": n, "total": T})
    return res
