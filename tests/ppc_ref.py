"""The definition of the posterior predictive checks (include/seriation.h "Posterior predictive checks") in numpy:
Philox4x32-10 over uint64 arrays, the thresholds through Python's math.exp (bit for bit the C library's, as the
library's own exp is; np.exp is not) and int(), which truncates, and an explicit loop over the chains, the rows and
the replicates.  Every output is an integer array.  Test infrastructure."""
import math

import numpy as np

STATS = ("ones", "span", "gaps", "f0", "f1")
KEY1 = 0x50504331
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: four uint64 arrays (or ints) of values below 2^32, key: two ints -> four uint64 arrays of 32-bit words"""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) for c in ctr)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        h0, l0, h1, l1 = p0 >> _S32, p0 & _M32, p1 >> _S32, p1 & _M32
        c0, c1, c2, c3 = h1 ^ c1 ^ np.uint64(k0), l1, h0 ^ c3 ^ np.uint64(k1), l0
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def key_of(seed):
    seed = int(seed)
    return seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ KEY1


def thresholds(c, d):
    """log-scale rates -> (thr_alive, thr_dead), Python ints in [0, 2^32]"""
    return int((1.0 - math.exp(d)) * 4294967296.0), int(math.exp(c) * 4294967296.0)


def words(N, M, t, rep, seed):
    """the random word of every cell of sample t, replicate rep: [N][M] uint64"""
    MQ = (M + 3) // 4
    n = np.arange(N, dtype=np.uint64)[:, None] + np.zeros((1, MQ), np.uint64)
    q = np.arange(MQ, dtype=np.uint64)[None, :] + np.zeros((N, 1), np.uint64)
    w = philox4x32_10((n, q, np.full((N, MQ), t, np.uint64), np.full((N, MQ), rep, np.uint64)), key_of(seed))
    return np.stack(w, axis=2).reshape(N, 4 * MQ)[:, :M]


def alive_of(row, N, M):
    r = np.asarray(row).astype(np.int32)
    a, b, pi = r[:M], r[M:2 * M], r[2 * M:2 * M + N]
    return (a[None, :] <= pi[:, None]) & (pi[:, None] < b[None, :]), pi


def stats(Y, alive, pi):
    """the five taxon discrepancies of the 0/1 matrix Y [N][M] under a sample: [5][M] int64"""
    Y = np.asarray(Y).astype(bool)
    pos = pi.astype(np.int64)[:, None] + np.zeros(Y.shape, np.int64)
    ones = Y.sum(axis=0).astype(np.int64)
    mx = np.where(Y, pos, -(1 << 40)).max(axis=0)
    mn = np.where(Y, pos, 1 << 40).min(axis=0)
    span = np.where(ones > 0, mx - mn + 1, 0)
    f0 = (alive & ~Y).sum(axis=0).astype(np.int64)
    f1 = (~alive & Y).sum(axis=0).astype(np.int64)
    return np.stack([ones, span, span - ones, f0, f1])


def replicate(row, N, M, thr_alive, thr_dead, t, rep, seed):
    """the replicate matrix [N][M] bool of sample t (its record row, its thresholds: ints or [M] arrays)"""
    alive, _ = alive_of(row, N, M)
    ta = np.broadcast_to(np.asarray(thr_alive, np.uint64), (M,))
    td = np.broadcast_to(np.asarray(thr_dead, np.uint64), (M,))
    return words(N, M, t, rep, seed) < np.where(alive, ta[None, :], td[None, :])


def ppc(X, ab_pi, cd, manycd=False, seed=0, reps=1):
    """X [N][M], ab_pi [n_sel][count][2M+N] int16, cd [n_sel][count][3] or, manycd, [n_sel][count][2M] -> the dict
    analysis.ppc_from_records returns with totals=True (without kernel_ms and the p-values)"""
    X = np.asarray(X) != 0
    N, M = X.shape
    rec = np.asarray(ab_pi)
    cd = np.asarray(cd, np.float64)
    n_sel, count = rec.shape[:2]
    rich_obs = X.sum(axis=1).astype(np.int64)
    res = {"taxon_gt": np.zeros((5, M), np.int64), "taxon_eq": np.zeros((5, M), np.int64),
           "taxon_sum_obs": np.zeros((5, M), np.int64), "taxon_sum_rep": np.zeros((5, M), np.int64),
           "site_gt": np.zeros(N, np.int64), "site_eq": np.zeros(N, np.int64), "site_sum_rep": np.zeros(N, np.int64),
           "total_obs": np.zeros((n_sel, count, 5), np.int64), "total_rep": np.zeros((n_sel, count, reps, 5), np.int64),
           "total_gt": np.zeros(5, np.int64), "total_eq": np.zeros(5, np.int64), "pairs": n_sel * count * reps}
    for k in range(n_sel):
        for r in range(count):
            t = k * count + r
            alive, pi = alive_of(rec[k, r], N, M)
            if manycd:
                th = [thresholds(cd[k, r, m], cd[k, r, M + m]) for m in range(M)]
                ta, td = np.array([v[0] for v in th], np.uint64), np.array([v[1] for v in th], np.uint64)
            else:
                ta, td = thresholds(cd[k, r, 0], cd[k, r, 1])
            obs = stats(X, alive, pi)
            res["total_obs"][k, r] = obs.sum(axis=1)
            for rep in range(reps):
                Y = replicate(rec[k, r], N, M, ta, td, t, rep, seed)
                st = stats(Y, alive, pi)
                res["taxon_gt"] += st > obs
                res["taxon_eq"] += st == obs
                res["taxon_sum_obs"] += obs
                res["taxon_sum_rep"] += st
                rich = Y.sum(axis=1).astype(np.int64)
                res["site_gt"] += rich > rich_obs
                res["site_eq"] += rich == rich_obs
                res["site_sum_rep"] += rich
                tot = st.sum(axis=1)
                res["total_rep"][k, r, rep] = tot
                res["total_gt"] += tot > res["total_obs"][k, r]
                res["total_eq"] += tot == res["total_obs"][k, r]
    return res


def pvalue(gt, eq, pairs):
    return (np.asarray(gt, np.float64) + 0.5 * np.asarray(eq, np.float64)) / np.float64(pairs)
