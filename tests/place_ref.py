"""The definition of the placement of query rows (include/seriation.h "Placement") in numpy, to the bit: the term
table and every exp and log through Python's math.exp / math.log (bit for bit the C library's, as the library's own
are; np.exp is not), explicit loops over the chains and the rows, np.cumsum for every sequential sum, and Z by the
64 strided columns: e padded with zeros to a multiple of 64, reshaped to (-1, 64), a cumsum down the columns and a
cumsum over the 64 column sums.  Test infrastructure."""
import math

import numpy as np

_EXP = np.frompyfunc(math.exp, 1, 1)
_LOG = np.frompyfunc(math.log, 1, 1)


def table(cd, M, manycd):
    """cd [n_sel][count][3] or, manycd, [n_sel][count][2M] -> l [n_sel][count][4][Mt], Mt = M or 1"""
    cd = np.asarray(cd, np.float64)
    Mt = M if manycd else 1
    c, d = cd[:, :, :Mt], cd[:, :, Mt:2 * Mt]
    ec, ed = _EXP(c).astype(np.float64), _EXP(d).astype(np.float64)
    return np.stack([_LOG(1.0 - ec).astype(np.float64), d, _LOG(1.0 - ed).astype(np.float64), c], axis=2)


def reflect(row, N, M):
    """one record row as int64, reflected: a' = N - b, b' = N - a, pi' = N - 1 - pi"""
    r = np.asarray(row).astype(np.int64)
    return np.concatenate([N - r[M:2 * M], N - r[:M], N - 1 - r[2 * M:2 * M + N]])


def profile(row, l, Y, N, M):
    """one (already reflected) row, its l [4][Mt] and Y [Q][M] -> L [Q][N]: the terms summed over m ascending"""
    r = np.asarray(row).astype(np.int64)
    a, b = r[:M], r[M:2 * M]
    p = np.arange(N, dtype=np.int64)
    alive = (a[None, :] <= p[:, None]) & (p[:, None] < b[None, :])          # [N][M]
    lt = np.broadcast_to(np.asarray(l, np.float64), (4, M))
    al = alive[None, :, :]
    t0, t1 = np.where(al, lt[1], lt[0]), np.where(al, lt[2], lt[3])           # the row's terms for y = 0 and y = 1
    out = []
    for q0 in range(0, len(Y), 16):                                           # 16 queries at a time: bounded memory
        y = np.asarray(Y)[q0:q0 + 16, None, :]                                # [.][1][M]
        term = np.where(y == 0, t0, np.where(y == 1, t1, 0.0))
        out.append(np.cumsum(np.concatenate([np.zeros(term.shape[:2] + (1,)), term], axis=2), axis=2)[:, :, -1])
    return np.concatenate(out, axis=0)


def normalise(L):
    """L [Q][N] -> (e [Q][N], Z [Q], lse [Q])"""
    L = np.asarray(L, np.float64)
    Q, N = L.shape
    mx = L.max(axis=1)
    e = _EXP(L - mx[:, None]).astype(np.float64)
    pad = np.zeros((Q, (-N) % 64))
    cols = np.cumsum(np.concatenate([e, pad], axis=1).reshape(Q, -1, 64), axis=1)[:, -1, :]   # z_0 .. z_63
    Z = np.cumsum(cols, axis=1)[:, -1]
    return e, Z, mx + _LOG(Z).astype(np.float64)


def underflow_case():
    """(N, rec [1][2][2M+N], cd [1][2][3], Y [2][M]) whose profiles fall, across the positions, into every range of
    exp: three taxa, all present in query 0, alive at positions 0..0, 0..1 and 0..2, c = -365 and d = -1.  With
    l2 = log(1 - exp(-1)) the profile is 3 l2, 2 l2 - 365, l2 - 730, -1095, so L - mx is 0, about -364.5 (a normal
    e), about -729.1 (inside (-745, -708): a subnormal e) and about -1093.6 (below -746: e == 0.0).  Query 1 is all
    absent; the second row has other limits."""
    N, M = 4, 3
    rec = np.zeros((1, 2, 2 * M + N), np.int16)
    rec[0, 0] = [0, 0, 0, 1, 2, 3, 3, 1, 0, 2]
    rec[0, 1] = [1, 0, 2, 4, 1, 3, 0, 2, 3, 1]
    cd = np.array([[[-365.0, -1.0, np.nan], [-365.0, -1.0, np.nan]]])
    Y = np.array([[1, 1, 1], [0, 0, 0]], np.uint8)
    return N, rec, cd, Y


def placement(N, ab_pi, cd, Y, manycd=False, flips=None):
    """ab_pi [n_sel][count][2M+N] int16, cd as table() takes it, Y [Q][M] -> the dict analysis.placement_from_records
    returns with lse=True (without kernel_ms)"""
    rec = np.asarray(ab_pi)
    n_sel, count = rec.shape[:2]
    Y = np.asarray(Y, np.uint8)
    Q, M = Y.shape
    T = np.float64(n_sel * count)
    l = table(cd, M, manycd)
    lse = np.zeros((n_sel, count, Q))
    tot_pos = tot_site = None
    for k in range(n_sel):
        s_pos = s_site = None
        for r in range(count):
            row = rec[k, r].astype(np.int64)
            if flips is not None and flips[k]:
                row = reflect(row, N, M)
            e, Z, lse[k, r] = normalise(profile(row, l[k, r], Y, N, M))
            w = e / Z[:, None]
            pi = row[2 * M:2 * M + N]
            ok = (pi >= 0) & (pi < N)
            ws = np.where(ok[None, :], w[:, np.where(ok, pi, 0)], 0.0)
            s_pos = np.zeros((Q, N)) + w if s_pos is None else s_pos + w
            s_site = np.zeros((Q, N)) + ws if s_site is None else s_site + ws
        tot_pos = np.zeros((Q, N)) + s_pos if tot_pos is None else tot_pos + s_pos
        tot_site = np.zeros((Q, N)) + s_site if tot_site is None else tot_site + s_site
    flat = lse.reshape(n_sel * count, Q)
    mxx = flat.max(axis=0)
    s = np.cumsum(_EXP(flat - mxx[None, :]).astype(np.float64), axis=0)[-1]
    lpd = mxx + _LOG(s / T).astype(np.float64) - math.log(float(N))
    return {"pos": tot_pos / T, "site": tot_site / T, "lse": lse, "lpd": lpd, "total": n_sel * count}
