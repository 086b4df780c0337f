"""The definition of the central sampled state (include/seriation.h) in plain numpy: pooled pair counts by a broadcast
compare of every site pair, the order loss as two masked sums against those counts, the limit loss through the
histogram of the clamped limits and the table of absolute differences written out as a matrix product, the argmin as a
Python min over tuples.  The rows are taken in blocks only to bound the [block][N][N] temporaries.  No tiles, no
bands and no masks shared with the library.  Test infrastructure: the reference of tests/test_central_host.py and
tests/test_gpu_central.py."""
import numpy as np

# Known answers on g10s10 as it is, chains of seeds 1, 2, 3, 50 saved mcmc_sample calls each and none before them (the
# CPU oracle's records, to which the GPU's are bit-equal), no flips: the central (chain, row) and its two losses,
# computed once with this module.
KNOWN = {"seeds": [1, 2, 3], "calls": 50, "central": (1, 27), "order_loss": 395027, "limit_loss": 1175715,
         "scale": 1143900, "best": [27, 27, 9]}


def oriented(rec, N, M, flips=None):
    """rec [n_sel][count][2M+N] -> (a, b, pi) int64 [T][M], [T][M], [T][N], a flagged chain's rows reflected"""
    x = np.asarray(rec).astype(np.int64)
    assert x.ndim == 3 and x.shape[2] == 2 * M + N
    a, b, pi = x[:, :, :M].copy(), x[:, :, M:2 * M].copy(), x[:, :, 2 * M:].copy()
    if flips is not None:
        for k in np.nonzero(np.asarray(flips))[0]:
            a[k], b[k], pi[k] = N - x[k, :, M:2 * M], N - x[k, :, :M], N - 1 - x[k, :, 2 * M:]
    return a.reshape(-1, M), b.reshape(-1, M), pi.reshape(-1, N)


def _blocks(T, N):
    step = max(1, (1 << 23) // (N * N))
    return [(t, min(t + step, T)) for t in range(0, T, step)]


def pair_counts(pi):
    """pi [T][N] -> uint32 [N][N]: entry [i][j] the rows with pi_i < pi_j"""
    T, N = pi.shape
    out = np.zeros((N, N), np.int64)
    for t0, t1 in _blocks(T, N):
        p = pi[t0:t1]
        out += np.count_nonzero(p[:, :, None] < p[:, None, :], axis=0)
    return out.astype(np.uint32)


def order_loss(pi, counts):
    """pi [T][N], counts [N][N] (any uint32) -> int64 [T]: sum over i < j of [pi_i < pi_j] counts[j][i] +
    [pi_i > pi_j] counts[i][j]"""
    T, N = pi.shape
    C = np.asarray(counts).astype(np.int64)
    upper = np.triu(np.ones((N, N), bool), 1)
    against_lt = np.where(upper, C.T, 0)   # at [i][j], i < j: counts[j][i]
    against_gt = np.where(upper, C, 0)     # at [i][j], i < j: counts[i][j]
    out = np.zeros(T, np.int64)
    for t0, t1 in _blocks(T, N):
        p = pi[t0:t1]
        lt, gt = p[:, :, None] < p[:, None, :], p[:, :, None] > p[:, None, :]
        out[t0:t1] = (lt * against_lt[None]).sum(axis=(1, 2)) + (gt * against_gt[None]).sum(axis=(1, 2))
    return out


def limit_loss(a, b, N):
    """a, b [T][M] (reflected) -> int64 [T]: sum over taxa and all rows s of |A_r - A_s| + |B_r - B_s|, A and B the
    limits clamped to [0, N]"""
    A = np.clip(np.concatenate([a, b], axis=1), 0, N)
    v = np.arange(N + 1, dtype=np.int64)
    absdiff = np.abs(v[:, None] - v[None, :])
    out = np.zeros(A.shape[0], np.int64)
    for c in range(A.shape[1]):
        table = absdiff @ np.bincount(A[:, c], minlength=N + 1).astype(np.int64)
        out += table[A[:, c]]
    return out


def central(rec, N, M, flips=None):
    """-> {"pair_counts", "order_loss", "limit_loss" [n_sel][count], "best" [n_sel], "central": (chain, row),
    "state": {"a", "b", "pi"} int32, "scale"}"""
    n_sel, count = np.asarray(rec).shape[:2]
    a, b, pi = oriented(rec, N, M, flips)
    C = pair_counts(pi)
    ol = order_loss(pi, C).reshape(n_sel, count)
    ll = limit_loss(a, b, N).reshape(n_sel, count)
    o, l = ol.tolist(), ll.tolist()
    best = [min(range(count), key=lambda t: (o[k][t], l[k][t], t)) for k in range(n_sel)]
    ck = min(range(n_sel), key=lambda k: (o[k][best[k]], l[k][best[k]], k))
    r = ck * count + best[ck]
    return {"pair_counts": C, "order_loss": ol, "limit_loss": ll, "best": np.array(best, np.int32),
            "central": (ck, best[ck]),
            "state": {"a": a[r].astype(np.int32), "b": b[r].astype(np.int32), "pi": pi[r].astype(np.int32)},
            "scale": n_sel * count * (N * (N - 1) // 2)}
