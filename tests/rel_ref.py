"""The definition of the taxon-pair relations, durations and richness (include/seriation.h) in plain numpy: the
flagged chains' limits reflected, then broadcast compares summed over the samples.  No histograms and no tiling of
its own (durations and richness are compares against every value as well), so it shares no structure with the
kernels.  Test infrastructure: the reference of tests/test_rel_host.py and tests/test_gpu_relations.py."""
import numpy as np

KINDS = ("orig_before", "ext_before", "precedes", "overlap", "dur_hist", "dur_outside", "rich_hist")


def limits(rec, N, M, flips=None):
    """rec [n_sel][count][2M+N] -> a, b [T][M] int32, T = n_sel * count, the flagged chains reflected:
    a <- N - b, b <- N - a."""
    x = np.asarray(rec).astype(np.int64)
    assert x.ndim == 3 and x.shape[2] >= 2 * M
    a, b = x[:, :, :M].copy(), x[:, :, M:2 * M].copy()
    if flips is not None:
        for k, f in enumerate(flips):
            if f:
                a[k], b[k] = N - x[k, :, M:2 * M], N - x[k, :, :M]
    return a.reshape(-1, M).astype(np.int32), b.reshape(-1, M).astype(np.int32)   # within +-65535


def relations(rec, N, M, flips=None, kinds=KINDS):
    """-> {kind: uint32 array} for the requested kinds.  The samples are summed in blocks of rows only to bound the
    [block][M][M], [block][M][N+1] and [block][N][M+1] temporaries."""
    a, b = limits(rec, N, M, flips)
    T = a.shape[0]
    block = max(1, min(256, (1 << 23) // max(M * M, M * (N + 1), N * (M + 1))))
    res = {}
    # overlap: max(a_i, a_j) < min(b_i, b_j) holds exactly when each of a_i, a_j lies below each of b_i, b_j
    lt = lambda X, Y: X[:, :, None] < Y[:, None, :]
    pair = {"orig_before": lambda A, B: lt(A, A),
            "ext_before": lambda A, B: lt(B, B),
            "precedes": lambda A, B: B[:, :, None] <= A[:, None, :],
            "overlap": lambda A, B: lt(A, B) & lt(A, B).transpose(0, 2, 1) & (A < B)[:, :, None] & (A < B)[:, None, :]}
    for k, fn in pair.items():
        if k in kinds:
            acc = np.zeros((M, M), np.int64)
            for t in range(0, T, block):
                acc += np.count_nonzero(fn(a[t:t + block], b[t:t + block]), axis=0)
            res[k] = acc.astype(np.uint32)
    d = b - a
    if "dur_hist" in kinds:
        acc = np.zeros((M, N + 1), np.int64)
        for t in range(0, T, block):
            acc += (d[t:t + block, :, None] == np.arange(N + 1)[None, None, :]).sum(axis=0)
        res["dur_hist"] = acc.astype(np.uint32)
    if "dur_outside" in kinds:
        res["dur_outside"] = ((d < 0) | (d > N)).sum(axis=0).astype(np.uint32)
    if "rich_hist" in kinds:
        acc = np.zeros((N, M + 1), np.int64)
        pos = np.arange(N)[None, :, None]
        for t in range(0, T, block):
            A, B = a[t:t + block, None, :], b[t:t + block, None, :]
            r = ((A <= pos) & (pos < B)).sum(axis=2)   # [block][N]: taxa alive at each position
            acc += (r[:, :, None] == np.arange(M + 1)[None, None, :]).sum(axis=0)
        res["rich_hist"] = acc.astype(np.uint32)
    return res


def diversity(rec, N, M, probs, flips=None):
    """The diversity curve without a histogram: per position the sorted richness of the samples, element k - 1 with
    k = clamp(ceil(p T), 1, T), and the Python-int sum divided once."""
    import math
    a, b = limits(rec, N, M, flips)
    pos = np.arange(N)[None, :, None]
    r = np.sort(((a[:, None, :] <= pos) & (pos < b[:, None, :])).sum(axis=2), axis=0)   # [T][N]
    T = r.shape[0]
    quant = np.array([[r[min(max(int(math.ceil(float(p) * float(T))), 1), T) - 1, j] for j in range(N)] for p in probs],
                     np.int32).reshape(len(probs), N)
    mean = np.array([int(r[:, j].sum()) / T for j in range(N)])
    return {"mean": mean, "quant": quant}
