"""The definition of the chain agreement (include/seriation.h) in plain numpy -- per chain a broadcast compare of every
site pair summed over the rows, then absolute differences over the upper triangle -- and the mode clustering in pure
Python.  No tiles, no bands and no queue arithmetic shared with the library.  Test infrastructure: the reference of
tests/test_agree_host.py and tests/test_gpu_agreement.py."""
import numpy as np

# Known answers on g10s10, 300 unsaved then 200 saved mcmc_sample calls per chain (the CPU oracle's records, to which
# the GPU's are bit-equal), computed once with numpy: "hard" the dataset as it is, chains of seeds 1, 3, 4, 5, 6;
# "plain" the dataset with its '*' marks removed (no hard sites), chains of seeds 1, 5, 7, of which seed 7 settled in
# the mirror image of seed 1's order.
KNOWN = {
    "hard": {"seeds": [1, 3, 4, 5, 6], "threshold": 0.1, "scale": 1525200, "mode": [0, 1, 1, 1, 1],
             "flip": [0, 0, 0, 0, 0], "medoid1": 4,
             "dist": {(1, 4): 53560, (1, 3): 100140}, "dist_mirror": {(0, 4): 412227}},
    "plain": {"seeds": [1, 5, 7], "threshold": 0.12, "scale": 1525200, "mode": [0, 0, 0], "flip": [0, 0, 1],
              "dist": {(0, 1): 127894}, "dist_mirror": {(0, 2): 158762, (1, 2): 214578}},
}


def check_known(name, res, cm):
    """res: an agreement result over KNOWN[name]'s chains in their order, cm: its modes at KNOWN[name]'s threshold"""
    kn = KNOWN[name]
    assert res["scale"] == kn["scale"]
    for key in ("dist", "dist_mirror"):
        for (k, l), v in kn[key].items():
            assert int(res[key][k][l]) == v, (name, key, k, l, int(res[key][k][l]))
    assert list(cm["mode"]) == kn["mode"] and list(cm["flip"]) == kn["flip"]
    if "medoid1" in kn:
        assert cm["medoid"][1] == kn["medoid1"]


def pair_counts(rec, N, M):
    """rec [n_sel][count][2M+N] -> uint32 [n_sel][N][N]: entry [k][i][j] the rows of chain k with pi_i < pi_j.  The
    rows are summed in blocks only to bound the [block][N][N] temporary."""
    x = np.asarray(rec)
    assert x.ndim == 3 and x.shape[2] == 2 * M + N
    pi = x[:, :, 2 * M:].astype(np.int32)
    out = np.zeros((x.shape[0], N, N), np.int64)
    block = max(1, (1 << 23) // (N * N))
    for k in range(x.shape[0]):
        for t in range(0, x.shape[1], block):
            p = pi[k, t:t + block]
            out[k] += np.count_nonzero(p[:, :, None] < p[:, None, :], axis=0)
    return out.astype(np.uint32)


def distances(counts):
    """counts [n_sel][N][N] (any uint32) -> (dist, dist_mirror) int64 [n_sel][n_sel]."""
    O = np.asarray(counts).astype(np.int64)
    n, N = O.shape[0], O.shape[1]
    iu = np.triu_indices(N, 1)
    up = O[:, iu[0], iu[1]]    # O_k[i][j], i < j
    lo = O[:, iu[1], iu[0]]    # O_k[j][i]
    dist, mir = np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
    for k in range(n):
        for l in range(n):
            dist[k, l] = np.abs(up[k] - up[l]).sum()
            mir[k, l] = np.abs(up[k] - lo[l]).sum()
    return dist, mir


def agreement(rec, N, M):
    """-> {"pair_counts", "dist", "dist_mirror", "scale"}"""
    pc = pair_counts(rec, N, M)
    dist, mir = distances(pc)
    return {"pair_counts": pc, "dist": dist, "dist_mirror": mir, "scale": int(np.asarray(rec).shape[1]) * (N * (N - 1) // 2)}


def modes(dist, dist_mirror, scale, threshold):
    """The clustering of include/seriation.h with Python ints and lists -> {"mode", "flip", "medoid", "size",
    "n_modes"}."""
    d, m = np.asarray(dist).tolist(), np.asarray(dist_mirror).tolist()
    n = len(d)

    def e(k, l):
        k, l = min(k, l), max(k, l)
        return min(d[k][l], m[k][l])

    lim = float(threshold) * float(scale)
    mode, flip = [None] * n, [0] * n
    medoid, size = [], []
    for root in range(n):
        if mode[root] is not None:
            continue
        g = len(size)
        mode[root] = g
        members, queue = [root], [root]
        while queue:
            k = queue.pop(0)
            for l in range(n):
                if mode[l] is None and float(e(k, l)) <= lim:
                    a, b = min(k, l), max(k, l)
                    mode[l] = g
                    flip[l] = flip[k] ^ int(m[a][b] < d[a][b])
                    members.append(l)
                    queue.append(l)
        sums = {x: sum(e(x, y) for y in members if y != x) for x in members}
        medoid.append(min(sorted(members), key=lambda x: sums[x]))   # min keeps the first of equals: the lowest index
        size.append(len(members))
    return {"mode": mode, "flip": flip, "medoid": medoid, "size": size, "n_modes": len(size)}
