"""The definition of cell occupancy and the per-site, per-taxon error tallies (include/seriation.h, "cell occupancy")
in numpy, built by broadcasting over samples; every output an exact integer."""
import numpy as np

KINDS = ("alive", "site_alive_hist", "site_f0_hist", "site_f1_hist", "taxon_alive_hist", "taxon_f0_hist",
         "taxon_f1_hist")
BATCH = 256   # samples per broadcast: bounds the [batch][N][M] boolean


def alive_of(rows, N, M):
    """rows [S][2M+N] int16 -> [S][N][M] bool: a_m <= pi_n < b_m, compared in int32"""
    r = np.asarray(rows).astype(np.int32)
    a, b, pi = r[:, None, :M], r[:, None, M:2 * M], r[:, 2 * M:, None]
    return (a <= pi) & (pi < b)


def _bin(hist, counts):
    """hist [C][O+1] += the tally of counts [S][C]"""
    np.add.at(hist, (np.broadcast_to(np.arange(hist.shape[0]), counts.shape), counts), 1)


def occupancy(X, ab_pi):
    """X [N][M] (non-zero = 1), ab_pi [n_sel][count][2M+N] int16 -> {kind: int64 array} for KINDS, plus "total"."""
    x = np.asarray(X) != 0
    N, M = x.shape
    rec = np.asarray(ab_pi)
    assert rec.ndim == 3 and rec.shape[2] == 2 * M + N
    rows = rec.reshape(-1, 2 * M + N)
    out = {"alive": np.zeros((N, M), np.int64)}
    for k in KINDS[1:4]:
        out[k] = np.zeros((N, M + 1), np.int64)
    for k in KINDS[4:]:
        out[k] = np.zeros((M, N + 1), np.int64)
    for s in range(0, len(rows), BATCH):
        al = alive_of(rows[s:s + BATCH], N, M)
        f0, f1 = al & ~x, ~al & x
        out["alive"] += al.sum(axis=0)
        for name, bits in (("alive", al), ("f0", f0), ("f1", f1)):
            _bin(out["site_%s_hist" % name], bits.sum(axis=2))
            _bin(out["taxon_%s_hist" % name], bits.sum(axis=1))
    out["total"] = len(rows)
    return out


def derived(alive, X, total):
    """the host-side f64 values of the Python layer, each one division of exact integers"""
    a = np.asarray(alive).astype(np.int64)
    x = np.asarray(X) != 0
    N, M = a.shape
    p = np.empty((N, M))
    p0, p1, comp = np.full((N, M), np.nan), np.full((N, M), np.nan), np.full(N, np.nan)
    for n in range(N):
        num = den = 0
        for m in range(M):
            p[n, m] = float(a[n, m]) / float(total)
            if x[n, m]:
                p1[n, m] = float(total - int(a[n, m])) / float(total)
                num += int(a[n, m])
            else:
                p0[n, m] = p[n, m]
            den += int(a[n, m])
        if den:
            comp[n] = float(num) / float(den)
    return {"p_alive": p, "p_false_zero": p0, "p_false_one": p1, "site_completeness": comp}
