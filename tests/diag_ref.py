"""The convergence diagnostics' definition (include/seriation.h) in Python: test infrastructure for
tests/test_diag_host.py and tests/test_gpu_diag.py.  Deliberately not a transcription of the C: the moments are
numpy int64 slices, the centred numerators Python integers (exact) rounded once by float(), the tail Python
floats in the stated order."""
import math

import numpy as np

MARGIN = 1e-9   # every Geyer pair sum compared with zero must be farther from it than this

# The library and this file evaluate the same IEEE-754 f64 operations in the same order (the C is compiled without
# contraction; the numerators are exact integers rounded once on both sides), so they agree bit for bit: the largest
# relative difference of rhat and ess measured over the cases of tests/test_diag_host.py is 0 (DESIGN.md
# "Convergence diagnostics").  The bound is 100 x that, never looser than 1e-9.
MEASURED_REL = 0.0
TOL = min(100.0 * MEASURED_REL, 1e-9)


def ar1(rng, phi, n_sel, count, scale):
    """[n_sel][count] stationary AR(1) with unit innovations, scaled (test data)."""
    e = rng.standard_normal((n_sel, count))
    x = np.empty((n_sel, count))
    x[:, 0] = e[:, 0] / math.sqrt(1.0 - phi * phi)
    for t in range(1, count):
        x[:, t] = phi * x[:, t - 1] + e[:, t]
    return x * scale


def lags_of(count, max_lag):
    h = count // 2
    return h, (h - 1 if max_lag == 0 else max_lag)


def split(x, count):
    """[n_sel][count][...] -> [2 n_sel][h][...]: rows [0, h) and [count - h, count) of every chain."""
    x = np.asarray(x)
    h = count // 2
    return np.stack([half for ch in x for half in (ch[:h], ch[count - h:count])])


def moments(ab_pi, max_lag=0):
    """ab_pi [n_sel][count][W] integers -> P, F, B [S][L+1][W], S1 [S][W] in int64."""
    ab_pi = np.asarray(ab_pi)
    count = ab_pi.shape[1]
    h, L = lags_of(count, max_lag)
    x = split(ab_pi, count).astype(np.int64)   # [S][h][W]
    S, _, W = x.shape
    P = np.zeros((S, L + 1, W), np.int64)
    F = np.zeros((S, L + 1, W), np.int64)
    B = np.zeros((S, L + 1, W), np.int64)
    for k in range(L + 1):
        P[:, k] = (x[:, :h - k] * x[:, k:]).sum(axis=1)
        F[:, k] = x[:, :k].sum(axis=1)
        B[:, k] = x[:, h - k:].sum(axis=1)
    return P, F, B, x.sum(axis=1)


def _tail(h, L, means, variances, gammas, margins):
    """means, variances [S]; gammas [S][L+1] -> (rhat, ess, cut_lag)."""
    S = len(means)
    sv = 0.0
    for v in variances:
        sv += v
    sm = 0.0
    for m in means:
        sm += m
    Wv, mm = sv / S, sm / S
    sb = 0.0
    for m in means:
        sb += (m - mm) * (m - mm)
    Bh = sb / (S - 1)
    vp = ((h - 1) / h) * Wv + Bh
    if Wv == 0.0 or not math.isfinite(vp):
        return math.nan, math.nan, -1
    rhat = math.sqrt(vp / Wv)

    def rho(k):
        g = 0.0
        for s in range(S):
            g += gammas[s][k]
        return 1.0 - (Wv - g / S) / vp

    prev = 1.0 + (rho(1) if L >= 1 else 0.0)
    total = prev
    cut = -1
    j = 1
    while 2 * j + 1 <= L:
        g = rho(2 * j) + rho(2 * j + 1)
        margins.append(abs(g))
        if g < 0.0:
            cut = 2 * j
            break
        g = min(g, prev)
        total += g
        prev = g
        j += 1
    tau, tmin = -1.0 + 2.0 * total, 1.0 / math.log10(float(S * h))
    if not tau >= tmin:   # the larger of the two; the floor also for a NaN tau, as the library writes it
        tau = tmin
    return rhat, S * h / tau, cut


def reduce(P, F, B, S1, count, max_lag=0, cdl=None):
    """Moments (+ scalar traces cdl [n_sel][count][3]) -> rhat, ess [W + 3] float64, cut_lag [W + 3] int.
    Asserts the margin condition: no Geyer pair sum within MARGIN of zero."""
    h, L = lags_of(count, max_lag)
    S, W = np.asarray(S1).shape
    Pl, Fl, Bl, Sl = (np.asarray(a).tolist() for a in (P, F, B, S1))
    rhat, ess, cut = np.full(W + 3, np.nan), np.full(W + 3, np.nan), np.full(W + 3, -1, np.int64)
    margins = []
    h3 = float(h) * h * h
    for j in range(W):
        means, variances, gammas = [], [], []
        for s in range(S):
            s1 = Sl[s][j]
            g = []
            for k in range(L + 1):
                G = h * h * Pl[s][k][j] - h * s1 * (2 * s1 - Bl[s][k][j] - Fl[s][k][j]) + (h - k) * s1 * s1
                g.append(float(G) / h3)
            gammas.append(g)
            means.append(float(s1) / h)
            variances.append(g[0] * h / (h - 1))
        rhat[j], ess[j], cut[j] = _tail(h, L, means, variances, gammas, margins)
    if cdl is not None:
        xs = split(np.asarray(cdl, np.float64), count).tolist()   # [S][h][3]
        for v in range(3):
            means, variances, gammas = [], [], []
            for s in range(S):
                x = [row[v] for row in xs[s]]
                tot = 0.0
                for t in range(h):
                    tot += x[t]
                m = tot / h
                g = []
                for k in range(L + 1):
                    acc = 0.0
                    for t in range(h - k):
                        acc += (x[t] - m) * (x[t + k] - m)
                    g.append(acc / h)
                gammas.append(g)
                means.append(m)
                variances.append(g[0] * h / (h - 1))
            rhat[W + v], ess[W + v], cut[W + v] = _tail(h, L, means, variances, gammas, margins)
    assert all(m > MARGIN for m in margins), "a Geyer pair sum within %g of zero: choose another seed" % MARGIN
    return rhat, ess, cut


def rel_diff(a, b):
    """Largest relative difference over the finite entries; NaN positions must coincide."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok])))
