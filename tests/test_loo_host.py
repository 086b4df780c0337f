"""The host side of PSIS-LOO: the numpy definition (tests/loo_ref.py) against a literal one-cell-at-a-time loop,
sr_loo_tail_len and sr_loo_tail (the source the finish kernel runs, here on the host) against it to the bit on random
tails, on every unsmoothed case and at the domain's edge, the recovery of a known Pareto shape, sr_loo_reduce, every
argument error of sr_loo, which must be reported before any kernel runs, and analysis.waic_compare on LOO results.
CPU only: the pointwise terms come from the GPU in tests/test_gpu_loo.py."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import loo_ref
import seriation_amd as sa
import waic_ref
from seriation_amd import _lib as L
from seriation_amd import analysis

_DBLP = ctypes.POINTER(ctypes.c_double)
INF = float("inf")


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def fdiv(a, b):
    """IEEE division of two floats (Python raises where IEEE gives inf or NaN)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def brute_tail(T, y, r_cut, Sr):
    """The definition read literally for one cell, in Python floats."""
    n = len(y)
    plain = (INF, loo_ref._log1(fdiv(float(T), Sr)))
    if n < 5:
        return plain
    nd = float(n)
    m = 30 + math.isqrt(n)
    x = [v - r_cut for v in y]
    xs = x[(n + 2) // 4 - 1]
    if not xs > 0.0:
        return plain
    theta, l = [], []
    for j in range(1, m + 1):
        G = (1.0 - math.sqrt(float(m) / (float(j) - 0.5))) / 3.0
        th = 1.0 / x[n - 1] + G / xs
        s = 0.0
        for i in range(n):
            s += loo_ref._log1(1.0 - th * x[i])
        kj = s / nd
        lj = nd * ((loo_ref._log1(fdiv(-th, kj)) - kj) - 1.0)
        if not math.isfinite(lj):
            return plain
        theta.append(th)
        l.append(lj)
    lmax = max(l)
    z = 0.0
    for lj in l:
        z += loo_ref._exp1(lj - lmax)
    th = 0.0
    for tj, lj in zip(theta, l):
        th += tj * (loo_ref._exp1(lj - lmax) / z)
    s = 0.0
    for i in range(n):
        s += loo_ref._log1(1.0 - th * x[i])
    k0 = s / nd
    sigma = fdiv(-k0, th)
    k = (k0 * nd + 5.0) / (nd + 10.0)
    if not all(math.isfinite(v) for v in (th, k0, sigma, k)):
        return plain
    St = Sw = Nn = 0.0
    for j in range(1, n + 1):
        Lj = math.log(1.0 - (float(j) - 0.5) / nd)
        sj = r_cut - sigma * Lj if k == 0.0 else r_cut + sigma * (loo_ref._exp1(-k * Lj) - 1.0) / k
        wt = sj if sj < y[n - 1] else y[n - 1]
        St += y[j - 1]
        Sw += wt
        Nn += wt / y[j - 1]
    D = (Sr - St) + Sw
    return k, loo_ref._log1((float(T - n) + Nn) / D)


@pytest.mark.parametrize("manycd", [False, True])
def test_ref_matches_brute_force(manycd):
    N, M, n_sel, count = 4, 3, 3, 10
    T = n_sel * count
    rng = np.random.RandomState(17 + manycd)
    X = rng.randint(0, 2, (N, M))
    rec = rng.randint(-1, N + 2, (n_sel, count, 2 * M + N))
    rec[0, 0, 0], rec[1, 2, M + 1], rec[2, 3, 2 * M] = -32768, 32767, 32767
    cd = -rng.uniform(0.05, 7.0, (n_sel, count, 2 * M if manycd else 3))
    got = loo_ref.loo(X, rec.astype(np.int16), cd, manycd)
    n = loo_ref.tail_len(T)
    assert n == 6 and got["tail_len"] == 6 and got["total"] == T
    lppd, elpd, pk = np.zeros((N, M)), np.zeros((N, M)), np.zeros((N, M))
    for i in range(N):
        for m in range(M):
            sp = sr = 0.0
            vals = []
            for k in range(n_sel):
                cp = cr = 0.0
                for t in range(count):
                    row = cd[k, t].tolist()
                    c, d = (row[m], row[M + m]) if manycd else (row[0], row[1])
                    ec, ed = math.exp(c), math.exp(d)
                    r = rec[k, t].tolist()
                    alive = r[m] <= r[2 * M + i] < r[M + m]
                    p = [1.0 - ec, ed, 1.0 - ed, ec][(2 if alive else 3) if X[i, m] else (1 if alive else 0)]
                    cp += p
                    cr += 1.0 / p
                    vals.append(1.0 / p)
                sp += cp
                sr += cr
            vals.sort()
            lppd[i, m] = math.log(sp / float(T))
            pk[i, m], elpd[i, m] = brute_tail(T, vals[T - n:], vals[T - n - 1], sr)
    assert np.array_equal(bits(got["lppd"]), bits(lppd))
    assert np.array_equal(bits(got["pareto_k"]), bits(pk))
    assert np.array_equal(bits(got["elpd"]), bits(elpd))
    assert np.array_equal(bits(got["p_loo_cell"]), bits(lppd - elpd))
    assert np.isfinite(pk).any()   # some tails are smoothed
    assert np.array_equal(bits(got["lppd"]), bits(waic_ref.waic(X, rec.astype(np.int16), cd, manycd)["lppd"]))


def test_tail_len():
    lib = sa.lib()
    for T in list(range(1, 2001)) + [2 ** 31 - 1]:
        n = lib.sr_loo_tail_len(T)
        assert n == loo_ref.tail_len(T), T
        s = next(s for s in range(max(0, math.isqrt(9 * T) - 1), math.isqrt(9 * T) + 3) if s * s >= 9 * T)
        assert n == min(T // 5, s)
    # T / 5 and 3 sqrt T cross at 225
    assert [lib.sr_loo_tail_len(T) for T in (24, 25, 225, 226)] == [4, 5, 45, 45]
    assert [loo_ref.tail_len(T) for T in (224, 230, 231)] == [44, 46, 46]
    # 139022^2 < 9 (2^31 - 1) = 19327352823 <= 139023^2
    assert lib.sr_loo_tail_len(2 ** 31 - 1) == 139023 and lib.sr_loo_tail_len(0) == 0 and lib.sr_loo_tail_len(2 ** 31) == 0
    assert lib.sr_loo_tail_len(1864135) == 4096 and lib.sr_loo_tail_len(1864136) == 4097


def c_tail(T, y, r_cut, Sr, rc=L.SR_OK):
    y = np.ascontiguousarray(y, np.float64)
    k, e = ctypes.c_double(7.0), ctypes.c_double(7.0)
    got = sa.lib().sr_loo_tail(T, len(y), y.ctypes.data_as(_DBLP), r_cut, Sr, ctypes.byref(k), ctypes.byref(e))
    assert got == rc
    return k.value, e.value


def seqsum(v):
    s = 0.0
    for a in v:
        s += a
    return s


def same(a, b):
    return bits(a[0]) == bits(b[0]) and bits(a[1]) == bits(b[1])


TAILS = {5: 25, 6: 30, 8: 40, 45: 225, 95: 1000, 269: 8000}


@pytest.mark.parametrize("n", sorted(TAILS))
def test_tail_equals_definition(n):
    T = TAILS[n]
    assert loo_ref.tail_len(T) == n
    rng = np.random.RandomState(n)
    smoothed = 0
    for trial in range(12):
        if trial % 3 == 0:     # heavy tails of every shape
            r = (1.0 - rng.uniform(0, 1, T)) ** -rng.uniform(0.1, 2.0) + rng.uniform(0, 3)
        elif trial % 3 == 1:   # the model's: a cell is alive or not, the rates vary a little from sample to sample
            p = np.where(rng.uniform(0, 1, T) < rng.uniform(0.02, 0.5), rng.uniform(0.001, 0.1, T), rng.uniform(0.5, 0.999, T))
            r = 1.0 / p
        else:                  # light tails
            r = 1.0 + rng.uniform(0, 1, T) ** 2 * 10.0 ** rng.randint(-3, 4)
        Sr = seqsum(r.tolist())
        s = np.sort(r)
        y, cut = s[T - n:], float(s[T - n - 1])
        got, want = c_tail(T, y, cut, Sr), loo_ref.tail(T, y, cut, Sr)
        assert same(got, want), (trial, got, want)
        assert same(want, brute_tail(T, y.tolist(), cut, Sr))
        smoothed += math.isfinite(got[0])
        if math.isfinite(got[0]):
            assert math.isfinite(got[1])
    assert smoothed >= 8


def test_unsmoothed_cases():
    T, n = 40, 8
    q = (n + 2) // 4
    assert q == 2
    plain = lambda Sr: (INF, math.log(float(T) / Sr))
    # all values equal
    y = [3.5] * n
    assert same(c_tail(T, y, 3.5, 140.0), plain(140.0)) and same(loo_ref.tail(T, y, 3.5, 140.0), plain(140.0))
    # ties up to index q: xs = 0; up to q - 1: xs just positive, the tail is fitted
    rest = [4.0, 4.5, 6.0, 9.0, 11.0, 30.0]
    tie_q = [3.5, 3.5] + rest
    tie_q1 = [3.5, np.nextafter(3.5, 4.0)] + rest
    for y, smooth in ((tie_q, False), (tie_q1, True)):
        Sr = seqsum([1.5] * (T - n) + y)
        got, want = c_tail(T, y, 3.5, Sr), loo_ref.tail(T, y, 3.5, Sr)
        assert same(got, want) and same(want, brute_tail(T, y, 3.5, Sr))
        assert math.isfinite(got[0]) == smooth
        if not smooth:
            assert same(got, plain(Sr))
    # n < 5: never fitted, whatever the values
    y = [2.0, 3.0, 50.0, 1e6]
    Sr = seqsum([1.25] * 16 + y)
    assert same(c_tail(20, y, 1.25, Sr), (INF, math.log(20.0 / Sr))) and same(loo_ref.tail(20, y, 1.25, Sr), (INF, math.log(20.0 / Sr)))
    assert same(c_tail(3, [], 1.0, 4.0), (INF, math.log(3.0 / 4.0)))


def test_theta_cancelling_to_zero():
    """theta_j = 1.0 / x_n + G_j / xs is exactly 0.0 for one j: k_j = 0, l_j = NaN, the tail is not smoothed.  With
    xs = 1.0 that takes an x_n whose reciprocal rounds to -G_j; x = y - r_cut is exact here."""
    T, n, cut = 40, 8, 1.0
    m, G, _ = loo_ref.tables(n)
    found = None
    for j in range(m):
        if not 0.05 < -G[j] < 0.9:
            continue
        xn = 1.0 / -G[j]
        for _ in range(8):
            yn = cut + xn
            if yn - cut == xn and 1.0 / xn + G[j] / 1.0 == 0.0:
                found = (j, yn)
                break
            xn = float(np.nextafter(xn, INF))
        if found:
            break
    assert found, "no representable x_n cancels any theta_j"
    j, yn = found
    assert yn > 2.625
    y = [1.5, 2.0, 2.125, 2.25, 2.375, 2.5, 2.625, yn]   # ascending, y_q = 2.0: xs = 1.0
    assert y[(n + 2) // 4 - 1] - cut == 1.0 and 1.0 / (yn - cut) + G[j] / 1.0 == 0.0
    Sr = seqsum([1.0] * (T - n) + y)
    got = c_tail(T, y, cut, Sr)
    assert same(got, (INF, math.log(float(T) / Sr))) and same(loo_ref.tail(T, y, cut, Sr), got)
    assert same(brute_tail(T, y, cut, Sr), got)
    # one ulp away nothing cancels and the tail is fitted
    y2 = y[:-1] + [float(np.nextafter(yn, 0.0))]
    got2 = c_tail(T, y2, cut, Sr)
    assert math.isfinite(got2[0]) and same(got2, loo_ref.tail(T, y2, cut, Sr))


def test_ratios_at_the_domain_edge():
    """y_n = e^600, the largest ratio the rate domain admits; the sums stay finite"""
    top = math.exp(600.0)
    assert 1.0 / math.exp(-600.0) <= top * (1 + 1e-15)
    for T, n in ((30, 6), (225, 45)):
        rng = np.random.RandomState(T)
        for low in (1.0, 1e100, top / 8):
            y = np.sort(np.concatenate([low * (1.0 + rng.uniform(0, 1, n - 2)), [top, top]]))
            Sr = seqsum([1.0] * (T - n) + y.tolist())
            got, want = c_tail(T, y, 1.0, Sr), loo_ref.tail(T, y, 1.0, Sr)
            assert same(got, want) and math.isfinite(got[1]), (got, want)
            assert same(want, brute_tail(T, y.tolist(), 1.0, Sr))
        y = np.full(n, top)   # T e^600 is finite: log(T / Sr) is
        Sr = seqsum([top] * T)
        assert math.isfinite(Sr) and same(c_tail(T, y, top, Sr), (INF, math.log(float(T) / Sr)))


@pytest.mark.parametrize("k", [0.3, 1.2])
def test_recovers_a_known_shape(k):
    """20000 draws (1 - u)^(-k) are Pareto with shape k: the fit finds it within 0.3 -- the definition alone first,
    then the library."""
    T = 20000
    u = np.random.RandomState(2017).uniform(0, 1, T)
    r = (1.0 - u) ** -k
    n = loo_ref.tail_len(T)
    assert n == 425
    s = np.sort(r)
    y, cut, Sr = s[T - n:], float(s[T - n - 1]), seqsum(r.tolist())
    want = loo_ref.tail(T, y, cut, Sr)
    assert abs(want[0] - k) < 0.3, want
    got = c_tail(T, y, cut, Sr)
    assert same(got, want) and abs(got[0] - k) < 0.3


def test_tail_argument_errors():
    y = [2.0, 3.0, 4.0, 5.0, 6.0]
    yp = np.array(y).ctypes.data_as(_DBLP)
    k, e = ctypes.c_double(7.0), ctypes.c_double(7.0)
    lib = sa.lib()
    kp, ep = ctypes.byref(k), ctypes.byref(e)
    assert lib.sr_loo_tail(25, 5, yp, 1.0, 40.0, None, ep) == L.SR_EINVAL
    assert lib.sr_loo_tail(25, 5, yp, 1.0, 40.0, kp, None) == L.SR_EINVAL
    assert lib.sr_loo_tail(25, 5, None, 1.0, 40.0, kp, ep) == L.SR_EINVAL
    assert lib.sr_loo_tail(0, 0, yp, 1.0, 40.0, kp, ep) == L.SR_EINVAL
    assert lib.sr_loo_tail(2 ** 31, 5, yp, 1.0, 40.0, kp, ep) == L.SR_EINVAL
    assert lib.sr_loo_tail(25, -1, yp, 1.0, 40.0, kp, ep) == L.SR_EINVAL
    assert lib.sr_loo_tail(5, 5, yp, 1.0, 40.0, kp, ep) == L.SR_EINVAL       # no cutoff left
    assert lib.sr_loo_tail(10 ** 6, 4097, yp, 1.0, 40.0, kp, ep) == L.SR_EUNSUPPORTED
    assert k.value == 7.0 and e.value == 7.0
    assert lib.sr_loo_tail(25, 5, yp, 1.0, 40.0, kp, ep) == L.SR_OK and k.value != 7.0


def c_reduce(lppd, elpd, pk, site=True, taxon=True):
    lppd, elpd, pk = (np.ascontiguousarray(a, np.float64) for a in (lppd, elpd, pk))
    N, M = lppd.shape
    out = L.sr_loo_out()
    se, te = np.full(N, 7.0), np.full(M, 7.0)
    if site:
        out.site_elpd = se.ctypes.data_as(_DBLP)
    if taxon:
        out.taxon_elpd = te.ctypes.data_as(_DBLP)
    out.tail_len = 77
    rc = sa.lib().sr_loo_reduce(N, M, lppd.ctypes.data_as(_DBLP), elpd.ctypes.data_as(_DBLP), pk.ctypes.data_as(_DBLP),
                                ctypes.byref(out))
    assert rc == L.SR_OK and out.tail_len == 77
    return out, se, te


def test_reduce_against_sequential_definition():
    rng = np.random.RandomState(5)
    for N, M in ((1, 1), (1, 5), (6, 1), (7, 9), (40, 33)):
        lppd = -rng.uniform(1e-3, 9.0, (N, M)) * 10.0 ** rng.randint(-3, 3, (N, M))
        elpd = lppd - rng.uniform(0.0, 0.8, (N, M))
        pk = rng.uniform(-0.2, 1.6, (N, M))
        edge = [0.5, np.nextafter(0.5, 1), 0.7, np.nextafter(0.7, 1), 1.0, np.nextafter(1.0, 2), INF, -0.3]
        pk.reshape(-1)[:len(edge)] = edge[:N * M]
        out, se, te = c_reduce(lppd, elpd, pk)
        sl = sp = tot = 0.0
        nk = [0, 0, 0, 0]
        for a, e, k in zip(lppd.reshape(-1).tolist(), elpd.reshape(-1).tolist(), pk.reshape(-1).tolist()):
            sl += a
            sp += a - e
            tot += e
            nk[0 if k <= 0.5 else 1 if k <= 0.7 else 2 if k <= 1.0 else 3] += 1
        me, q = tot / float(N * M), 0.0
        for e in elpd.reshape(-1).tolist():
            q += (e - me) * (e - me)
        assert bits(out.lppd_sum) == bits(sl) and bits(out.p_loo) == bits(sp) and bits(out.elpd) == bits(tot)
        assert bits(out.looic) == bits(-2.0 * tot) and list(out.n_k) == nk and sum(nk) == N * M
        if N * M == 1:
            assert math.isnan(out.se)
        else:
            assert bits(out.se) == bits(math.sqrt(float(N * M) * (q / float(N * M - 1))))
        want = loo_ref.reduce(lppd, elpd, pk)
        for key, v in (("elpd_loo", out.elpd), ("se", out.se), ("p_loo", out.p_loo), ("lppd_sum", out.lppd_sum),
                       ("looic", out.looic)):
            assert bits(want[key]) == bits(v), key
        assert want["n_k"] == nk
        assert np.array_equal(bits(se), bits(want["site_elpd"])) and np.array_equal(bits(te), bits(want["taxon_elpd"]))
        out2, se2, te2 = c_reduce(lppd, elpd, pk, site=False, taxon=False)
        assert (se2 == 7.0).all() and (te2 == 7.0).all() and bits(out2.elpd) == bits(tot)
        if N * M >= 8:   # the edges fall on the lower side: <= 0.5, <= 0.7, <= 1; +inf above
            only = np.full((N, M), 0.6)
            only.reshape(-1)[:8] = edge
            assert list(c_reduce(lppd, elpd, only)[0].n_k) == [2, N * M - 8 + 2, 2, 2]
    lib = sa.lib()
    one = np.zeros(1)
    o = L.sr_loo_out()
    p = one.ctypes.data_as(_DBLP)
    assert lib.sr_loo_reduce(1, 1, None, p, p, ctypes.byref(o)) == L.SR_EINVAL
    assert lib.sr_loo_reduce(1, 1, p, None, p, ctypes.byref(o)) == L.SR_EINVAL
    assert lib.sr_loo_reduce(1, 1, p, p, None, ctypes.byref(o)) == L.SR_EINVAL
    assert lib.sr_loo_reduce(1, 1, p, p, p, None) == L.SR_EINVAL
    assert lib.sr_loo_reduce(0, 1, p, p, p, ctypes.byref(o)) == L.SR_EINVAL
    assert lib.sr_loo_reduce(1, 0, p, p, p, ctypes.byref(o)) == L.SR_EINVAL


def call(n_sel, count, N=3, M=2, manycd=0, cd=None, ds=True, rec=True, cdp=True, out=True, X=True):
    """sr_loo through ctypes on a dataset of any claimed shape (the checks before the rates read N and M only); every
    output points at a small buffer, which no refused call touches.  cd: the values of the first row."""
    buf = np.full(16, 5.0)
    r = np.zeros((1, 8, 7), np.int16)
    r[:, :, 2:4] = 3
    x = np.zeros(6, np.uint8)
    rates = np.full((8, 4 if manycd else 3), -1.0)
    if cd is not None:
        rates[0, :len(cd)] = cd
    d = L.sr_dataset()
    d.N, d.M = N, M
    if X:
        d.X = x.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    o = L.sr_loo_out()
    for k in ("elpd_loo", "pareto_k", "lppd", "p_loo_i", "site_elpd", "taxon_elpd"):
        setattr(o, k, buf.ctypes.data_as(_DBLP))
    o.elpd = o.kernel_ms = 5.0
    o.tail_len = 55
    rc = sa.lib().sr_loo(ctypes.byref(d) if ds else None, r.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)) if rec else None,
                         rates.ctypes.data_as(_DBLP) if cdp else None, manycd, n_sel, count, 0,
                         ctypes.byref(o) if out else None)
    if rc != L.SR_OK:
        assert (buf == 5.0).all() and o.elpd == 5.0 and o.kernel_ms == 5.0 and o.tail_len == 55
    return rc


def accepted():
    """what a call whose arguments are in order returns: the device's answer"""
    return L.SR_OK if sa.lib().sr_device_count() > 0 else L.SR_EDEVICE


def test_argument_checks():
    """Every SR_EINVAL case of the definition; none of them reaches the device (this test runs without one)."""
    assert call(1, 8, ds=False) == L.SR_EINVAL
    assert call(1, 8, rec=False) == L.SR_EINVAL
    assert call(1, 8, cdp=False) == L.SR_EINVAL
    assert call(1, 8, out=False) == L.SR_EINVAL
    assert call(1, 8, X=False) == L.SR_EINVAL
    assert call(0, 8) == L.SR_EINVAL                 # n_sel <= 0
    assert call(-1, 8) == L.SR_EINVAL
    assert call(1, 0) == L.SR_EINVAL                 # count < 1
    assert call(1, -3) == L.SR_EINVAL
    assert call(1, 1) == L.SR_EINVAL                 # T < 2
    assert call(65536, 32768) == L.SR_EINVAL         # T = 2^31
    assert call(2, 2 ** 30) == L.SR_EINVAL
    assert call(1, 8, N=0) == L.SR_EINVAL            # N outside 1..32767
    assert call(1, 8, N=-4) == L.SR_EINVAL
    assert call(1, 8, N=32768) == L.SR_EINVAL
    assert call(1, 8, M=0) == L.SR_EINVAL            # M < 1
    assert call(1, 8, M=-1) == L.SR_EINVAL
    assert sa.lib().sr_session_loo(None, None, 1, 0, 8, ctypes.byref(L.sr_loo_out())) == L.SR_EINVAL
    # an invalid argument wins over a matrix that is too large
    assert call(0, 8, N=1, M=2 ** 27 + 1) == L.SR_EINVAL
    assert call(1, 8) == accepted()


def test_unsupported():
    assert call(1, 8, N=1, M=2 ** 27 + 1) == L.SR_EUNSUPPORTED
    assert call(1, 8, N=32767, M=4097) == L.SR_EUNSUPPORTED      # 32767 * 4097 > 2^27
    # n > 4096: the rates of all T samples are checked first, so the case needs them all
    T = 1864136
    assert loo_ref.tail_len(T) == 4097 and loo_ref.tail_len(T - 1) == 4096
    d = L.sr_dataset()
    d.N, d.M = 1, 1
    x = np.zeros(1, np.uint8)
    d.X = x.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    rec = np.zeros((1, T, 3), np.int16)
    rates = np.full((1, T, 3), -1.0)
    o = L.sr_loo_out()
    o.elpd = 5.0
    args = (ctypes.byref(d), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), rates.ctypes.data_as(_DBLP), 0)
    assert sa.lib().sr_loo(*args, 1, T, 0, ctypes.byref(o)) == L.SR_EUNSUPPORTED and o.elpd == 5.0
    rates[0, T - 1, 1] = 0.5   # a bad rate wins
    assert sa.lib().sr_loo(*args, 1, T, 0, ctypes.byref(o)) == L.SR_EINVAL


LO, HI = -600.0, -2.0 ** -50


@pytest.mark.parametrize("manycd", [0, 1])
def test_rate_domain(manycd):
    """c, d in [-600, -2^-50]: the edges are accepted (the call goes on to the device), everything just outside
    (WAIC's -700 too), +0.0, NaN and the infinities are refused, in either slot and, manycd, in any taxon's."""
    slots = range(4) if manycd else range(2)
    for edge in (LO, HI):
        for j in slots:
            cd = [-1.0] * len(slots)
            cd[j] = edge
            assert call(1, 8, manycd=manycd, cd=cd) == accepted()
    bad = (np.nextafter(LO, -np.inf), -700.0, np.nextafter(HI, 0.0), -0.0, 0.0, 1e-300, 1.0, float("nan"),
           float("inf"), float("-inf"), -1e308)
    for v in bad:
        for j in slots:
            cd = [-1.0] * len(slots)
            cd[j] = v
            assert call(1, 8, manycd=manycd, cd=cd) == L.SR_EINVAL, (v, j)
    if not manycd:   # the loglik entry is not read
        for v in (0.0, float("nan"), float("inf"), 12.5):
            assert call(1, 8, cd=[-1.0, -1.0, v]) == accepted()


def test_host_only_library_exports_and_refuses():
    """The fake-device library (no device layer, so no LOO kernels) still links, exports the five functions, answers a
    valid sr_loo call with SR_EUNSUPPORTED and an invalid one with SR_EINVAL, and runs the host-only functions."""
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(sa.__file__)))
    subprocess.check_call(["make", "-s", "-C", pkg, "build/fake/libseriation.so"])
    code = ("import ctypes, numpy as np, seriation_amd as sa\n"
            "from seriation_amd import _lib as L\n"
            "lib = sa.lib()\n"
            "assert all(hasattr(lib, s) for s in ('sr_loo', 'sr_session_loo', 'sr_loo_reduce', 'sr_loo_tail', 'sr_loo_tail_len'))\n"
            "ds = sa.Dataset.parse(b'3 2\\n1 0\\n1 1\\n0 1\\n')\n"
            "rec = np.zeros((1, 8, 7), np.int16)\n"
            "recp = rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))\n"
            "cd = np.full((1, 8, 3), -1.0)\n"
            "cdp = cd.ctypes.data_as(ctypes.POINTER(ctypes.c_double))\n"
            "out = L.sr_loo_out()\n"
            "k, e = ctypes.c_double(), ctypes.c_double()\n"
            "print(lib.sr_loo(ctypes.byref(ds.c), recp, cdp, 0, 1, 8, 0, ctypes.byref(out)),"
            " lib.sr_loo(ctypes.byref(ds.c), recp, cdp, 0, 0, 8, 0, ctypes.byref(out)),"
            " lib.sr_loo_reduce(1, 3, cdp, cdp, cdp, ctypes.byref(out)), out.elpd, lib.sr_loo_tail_len(1000),"
            " lib.sr_loo_tail(3, 0, None, 1.0, 3.0, ctypes.byref(k), ctypes.byref(e)), e.value)\n")
    env = dict(os.environ, SERIATION_LIB=os.path.join(pkg, "build", "fake", "libseriation.so"),
               PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == [str(L.SR_EUNSUPPORTED), str(L.SR_EINVAL), "0", "-3.0", "95", "0",
                                                      "0.0"], r.stdout + r.stderr


def test_compare_on_loo_results():
    """analysis.waic_compare reads only the pointwise array "elpd": two LOO-shaped results, and a LOO against a
    WAIC-shaped one, compare as two WAIC results do."""
    rng = np.random.RandomState(9)
    for shape in ((1, 1), (3, 4), (25, 31)):
        a = {"elpd_loo": -1.0, "elpd": -rng.uniform(0.01, 5.0, shape), "pareto_k": rng.uniform(0, 1, shape)}
        b = {"elpd_loo": -2.0, "elpd": -rng.uniform(0.01, 5.0, shape), "pareto_k": rng.uniform(0, 1, shape)}
        w = {"elpd_waic": -2.0, "elpd": -rng.uniform(0.01, 5.0, shape), "pwaic": rng.uniform(0, 1, shape)}
        for x, y in ((a, b), (a, w), (w, b)):
            got, want = analysis.waic_compare(x, y), waic_ref.compare(x, y)
            assert set(got) == {"elpd_diff", "se_diff"} and bits(got["elpd_diff"]) == bits(want["elpd_diff"])
            if shape == (1, 1):
                assert math.isnan(got["se_diff"])
            else:
                assert bits(got["se_diff"]) == bits(want["se_diff"]) and got["se_diff"] > 0
    assert "LOO" in analysis.waic_compare.__doc__
    assert callable(analysis.loo_from_records) and callable(analysis.loo_from_session)


@pytest.mark.parametrize("extra", [[], ["--select", "2", "--no-save"]])
def test_cli_loo_needs_select(capsys, extra):
    from seriation_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["nowhere.txt", "--loo"] + extra)
    assert e.value.code == 2 and "--loo" in capsys.readouterr().err
