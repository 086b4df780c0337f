"""The host side of the posterior predictive checks: the numpy definition (tests/ppc_ref.py) held to Philox's known
answers and to a literal per-cell, per-sample loop, every argument error of sr_ppc, which must be reported before any
kernel runs, the p-value arithmetic, and a sanity check of the definition itself.  CPU only: the counts come from the
GPU in tests/test_gpu_ppc.py."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import ppc_ref
import seriation_amd as sa
from seriation_amd import _lib as L
from seriation_amd import analysis

_DBLP = ctypes.POINTER(ctypes.c_double)
_U32P = ctypes.POINTER(ctypes.c_uint32)
_I64P = ctypes.POINTER(ctypes.c_int64)

# Philox4x32-10 known answers (Random123's published kat_vectors for philox4x32_10; tests/test_oracle_rng.py holds
# the oracle and the library to the same three)
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_reference_philox_known_answers():
    for ctr, key, want in PHILOX_KAT:
        got = ppc_ref.philox4x32_10(ctr, key)
        assert tuple(int(v) for v in got) == want
    # over arrays: every element its own counter
    ctrs = np.array([k[0] for k in PHILOX_KAT[:1] * 2 + PHILOX_KAT[:1]], np.uint64).T
    got = ppc_ref.philox4x32_10(tuple(ctrs), PHILOX_KAT[0][1])
    assert [tuple(int(v[i]) for v in got) for i in range(3)] == [PHILOX_KAT[0][2]] * 3
    # the library's generator is the same function
    for ctr, key, want in PHILOX_KAT:
        out = (ctypes.c_uint32 * 4)()
        sa.lib().sr_host_philox((ctypes.c_uint32 * 4)(*ctr), (ctypes.c_uint32 * 2)(*key), out)
        assert tuple(out) == want


def philox_scalar(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def brute(X, rec, cd, manycd, seed, reps):
    """The definition read literally, one cell and one sample at a time, in Python integers."""
    N, M = len(X), len(X[0])
    n_sel, count = len(rec), len(rec[0])
    key = (seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ 0x50504331)
    zero5 = lambda n: [[0] * n for _ in range(5)]   # noqa: E731
    res = {"taxon_gt": zero5(M), "taxon_eq": zero5(M), "taxon_sum_obs": zero5(M), "taxon_sum_rep": zero5(M),
           "site_gt": [0] * N, "site_eq": [0] * N, "site_sum_rep": [0] * N, "total_gt": [0] * 5, "total_eq": [0] * 5,
           "total_obs": [[None] * count for _ in range(n_sel)],
           "total_rep": [[[None] * reps for _ in range(count)] for _ in range(n_sel)]}

    def taxon_stats(Y, alive, pi, m):
        at = [pi[n] for n in range(N) if Y[n][m]]
        ones = len(at)
        span = max(at) - min(at) + 1 if ones else 0
        f0 = sum(1 for n in range(N) if alive[n][m] and not Y[n][m])
        f1 = sum(1 for n in range(N) if not alive[n][m] and Y[n][m])
        return [ones, span, span - ones, f0, f1]

    for k in range(n_sel):
        for r in range(count):
            t = k * count + r
            row = rec[k][r]
            a, b, pi = row[:M], row[M:2 * M], row[2 * M:]
            alive = [[a[m] <= pi[n] < b[m] for m in range(M)] for n in range(N)]
            obs = [taxon_stats(X, alive, pi, m) for m in range(M)]
            tobs = [sum(obs[m][i] for m in range(M)) for i in range(5)]
            res["total_obs"][k][r] = tobs
            for rep in range(reps):
                Y = [[0] * M for _ in range(N)]
                for n in range(N):
                    for m in range(M):
                        c, d = (cd[k][r][m], cd[k][r][M + m]) if manycd else (cd[k][r][0], cd[k][r][1])
                        thr = int((1.0 - math.exp(d)) * 4294967296.0) if alive[n][m] else int(math.exp(c) * 4294967296.0)
                        w = philox_scalar((n, m >> 2, t, rep), key)[m & 3]
                        Y[n][m] = int(w < thr)
                st = [taxon_stats(Y, alive, pi, m) for m in range(M)]
                for m in range(M):
                    for i in range(5):
                        res["taxon_gt"][i][m] += st[m][i] > obs[m][i]
                        res["taxon_eq"][i][m] += st[m][i] == obs[m][i]
                        res["taxon_sum_obs"][i][m] += obs[m][i]
                        res["taxon_sum_rep"][i][m] += st[m][i]
                for n in range(N):
                    rich, ro = sum(Y[n]), sum(X[n])
                    res["site_gt"][n] += rich > ro
                    res["site_eq"][n] += rich == ro
                    res["site_sum_rep"][n] += rich
                trep = [sum(st[m][i] for m in range(M)) for i in range(5)]
                res["total_rep"][k][r][rep] = trep
                for i in range(5):
                    res["total_gt"][i] += trep[i] > tobs[i]
                    res["total_eq"][i] += trep[i] == tobs[i]
    return res


@pytest.mark.parametrize("manycd", [False, True])
def test_ref_matches_literal_loop(manycd):
    N, M, n_sel, count, reps, seed = 3, 5, 2, 4, 2, (7 << 32) | 9
    rng = np.random.RandomState(5 + manycd)
    X = rng.randint(0, 2, (N, M))
    rec = rng.randint(-1, N + 2, (n_sel, count, 2 * M + N))
    rec[0, 0, 0], rec[1, 2, M + 1], rec[1, 3, 2 * M] = -32768, 32767, 32767
    cd = np.log(rng.uniform(0.05, 0.9, (n_sel, count, 2 * M if manycd else 3)))
    want = brute(X.tolist(), rec.tolist(), cd.tolist(), manycd, seed, reps)
    got = ppc_ref.ppc(X, rec.astype(np.int16), cd, manycd, seed, reps)
    assert set(got) == set(want) | {"pairs"} and got["pairs"] == n_sel * count * reps
    for k, v in want.items():
        assert np.array_equal(got[k], np.array(v, np.int64)), k
    # the case is not degenerate: the replicates differ from X, both tallies occur, ones occur dead and alive
    assert got["taxon_gt"].any() and got["taxon_eq"].any() and got["taxon_sum_rep"][3].any() and got["taxon_sum_rep"][4].any()
    assert got["site_gt"].any() and (got["total_gt"] + got["total_eq"] <= got["pairs"]).all()


def test_thresholds_reach_both_ends():
    assert ppc_ref.thresholds(-700.0, -700.0) == (1 << 32, 0)
    # exp(-2^-50) = 1 - 2^-50: 2^-50 * 2^32 truncates to 0, (1 - 2^-50) * 2^32 to 2^32 - 1
    assert ppc_ref.thresholds(-2.0 ** -50, -2.0 ** -50) == (0, (1 << 32) - 1)
    ta, td = ppc_ref.thresholds(math.log(0.012), math.log(0.5))
    assert abs(ta - (1 << 31)) <= 1 and abs(td - 0.012 * 2 ** 32) <= 1


def test_pvalue_arithmetic():
    gt, eq = np.array([[0, 3, 10], [5, 0, 0]], np.uint32), np.array([[10, 1, 0], [0, 0, 7]], np.uint32)
    want = [[0.5, 0.35, 1.0], [0.5, 0.0, 0.35]]
    assert np.array_equal(analysis.ppc_pvalue(gt, eq, 10), np.array(want))
    assert np.array_equal(ppc_ref.pvalue(gt, eq, 10), np.array(want))
    assert analysis.ppc_pvalue(gt, eq, 10).dtype == np.float64
    big = analysis.ppc_pvalue(np.array([2 ** 31 - 2], np.uint32), np.array([1], np.uint32), 2 ** 31 - 1)
    assert big[0] == (2.0 ** 31 - 1.5) / (2.0 ** 31 - 1.0)   # no uint32 wrap in gt + eq / 2
    assert analysis.PPC_STATS == ppc_ref.STATS == ("ones", "span", "gaps", "f0", "f1")


def call(n_sel, count, reps=1, N=3, M=2, manycd=0, cd=None, ds=True, rec=True, cdp=True, out=True, X=True):
    """sr_ppc through ctypes on a dataset of any claimed shape (the checks before the rates read N and M only); every
    output points at a small buffer, which no refused call touches.  cd: the values of the first row."""
    b32, b64 = np.full(16, 5, np.uint32), np.full(64, 5, np.int64)
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
    o = L.sr_ppc_out()
    for k in ("taxon_gt", "taxon_eq", "site_gt", "site_eq"):
        setattr(o, k, b32.ctypes.data_as(_U32P))
    for k in ("taxon_sum_obs", "taxon_sum_rep", "site_sum_rep", "total_obs", "total_rep"):
        setattr(o, k, b64.ctypes.data_as(_I64P))
    o.pairs, o.kernel_ms = 5, 5.0
    for i in range(5):
        o.total_gt[i] = o.total_eq[i] = 5
    rc = sa.lib().sr_ppc(ctypes.byref(d) if ds else None, r.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)) if rec else None,
                         rates.ctypes.data_as(_DBLP) if cdp else None, manycd, n_sel, count, 12345, reps, 0,
                         ctypes.byref(o) if out else None)
    if rc != L.SR_OK:
        assert (b32 == 5).all() and (b64 == 5).all() and o.pairs == 5 and o.kernel_ms == 5.0
        assert list(o.total_gt) == [5] * 5 and list(o.total_eq) == [5] * 5
    return rc


def accepted():
    """what a call whose arguments are in order returns: the device's answer"""
    return L.SR_OK if sa.lib().sr_device_count() > 0 else L.SR_EDEVICE


def test_argument_checks():
    """Every SR_EINVAL case of the definition, each with that error alone; none of them reaches the device (this test
    runs without one)."""
    assert call(1, 8) == accepted()                  # the base case every line below spoils in one way
    assert call(1, 1) == accepted()                  # one sample is legal here
    assert call(1, 8, ds=False) == L.SR_EINVAL
    assert call(1, 8, rec=False) == L.SR_EINVAL
    assert call(1, 8, cdp=False) == L.SR_EINVAL
    assert call(1, 8, out=False) == L.SR_EINVAL
    assert call(1, 8, X=False) == L.SR_EINVAL
    assert call(0, 8) == L.SR_EINVAL                 # n_sel <= 0
    assert call(-1, 8) == L.SR_EINVAL
    assert call(1, 0) == L.SR_EINVAL                 # count < 1
    assert call(1, -3) == L.SR_EINVAL
    assert call(1, 8, reps=0) == L.SR_EINVAL         # reps outside 1..64
    assert call(1, 8, reps=-1) == L.SR_EINVAL
    assert call(1, 8, reps=65) == L.SR_EINVAL
    assert call(65536, 32768) == L.SR_EINVAL         # T reps = 2^31
    assert call(2, 2 ** 24, reps=64) == L.SR_EINVAL
    assert call(32768, 32768, reps=2) == L.SR_EINVAL
    assert call(1, 8, N=0) == L.SR_EINVAL            # N outside 1..32767
    assert call(1, 8, N=-4) == L.SR_EINVAL
    assert call(1, 8, N=32768) == L.SR_EINVAL
    assert call(1, 8, M=0) == L.SR_EINVAL            # M < 1
    assert call(1, 8, M=-1) == L.SR_EINVAL
    assert sa.lib().sr_session_ppc(None, None, 1, 0, 8, 0, 1, ctypes.byref(L.sr_ppc_out())) == L.SR_EINVAL
    # an invalid argument wins over a matrix that is too large
    assert call(0, 8, N=1, M=2 ** 27 + 1) == L.SR_EINVAL
    assert call(1, 8, reps=65, N=1, M=2 ** 27 + 1) == L.SR_EINVAL


def test_cells_beyond_limit_unsupported():
    assert call(1, 8, N=1, M=2 ** 27 + 1) == L.SR_EUNSUPPORTED
    assert call(1, 8, N=32767, M=4097) == L.SR_EUNSUPPORTED      # 32767 * 4097 > 2^27


LO, HI = -700.0, -2.0 ** -50


@pytest.mark.parametrize("manycd", [0, 1])
def test_rate_domain(manycd):
    """c, d in [-700, -2^-50]: the edges are accepted (the call goes on to the device), everything just outside,
    +0.0, NaN and the infinities are refused, in either slot and, manycd, in any taxon's."""
    slots = range(4) if manycd else range(2)
    for edge in (LO, HI):
        for j in slots:
            cd = [-1.0] * len(slots)
            cd[j] = edge
            assert call(1, 8, manycd=manycd, cd=cd) == accepted()
    bad = (np.nextafter(LO, -np.inf), np.nextafter(HI, 0.0), -0.0, 0.0, 1.0, float("nan"), float("inf"), float("-inf"))
    for v in bad:
        for j in slots:
            cd = [-1.0] * len(slots)
            cd[j] = v
            assert call(1, 8, manycd=manycd, cd=cd) == L.SR_EINVAL, (v, j)
    if not manycd:   # the loglik entry is not read
        for v in (0.0, float("nan"), 12.5):
            assert call(1, 8, cd=[-1.0, -1.0, v]) == accepted()


def test_host_only_library_exports_and_refuses():
    """The fake-device library (no device layer, so no kernels of this unit) still links, exports both functions,
    and answers a valid sr_ppc call with SR_EUNSUPPORTED and an invalid one with SR_EINVAL."""
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(sa.__file__)))
    subprocess.check_call(["make", "-s", "-C", pkg, "build/fake/libseriation.so"])
    code = ("import ctypes, numpy as np, seriation_amd as sa\n"
            "from seriation_amd import _lib as L\n"
            "lib = sa.lib()\n"
            "assert all(hasattr(lib, s) for s in ('sr_ppc', 'sr_session_ppc'))\n"
            "ds = sa.Dataset.parse(b'3 2\\n1 0\\n1 1\\n0 1\\n')\n"
            "rec = np.zeros((1, 8, 7), np.int16)\n"
            "recp = rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))\n"
            "cd = np.full((1, 8, 3), -1.0)\n"
            "cdp = cd.ctypes.data_as(ctypes.POINTER(ctypes.c_double))\n"
            "out = L.sr_ppc_out()\n"
            "print(lib.sr_ppc(ctypes.byref(ds.c), recp, cdp, 0, 1, 8, 5, 1, 0, ctypes.byref(out)),"
            " lib.sr_ppc(ctypes.byref(ds.c), recp, cdp, 0, 1, 8, 5, 0, 0, ctypes.byref(out)), out.pairs)\n")
    env = dict(os.environ, SERIATION_LIB=os.path.join(pkg, "build", "fake", "libseriation.so"),
               PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == [str(L.SR_EUNSUPPORTED), str(L.SR_EINVAL), "0"], \
        r.stdout + r.stderr


@pytest.mark.parametrize("extra", [[], ["--select", "2", "--no-save"], ["--select", "2", "--ppc-reps", "65"],
                                   ["--select", "2", "--ppc-seed", "-1"]])
def test_cli_ppc_preconditions(capsys, extra):
    from seriation_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["nowhere.txt", "--ppc"] + extra)
    assert e.value.code == 2 and "--ppc" in capsys.readouterr().err


def test_definition_is_sane():
    """One fixed valid state at 124 x 139, c = log 0.012, d = log 0.5, 300 identical rows, seed 12345: the mean of the
    replicates' total ones lies within six standard deviations of the sum of the cell probabilities,
    6 sqrt(sum p (1 - p) / 300) -- a derived bound.  The counter's t is all that separates the rows, so this fails
    if samples share words (the mean of 300 copies of one draw has 300 times the variance)."""
    N, M, T = 124, 139, 300
    rng = np.random.RandomState(1)
    pi = rng.permutation(N)
    a = rng.randint(0, N + 1, M)
    b = a + rng.randint(0, N + 1, M) % (N + 1 - a)
    row = np.concatenate([a, b, pi]).astype(np.int16)
    c, d = math.log(0.012), math.log(0.5)
    ta, td = ppc_ref.thresholds(c, d)
    alive, _ = ppc_ref.alive_of(row, N, M)
    p = np.where(alive, ta / 4294967296.0, td / 4294967296.0)
    assert alive.any() and not alive.all()
    tot = [int(ppc_ref.replicate(row, N, M, ta, td, t, 0, 12345).sum()) for t in range(T)]
    dist, bound = abs(np.mean(tot) - p.sum()), 6.0 * math.sqrt((p * (1.0 - p)).sum() / T)
    print("distance %.3f bound %.3f" % (dist, bound))
    assert dist <= bound
    assert len(set(tot)) > T // 10   # the rows do not share their words
    # the vectorised definition gives the same totals through its own loop
    rec = np.repeat(row[None, None, :], 3, axis=1)
    cd = np.tile(np.array([c, d, 0.0]), (1, 3, 1))
    X = rng.randint(0, 2, (N, M))
    got = ppc_ref.ppc(X, rec, cd, False, 12345, 1)
    assert got["total_rep"][0, :, 0, 0].tolist() == tot[:3]
