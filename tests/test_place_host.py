"""Placement of query rows without a GPU: the numpy definition (tests/place_ref.py) against a literal loop in Python
floats on tiny shapes, the crafted underflow case (the reference alone produces a subnormal e and an e == 0.0),
read_queries and its format errors, placement_summary on hand-made distributions, every argument error of
sr_placement (reported before the device is touched, the outputs untouched), the host-only library's refusal and
the command line's argument check."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import place_ref
import seriation_amd as sa
from seriation_amd import _lib as L
from seriation_amd import analysis

_DBLP = ctypes.POINTER(ctypes.c_double)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def literal(N, rec, cd, Y, manycd, flips):
    """the definition term by term in Python floats: every sum one add after the other"""
    n_sel, count = rec.shape[:2]
    Q, M = Y.shape
    T = n_sel * count
    pos = [[0.0] * N for _ in range(Q)]
    site = [[0.0] * N for _ in range(Q)]
    lse = np.zeros((n_sel, count, Q))
    for k in range(n_sel):
        cpos = [[0.0] * N for _ in range(Q)]
        csite = [[0.0] * N for _ in range(Q)]
        for r in range(count):
            row = [int(v) for v in rec[k, r]]
            a, b, pi = row[:M], row[M:2 * M], row[2 * M:]
            if flips is not None and flips[k]:
                a, b, pi = [N - v for v in row[M:2 * M]], [N - v for v in row[:M]], [N - 1 - v for v in pi]
            for q in range(Q):
                Lp = []
                for p in range(N):
                    s = 0.0
                    for m in range(M):
                        c, d = (cd[k, r, m], cd[k, r, M + m]) if manycd else (cd[k, r, 0], cd[k, r, 1])
                        l = (math.log(1.0 - math.exp(c)), d, math.log(1.0 - math.exp(d)), c)
                        alive, y = a[m] <= p < b[m], int(Y[q, m])
                        if y == 2:
                            continue
                        s += l[(2 if alive else 3) if y else (1 if alive else 0)]
                    Lp.append(s)
                mx = max(Lp)
                e = [math.exp(v - mx) for v in Lp]
                z = [0.0] * 64
                for p in range(N):
                    z[p % 64] += e[p]
                Z = 0.0
                for j in range(64):
                    Z += z[j]
                lse[k, r, q] = mx + math.log(Z)
                for p in range(N):
                    cpos[q][p] += e[p] / Z
                for n in range(N):
                    csite[q][n] += e[pi[n]] / Z if 0 <= pi[n] < N else 0.0
        for q in range(Q):
            for p in range(N):
                pos[q][p] += cpos[q][p]
                site[q][p] += csite[q][p]
    lpd = []
    for q in range(Q):
        flat = [float(v) for v in lse[:, :, q].reshape(-1)]
        mxx, s = max(flat), 0.0
        for v in flat:
            s += math.exp(v - mxx)
        lpd.append(mxx + math.log(s / float(T)) - math.log(float(N)))
    return {"pos": np.array(pos) / float(T), "site": np.array(site) / float(T), "lse": lse, "lpd": np.array(lpd)}


def tiny(N, M, n_sel, count, Q, manycd, seed=0):
    rng = np.random.RandomState(100 * N + 10 * M + count + seed)
    rec = rng.randint(-2, N + 3, (n_sel, count, 2 * M + N)).astype(np.int16)
    rec[0, 0, 2 * M:] = rng.permutation(N)
    Mt = M if manycd else 1
    c = rng.uniform(np.log(0.001), np.log(0.1), (n_sel, count, Mt))
    d = rng.uniform(np.log(0.2), np.log(0.8), (n_sel, count, Mt))
    cd = np.concatenate([c, d] + ([] if manycd else [np.full((n_sel, count, 1), np.nan)]), axis=2)
    Y = rng.randint(0, 3, (Q, M)).astype(np.uint8)
    return rec, cd, Y


@pytest.mark.parametrize("manycd", [False, True], ids=["shared", "manycd"])
@pytest.mark.parametrize("N,M,n_sel,count,Q", [(1, 1, 1, 1, 1), (5, 4, 3, 3, 3), (66, 3, 2, 2, 2), (130, 2, 1, 2, 1)])
def test_reference_equals_literal_loop(N, M, n_sel, count, Q, manycd):
    rec, cd, Y = tiny(N, M, n_sel, count, Q, manycd)
    for flips in (None, [k % 2 == 0 for k in range(n_sel)]):
        want, got = literal(N, rec, cd, Y, manycd, flips), place_ref.placement(N, rec, cd, Y, manycd, flips)
        for k in ("pos", "site", "lse", "lpd"):
            assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), (k, flips)
        assert got["total"] == n_sel * count
        assert np.allclose(got["pos"].sum(axis=1), 1.0, atol=1e-12)


def test_reference_all_unassessed_row_is_uniform():
    """a row of 2s has L = 0 everywhere: w = 1 / N, lse = log N, lpd = 0"""
    N, M = 70, 3
    rec, cd, _ = tiny(N, M, 2, 2, 1, False)
    r = place_ref.placement(N, rec, cd, np.full((1, M), 2, np.uint8))
    assert np.array_equal(bits(r["lse"]), bits(np.full((2, 2, 1), math.log(float(N)))))
    assert np.array_equal(bits(r["pos"]), bits(np.full((1, N), 1.0 / N))) and abs(r["lpd"][0]) < 1e-15


def test_underflow_case_holds_both_kinds():
    """The crafted case does hold what it is for, by the reference alone: in the first sample query 0 has a gap
    inside (-745, -708) whose e is subnormal and a gap below -746 whose e is exactly 0.0."""
    N, rec, cd, Y = place_ref.underflow_case()
    M = Y.shape[1]
    L0 = place_ref.profile(rec[0, 0], place_ref.table(cd, M, False)[0, 0], Y, N, M)
    gap = L0[0] - L0[0].max()
    e, Z, lse = place_ref.normalise(L0)
    assert gap[0] == 0.0 and -745.0 < gap[2] < -708.0 and gap[3] < -746.0
    assert 0.0 < e[0, 2] < sys.float_info.min and e[0, 3] == 0.0 and e[0, 1] > sys.float_info.min
    assert Z[0] >= 1.0 and (e[0] / Z[0])[2] > 0.0
    r = place_ref.placement(N, rec, cd, Y)
    assert np.array_equal(bits(r["pos"]), bits(literal(N, rec, cd, Y, False, None)["pos"]))


def test_read_queries(tmp_path):
    p = tmp_path / "q.txt"
    p.write_text("3 4\n0 1 ? 1\n? ? ? ? *\n1 1 0 0*\n")
    y = analysis.read_queries(str(p), 4)
    assert y.dtype == np.uint8 and y.tolist() == [[0, 1, 2, 1], [2, 2, 2, 2], [1, 1, 0, 0]]
    bad = {"": "first line", "3\n0 1\n": "first line", "x 4\n": "first line", "1 3\n0 1 1\n": "taxa",
           "2 4\n0 1 1 1\n": "announced", "1 4\n0 1 1 1\n0 0 0 0\n": "announced", "0 4\n": "announced",
           "1 4\n0 1 1\n": "tokens", "1 4\n0 1 1 1 1\n": "tokens", "1 4\n0 1 2 1\n": "not 0, 1 or ?",
           "1 4\n0 1 x 1\n": "not 0, 1 or ?"}
    for text, what in bad.items():
        p.write_text(text)
        with pytest.raises(ValueError, match=what):
            analysis.read_queries(str(p), 4)


def test_placement_summary():
    pos = np.array([[0.0, 0.0, 1.0, 0.0], [0.25, 0.25, 0.25, 0.25], [0.5, 0.0, 0.0, 0.5], [0.01, 0.02, 0.96, 0.01]])
    site = np.array([[0.0, 1.0, 0.0, 0.0], [0.25, 0.25, 0.25, 0.25], [0.0, 0.5, 0.5, 0.0], [0.96, 0.02, 0.01, 0.01]])
    s = analysis.placement_summary(pos, site, (0.025, 0.5, 0.975))
    assert s["mean"].tolist() == [2.0, 1.5, 1.5, 0.02 + 1.92 + 0.03]
    assert s["mode"].tolist() == [2, 0, 0, 2] and s["best_site"].tolist() == [1, 0, 1, 0]
    assert s["p_best_site"].tolist() == [1.0, 0.25, 0.5, 0.96]
    assert s["quant"].tolist() == [[2, 0, 0, 1], [2, 1, 0, 2], [2, 3, 3, 2]]
    one = analysis.placement_summary(pos[0], site[0], (0.5,))
    assert one["quant"].tolist() == [[2]] and one["mode"].tolist() == [2]
    low = analysis.placement_summary(np.array([[0.5, 0.49999]]), np.array([[0.5, 0.5]]), (1.0,))
    assert low["quant"].tolist() == [[1]]   # the total stays below the probability: the last position


def raw_dataset(N, M, X=True):
    """an sr_dataset of any claimed shape: the checks read N, M and whether X is there"""
    ds = L.sr_dataset()
    ds.N, ds.M = N, M
    keep = np.zeros(1, np.uint8)
    if X:
        ds.X = keep.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    return ds, keep


def call(n_sel=1, count=8, N=3, M=2, Q=2, manycd=0, ds=True, X=True, rec=True, cd=True, Y=True, out=True, yval=None,
         rate=None):
    """sr_placement through ctypes; every output points at one small buffer, which no refused call touches."""
    buf = np.zeros(64)
    r = np.zeros((1, 8, 2 * M + N if M > 0 and N > 0 else 1), np.int16)
    rates = np.full((8, 2 * max(M, 1) if manycd else 3), -1.0)   # a refused call reads no more than a valid one's n_sel * count rows
    if rate is not None:
        rates[-1, rate[0]] = rate[1]
    y = np.zeros((max(Q, 1), max(M, 1)), np.uint8)
    if yval is not None:
        y[-1, -1] = yval
    o = L.sr_place_out()
    o.kernel_ms = -1.0
    for k in ("pos", "site", "lse", "lpd"):
        setattr(o, k, buf.ctypes.data_as(_DBLP))
    d, _keep = raw_dataset(N, M, X)
    rc = sa.lib().sr_placement(ctypes.byref(d) if ds else None,
                               r.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)) if rec else None,
                               rates.ctypes.data_as(_DBLP) if cd else None, manycd, n_sel, count,
                               y.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if Y else None, Q, 0,
                               ctypes.byref(o) if out else None)
    assert not buf.any() and o.kernel_ms == -1.0
    return rc


def test_argument_checks():
    """Every SR_EINVAL case of the definition; none of them reaches the device (this test runs without one)."""
    for kw in (dict(ds=False), dict(X=False), dict(rec=False), dict(cd=False), dict(out=False), dict(Y=False)):
        assert call(**kw) == L.SR_EINVAL, kw
    assert call(Q=0) == L.SR_EINVAL and call(Q=-1) == L.SR_EINVAL
    assert call(yval=3) == L.SR_EINVAL and call(yval=255) == L.SR_EINVAL
    assert call(n_sel=0) == L.SR_EINVAL and call(n_sel=-1) == L.SR_EINVAL          # T < 1
    assert call(count=0) == L.SR_EINVAL and call(count=-3) == L.SR_EINVAL
    assert call(n_sel=65536, count=32768) == L.SR_EINVAL and call(n_sel=2, count=2 ** 30) == L.SR_EINVAL   # T = 2^31
    assert call(N=0) == L.SR_EINVAL and call(N=-4) == L.SR_EINVAL and call(N=32768) == L.SR_EINVAL
    assert call(M=0) == L.SR_EINVAL and call(M=-1) == L.SR_EINVAL
    for v in (-700.0000001, -2.0 ** -51, 0.0, 1.0, float("nan"), float("inf"), -float("inf")):
        assert call(rate=(0, v)) == L.SR_EINVAL, v                                    # c outside the domain
        assert call(rate=(1, v)) == L.SR_EINVAL, v                                    # d
        assert call(manycd=1, rate=(3, v)) == L.SR_EINVAL, v                          # the last taxon's d
    assert sa.lib().sr_session_placement(None, None, 1, 0, 8, None, 1, ctypes.byref(L.sr_place_out())) == L.SR_EINVAL
    # an invalid argument wins over an output that is too large
    assert call(N=32767, Q=4097, yval=3) == L.SR_EINVAL
    assert call(N=32767, Q=4097, rate=(1, 0.0)) == L.SR_EINVAL


def test_outputs_too_large_unsupported():
    """Q N > 2^27: SR_EUNSUPPORTED before any device call; exactly 2^27 is not refused for its size (it is not run
    here: nothing smaller than the device could answer it)."""
    assert call(N=32767, Q=4097) == L.SR_EUNSUPPORTED        # Q N = 2^27 + 28671
    assert call(N=16384, Q=8193) == L.SR_EUNSUPPORTED


def test_host_only_library_exports_and_refuses():
    """The fake-device library (no device layer, so no placement kernels) still links, exports both functions, and
    answers a valid sr_placement call with SR_EUNSUPPORTED, an invalid one with SR_EINVAL, the outputs untouched."""
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(sa.__file__)))
    subprocess.check_call(["make", "-s", "-C", pkg, "build/fake/libseriation.so"])
    code = ("import ctypes, numpy as np, seriation_amd as sa\n"
            "from seriation_amd import _lib as L\n"
            "lib = sa.lib()\n"
            "assert all(hasattr(lib, s) for s in ('sr_placement', 'sr_session_placement'))\n"
            "ds = sa.Dataset.parse(b'3 2\\n1 0\\n1 1\\n0 1\\n')\n"
            "rec = np.zeros((1, 8, 7), np.int16)\n"
            "recp = rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))\n"
            "cd = np.full((8, 3), -1.0)\n"
            "cdp = cd.ctypes.data_as(ctypes.POINTER(ctypes.c_double))\n"
            "y = np.zeros((2, 2), np.uint8)\n"
            "yp = y.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))\n"
            "buf = np.zeros(6)\n"
            "out = L.sr_place_out()\n"
            "out.pos = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))\n"
            "print(lib.sr_placement(ctypes.byref(ds.c), recp, cdp, 0, 1, 8, yp, 2, 0, ctypes.byref(out)),"
            " lib.sr_placement(ctypes.byref(ds.c), recp, cdp, 0, 0, 8, yp, 2, 0, ctypes.byref(out)), int(buf.any()))\n")
    env = dict(os.environ, SERIATION_LIB=os.path.join(pkg, "build", "fake", "libseriation.so"),
               PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == [str(L.SR_EUNSUPPORTED), str(L.SR_EINVAL), "0"], r.stdout + r.stderr


@pytest.mark.parametrize("extra", [[], ["--select", "2", "--no-save"]])
def test_cli_place_needs_select(capsys, extra):
    from seriation_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["nowhere.txt", "--place", "queries.txt"] + extra)
    assert e.value.code == 2 and "--place needs --select" in capsys.readouterr().err
