"""The host side of the posterior marginals: the numpy definition (tests/marg_ref.py) against a brute-force loop,
analysis.chain_orientation on constructed sums, and every argument error of sr_marginals, which must be reported
before any device call.  CPU only: the histograms come from the GPU in tests/test_gpu_marginals.py."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np

import marg_ref
import seriation_amd as sa
from seriation_amd import _lib as L
from seriation_amd import analysis


def brute(rec, N, M, probs, flips):
    """The definition read literally: counts per value, the cumulative count walked from 0."""
    n_sel, count, W = len(rec), len(rec[0]), 2 * M + N
    out = {"quant": [[0] * W for _ in probs], "mode": [0] * W, "mean": [0.0] * W, "outside": [0] * W,
           "hist": [[0] * (N + 1) for _ in range(W)],
           "pi_sum": [[sum(rec[k][t][2 * M + i] for t in range(count)) for i in range(N)] for k in range(n_sel)]}
    for j in range(W):
        for k in range(n_sel):
            for t in range(count):
                row = rec[k][t]
                v = row[j]
                if flips[k]:
                    v = N - row[j + M] if j < M else (N - row[j - M] if j < 2 * M else N - 1 - row[j])
                if 0 <= v <= N:
                    out["hist"][j][v] += 1
                else:
                    out["outside"][j] += 1
        h = out["hist"][j]
        T = sum(h)
        if T == 0:
            out["mode"][j], out["mean"][j] = -1, float("nan")
            for q in range(len(probs)):
                out["quant"][q][j] = -1
            continue
        out["mode"][j] = max(range(N + 1), key=lambda v: (h[v], -v))
        out["mean"][j] = sum(v * h[v] for v in range(N + 1)) / T
        for q, p in enumerate(probs):
            k = min(max(math.ceil(p * float(T)), 1), T)
            c = 0
            for v in range(N + 1):
                c += h[v]
                if c >= k:
                    out["quant"][q][j] = v
                    break
    return out


def test_ref_matches_brute_force():
    N, M, n_sel, count = 4, 3, 3, 7
    rng = np.random.RandomState(43)
    rec = rng.randint(-2, N + 3, (n_sel, count, 2 * M + N))   # some values outside [0, N] on both sides
    rec[:, :, 1] = -5                                         # a column without any in-range value: the flagged
    rec[1, :, 4] = 32767                                      # chain's a column 1 reads its b column 4, N - 32767
    rec[0, 0, 0], rec[1, 2, 5] = -32768, 32767
    probs, flips = (0.0, 0.025, 0.5, 0.51, 1.0), [0, 1, 0]
    want = brute(rec.tolist(), N, M, probs, flips)
    got = marg_ref.marginals(rec.astype(np.int16), N, M, probs, flips, hist=True)
    for k in ("quant", "mode", "outside", "hist", "pi_sum"):
        assert np.array_equal(got[k], np.array(want[k])), k
    assert marg_ref.same_mean(got["mean"], want["mean"])
    # column 1 holds nothing in range in any chain; the flagged chain's b column 4 reads a column 1: N + 5
    assert got["mode"][1] == -1 and math.isnan(got["mean"][1]) and (got["quant"][:, 1] == -1).all()
    assert got["outside"][1] == n_sel * count and got["outside"][4] >= count
    assert (got["hist"].sum(axis=1) + got["outside"] == n_sel * count).all()


def test_ref_lower_median_and_extremes():
    rec = np.zeros((1, 4, 2 * 1 + 6), np.int16)
    rec[0, :, 0] = [5, 1, 3, 2]   # even T: the lower of the two middle values
    r = marg_ref.marginals(rec, 6, 1, (0.0, 0.5, 1.0))
    assert r["quant"][:, 0].tolist() == [1, 2, 5]
    assert r["mode"][1] == 0 and r["mean"][0] == 11 / 4


def test_chain_orientation():
    N = 9
    base = np.array([40, 10, 30, 0, 80, 50, 20, 70, 60], np.int64)   # count * position of each site
    pi_sum = np.stack([base, base, 10 * (N - 1) - base, np.full(N, 35), base + np.arange(N)])
    assert analysis.chain_orientation(pi_sum).tolist() == [0, 0, 1, 0, 0]
    assert analysis.chain_orientation(pi_sum).dtype == np.uint8
    # chain 0 itself constant: every correlation undefined, nothing flagged
    assert analysis.chain_orientation(np.stack([np.full(N, 35), base, 80 - base])).tolist() == [0, 0, 0]
    # sums too large for a float product: the sign is still exact
    big = base * (2 ** 40)
    assert analysis.chain_orientation(np.stack([big, big.max() - big, big])).tolist() == [0, 1, 0]


def call(n_sel, count, probs=(0.5,), n_probs=None, N=3, M=2, rec_shape=(1, 8)):
    """sr_marginals through ctypes with outputs for one chain of 8 rows, whatever n_sel and count claim."""
    ds = sa.Dataset(np.zeros((N, M), np.uint8), np.zeros(N, bool))
    W = 2 * M + N
    rec = np.zeros(rec_shape + (W,), np.int16)
    p = np.array(probs, np.float64)
    quant, mode = np.zeros((max(len(p), 1), W), np.int32), np.zeros(W, np.int32)
    out = L.sr_marg_out()
    out.probs = p.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    out.n_probs = len(p) if n_probs is None else n_probs
    out.quant = quant.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    out.mode = mode.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    return sa.lib().sr_marginals(ctypes.byref(ds.c), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), n_sel, count, 0,
                                 ctypes.byref(out))


def test_argument_checks():
    """Every SR_EINVAL case of the definition; none of them reaches the device (this test runs without one)."""
    assert call(0, 8) == L.SR_EINVAL                 # n_sel = 0
    assert call(-1, 8) == L.SR_EINVAL
    assert call(1, 0) == L.SR_EINVAL                 # count < 1
    assert call(1, -3) == L.SR_EINVAL
    assert call(65536, 32768) == L.SR_EINVAL         # n_sel * count = 2^31
    assert call(2, 2 ** 30) == L.SR_EINVAL
    assert call(1, 8, probs=[0.5] * 17) == L.SR_EINVAL   # Q > 16
    assert call(1, 8, n_probs=-1) == L.SR_EINVAL
    for p in (-1e-300, 1.0000000000000002, float("nan"), float("inf"), -0.5, 2.0):
        assert call(1, 8, probs=(0.5, p)) == L.SR_EINVAL, p
    lib = sa.lib()
    out = L.sr_marg_out()
    rec = np.zeros((1, 8, 7), np.int16)
    ds = sa.Dataset(np.zeros((3, 2), np.uint8), np.zeros(3, bool))
    recp = rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))
    assert lib.sr_marginals(None, recp, 1, 8, 0, ctypes.byref(out)) == L.SR_EINVAL
    assert lib.sr_marginals(ctypes.byref(ds.c), None, 1, 8, 0, ctypes.byref(out)) == L.SR_EINVAL
    assert lib.sr_marginals(ctypes.byref(ds.c), recp, 1, 8, 0, None) == L.SR_EINVAL
    out.n_probs = 2                                   # probabilities announced, none given
    assert lib.sr_marginals(ctypes.byref(ds.c), recp, 1, 8, 0, ctypes.byref(out)) == L.SR_EINVAL
    assert lib.sr_session_marginals(None, None, 1, 0, 8, ctypes.byref(L.sr_marg_out())) == L.SR_EINVAL


def test_host_only_library_exports_and_refuses():
    """The fake-device library (no device layer, so no histogram kernels) still links, exports both functions, and
    answers a valid sr_marginals call with SR_EUNSUPPORTED, an invalid one with SR_EINVAL."""
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(sa.__file__)))
    subprocess.check_call(["make", "-s", "-C", pkg, "build/fake/libseriation.so"])
    code = ("import ctypes, numpy as np, seriation_amd as sa\n"
            "from seriation_amd import _lib as L\n"
            "lib = sa.lib()\n"
            "assert all(hasattr(lib, s) for s in ('sr_marginals', 'sr_session_marginals'))\n"
            "ds = sa.Dataset.parse(b'3 2\\n1 0\\n1 1\\n0 1\\n')\n"
            "rec = np.zeros((1, 8, 7), np.int16)\n"
            "recp = rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))\n"
            "out = L.sr_marg_out()\n"
            "print(lib.sr_marginals(ctypes.byref(ds.c), recp, 1, 8, 0, ctypes.byref(out)),"
            " lib.sr_marginals(ctypes.byref(ds.c), recp, 0, 8, 0, ctypes.byref(out)))\n")
    env = dict(os.environ, SERIATION_LIB=os.path.join(pkg, "build", "fake", "libseriation.so"),
               PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == [str(L.SR_EUNSUPPORTED), str(L.SR_EINVAL)], r.stdout + r.stderr


def test_cli_marginals_needs_select(capsys):
    from seriation_amd.__main__ import main
    import pytest
    with pytest.raises(SystemExit) as e:
        main(["nowhere.txt", "--marginals"])
    assert e.value.code == 2 and "--marginals" in capsys.readouterr().err
