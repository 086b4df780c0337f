"""The host side of the convergence diagnostics (sr_diag_reduce: exact centred numerators, the f64 tail, argument
checks) against the definition in tests/diag_ref.py, and an independent anchor for the formulas (AR(1) chains of
known autocorrelation time).  CPU only: the moments come from numpy here, from the GPU in tests/test_gpu_diag.py."""
import ctypes
import math

import numpy as np
import pytest

import diag_ref
import seriation_amd as sa
from seriation_amd import _lib as L
from seriation_amd import analysis

from diag_ref import TOL, ar1


def traces(seed, n_sel, count):
    """Integer columns: AR(1) phi = 0.5, 0.9, 0 (white), a constant, an alternating one (negative rho_1), a slow
    random walk bounded to int16; plus scalar traces [n_sel][count][3]."""
    rng = np.random.RandomState(seed)
    t = np.arange(count)
    cols = [np.rint(ar1(rng, 0.5, n_sel, count, 40.0)) + 100, np.rint(ar1(rng, 0.9, n_sel, count, 25.0)),
            np.rint(ar1(rng, 0.0, n_sel, count, 300.0)) - 2000, np.full((n_sel, count), 7.0),
            np.rint(100.0 * (-1.0) ** t + 10.0 * rng.standard_normal((n_sel, count))),
            np.rint(ar1(rng, 0.97, n_sel, count, 60.0))]
    x = np.stack(cols, axis=2).astype(np.int64)
    assert np.abs(x).max() < 32768
    cdl = np.stack([ar1(rng, 0.6, n_sel, count, 0.05) - 3.0, ar1(rng, 0.3, n_sel, count, 0.02) - 1.5,
                    ar1(rng, 0.8, n_sel, count, 9.0) - 4000.0], axis=2)
    return x, cdl


# (seed, n_sel, count, max_lag, with scalars)
CASES = [
    pytest.param(11, 1, 60, 0, True, id="one-chain"),
    pytest.param(12, 4, 80, 0, True, id="four-chains"),
    pytest.param(13, 3, 61, 0, False, id="odd-count-no-scalars"),
    pytest.param(14, 3, 200, 2, True, id="max-lag-2-no-cut"),
    pytest.param(15, 2, 41, 7, True, id="odd-count-truncated"),
    pytest.param(16, 5, 4, 0, True, id="smallest"),
]


@pytest.mark.parametrize("seed,n_sel,count,max_lag,scalars", CASES)
def test_reduce_matches_definition(seed, n_sel, count, max_lag, scalars):
    x, cdl = traces(seed, n_sel, count)
    cd = cdl if scalars else None
    P, F, B, S1 = diag_ref.moments(x, max_lag)
    want = diag_ref.reduce(P, F, B, S1, count, max_lag, cd)   # asserts the margin condition
    got = analysis.diag_reduce(P, F, B, S1, count, max_lag, cd)
    W = x.shape[2]
    print("rel diff rhat %.3e ess %.3e" % (diag_ref.rel_diff(got[0], want[0]), diag_ref.rel_diff(got[1], want[1])))
    assert np.array_equal(got[2], want[2])
    assert diag_ref.rel_diff(got[0], want[0]) <= TOL
    assert diag_ref.rel_diff(got[1], want[1]) <= TOL
    # the constant column: NaN, NaN, -1
    assert math.isnan(got[0][3]) and math.isnan(got[1][3]) and got[2][3] == -1
    if not scalars:
        assert np.isnan(got[0][W:]).all() and np.isnan(got[1][W:]).all() and (got[2][W:] == -1).all()
    if max_lag == 2:   # a single pair, never compared with zero: the lags run out
        assert (got[2] == -1).all()


def test_alternating_column_has_negative_rho1():
    x, _ = traces(12, 4, 80)
    P, F, B, S1 = diag_ref.moments(x, 0)
    _, ess, _ = analysis.diag_reduce(P, F, B, S1, 80, 0)
    assert ess[4] > 8 * 40   # more effective draws than draws: antithetic


@pytest.fixture(scope="module")
def anchor():
    phi, n_sel, count = 0.9, 8, 20000
    x = np.rint(ar1(np.random.RandomState(2021), phi, n_sel, count, 1000.0)).astype(np.int64)[:, :, None]
    assert np.abs(x).max() < 32768
    return phi, x, count


def test_anchor_ar1_ess_and_rhat(anchor):
    phi, x, count = anchor
    S, h = 2 * x.shape[0], count // 2
    P, F, B, S1 = diag_ref.moments(x, 200)
    expect = (1.0 - phi) / (1.0 + phi)
    for rhat, ess, cut in (diag_ref.reduce(P, F, B, S1, count, 200), analysis.diag_reduce(P, F, B, S1, count, 200)):
        print("anchor: ess/(S h) = %.5f (expected %.5f), rhat = %.5f, cut_lag = %d" % (ess[0] / (S * h), expect, rhat[0], cut[0]))
        assert 0.75 * expect <= ess[0] / (S * h) <= 1.25 * expect
        assert rhat[0] < 1.01


def test_anchor_shifted_chain_raises_rhat(anchor):
    phi, x, count = anchor
    y = x.copy()
    y[3] += int(round(3 * 1000.0 / math.sqrt(1.0 - phi * phi)))   # three standard deviations
    assert np.abs(y).max() < 32768
    P, F, B, S1 = diag_ref.moments(y, 200)
    assert diag_ref.reduce(P, F, B, S1, count, 200)[0][0] > 1.1
    assert analysis.diag_reduce(P, F, B, S1, count, 200)[0][0] > 1.1


def test_host_only_library_exports_and_refuses():
    """The fake-device library (no device layer, so no moment kernels) still links, exports the three diagnostics
    functions, and answers sr_diagnostics with SR_EUNSUPPORTED."""
    import os
    import subprocess
    import sys
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(sa.__file__)))
    subprocess.check_call(["make", "-s", "-C", pkg, "build/fake/libseriation.so"])
    code = ("import ctypes, numpy as np, seriation_amd as sa\n"
            "from seriation_amd import _lib as L\n"
            "lib = sa.lib()\n"
            "assert all(hasattr(lib, s) for s in ('sr_diagnostics', 'sr_session_diagnostics', 'sr_diag_reduce'))\n"
            "ds = sa.Dataset.parse(b'3 2\\n1 0\\n1 1\\n0 1\\n')\n"
            "rec = np.zeros((1, 8, 7), np.int16)\n"
            "out = L.sr_diag_out()\n"
            "print(lib.sr_diagnostics(ctypes.byref(ds.c), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), None, 1, 8, 0,"
            " ctypes.byref(out)))\n")
    env = dict(os.environ, SERIATION_LIB=os.path.join(pkg, "build", "fake", "libseriation.so"),
               PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == str(L.SR_EUNSUPPORTED), r.stdout + r.stderr


def test_argument_checks():
    lib = sa.lib()
    I64P, DBLP = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    W, n_sel = 2, 1
    z = np.zeros((2, 8, W), np.int64)
    s1 = np.zeros((2, W), np.int64)
    r, e = np.zeros(W + 3), np.zeros(W + 3)
    c = np.zeros(W + 3, np.int32)

    def reduce(count, max_lag, P=z):
        p = P.ctypes.data_as(I64P) if P is not None else None
        return lib.sr_diag_reduce(W, n_sel, count, max_lag, p, z.ctypes.data_as(I64P), z.ctypes.data_as(I64P),
                                  s1.ctypes.data_as(I64P), None, r.ctypes.data_as(DBLP), e.ctypes.data_as(DBLP),
                                  c.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))

    assert reduce(8, 0) == L.SR_OK
    assert reduce(8, 3) == L.SR_OK
    assert reduce(3, 0) == L.SR_EINVAL          # count = 3
    assert reduce(8, 4) == L.SR_EINVAL          # max_lag = h
    assert reduce(8, -1) == L.SR_EINVAL         # max_lag = -1
    assert reduce(8, 0, None) == L.SR_EINVAL    # NULL moments
    ds = sa.Dataset.parse(b"3 2\n1 0\n1 1\n0 1\n")
    rec = np.zeros((1, 8, 7), np.int16)
    out = L.sr_diag_out()
    assert lib.sr_diagnostics(ctypes.byref(ds.c), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), None, 0, 8, 0,
                              ctypes.byref(out)) == L.SR_EINVAL   # n_sel = 0
    assert lib.sr_session_diagnostics(None, None, 1, 0, 8, ctypes.byref(out)) == L.SR_EINVAL
