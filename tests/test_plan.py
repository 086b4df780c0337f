"""Every shape the C ABI accepts has a sweep kernel (CPU test: srk_plan, the library's own kernel choice, needs no
GPU).  Round 5 found sessions of more than ~1250 sites and more than 512 taxa without one: the HBM-column kernels
at 1024 threads kept 16 per-wave copies of the hard-site tables (64 N bytes of LDS); they share one copy now.
The only refusals are the documented ones: N > 4095, hard sites > N, and manycd below 1024 threads."""
import ctypes
import os
import subprocess
import sys

import pytest

from seriation_amd import _lib as L

SITES = (2, 64, 256, 287, 288, 543, 600, 1024, 1250, 1300, 1700, 2000, 2500, 3000, 4000, 4095)
TAXA = (1, 100, 256, 512, 513, 1024, 1025, 1100, 2048, 2049, 5000, 40000)


def _plan():
    f = L.lib().srk_plan
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p]
    return f


@pytest.mark.parametrize("manycd", [0, 1])
def test_every_shape_has_a_kernel(manycd):
    f = _plan()
    buf = ctypes.create_string_buffer(512)
    missing = []
    for N in SITES:
        for M in TAXA:
            for nh in (0, 12, 64, 65, 200):
                if nh > N:
                    continue
                for tb in ((0, 1024) if manycd else (0, 256, 512, 1024)):
                    if f(N, M, nh, tb, -1, manycd, buf) < 0:
                        missing.append((N, M, nh, tb))
    assert not missing, missing[:10]


_PLAN_CHILD = """
import ctypes
from seriation_amd import _lib as L
f = L.lib().srk_plan
f.restype = ctypes.c_int
f.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p]
shape = (ctypes.c_int * 6)()   # sr_spec_shape: TB, NWM, N, M, NH, force
print(f(256, 512, 12, 0, -1, 0, shape), shape[0], shape[1])
"""


def test_kernel_choice_ignores_the_retired_pair_switch():
    """SR_KERNEL is no longer read: with SR_KERNEL=pair in the environment (it once selected the retired pair kernel,
    which had no specialised form: srk_plan returned 0) the bench shape plans what it plans with it unset -- the
    specialised 512-thread kernel with 9 walk words.  A child process: the variable is set before the library plans."""
    env = dict(os.environ, SR_KERNEL="pair",
               PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.dirname(os.path.abspath(L.__file__)))] +
                                          [p for p in [os.environ.get("PYTHONPATH")] if p]))
    out = subprocess.run([sys.executable, "-c", _PLAN_CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["1", "512", "9"], out.stdout


def test_documented_refusals():
    f = _plan()
    buf = ctypes.create_string_buffer(512)
    assert f(4096, 512, 0, 0, -1, 0, buf) == L.SR_EUNSUPPORTED
    assert f(100, 512, 101, 0, -1, 0, buf) == L.SR_EUNSUPPORTED
    assert f(256, 512, 12, 512, -1, 1, buf) == L.SR_EUNSUPPORTED   # manycd: 1024 threads only
