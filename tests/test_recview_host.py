"""The view of a session selection (csrc/sr_host.c's session_view), which all six sr_session_* analyses go through:
a selection outside the saved rows or the session's chains is SR_EINVAL in every family -- first + count beyond
int32 included, which must neither wrap nor trap -- and a valid one is SR_EUNSUPPORTED on the host-only library, which
has no analysis kernels.  CPU only: one child process on build/fake/libseriation.so, one fake session with 8 saved
rows.  The selections' results on a GPU are in tests/test_gpu_recview.py."""
import json
import os
import subprocess
import sys

import pytest

import seriation_amd as sa
from seriation_amd import _lib as L

FAMILIES = ("posterior", "diagnostics", "marginals", "relations", "waic", "agreement")
NCHAINS, NREC = 3, 8
INT32_MAX = 2 ** 31 - 1
# name: (chains, first, count, expected code)
CASES = {
    "chain -1": ([2, -1], 2, 6, L.SR_EINVAL),
    "chain nchains": ([0, NCHAINS], 2, 6, L.SR_EINVAL),
    "first -1": ([2, 0], -1, 6, L.SR_EINVAL),
    "one row past nrec": ([2, 0], 3, NREC - 3 + 1, L.SR_EINVAL),
    # one chain, so that n_sel * count < 2^31 and every family gets as far as the range check
    "first + count overflows": ([1], INT32_MAX, INT32_MAX, L.SR_EINVAL),
    "valid": ([2, 0, 2], 2, 6, L.SR_EUNSUPPORTED),
}

CHILD = r"""
import ctypes, json, sys
import numpy as np
import seriation_amd as sa
from seriation_amd import _lib as L
families, cases, nchains, nrec = json.loads(sys.argv[1])
lib = sa.lib()
ds = sa.Dataset.parse(b'4 3\n1 0 1\n1 1 0\n0 1 1\n1 1 1\n')
s = sa.Session(ds, list(range(1, nchains + 1)))
s.run(nrec, save=True)
assert lib.sr_session_records(s.h) == nrec
res = {}
for fam in families:
    for name, (chains, first, count, _want) in cases.items():
        ch = (ctypes.c_int32 * len(chains))(*chains)
        out = getattr(L, {'posterior': 'sr_posterior_out', 'diagnostics': 'sr_diag_out', 'marginals': 'sr_marg_out',
                          'relations': 'sr_rel_out', 'waic': 'sr_waic_out', 'agreement': 'sr_agree_out'}[fam])()
        keep = np.zeros(ds.N)
        args = [s.h, ch, len(chains), first, count]
        if fam == 'posterior':
            out.exp_pi = keep.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
            args.append(1)   # chains_selected
        res[fam + '/' + name] = getattr(lib, 'sr_session_' + fam)(*args, ctypes.byref(out))
        assert not keep.any()
print(json.dumps(res))
"""


@pytest.fixture(scope="module")
def codes():
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(sa.__file__)))
    subprocess.check_call(["make", "-s", "-C", pkg, "build/fake/libseriation.so"])
    env = dict(os.environ, SERIATION_LIB=os.path.join(pkg, "build", "fake", "libseriation.so"),
               PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps([FAMILIES, CASES, NCHAINS, NREC])], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr   # a trap on the overflow pair ends the child here
    return json.loads(r.stdout.splitlines()[-1])


@pytest.mark.parametrize("family", FAMILIES)
def test_session_selection_checks(codes, family):
    for name, (_chains, _first, _count, want) in CASES.items():
        assert codes[family + "/" + name] == want, (family, name, codes[family + "/" + name])
