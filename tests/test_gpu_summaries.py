"""Two pieces of device code on the path every run ends with, against independent values:

* sr_exp_data_kernel (sr_session_summaries, csrc/sr_device.hip): each chain's exp_data sums over record rows
  [first, first + count), taken in chunks of 1024 rows that thread 0 adds in row order -- at the chunk edges
  (count 1023, 1024, 1025, 2048, 2049), from a first row other than 0 and over no rows, against the sums in plain
  Python floats (math.exp is the C library's, bit-equal to the device's sr_exp_m: tests/test_host.py);
* sr_session_copy_chain_records: the device-to-device copies that gather the selected chains, into torch tensors on
  the GPU, against sr_session_fetch_chain_records of the same rows, with a guard row behind every destination."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import copy_records_child as child   # (importing it touches no GPU)
import seriation_amd as sa
from seriation_amd import _lib as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DS = os.path.join(ROOT, "tests", "golden", "datasets")
SAVED = 2049            # two full chunks of sr_exp_data_kernel and one row; the record capacity has no upper bound
CHAIN_IDS = [7, 100, 3]


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def long_session():
    """g2s2, three chains, one sweep per call, 2049 saved calls in a buffer of 2049 rows; cdl fetched once"""
    ds = sa.Dataset.load(os.path.join(DS, "g2s2.txt"))
    with sa.Session(ds, [11, 12, 13], sweeps_per_call=1, calls_per_launch=SAVED, chain_ids=CHAIN_IDS) as s:
        assert s.record_capacity == SAVED
        s.run(SAVED, save=True)
        ab, cdl = s.fetch_records()
        assert cdl.shape == (3, SAVED, 3) and len(np.unique(cdl[:, :, 2])) > 100
        yield s, ab, cdl


def reference(cdl, first, count):
    """compute_exp_data / print_exp_data (mcmc.c:53-67) in Python floats: from +0.0, in row order"""
    out = []
    for k in range(cdl.shape[0]):
        ls = cs = ds = 0.0
        for c, d, loglik in cdl[k, first:first + count].tolist():
            ls += -loglik
            cs += math.exp(c)
            ds += math.exp(d)
        out.append([float(CHAIN_IDS[k]), ls / 1000, cs / 1000, ds / 1000])
    return np.array(out, np.float64)


RANGES = [(0, 2049), (0, 2048), (0, 1025), (0, 1024), (0, 1023), (0, 1), (1, 1024), (1025, 1024), (2048, 1), (7, 0)]


@pytest.mark.parametrize("first,count", RANGES)
def test_summaries_at_chunk_edges(long_session, first, count):
    s, _, cdl = long_session
    got = s.summaries(first, count)
    want = reference(cdl, first, count)
    assert got.shape == (3, 4) and np.array_equal(bits(got), bits(want)), (got, want)
    if count == 0:
        assert np.array_equal(bits(got[:, 1:]), np.zeros((3, 3), np.uint64))   # +0.0, not -0.0


def test_summaries_refusals_and_session_untouched(long_session):
    s, ab, cdl = long_session
    for first, count in [(0, SAVED + 1), (1, SAVED), (SAVED, 1), (SAVED + 1, 0), (-1, 1), (-1, 0), (0, -1),
                         (5, -5)]:
        with pytest.raises(L.SrError) as e:
            s.summaries(first, count)
        assert e.value.code == L.SR_EINVAL, (first, count)
    assert s.summaries(SAVED, 0).shape == (3, 4)   # no rows at the end of the buffer: allowed
    ab2, cdl2 = s.fetch_records()
    assert np.array_equal(ab, ab2) and np.array_equal(bits(cdl), bits(cdl2))


# ---- sr_session_copy_chain_records (tests/copy_records_child.py)
@pytest.fixture(scope="module")
def copies():
    """one child process for all cases: torch must initialise the GPU before the library does"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "copy_records_child.py")], capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("name", [child.case_name(c) for c in child.CASES])
def test_copy_chain_records_on_device(copies, name):
    """after the stream is drained the copied bytes equal sr_session_fetch_chain_records of the same rows (NULL
    skips an array) and the row behind them still holds the guard value"""
    assert copies["cases"][name] == []


def test_copy_chain_records_refusals(copies):
    assert copies["refusals"] == []
