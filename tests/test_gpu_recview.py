"""The record view (csrc/sr_records.h) under all six analyses: a session selection out of order and with a repeat,
[2, 0, 2], rows [3, 39) of 40 saved ones -- so the session's row capacity is not the count, the first row is not 0
and chains[k] is not k -- must give, bit for bit, what the host form gives on the same rows fetched with
sr_session_fetch_chain_records.  Every output of every family is requested."""
import os
import struct

import numpy as np
import pytest

import seriation_amd as sa
from seriation_amd import analysis

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G10S10 = os.path.join(ROOT, "tests", "golden", "datasets", "g10s10.txt")   # the smallest committed dataset
SEL, FIRST, COUNT, SAVED = [2, 0, 2], 3, 36, 40
FLIPS = [0, 1, 0]


def same_bits(a, b, path=""):
    """Two results of one analysis, equal to the bit: dicts key by key (kernel_ms apart), arrays by dtype, shape and
    bytes (so NaNs and signed zeros count), floats by their 8 bytes."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), path
        for k in a:
            if k != "kernel_ms":
                same_bits(a[k], b[k], path + "/" + str(k))
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, path
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), path
    elif isinstance(a, float):
        assert struct.pack("<d", a) == struct.pack("<d", b), path
    else:
        assert a == b, path


@pytest.fixture(scope="module")
def sampled():
    """(dataset, session with 40 saved rows, the selection's rows ab_pi [3][36][2M+N] and cdl [3][36][3])"""
    ds = sa.Dataset.parse(open(G10S10, "rb").read())
    with sa.Session(ds, [1, 2, 3, 4]) as s:
        s.run(20)
        s.reset_records()
        s.run(SAVED, save=True)
        assert analysis.session_records(s) == SAVED and s.record_capacity != COUNT
        rows = [s.fetch_chain_records(c, FIRST, COUNT) for c in SEL]
        ab, cdl = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
        assert ab.shape == (3, COUNT, 2 * ds.M + ds.N) and not np.array_equal(ab[0], ab[1])
        yield ds, s, ab, cdl


def test_posterior(sampled):
    ds, s, ab, _ = sampled
    got = analysis.posterior_from_session(s, SEL, 3, first=FIRST, count=COUNT)
    assert set(analysis.KINDS) <= got.keys()
    same_bits(got, analysis.posterior_from_records(ds, ab, 3))


def test_diagnostics(sampled):
    ds, s, ab, cdl = sampled
    got = analysis.diagnostics_from_session(s, SEL, first=FIRST, count=COUNT, moments=True)
    assert {"rhat", "ess", "cut_lag", "P", "F", "B", "S1"} <= got.keys()
    same_bits(got, analysis.diagnostics_from_records(ds, ab, cdl, moments=True))


def test_marginals(sampled):
    ds, s, ab, _ = sampled
    got = analysis.marginals_from_session(s, SEL, first=FIRST, count=COUNT, flips=FLIPS, hist=True)
    assert {"quant", "mode", "mean", "outside", "pi_sum", "hist"} <= got.keys()
    same_bits(got, analysis.marginals_from_records(ds, ab, flips=FLIPS, hist=True))


def test_relations(sampled):
    ds, s, ab, _ = sampled
    got = analysis.relations_from_session(s, SEL, first=FIRST, count=COUNT, flips=FLIPS)
    assert set(analysis.REL_KINDS) <= got.keys()
    same_bits(got, analysis.relations_from_records(ds, ab, flips=FLIPS))


def test_waic(sampled):
    ds, s, ab, cdl = sampled
    got = analysis.waic_from_session(s, SEL, first=FIRST, count=COUNT, pointwise=True)
    assert {"lppd", "ll_mean", "pwaic", "site_elpd", "taxon_elpd", "elpd_waic", "se"} <= got.keys()
    same_bits(got, analysis.waic_from_records(ds, ab, cdl, pointwise=True))


def test_agreement(sampled):
    ds, s, ab, _ = sampled
    got = analysis.agreement_from_session(s, SEL, first=FIRST, count=COUNT, pair_counts=True)
    assert {"pair_counts", "dist", "dist_mirror", "scale"} <= got.keys()
    same_bits(got, analysis.agreement_from_records(ds, ab, pair_counts=True))
