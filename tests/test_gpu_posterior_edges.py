"""The posterior kernel (csrc/sr_post.hip) at its edges, every f64 bit against oracle/om_script.py: the case matrix
of tests/post_cases.py -- output shapes that hit each edge of the 16 x 64 tile and cross it by one element, sample
streams of 1, 63, 64, 65, 128 and 129 rows, chain ends inside a 64-sample chunk, on its edge and 70 of them in two
chunks, a view of no rows, limits equal to the row index and one off it in every row tile, every int16, X of ones,
zeros, halves and with entries of 2, chains_selected unlike the number of chains and negative -- then every kind
requested alone, and a session's rows [first, first + 64) and [first, first + 65) with first > 0.
tests/test_posterior_edges_host.py shows (without a GPU) that these inputs tell a subtly wrong kernel from a right
one; tests/test_posterior_oracle.py checks om_script itself at the new edges."""
import os

import numpy as np
import pytest

import om_script
import post_cases
import seriation_amd as sa
from seriation_amd import analysis

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G10S10 = os.path.join(ROOT, "tests", "golden", "datasets", "g10s10.txt")


def same(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def script(rows, cs, X, N, M):
    return {"pair_order": om_script.pair_order_matrix(rows, cs, N, M),
            "alive": om_script.alive_sum(rows, cs, N, M),
            "false_alive": om_script.false_alive_sum(rows, cs, N, M),
            "false_ones": om_script.false_ones_sum(rows, cs, X, N, M),
            "exp_pi": om_script.exp_pi(rows, N, cs, M),
            "exp_a": om_script.exp_a(rows, cs, M)}


_RUN = {}


def run_case(case):
    """One all-kinds GPU call and one om_script reference per case, shared by the tests."""
    if case not in _RUN:
        rec, X = post_cases.build(case)
        ds = sa.Dataset(X, np.zeros(case.N, bool))
        got = analysis.posterior_from_records(ds, rec, case.cs)
        _RUN[case] = (ds, rec, got, script(post_cases.chain_rows(rec), case.cs, X, case.N, case.M))
    return _RUN[case]


@pytest.mark.parametrize("case", post_cases.CASES, ids=post_cases.case_id)
def test_posterior_edge_case(case):
    _, _, got, want = run_case(case)
    bad = [k for k in analysis.KINDS if not same(got[k], want[k])]
    assert not bad, bad


ALONE = post_cases.Case("limits", 17, 65, 5, 13, 8, "twos")


@pytest.mark.parametrize("kind", analysis.KINDS)
def test_each_kind_alone(kind):
    """kinds=(k,) leaves the other outputs NULL: the same bits as the all-kinds call, and the script's."""
    ds, rec, all_kinds, want = run_case(ALONE)
    got = analysis.posterior_from_records(ds, rec, ALONE.cs, kinds=(kind,))
    assert set(got) == {kind, "kernel_ms"}
    assert same(got[kind], all_kinds[kind]) and same(got[kind], want[kind])


@pytest.fixture(scope="module")
def session_rows():
    """a short g10s10 session: 4 chains, 75 saved rows (capacity 100), every chain's rows on the host"""
    ds = sa.Dataset.parse(open(G10S10, "rb").read())
    with sa.Session(ds, [5, 9, 13, 21]) as s:
        s.run(3)
        s.run(75, save=True)
        ab, _ = s.fetch_records()
        yield ds, s, ab


@pytest.mark.parametrize("first,count", [(7, 64), (7, 65), (10, 65), (75, 0)])
def test_session_rows_against_script(session_rows, first, count):
    """sr_session_posterior over rows [first, first + count), first > 0, the selection out of order: one chunk
    exactly and one row more, up to the last saved row, and no rows at the end of the buffer -- against om_script on
    the same rows as fetched (tests/test_gpu_recview.py compares the two GPU forms with each other only)."""
    ds, s, ab = session_rows
    sel, cs = [2, 0, 3], 8
    got = analysis.posterior_from_session(s, sel, cs, first=first, count=count)
    rows = [ab[k, first:first + count].astype(np.int64) for k in sel]
    want = script(rows, cs, ds.X, ds.N, ds.M)
    bad = [k for k in analysis.KINDS if not same(got[k], want[k])]
    assert not bad, bad
