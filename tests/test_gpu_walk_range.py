"""The 9-word Gibbs walks without a window (draw_fast_s<9>, csrc/sr_device.hip), on the device.

The walk sums every word from y = 1 at walk entry 0; tests/test_walk_range_host.py states why that is sound and
checks a host model of it.  Here the device function itself runs, through the certification self-test hook, on the
columns that take the chain to the ends of its range (tests/walk_range_cases.py) at the largest 9-word shape (N = 287)
and at N = 256, and on walks that end on the boundaries of pass 1's cases: L = 262 / 263 (word 8 holds its first whole
byte from L = 263: the specialised kernels' table trim), 31 / 32 (one word / two words), 7 (a partial byte only);
forward and reversed.  Every pick and its count deltas equal the oracle's, certified or not.  Then the sweep kernels,
generic and specialised, on two small steep datasets against the oracle's chains, with equal fallback counters.
"""
import numpy as np
import pytest

import cert_cases
import cert_run
import oracle_ref
import seriation_amd as sa
import walk_range_cases as wr
from test_gpu_edge import make_text

pytestmark = pytest.mark.gpu

ENDS = (262, 263, 31, 32, 7)


def _check(cs):
    out, fb = cert_run.run_gibbs(sa.lib(), 0, cs)
    N = cs["N"]
    wrong = np.nonzero(out[:, 0] != cs["expected"])[0]
    print("N=%d cases=%d certified=%d wrong=%d" % (N, cs["n"], int((fb == 0).sum()), len(wrong)))
    assert len(wrong) == 0, [(cs["walk"][k], float(cs["u"][k]).hex(), int(out[k, 0]), int(cs["expected"][k]),
                              bool(fb[k] == 0)) for k in wrong[:5]]
    for k in range(cs["n"]):
        want = cert_cases.pick_counts(cs["cols"][cs["cidx"][k]], N, bool(cs["rev"][k]), int(cs["o"][k]), int(out[k, 0]))
        assert tuple(int(v) for v in out[k, 1:]) == want, (cs["walk"][k], k)


@pytest.mark.parametrize("N", [287, 256])
def test_extreme_columns(N):
    _check(wr.extreme_cases(N, both_directions=True))


@pytest.mark.parametrize("N", [287, 256])
def test_walk_ends(N):
    _check(wr.build(N, wr.end_walks(N, ENDS, seed=N), revs=(False, True)))


@pytest.mark.parametrize("N,M", [(287, 64), (40, 70)])
def test_steep_chain_parity_generic_and_specialised(N, M):
    text = make_text(N, M, 5, seed=N * 7 + M, density=0.34, noise=0.003)   # as test_gpu_edge.test_steep_walks
    ds = sa.Dataset.parse(text, maxs=0)
    seeds = [4, 19]
    oracle = [oracle_ref.run_chain(text, s, 2, 3, maxs=0) for s in seeds]
    fallbacks = {}
    for generic in (True, False):
        with sa.Session(ds, seeds, generic=generic) as s:
            assert s.specialized == (not generic)
            s.run(2, save=False)
            s.run(3, save=True)
            ri, rd = s.fetch_records()
            fallbacks[generic] = np.array([s.fallback_counts(k) for k in range(len(seeds))])
        for k, o in enumerate(oracle):
            assert o["rc"] == 0
            np.testing.assert_array_equal(ri[k], o["rec_int"], err_msg="generic=%s seed %d" % (generic, seeds[k]))
            assert np.array_equal(rd[k].view(np.uint64), o["rec_dbl"].view(np.uint64)), (generic, seeds[k])
    np.testing.assert_array_equal(fallbacks[True], fallbacks[False])
