"""The one-wave mcmc_logl sum and the trimmed pass 1 of the Gibbs draw against the CPU oracle, bit for bit.

The one-workgroup LDS-column kernels sum mcmc_logl's terms (mcmc.c:639-645) in thread 0 alone, 16 terms per
block of reads with a guarded tail, and the shape-specialised 9-word kernels skip pass 1 of draw_fast_s for the
walk words that can never hold a whole walk byte (word 8 below N = 263).  Each case here runs 2 chains x 4 saved
calls from init (young chains accept moves in nearly every sweep, so loglik += delta follows the sum) at
sweeps_per_call = 1 (every sweep is a logl sweep), on the specialised kernel and on the generic one, and compares
a, b, pi and c, d, loglik (as uint64) with the oracle:

  - sum tails: N = 40 with M covering every remainder of 4-, 8-, 16- and 64-term blocks, fewer taxa than a
    wave, and waves without taxa;
  - the word-count boundary of the 9-word family: N = 255 .. 287 (262 | 263: 8 | 9 words with whole bytes);
    the oracle's records must contain full-length walks (b == N, a == 0), else the case proves nothing;
  - the 17-word family (its pass 1 is unchanged) at N = 512 .. 543, with the same condition;
  - depth: the bench's 256 x 512 dataset, 4 chains x (20 + 20) calls at 10 sweeps per call, the sum and its
    deltas carried across launches by the bench's own kernel.
"""
import functools
import os

import numpy as np
import pytest

import oracle_ref
import seriation_amd as sa
from test_gpu_edge import make_text

pytestmark = pytest.mark.gpu

NH = 3
SEEDS = [7, 8]
TAIL_M = [2, 3, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129]
WALK9_N = [255, 256, 257, 262, 263, 287]
WALK17_N = [512, 519, 520, 543]
WALK_M = 130
# (N, M) of every case; the walk cases must reach the full-length walk in the oracle's records
TAILS = [(40, M) for M in TAIL_M]
WALKS = [(N, WALK_M) for N in WALK9_N + WALK17_N]


def lds_shapes():
    """(N, M, nh, block_threads) of the shapes here (__graft_entry__.prewarm compiles their specialised kernels
    ahead, so the GPU box loads them instead of compiling at session creation)."""
    return [(N, M, NH, 0) for N, M in TAILS + WALKS]


def data_seed(N, M):
    return 4242 + N + M


@functools.lru_cache(maxsize=None)
def case(N, M):
    """The case's dataset text and the oracle's records of its chains (computed once, shared by both kernels)."""
    text = make_text(N, M, NH, seed=data_seed(N, M))
    orc = [oracle_ref.run_chain(text, s, 0, 4, sweeps=1, maxs=0) for s in SEEDS]
    for o in orc:
        assert o["rc"] == 0
    return text, orc


def check(N, M, generic):
    text, orc = case(N, M)
    ds = sa.Dataset.parse(text, maxs=0)
    with sa.Session(ds, SEEDS, sweeps_per_call=1, generic=generic) as s:
        assert s.variant == "lds"
        assert s.specialized == (not generic)
    summ, (ri, rd) = sa.run_chains(ds, SEEDS, burnin_calls=0, sample_calls=4, sweeps_per_call=1, keep_records=True,
                                   generic=generic)
    for k, o in enumerate(orc):
        np.testing.assert_array_equal(ri[k], o["rec_int"], err_msg="N %d M %d seed %d" % (N, M, SEEDS[k]))
        assert np.array_equal(rd[k].view(np.uint64), o["rec_dbl"].view(np.uint64)), (N, M, SEEDS[k])
        assert summ[k]["consistent"] == 0


@pytest.mark.parametrize("generic", [False, True], ids=["spec", "generic"])
@pytest.mark.parametrize("M", TAIL_M)
def test_logl_sum_tails(M, generic):
    check(40, M, generic)


@pytest.mark.parametrize("generic", [False, True], ids=["spec", "generic"])
@pytest.mark.parametrize("N", WALK9_N + WALK17_N)
def test_walk_word_boundary(N, generic):
    _, orc = case(N, WALK_M)
    rec = np.concatenate([o["rec_int"] for o in orc])
    full_b = int((rec[:, WALK_M:2 * WALK_M] == N).sum())
    full_a = int((rec[:, :WALK_M] == 0).sum())
    print("N %d: oracle records with b == N %d, a == 0 %d" % (N, full_b, full_a))
    assert full_b > 0 and full_a > 0   # the full-length walk L = N occurs in both directions
    check(N, WALK_M, generic)


def test_bench_kernel_depth():
    """256 x 512 (the bench's dataset and embedded kernel): 4 chains x (20 burn-in + 20 saved) calls of 10 sweeps."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datasets", "synth_256x512.txt")
    with open(path, "rb") as fh:
        text = fh.read()
    ds = sa.Dataset.parse(text, maxs=0)
    seeds = [1, 2, 3, 4]
    with sa.Session(ds, seeds) as s:
        assert s.variant == "lds" and s.specialized and s.block_threads == 512
    summ, (ri, rd) = sa.run_chains(ds, seeds, burnin_calls=20, sample_calls=20, keep_records=True)
    for k, sd in enumerate(seeds):
        o = oracle_ref.run_chain(text, sd, 20, 20, maxs=0)
        assert o["rc"] == 0
        np.testing.assert_array_equal(ri[k], o["rec_int"], err_msg="seed %d" % sd)
        assert np.array_equal(rd[k].view(np.uint64), o["rec_dbl"].view(np.uint64)), sd
        assert summ[k]["consistent"] == 0
