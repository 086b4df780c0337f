"""The one-phase form of an MT19937 block (csrc/sr_rng.h: sr_mt_block_word) -- CPU only.

The sweep kernels top their ring up with it: every word of block g + 1 from block g alone, in any order, with no
barrier between the recurrence's three dependency phases.  It must produce the sequential recurrence's block
(sr_mt_next_block), word for word; the sequential blocks themselves are pinned against numpy's MT19937, which is
seeded like GSL's (seed 0 -> 4357).  The hook sr_host_mt_block runs the header's own functions (the kernel compiles
the same text)."""
import ctypes

import numpy as np
import pytest

import seriation_amd as sa

MT_N = 624
NBLOCKS = 6
SEEDS = [0, 1, 2, 42, 4357, 2 ** 31 + 7, 2 ** 32 - 1]
# the recurrence's phase boundaries: [0, 227) reads the old block only, [227, 454) one new word, [454, 623) a new
# word that itself needed one, word 623 needs new words 0 and 396
EDGE_WORDS = [0, 226, 227, 453, 454, 622, 623]


def temper(w):
    w = w.astype(np.uint64)
    w ^= w >> np.uint64(11)
    w ^= (w << np.uint64(7)) & np.uint64(0x9d2c5680)
    w ^= (w << np.uint64(15)) & np.uint64(0xefc60000)
    w ^= w >> np.uint64(18)
    return w & np.uint64(0xffffffff)


def blocks(seed):
    P = ctypes.POINTER(ctypes.c_uint32)
    seq = np.zeros((NBLOCKS, MT_N), np.uint32)
    one = np.full((NBLOCKS, MT_N), 0xdeadbeef, np.uint32)
    assert sa.lib().sr_host_mt_block(seed, NBLOCKS, seq.ctypes.data_as(P), one.ctypes.data_as(P)) == 0
    return seq, one


@pytest.mark.parametrize("seed", SEEDS)
def test_one_phase_block_equals_the_recurrence(seed):
    seq, one = blocks(seed)
    for b in range(NBLOCKS):
        for k in EDGE_WORDS:
            assert int(one[b, k]) == int(seq[b, k]), "seed %d block %d word %d" % (seed, b + 1, k)
    np.testing.assert_array_equal(one, seq)


@pytest.mark.parametrize("seed", SEEDS)
def test_sequential_blocks_are_the_mt19937_stream(seed):
    seq, _ = blocks(seed)
    rs = np.random.RandomState(4357 if seed == 0 else seed)
    want = rs.randint(0, 2 ** 32, size=NBLOCKS * MT_N, dtype=np.uint64)
    np.testing.assert_array_equal(temper(seq.reshape(-1)), want)


def test_hook_rejects_bad_arguments():
    assert sa.lib().sr_host_mt_block(1, -1, None, None) != 0
    assert sa.lib().sr_host_mt_block(1, 1, None, None) != 0
