"""Stream injection -- TEST INFRASTRUCTURE (tests/test_stream_inject_host.py, tests/test_gpu_stream_inject.py).

A checkpoint carries every chain's MT19937 ring (mt [8][624], raw words) and cursor (rng: pos, gen), and
sr_session_restore does not constrain the ring words.  The CPU oracle's generator is one block mt[624] + mti.  So a
test can put any tempered word at any stream offset on both sides: untemper(value) into the resident block of the
checkpoint with the cursor at the block's start, and the same block with mti = 0 into oracle_run_chain_mt.  The
sampler's paths that speculate on the random stream (proposal tables and phase C's scan: no uniform_int rejects, no
zero uniform_pos word; draw_cd_fast: two words per gamma) then meet the words that break their hypotheses, which
seeded chains almost never draw.

This module holds the checkpoint layout (one copy, shared with tests/test_abi.py), the case builder and the oracle
side; the GPU side is in tests/test_gpu_stream_inject.py."""
import ctypes

import numpy as np

import oracle_ref
from seriation_amd import _lib as L

RING, MT_N, NACC, HEADER = 8, 624, 10, 40   # sr_internal.h: SR_RING, SR_MT_N, SR_NACC; the version-7 / 8 file header


def nhcap(nh):
    """sr_internal.h's SR_NHCAP: hard positions kept per chain (64, or nh rounded up to whole waves beyond)."""
    return 64 if nh <= 64 else (nh + 63) & ~63


def ck_layout(N, M, nh, C, manycd=False):
    """Byte offset of every part of a checkpoint's chain state (sr_host.c's ck_parts, after the header and the C
    chain specs) and the offset of its end (where the buffered records start): ({name: offset}, end)."""
    NW = (N + 31) // 32
    sizes = [("P", C * NW * M * 4), ("rpi", C * N * 4), ("hp", C * nhcap(nh) * 4), ("ab", C * 2 * M * 4),
             ("cnt", C * 4 * M * 4), ("cdl", C * 4 * 8), ("mt", C * RING * MT_N * 4), ("rng", C * 2 * 8),
             ("acc", C * NACC * 8)]
    if manycd:
        sizes.append(("cdv", C * 2 * M * 8))
    off = HEADER + C * ctypes.sizeof(L.sr_chain_spec)
    base = {}
    for name, n in sizes:
        base[name] = off
        off += n
    return base, off


def untemper(values):
    """The raw MT19937 words whose tempering gives `values` (sr_host_mt_untemper), checked to round-trip."""
    v = np.ascontiguousarray(values, np.uint32)
    raw = np.zeros_like(v)
    back = np.zeros_like(v)
    P = ctypes.POINTER(ctypes.c_uint32)
    L.lib().sr_host_mt_untemper(v.ctypes.data_as(P), v.size, raw.ctypes.data_as(P), back.ctypes.data_as(P))
    assert np.array_equal(back, v)
    return raw


def temper(raw):
    """MT19937's tempering (numpy restatement of the published shifts and masks)."""
    k = np.array(raw, np.uint32)
    k ^= k >> 11
    k ^= (k << 7) & np.uint32(0x9d2c5680)
    k ^= (k << 15) & np.uint32(0xefc60000)
    k ^= k >> 18
    return k


# ---------------------------------------------------------------------------------------------------- cases
FF, ZERO, WEDGE = 0xffffffff, 0, 0xffffff85
# per-taxon leg: (j << 8) | i, negative deviates (sign bit 0x80 clear) in strips 0x7e, 0x7c, 0x78 with j large
# enough for 1 + c x <= 0 at shape 1
NEG_TAIL = tuple((j << 8) | i for i in (0x7e, 0x7c, 0x78) for j in (0xf00000, 0xc00000))


def boundary_values(N, nh):
    """For each divisor n the sampler's uniform_int calls use, with s = 0xffffffff // n: the first rejected word
    n s and the last accepted word n s - 1 (clipped to 32 bits: n = 1 rejects only 0xffffffff)."""
    out = []
    for n in (N, N - 1, N - nh, N - nh - 1, 2):
        n = max(n, 1)   # (the sampler's own clamp: make_udivm(1) where N - nh - 1 < 1)
        s = 0xffffffff // n
        out += [min(n * s, 0xffffffff), min(n * s, 0xffffffff) - 1]
    return out


def single_values(N, nh, neg_tail=False):
    """The single-word values of a leg, in a fixed order without repeats."""
    vals = [FF, ZERO] + boundary_values(N, nh) + [WEDGE] + (list(NEG_TAIL) if neg_tail else [])
    return list(dict.fromkeys(vals))


RUNS = ((FF, 2), (FF, 3), (ZERO, 2), (ZERO, 3))   # consecutive equal words: a redraw that rejects again


def build_cases(w1, values, runs=RUNS):
    """Every offset 0 .. w1 + 7 with each value and each run: [(label, [(offset, value), ...]), ...] where label =
    (value, run length, offset)."""
    cases = []
    for v in values:
        for off in range(w1 + 8):
            cases.append(((v, 1, off), [(off, v)]))
    for v, n in runs:
        for off in range(w1 + 8):
            cases.append(((v, n, off), [(off + k, v) for k in range(n)]))
    return cases


# ---------------------------------------------------------------------------------------------------- oracle side
class Base:
    """The unpatched chain of a leg: its resident block after mcmc_randomize (raw words), and sweep 1's word and
    event counts from that block's start."""

    def __init__(self, text, seed, manycd=0):
        self.text, self.seed, self.manycd = text, seed, manycd
        rc, X, h = oracle_ref.parse(text, 0)
        assert rc == 0
        self.N, self.M = X.shape
        self.nh = int(np.count_nonzero(h))
        o = oracle_ref.run_chain_mt(text, seed, ts=0, manycd=manycd, shape=X.shape)
        self.block, self.mti0 = o["mt0"], o["mti0"]
        s1 = self.run([], ts=1, sweeps=1)
        assert s1["rc"] == 0
        self.w1, self.ev1 = s1["words"], s1["ev"]
        assert self.w1 + 8 + 3 <= MT_N   # every patched offset lies inside the resident block

    def patched(self, patch):
        blk = self.block.copy()
        if patch:
            offs = np.array([o for o, _ in patch])
            blk[offs] = untemper([v for _, v in patch])
        return blk

    def run(self, patch, ts=1, sweeps=2, ok_ignored=False):
        """The oracle from the block's start (mti = 0) with `patch` = [(offset, tempered value), ...] applied."""
        return oracle_ref.run_chain_mt(self.text, self.seed, self.patched(patch), 0, ts=ts, sweeps=sweeps,
                                       manycd=self.manycd, shape=(self.N, self.M), ok_ignored=ok_ignored)


def same_run(a, b):
    """Two oracle runs gave the same records, counters and words consumed."""
    return (np.array_equal(a["rec_int"], b["rec_int"]) and
            np.array_equal(a["rec_dbl"].view(np.uint64), b["rec_dbl"].view(np.uint64)) and
            np.array_equal(a["acc"], b["acc"]) and a["words"] == b["words"] and
            ("rec_cdv" not in a or np.array_equal(a["rec_cdv"].view(np.uint64), b["rec_cdv"].view(np.uint64))))


def coverage(base, cases, runs):
    """The coverage conditions of a leg, from the oracle's counters alone (runs[k] = the oracle's run of cases[k]):
    the 0xffffffff scan rejects at least once per uniform_int call of the base sweep, the 0 scan retries at least
    once per uniform_pos call of it.  Returns the event totals over the cases (require_events asserts the rest:
    wedge, tail, ziggurat rejection and gamma rejection each occur; on the per-taxon leg v <= 0 and Johnk's branch
    too) and the two scans' counts."""
    tot = {k: 0 for k in oracle_ref.EVENTS}
    scan = {FF: 0, ZERO: 0}
    for (label, _), r in zip(cases, runs):
        for k in tot:
            tot[k] += r["ev"][k]
        v, n, _ = label
        if n == 1 and v == FF:
            scan[FF] += r["ev"]["uint_reject"]
        if n == 1 and v == ZERO:
            scan[ZERO] += r["ev"]["upos_retry"]
    labels = {(v, n) for (v, n, _), _ in cases}
    if (FF, 1) in labels:
        assert base.ev1["uint_calls"] >= 1 and scan[FF] >= base.ev1["uint_calls"], (scan, base.ev1)
    if (ZERO, 1) in labels:
        assert base.ev1["upos_calls"] >= 1 and scan[ZERO] >= base.ev1["upos_calls"], (scan, base.ev1)
    return tot, scan


def patches_matter(base, runs):
    """The injected words are words the chain really reads: most cases leave the base chain's records, counters or
    word count (so a comparison that passes has seen the patches, not the unpatched stream)."""
    plain = base.run([])
    moved = sum(not same_run(plain, r) for r in runs)
    assert 2 * moved > len(runs), (moved, len(runs))
    return moved


def require_events(tot, per_taxon=False):
    for k in ("zig_wedge", "zig_tail", "zig_reject", "gamma_reject") + (("gamma_vneg", "johnk") if per_taxon else ()):
        assert tot[k] >= 1, (k, tot)
