"""Crafted RNG words against the sampler's rare stream branches (GPU; helper and method: tests/stream_inject.py).

The sweep kernel's proposal tables and phase C's scan assume that no gsl_rng_uniform_int rejects and that the
uniform_pos word is nonzero, else the scalar path takes over at that proposal; draw_cd_fast assumes two words per
gamma, else d_samplebeta takes over.  Seeded chains draw the words that break those hypotheses about once per 1e7
proposals (a zero uniform_pos word: never).  Here every offset of the base chain's first sweep (and 8 beyond) gets each
of: 0xffffffff (every uniform_int rejects it; a ziggurat tail word), 0 (uniform_pos retry, u = 0, w1 == 0), the first
rejected and last accepted word of every divisor the sampler uses, a wedge word, and runs of 2 and 3 equal words --
one chain per case, restored from a checkpoint whose ring holds the untempered words, 1 saved call of 2 sweeps, and
every chain compared bit for bit with the oracle started from the same block: a, b, pi, c, d, loglik (per-taxon c, d
on the manycd leg), the 7 acceptance counters and the words consumed (the cursor after the run).  No case is skipped
or filtered.  The oracle's own event counters assert that the cases reach what they are written for.

The divider behind uniform_int (make_udivm / udivm / udivm_v, "exact for every 32-bit g") is checked separately on
every divisor 1..4095 at the words around every multiple of its scale.

If a case fails, its (leg, value, run length, offset) is in the assertion message; the oracle's counters for that
case (stream_inject.Base.run(patch)["ev"]) say which branch it took."""
import ctypes
import os

import numpy as np
import pytest

import oracle_ref
import seriation_amd as sa
import stream_inject as si
from seriation_amd import _lib as L
from test_gpu_edge import make_text

pytestmark = pytest.mark.gpu

TEXT_SEED, CHAIN_SEED = 11, 7

# name: N, M, nh, session options, expected (variant, kernel, specialized, block_threads, walk words or None),
# chains per session (0: the whole part in one), parts (the leg's values dealt over this many test cases)
LEGS = {
    "reg9": (40, 24, 3, {}, ("lds", "single", True, 256, 9), 0, 1),
    "reg9-generic": (40, 24, 3, {"generic": True}, ("lds", "single", False, 256, 9), 0, 1),
    "reg17": (300, 12, 9, {}, ("lds", "single", True, 256, 17), 0, 1),
    # more than 32 hard sites: 64-bit hard-site masks, which only the LDS-walk kernels carry (sr_regwalk)
    "nh33": (300, 12, 33, {}, ("lds", "single", True, 256, 0), 0, 1),
    "lds-walk": (560, 12, 5, {}, ("lds", "single", True, 256, 0), 0, 1),
    "two-sites": (2, 4, 0, {}, ("lds", "single", True, 256, 9), 0, 1),
    "hbm": (40, 24, 3, {"columns": "hbm"}, ("hbm", "single", False, 256, None), 0, 1),
    # two workgroups per chain, launched only while the whole grid is co-resident: 64 chains per session
    "split": (64, 160, 6, {"columns": "hbm", "block_threads": 1024}, ("hbm", "split", False, 1024, None), 64, 1),
    "per-taxon": (40, 24, 3, {"manycd": 1}, ("lds", "single", False, 1024, None), 0, 3),
}

_BASES = {}


def leg_base(name):
    """The leg's base chain and all its cases with the oracle's run of each (computed once per shape)."""
    N, M, nh, opts = LEGS[name][:4]
    manycd = opts.get("manycd", 0)
    key = (N, M, nh, manycd, name == "split")
    if key not in _BASES:
        base = si.Base(make_text(N, M, nh, seed=TEXT_SEED), CHAIN_SEED, manycd=manycd)
        # the split leg: 0xffffffff, 0 and the runs at every offset (the case count of all values makes ~20 sessions more)
        vals = [si.FF, si.ZERO] if name == "split" else si.single_values(N, nh, neg_tail=bool(manycd))
        cases = si.build_cases(base.w1, vals)
        runs = [base.run(p) for _, p in cases]
        _BASES[key] = (base, cases, runs)
    return _BASES[key]


def _plan_walk_words(N, M, nh):
    f = L.lib().srk_plan
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p]
    shape = (ctypes.c_int * 6)()   # sr_spec_shape: TB, NWM, N, M, NH, force
    assert f(N, M, nh, 0, -1, 0, shape) == 1
    return shape[1]


def run_session(name, base, ds, cases, tmp_path):
    """One restored session over `cases`: returns per chain (rec_int, rec_dbl, rec_cdv or None, acc10, words)."""
    N, M, nh, opts, want = LEGS[name][:5]
    manycd = opts.get("manycd", 0)
    C = len(cases)
    ck0, ck1, ck2 = (str(tmp_path / n) for n in ("base.srck", "patched.srck", "after.srck"))
    seeds = [CHAIN_SEED] * C
    if manycd:
        with sa.Session(ds, seeds, manycd=1, calls_per_launch=1) as s:
            s.checkpoint(ck0)
    else:   # the same file without a device
        assert L.lib().sr_host_initial_checkpoint(ctypes.byref(ds.c), sa.core.make_specs(seeds), C, os.fsencode(ck0)) == 0
    raw = bytearray(open(ck0, "rb").read())
    lay, end = si.ck_layout(N, M, nh, C, manycd=bool(manycd))
    assert len(raw) == end
    rng = np.frombuffer(raw, "<u8", 2 * C, lay["rng"]).reshape(C, 2)
    mt = np.frombuffer(raw, "<u4", C * si.RING * si.MT_N, lay["mt"]).reshape(C, si.RING, si.MT_N)
    start = np.zeros(C, np.uint64)
    for k, (_, patch) in enumerate(cases):
        pos, gen = int(rng[k, 0]), int(rng[k, 1])
        blk = pos // si.MT_N
        assert gen == blk + 1 and pos % si.MT_N == base.mti0
        slot = mt[k, blk % si.RING]
        assert np.array_equal(slot, base.block)   # the oracle's generator is this resident block
        rng[k, 0] = start[k] = blk * si.MT_N      # the cursor to the block's start
        slot[:] = base.patched(patch)
    with open(ck1, "wb") as fh:
        fh.write(raw)
    ropts = {k: v for k, v in opts.items()}
    with sa.Session.restore(ds, ck1, sweeps_per_call=2, calls_per_launch=1, **ropts) as s:
        assert s.n == C
        assert (s.variant, s.kernel, s.specialized, s.block_threads) == want[:4], name
        assert bool(s.manycd) == bool(manycd)
        s.run(1, save=True)
        ab, cdl = s.fetch_records()
        cdv = s.fetch_cd_vectors() if manycd else None
        s.checkpoint(ck2)
        probe = sorted({0, C // 2, C - 1})
        api = {k: np.concatenate([s.accept_counts(k), s.fallback_counts(k)]) for k in probe}
    after = open(ck2, "rb").read()
    W = 2 * M + N   # (the checkpoint after the run carries the one buffered record behind the state)
    assert len(after) == end + C * (W * 2 + 24 + (16 * M if manycd else 0))
    pos1 = np.frombuffer(after, "<u8", 2 * C, lay["rng"]).reshape(C, 2)[:, 0]
    acc = np.frombuffer(after, "<u8", si.NACC * C, lay["acc"]).reshape(C, si.NACC).astype(np.int64)
    for k, v in api.items():   # the file's counters are the ones the session API reports
        np.testing.assert_array_equal(acc[k], v)
    words = (pos1 - start).astype(np.int64)
    return [(ab[k, 0].astype(np.int32), cdl[k, 0], cdv[k, 0] if manycd else None, acc[k], int(words[k])) for k in range(C)]


def compare(name, label, got, ref):
    ri, rd, rv, acc, words = got
    assert ref["rc"] == 0, (name, label)
    np.testing.assert_array_equal(ri, ref["rec_int"][0], err_msg="%s %r: a, b, pi" % (name, label))
    assert np.array_equal(rd.view(np.uint64), ref["rec_dbl"][0].view(np.uint64)), (name, label, "c, d, loglik", rd, ref["rec_dbl"][0])
    if rv is not None:
        assert np.array_equal(rv.view(np.uint64), ref["rec_cdv"][0].view(np.uint64)), (name, label, "per-taxon c, d")
    np.testing.assert_array_equal(acc[:7], ref["acc"], err_msg="%s %r: acceptance counters" % (name, label))
    assert words == ref["words"], (name, label, "words consumed", words, ref["words"])


def cd_handover(name, base, label, acc):
    """draw_cd_fast handed over to the sequential draw where it must: a tail word at a gamma's ziggurat word, a zero
    at its uniform_pos word (the base chain's c / d draws took exactly 8 words: 4 gammas of 2)."""
    v, n, off = label
    if n == 1 and ((v == si.FF and off in (0, 2, 4, 6)) or (v == si.ZERO and off in (1, 3, 5, 7))):
        assert acc[9] >= 1, (name, label, "no sequential c/d draw counted")
        return 1
    return 0


LEG_PARTS = [(name, part) for name, leg in LEGS.items() for part in range(leg[6])]


@pytest.mark.parametrize("name,part", LEG_PARTS, ids=["%s-%d" % lp if LEGS[lp[0]][6] > 1 else lp[0] for lp in LEG_PARTS])
def test_injected_words_match_the_oracle(monkeypatch, tmp_path, name, part):
    N, M, nh, opts, want, per_session, parts = LEGS[name]
    manycd = opts.get("manycd", 0)
    if name == "split":
        monkeypatch.setenv("SR_SPLIT", "1")
    else:
        monkeypatch.delenv("SR_SPLIT", raising=False)
    base, cases, runs = leg_base(name)
    if want[4] is not None:
        assert _plan_walk_words(N, M, nh) == want[4], name   # the register walk this leg is about
    if not manycd:   # 4 gammas of 2 words: the hand-over checks below apply
        e = base.ev1
        assert e["zig_wedge"] + e["zig_tail"] + e["zig_reject"] + e["gamma_vneg"] + e["gamma_reject"] + e["upos_retry"] + \
            e["johnk"] == 0, e
    # the leg's coverage conditions, from the oracle's counters alone (over the whole leg, whichever part this is)
    tot, _ = si.coverage(base, cases, runs)
    si.require_events(tot, per_taxon=bool(manycd))
    si.patches_matter(base, runs)
    # this part's cases: the leg's (value, run length) groups dealt round-robin, every offset of each
    groups = list(dict.fromkeys((v, n) for (v, n, _), _ in cases))
    mine = set(groups[part::parts])
    idx = [k for k, ((v, n, _), _) in enumerate(cases) if (v, n) in mine]
    assert len(idx) == len(mine) * (base.w1 + 8)
    ds = sa.Dataset.parse(base.text, maxs=0)
    step = per_session or len(idx)
    handed = 0
    for lo in range(0, len(idx), step):
        chunk = idx[lo:lo + step]
        got = run_session(name, base, ds, [cases[k] for k in chunk], tmp_path)
        for k, g in zip(chunk, got):
            compare(name, cases[k][0], g, runs[k])
            if not manycd:
                handed += cd_handover(name, base, cases[k][0], g[3])
    if not manycd:
        assert handed == 8   # 0xffffffff at offsets 0, 2, 4, 6 and 0 at 1, 3, 5, 7 are all in this leg


def test_divider_at_every_boundary():
    """make_udivm + udivm / udivm_v (sr_device_selftest_udiv) against numpy's g // s in uint64, s = 0xffffffff // n: for
    every divisor n = 1..4095 and every q = 0..n + 1 the words q s - 1, q s, q s + 1 (clipped to 32 bits), plus 0 and
    0xffffffff -- 25 million cases, every one equal.  4096 is refused before any device call."""
    lib = sa.lib()
    P = ctypes.POINTER(ctypes.c_uint32)
    one = np.array([4096], np.uint32)
    out = np.zeros(1, np.uint32)
    assert lib.sr_device_selftest_udiv(0, one.ctypes.data_as(P), one.ctypes.data_as(P), 1, out.ctypes.data_as(P)) == -1
    zero = np.array([0], np.uint32)
    assert lib.sr_device_selftest_udiv(0, zero.ctypes.data_as(P), one.ctypes.data_as(P), 1, out.ctypes.data_as(P)) == -1
    total = 0
    for lo in range(1, 4096, 1024):
        ns, gs = [], []
        for n in range(lo, min(lo + 1024, 4096)):
            s = 0xffffffff // n
            q = np.arange(n + 2, dtype=np.int64) * s
            g = np.clip(np.concatenate([q - 1, q, q + 1, [0, 0xffffffff]]), 0, 0xffffffff)
            gs.append(g)
            ns.append(np.full(g.size, n, np.int64))
        n_all = np.concatenate(ns).astype(np.uint32)
        g_all = np.concatenate(gs).astype(np.uint32)
        # (both parities of the case index see every case: udivm on even k, udivm_v on odd k)
        for shift in (0, 1):
            nn = np.concatenate([np.ones(shift, np.uint32), n_all])
            gg = np.concatenate([np.zeros(shift, np.uint32), g_all])
            q = np.zeros(nn.size, np.uint32)
            assert lib.sr_device_selftest_udiv(0, nn.ctypes.data_as(P), gg.ctypes.data_as(P), nn.size,
                                               q.ctypes.data_as(P)) == 0
            want = gg.astype(np.uint64) // (np.uint64(0xffffffff) // nn.astype(np.uint64))
            bad = np.flatnonzero(q.astype(np.uint64) != want)
            assert bad.size == 0, [(int(nn[k]), hex(int(gg[k])), int(q[k]), int(want[k]), int(k) & 1) for k in bad[:8]]
        total += n_all.size
    assert total == sum(3 * (n + 2) + 2 for n in range(1, 4096))
