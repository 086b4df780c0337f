"""The sweep kernel's role split against the CPU oracle, bit for bit.

Between the phase-A barrier and the K barrier of a sweep the first half of a one-workgroup LDS-column kernel's waves
draws c, d (draw_cd_fast) and publishes them in LDS, while the first wave of the second half draws the sweep's first
proposal batch at the cursor the c, d draws' fast path leads to; phase C takes that batch from LDS when it starts
there.  What can go wrong is a batch used when it should not be (the c, d draws left their fast path, the cursor is
elsewhere, the tables were rebuilt) or one that differs from what phase C would have drawn in place (a uniform_int
rejection or a zero uniform_pos word inside it: the batch must end where phase C's scan ends).  So:
  * the injected words of tests/test_gpu_stream_inject.py at every offset of a sweep on 8-wave kernels (two waves per
    SIMD: the bench kernel's arrangement; the legs there are 4-wave), specialised and generic, and on the 16-wave
    generic kernel;
  * a c, d mis-speculation in a sweep that is not the launch's first, followed by another launch or by more sweeps
    of the same launch: nothing of the abandoned batch may reach a later sweep;
  * chains from birth (many accepted proposals, hard sites that move, so the tables the batch is drawn from are
    rebuilt), one launch against a launch per call: the LDS records are not state;
  * a Philox session, which takes the same path.
Every oracle run is shared with the tests it comes from (stream_inject's cases, test_gpu_sweep_tail's chains)."""
import ctypes
import os

import numpy as np
import pytest

import seriation_amd as sa
import stream_inject as si
import test_gpu_stream_inject as inj
import test_gpu_sweep_tail as tail
from seriation_amd import _lib as L

pytestmark = pytest.mark.gpu

# the legs of test_gpu_stream_inject.py's table that this file adds (same fields); 40 x 24 with 3 hard sites shares
# that file's base chain, cases and oracle runs
LEGS = {
    "role-8-waves": (40, 24, 3, {"block_threads": 512}, ("lds", "single", True, 512, None), 0, 1),
    "role-8-waves-generic": (40, 24, 3, {"block_threads": 512, "generic": True}, ("lds", "single", False, 512, None), 0, 1),
    "role-16-waves-generic": (40, 24, 3, {"block_threads": 1024, "generic": True}, ("lds", "single", False, 1024, None), 0, 1),
}


@pytest.mark.parametrize("name", list(LEGS))
def test_injected_words_at_every_offset(monkeypatch, tmp_path, name):
    """stream_inject.single_values and the runs at every offset of the first sweep and 8 beyond (the second sweep's
    c, d words): records, the 7 acceptance counters and the words consumed equal the oracle's; the c, d cases count a
    sequential draw.  Coverage from the oracle's event counters, as in test_gpu_stream_inject.py."""
    monkeypatch.setitem(inj.LEGS, name, LEGS[name])
    monkeypatch.delenv("SR_SPLIT", raising=False)
    base, cases, runs = inj.leg_base(name)
    e = base.ev1   # the base chain's c, d draws take 4 gammas of 2 words: the hand-over cases below are the 8 of them
    assert e["zig_wedge"] + e["zig_tail"] + e["zig_reject"] + e["gamma_vneg"] + e["gamma_reject"] + e["upos_retry"] + \
        e["johnk"] == 0, e
    tot, _ = si.coverage(base, cases, runs)
    si.require_events(tot)
    si.patches_matter(base, runs)
    assert {v for (v, n, _), _ in cases if n == 1} == set(si.single_values(base.N, base.nh))
    ds = sa.Dataset.parse(base.text, maxs=0)
    got = inj.run_session(name, base, ds, cases, tmp_path)
    handed = 0
    for case, g, ref in zip(cases, got, runs):
        inj.compare(name, case[0], g, ref)
        handed += inj.cd_handover(name, base, case[0], g[3])
    assert handed == 8


def _run_patched(ds, base, opts, patches, tmp_path, launches):
    """Chains restored with `patches` in their resident block (as test_gpu_stream_inject.run_session), run for
    sum(launches) saved calls of 2 sweeps, one launch per entry: per chain (rec_int, rec_dbl, acc10, words)."""
    N, M, nh, C = base.N, base.M, base.nh, len(patches)
    ck0, ck1, ck2 = (str(tmp_path / n) for n in ("base.srck", "patched.srck", "after.srck"))
    seeds = [base.seed] * C
    assert L.lib().sr_host_initial_checkpoint(ctypes.byref(ds.c), sa.core.make_specs(seeds), C, os.fsencode(ck0)) == 0
    raw = bytearray(open(ck0, "rb").read())
    lay, end = si.ck_layout(N, M, nh, C)
    assert len(raw) == end
    rng = np.frombuffer(raw, "<u8", 2 * C, lay["rng"]).reshape(C, 2)
    mt = np.frombuffer(raw, "<u4", C * si.RING * si.MT_N, lay["mt"]).reshape(C, si.RING, si.MT_N)
    start = np.zeros(C, np.uint64)
    for k, patch in enumerate(patches):
        blk = int(rng[k, 0]) // si.MT_N
        assert int(rng[k, 1]) == blk + 1 and int(rng[k, 0]) % si.MT_N == base.mti0
        assert np.array_equal(mt[k, blk % si.RING], base.block)
        rng[k, 0] = start[k] = blk * si.MT_N
        mt[k, blk % si.RING][:] = base.patched(patch)
    with open(ck1, "wb") as fh:
        fh.write(raw)
    T = sum(launches)
    with sa.Session.restore(ds, ck1, sweeps_per_call=2, calls_per_launch=T, **opts) as s:   # (room for T records)
        assert (s.variant, s.kernel, s.block_threads) == ("lds", "single", opts["block_threads"])
        assert s.specialized == (not opts.get("generic", False))
        for n in launches:
            s.run(n, save=True)
        ab, cdl = s.fetch_records()
        s.checkpoint(ck2)
    after = open(ck2, "rb").read()
    pos1 = np.frombuffer(after, "<u8", 2 * C, lay["rng"]).reshape(C, 2)[:, 0]
    acc = np.frombuffer(after, "<u8", si.NACC * C, lay["acc"]).reshape(C, si.NACC).astype(np.int64)
    assert ab.shape[1] == T
    return [(ab[k].astype(np.int32), cdl[k], acc[k], int(pos1[k] - start[k])) for k in range(C)]


@pytest.mark.parametrize("generic", [False, True], ids=["specialized", "generic"])
def test_cd_misspeculation_in_a_later_sweep_leaves_nothing_behind(tmp_path, generic):
    """A ziggurat tail word at each gamma's first word and a zero at each gamma's uniform_pos word of the SECOND
    sweep's c, d draws (offsets w1 .. w1 + 7; the first sweep reads none of them), 8-wave kernels.  That sweep's
    pre-drawn batch is abandoned; two more sweeps follow, in the next launch (launches of 1 call) or in the same one
    (one launch of 2 calls).  Both equal the oracle's 2 calls: records, acceptance counters, words consumed."""
    base, _, _ = inj.leg_base("reg9")
    w1 = base.w1
    patches = [[(w1 + off, si.FF)] for off in (0, 2, 4, 6)] + [[(w1 + off, si.ZERO)] for off in (1, 3, 5, 7)]
    patches.append([])   # the plain chain beside them
    refs = [base.run(p, ts=2, sweeps=2) for p in patches]
    plain = refs[-1]
    assert all(r["rc"] == 0 for r in refs)
    rare = ("zig_wedge", "zig_tail", "zig_reject", "gamma_vneg", "gamma_reject", "upos_retry")
    for r in refs[:-1]:   # the words are read, and take the draws off their two-words-per-gamma path
        assert not si.same_run(r, plain)
        assert sum(r["ev"][k] for k in rare) > sum(plain["ev"][k] for k in rare), r["ev"]
    ds = sa.Dataset.parse(base.text, maxs=0)
    opts = {"block_threads": 512, "generic": generic}
    for launches in ([1, 1], [2]):
        got = _run_patched(ds, base, opts, patches, tmp_path, launches)
        for k, ((ri, rd, acc, words), ref) in enumerate(zip(got, refs)):
            what = (launches, patches[k])
            np.testing.assert_array_equal(ri, ref["rec_int"], err_msg=str(what))
            assert np.array_equal(rd.view(np.uint64), ref["rec_dbl"].view(np.uint64)), what
            np.testing.assert_array_equal(acc[:7], ref["acc"], err_msg=str(what))
            assert words == ref["words"], (what, words, ref["words"])
            assert acc[9] >= 1 or not patches[k], (what, acc[9])   # the sequential c, d draw was taken


# chains from birth: test_gpu_sweep_tail's cases (and oracle runs) at these block sizes
BIRTH = [("64x96-hard20", 512, False), ("64x96-hard20", 512, True), ("64x96-hard20", 0, True),
         ("256x512-specialized", 0, False), ("256x512-generic", 0, True)]


@pytest.mark.parametrize("name,tb,generic", BIRTH, ids=["%s-tb%d-%s" % (n, t, "generic" if g else "specialized") for n, t, g in BIRTH])
def test_chains_from_birth_one_launch_and_a_launch_per_call(name, tb, generic):
    """12 calls of 3 seeds from birth: the hard sites move (64 x 96 with 20 of them), so the pre-drawn batch has to
    follow the rebuilt tables; a launch per call stores and reloads the state between any two calls, and the LDS
    records are not part of it."""
    ri, rd = tail._oracle(name)
    ds = sa.Dataset.parse(tail._text(name), maxs=0)
    for runs in ([tail.T], [1] * tail.T):
        with sa.Session(ds, tail.SEEDS, calls_per_launch=tail.T, block_threads=tb, generic=generic) as s:
            assert (s.variant, s.kernel, s.specialized) == ("lds", "single", not generic), name
            assert tb == 0 or s.block_threads == tb
            for n in runs:
                s.run(n, save=True)
            tail._equal(*s.fetch_records(), ri, rd, (name, tb, generic, runs))


def test_philox_session_takes_the_role_split():
    """The Philox stream differs only in how ring blocks are made (rng_gen_block, no top-up): its sessions run the
    same role split.  8 waves, hard sites that move, one launch and a launch per call against the oracle's Philox mode."""
    name = "64x96-hard20"
    ri, rd = tail._oracle(name, rng="philox")
    ds = sa.Dataset.parse(tail._text(name), maxs=0)
    for runs in ([tail.T], [1] * tail.T):
        with sa.Session(ds, tail.SEEDS, calls_per_launch=tail.T, block_threads=512, rng="philox") as s:
            assert (s.variant, s.kernel, s.specialized, s.block_threads) == ("lds", "single", True, 512)
            for n in runs:
                s.run(n, save=True)
            tail._equal(*s.fetch_records(), ri, rd, (name, "philox", runs))
