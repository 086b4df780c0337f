"""Stream injection, the CPU half (no GPU): the oracle's chain from an explicit MT19937 state, the case builder's
untempering, and the sensitivity control of the GPU scan (tests/test_gpu_stream_inject.py).

The control answers one question: would the scan's comparison notice a kernel that ignored a table entry's "no
rejection" bit?  The oracle runs the 0xffffffff and 0 scans twice -- right, and with om_gsl.h's om_ok_ignored (a
rejected uniform_int quotient clamped to n - 1, a zero uniform_pos word passed through, every ziggurat word taken as
inside the box) -- and the two must differ wherever the right run met such an event, and nowhere else."""
import ctypes
import os

import numpy as np
import pytest

import oracle_ref
import stream_inject as si
from seriation_amd import _lib as L
from test_gpu_edge import make_text

HERE = os.path.dirname(os.path.abspath(__file__))


def _g10s10():
    with open(os.path.join(HERE, "golden", "datasets", "g10s10.txt"), "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("manycd", [0, 1])
def test_unmodified_state_equals_run_chain(manycd):
    """Handing the state after mcmc_randomize back unmodified gives oracle_ref.run_chain's chain bit for bit: records,
    acceptance counters, words drawn (g10s10, seeds 1-4, 3 calls of 10 sweeps)."""
    text = _g10s10()
    for seed in (1, 2, 3, 4):
        ref = oracle_ref.run_chain(text, seed, 0, 3, manycd=manycd)
        first = oracle_ref.run_chain_mt(text, seed, ts=0, manycd=manycd)
        init = oracle_ref.run_chain(text, seed, 0, 0)["words"]   # words mcmc_randomize drew
        assert 0 <= first["mti0"] <= 624
        for mt in (None, first["mt0"]):
            o = oracle_ref.run_chain_mt(text, seed, mt, first["mti0"], ts=3, sweeps=10, manycd=manycd)
            assert o["rc"] == 0 and ref["rc"] == 0
            np.testing.assert_array_equal(o["rec_int"], ref["rec_int"])
            assert np.array_equal(o["rec_dbl"].view(np.uint64), ref["rec_dbl"].view(np.uint64))
            np.testing.assert_array_equal(o["acc"], ref["acc"])
            assert o["words"] == ref["words"] - init
            if manycd:
                assert np.array_equal(o["rec_cdv"].view(np.uint64), ref["rec_cdv"].view(np.uint64))
            assert o["ev"]["uint_calls"] > 0 and o["ev"]["upos_calls"] > 0


def test_consumed_word_matters_only_to_the_next_block():
    """Overwriting a word the cursor has passed (offset below mti, cursor unmoved) changes no draw of the resident
    block -- every call that ends inside it gives the same record -- but the next block is generated from it
    (MT19937's twist reads word k + 1 for word k), so later calls differ."""
    text = _g10s10()
    first = oracle_ref.run_chain_mt(text, 3, ts=0)
    mti = first["mti0"]
    assert 6 <= mti < 624
    T = 14
    left = 624 - mti   # words of the resident block still to draw
    cum = [oracle_ref.run_chain_mt(text, 3, first["mt0"], mti, ts=t, sweeps=1)["words"] for t in range(1, T + 1)]
    inside = sum(1 for w in cum if w <= left)
    assert 1 <= inside < T - 1, (cum, left)   # calls on both sides of the block's end
    base = oracle_ref.run_chain_mt(text, 3, first["mt0"], mti, ts=T, sweeps=1)
    mt = first["mt0"].copy()
    mt[5] ^= np.uint32(0xffffffff)
    o = oracle_ref.run_chain_mt(text, 3, mt, mti, ts=T, sweeps=1)
    assert o["rc"] == 0 and base["rc"] == 0
    np.testing.assert_array_equal(o["rec_int"][:inside], base["rec_int"][:inside])
    assert np.array_equal(o["rec_dbl"][:inside].view(np.uint64), base["rec_dbl"][:inside].view(np.uint64))
    assert not np.array_equal(o["rec_dbl"][inside:].view(np.uint64), base["rec_dbl"][inside:].view(np.uint64))


def test_bad_cursor_refused():
    text = _g10s10()
    mt = np.zeros(624, np.uint32)
    assert oracle_ref.run_chain_mt(text, 1, mt, 625, ts=1)["rc"] == -1
    assert oracle_ref.run_chain_mt(text, 1, mt, -1, ts=1)["rc"] == -1


def test_untemper_inverts_the_tempering():
    """The case builder's untemper (sr_host_mt_untemper) inverts MT19937's tempering on the injected values, on every
    single-bit word and on random words -- against a numpy restatement of the tempering, not the library's own."""
    rng = np.random.default_rng(5)
    vals = np.concatenate([np.array(si.single_values(40, 3, neg_tail=True) + si.single_values(2, 0), np.uint32),
                           np.uint32(1) << np.arange(32, dtype=np.uint32),
                           rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32)])
    raw = si.untemper(vals)
    np.testing.assert_array_equal(si.temper(raw), vals)


def test_layout_matches_an_initial_checkpoint(tmp_path):
    """ck_layout's end is the length of a host-written checkpoint, and its rng / mt parts hold the oracle's state
    after mcmc_randomize: cursor pos % 624 = mti, the resident block = the oracle's 624 raw words."""
    import seriation_amd as sa
    text = make_text(40, 24, 3, seed=11)
    ds = sa.Dataset.parse(text, maxs=0)
    C = 3
    path = tmp_path / "init.srck"
    assert L.lib().sr_host_initial_checkpoint(ctypes.byref(ds.c), sa.core.make_specs([7] * C), C, os.fsencode(str(path))) == 0
    raw = path.read_bytes()
    base, end = si.ck_layout(ds.N, ds.M, ds.nh, C)
    assert len(raw) == end
    o = oracle_ref.run_chain_mt(text, 7, ts=0)
    rng = np.frombuffer(raw, "<u8", 2 * C, base["rng"]).reshape(C, 2)
    mt = np.frombuffer(raw, "<u4", C * si.RING * si.MT_N, base["mt"]).reshape(C, si.RING, si.MT_N)
    for k in range(C):
        pos, gen = int(rng[k, 0]), int(rng[k, 1])
        assert pos % si.MT_N == o["mti0"] and gen == pos // si.MT_N + 1
        np.testing.assert_array_equal(mt[k, (pos // si.MT_N) % si.RING], o["mt0"])


def test_case_builder_covers_every_offset():
    cases = si.build_cases(115, si.single_values(40, 3))
    labels = [c[0] for c in cases]
    assert len(set(labels)) == len(labels)
    for v in si.single_values(40, 3):
        assert [o for (vv, n, o) in labels if vv == v and n == 1] == list(range(123))
    for v, n in si.RUNS:
        assert [o for (vv, nn, o) in labels if vv == v and nn == n] == list(range(123))
    assert dict(cases)[(si.FF, 3, 10)] == [(10, si.FF), (11, si.FF), (12, si.FF)]
    # the boundary words: n s is the first word uniform_int(n) rejects, n s - 1 the last it accepts
    for n, (rej, acc) in zip((40, 39, 37, 36, 2), zip(*[iter(si.boundary_values(40, 3))] * 2)):
        s = 0xffffffff // n
        assert rej // s == n and acc // s == n - 1 and rej == acc + 1
    assert si.boundary_values(2, 0)[2:4] == [0xffffffff, 0xfffffffe]   # uniform_int(1) rejects only 0xffffffff


SENSITIVITY_FLOOR = 0.90


def test_sensitivity_control(capsys):
    """On the reg9 shape (40 x 24, 3 hard sites; text seed 11, chain seed 7) the 0xffffffff and 0 scans through the
    oracle right and with the "ok bit ignored" answers: the two runs differ (records, counters or words consumed) on at
    least 90 % of the cases whose right run counted a uniform_int rejection, a uniform_pos retry or a ziggurat word
    outside the box, and on none of the others.  Measured share: see the printed line."""
    base = si.Base(make_text(40, 24, 3, seed=11), 7)
    cases = si.build_cases(base.w1, [si.FF, si.ZERO], runs=())
    assert len(cases) == 2 * (base.w1 + 8)
    hit = differ = quiet = 0
    for label, patch in cases:
        right = base.run(patch)
        wrong = base.run(patch, ok_ignored=True)
        assert right["rc"] == 0
        ev = right["ev"]
        event = ev["uint_reject"] + ev["upos_retry"] + ev["zig_wedge"] + ev["zig_tail"] > 0
        same = si.same_run(right, wrong)
        if event:
            hit += 1
            differ += not same
        else:
            quiet += 1
            assert same, label   # no event: the flag changes nothing
    share = differ / hit
    with capsys.disabled():
        print("\nstream injection sensitivity: %d of %d event cases differ (%.1f %%), %d quiet cases equal"
              % (differ, hit, 100 * share, quiet))
    assert hit >= base.ev1["uint_calls"] + base.ev1["upos_calls"]
    assert share >= SENSITIVITY_FLOOR, (differ, hit)


@pytest.mark.parametrize("N,M,nh,manycd", [(40, 24, 3, 0), (300, 12, 9, 0), (300, 12, 33, 0), (560, 12, 5, 0),
                                           (2, 4, 0, 0), (40, 24, 3, 1)],
                         ids=["reg9", "reg17", "nh33", "lds-walk", "two-sites", "per-taxon"])
def test_coverage_conditions_on_the_cpu(N, M, nh, manycd):
    """The GPU legs' coverage conditions hold at their shapes and seeds (checked here without a GPU, so a change of
    seed or shape that loses an event is seen at once), and every case leaves the oracle consistent."""
    base = si.Base(make_text(N, M, nh, seed=11), 7, manycd=manycd)
    cases = si.build_cases(base.w1, si.single_values(N, nh, neg_tail=bool(manycd)))
    runs = [base.run(p) for _, p in cases]
    assert all(r["rc"] == 0 for r in runs)
    tot, _ = si.coverage(base, cases, runs)
    si.require_events(tot, per_taxon=bool(manycd))
    si.patches_matter(base, runs)
