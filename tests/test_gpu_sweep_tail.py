"""The one-workgroup LDS-column sweep kernels around their barriers: chains from birth against the CPU oracle.

Fresh chains accept many proposals, so a sweep has several batches and the MT19937 ring is topped up before the
phase-A barrier, every later batch barrier and the end-of-sweep barrier (rng_topup: one block in one dependency
phase, published by the barrier that follows), mixed with rng_ensure's barriered refills when a sweep consumes more
than the top-ups give (128 x 1000: more than three blocks per sweep).  Every case runs a handful of chains for T calls four ways, each
equal to the oracle bit for bit (a, b, pi, c, d, loglik):
  * one launch of T saved calls;
  * T launches of one saved call (launch boundaries: the ring and its cursor stored and reloaded every call);
  * T - 1 unsaved calls, then one saved call (a save on every call equals a save on none followed by one);
  * a checkpoint in the middle, restored into a new session.
The oracle runs once per case and is shared."""
import os

import numpy as np
import pytest

import oracle_ref
import seriation_amd as sa
from test_gpu_edge import _all_ones_text, make_text

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden", "datasets")
T = 12          # calls per chain (120 sweeps from birth)
H = 5           # the checkpoint's call
SEEDS = [3, 17, 255]

# name: (dataset file or (N, M, nh) of a generated one or "ones", block_threads, generic)
CASES = {
    "g2s2": ("g2s2.txt", 0, False),
    "40x70-idle-threads": ((40, 70, 0), 0, False),          # threads without a taxon
    "64x96-hard20": ((64, 96, 20), 0, False),               # hard sites move: the proposal tables follow the rebuilds
    "128x1000-tb512": ((128, 1000, 5), 512, False),         # two taxa per thread, > 3 blocks per sweep
    "256x512-specialized": ("synth_256x512.txt", 0, False),
    "256x512-generic": ("synth_256x512.txt", 0, True),
    "all-ones": ("ones", 0, False),                         # Johnk branch: the sequential c, d draws
}


def lds_shapes():
    """(N, M, nh, block_threads) of the generated shapes (__graft_entry__.prewarm compiles their specialised kernels
    ahead)."""
    return [(src[0], src[1], src[2], tb) for src, tb, _ in CASES.values() if isinstance(src, tuple)]


_TEXT = {}
_ORACLE = {}


def _text(name):
    if name not in _TEXT:
        src = CASES[name][0]
        if src == "ones":
            _TEXT[name] = _all_ones_text(40, 24, {5, 17, 30})
        elif isinstance(src, tuple):
            _TEXT[name] = make_text(src[0], src[1], src[2], seed=src[0] * 1000 + src[1])
        else:
            with open(os.path.join(DATA, src), "rb") as fh:
                _TEXT[name] = fh.read()
    return _TEXT[name]


def _oracle(name, rng="mt"):
    """The oracle's T saved calls from birth per seed (computed once, shared, never modified)."""
    key = (CASES[name][0], rng)
    if key not in _ORACLE:
        outs = [oracle_ref.run_chain(_text(name), s, 0, T, maxs=0, rng=rng) for s in SEEDS]
        assert all(o["rc"] == 0 for o in outs)
        _ORACLE[key] = (np.stack([o["rec_int"] for o in outs]), np.stack([o["rec_dbl"] for o in outs]))
    return _ORACLE[key]


def _session(name, rng="mt"):
    """A session with room for T records; run(n) is one launch of n calls."""
    _, tb, generic = CASES[name]
    ds = sa.Dataset.parse(_text(name), maxs=0)
    s = sa.Session(ds, SEEDS, calls_per_launch=T, block_threads=tb, rng=rng, generic=generic)
    assert s.variant == "lds" and s.kernel == "single", (name, s.variant, s.kernel)
    assert s.specialized == (not generic), name
    return ds, s


def _equal(ab, cdl, ri, rd, what):
    np.testing.assert_array_equal(ab.astype(np.int32), ri, err_msg=str(what))
    assert np.array_equal(cdl.view(np.uint64), rd.view(np.uint64)), what


ALL = pytest.mark.parametrize("name", list(CASES))


@ALL
def test_one_launch_and_a_launch_per_call_equal_the_oracle(name):
    ri, rd = _oracle(name)
    _, s = _session(name)
    with s:
        s.run(T, save=True)
        _equal(*s.fetch_records(), ri, rd, (name, "run(T)"))
    _, s = _session(name)
    with s:
        for _ in range(T):
            s.run(1, save=True)
        _equal(*s.fetch_records(), ri, rd, (name, "run(1) x T"))


@ALL
def test_save_on_the_last_call_only(name):
    ri, rd = _oracle(name)
    _, s = _session(name)
    with s:
        s.run(T - 1, save=False)
        s.run(1, save=True)
        ab, cdl = s.fetch_records()
    assert ab.shape[1] == 1
    _equal(ab, cdl, ri[:, T - 1:], rd[:, T - 1:], (name, "save on the last call"))


@ALL
def test_checkpoint_in_the_middle(name, tmp_path):
    ri, rd = _oracle(name)
    ck = str(tmp_path / "tail.srck")
    ds, s = _session(name)
    with s:
        s.run(H, save=True)
        _equal(*s.fetch_records(), ri[:, :H], rd[:, :H], (name, "before the checkpoint"))
        s.checkpoint(ck)
    r = sa.Session.restore(ds, ck, calls_per_launch=T, block_threads=CASES[name][1])
    try:
        r.run(T - H, save=True)
        ab, cdl = r.fetch_records()
    finally:
        r.close()
    _equal(ab[:, -(T - H):], cdl[:, -(T - H):], ri[:, H:], rd[:, H:], (name, "after the restore"))


def test_philox_session_keeps_its_refill_path():
    """The Philox stream is not topped up (its blocks come from counters, rng_gen_block): same bits as the oracle's
    Philox mode, one launch and a launch per call."""
    name = "64x96-hard20"
    ri, rd = _oracle(name, rng="philox")
    for runs in ([T], [1] * T):
        _, s = _session(name, rng="philox")
        with s:
            for n in runs:
                s.run(n, save=True)
            _equal(*s.fetch_records(), ri, rd, (name, "philox", runs))
