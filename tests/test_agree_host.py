"""The host side of the chain agreement: the numpy definition (tests/agree_ref.py) against a literal triple loop,
sr_agreement_modes against the pure-Python clustering on constructed matrices, every argument error (reported before
any device call, the outputs untouched), the host-only library, the command line's refusal, and the known answers on
the oracle's g10s10 records.  CPU only: counts and distances come from the GPU in tests/test_gpu_agreement.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import agree_ref
import oracle_ref
import seriation_amd as sa
from seriation_amd import _lib as L
from seriation_amd import analysis

I64P = ctypes.POINTER(ctypes.c_int64)
U32P = ctypes.POINTER(ctypes.c_uint32)
G10S10 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datasets", "g10s10.txt")


def test_ref_matches_triple_loop():
    N, M, n_sel, count = 4, 2, 3, 7
    rng = np.random.RandomState(11)
    rec = rng.randint(-3, 4, (n_sel, count, 2 * M + N))   # few values: many ties
    rec[0, 0, 2 * M], rec[0, 0, 2 * M + 1], rec[1, 3, 2 * M + 3], rec[2, 6, 2 * M] = -32768, 32767, 32767, -32768
    rec[2, 5, 2 * M:] = 32767                             # a row of ties at the extreme
    rec = rec.astype(np.int16)
    O = [[[0] * N for _ in range(N)] for _ in range(n_sel)]
    for k in range(n_sel):
        for row in rec[k].tolist():
            pi = row[2 * M:]
            for i in range(N):
                for j in range(N):
                    O[k][i][j] += pi[i] < pi[j]
    dist = [[sum(abs(O[k][i][j] - O[l][i][j]) for i in range(N) for j in range(i + 1, N)) for l in range(n_sel)]
            for k in range(n_sel)]
    mir = [[sum(abs(O[k][i][j] - O[l][j][i]) for i in range(N) for j in range(i + 1, N)) for l in range(n_sel)]
           for k in range(n_sel)]
    got = agree_ref.agreement(rec, N, M)
    assert got["pair_counts"].dtype == np.uint32 and np.array_equal(got["pair_counts"], np.array(O))
    assert got["dist"].dtype == np.int64 and np.array_equal(got["dist"], np.array(dist))
    assert np.array_equal(got["dist_mirror"], np.array(mir))
    assert got["scale"] == count * 6
    pc = got["pair_counts"].astype(np.int64)
    assert not pc[:, range(N), range(N)].any() and not np.diag(got["dist"]).any()
    assert (pc + pc.transpose(0, 2, 1) < count).any()     # the ties: the two orders of a pair do not add up to count
    assert not np.array_equal(got["dist_mirror"], got["dist_mirror"].T)


def modes_c(dist, mir, scale, threshold):
    return analysis.chain_modes(np.array(dist, np.int64), np.array(mir, np.int64), scale, threshold)


def same_modes(dist, mir, scale, threshold):
    got, want = modes_c(dist, mir, scale, threshold), agree_ref.modes(dist, mir, scale, threshold)
    assert got["mode"].dtype == np.int32 and got["flip"].dtype == np.uint8
    for k in ("mode", "flip", "medoid", "size"):
        assert list(got[k]) == want[k], (k, list(got[k]), want[k])
    assert got["n_modes"] == want["n_modes"] == len(got["size"]) == len(got["medoid"])
    return got


def upper(n, fill, entries):
    """[n][n] with `fill` everywhere and entries {(k, l): v} in the upper triangle; the lower triangle holds a value
    that would link everything if it were read"""
    a = [[fill] * n for _ in range(n)]
    for k in range(n):
        for l in range(k):
            a[k][l] = 0
    for (k, l), v in entries.items():
        assert k < l
        a[k][l] = v
    return a


def test_modes_single_linkage():
    """0 - 1 - 2 are one mode although 0 and 2 are not linked; 3 is alone"""
    far = 900
    dist = upper(4, far, {(0, 1): 10, (1, 2): 10})
    mir = upper(4, far, {})
    got = same_modes(dist, mir, 1000, 0.05)
    assert list(got["mode"]) == [0, 0, 0, 1] and list(got["size"]) == [3, 1] and list(got["flip"]) == [0, 0, 0, 0]
    assert list(got["medoid"]) == [1, 3]   # chain 1: 10 + 10; chains 0 and 2: 10 + 900


def test_modes_flip_parity():
    """1 is reached from 0 through a mirrored link only (flip 1), 2 from 1 through a second mirrored link (flip 0
    again), 3 from 2 through a plain link (0); 4 hangs on 0 by a mirrored link (1)."""
    far = 900
    dist = upper(5, far, {(2, 3): 7})
    mir = upper(5, far, {(0, 1): 5, (1, 2): 6, (0, 4): 8})
    got = same_modes(dist, mir, 1000, 0.01)
    assert list(got["mode"]) == [0] * 5 and list(got["flip"]) == [0, 1, 0, 0, 1] and got["n_modes"] == 1


def test_modes_boundary_and_extreme_thresholds():
    dist = upper(3, 8, {(0, 1): 2, (0, 2): 3, (1, 2): 3})
    mir = upper(3, 8, {})
    got = same_modes(dist, mir, 8, 0.25)   # 0.25 * 8 = 2.0: e = 2 links, e = 3 does not
    assert list(got["mode"]) == [0, 0, 1] and list(got["size"]) == [2, 1]
    dist0 = upper(3, 8, {(0, 2): 0, (0, 1): 1})
    got = same_modes(dist0, mir, 8, 0.0)   # threshold 0: only e = 0 links
    assert list(got["mode"]) == [0, 1, 0] and list(got["medoid"]) == [0, 1]
    got = same_modes(upper(3, 8, {}), mir, 8, 1.0)   # threshold 1: e = scale links, one mode
    assert list(got["mode"]) == [0, 0, 0] and got["n_modes"] == 1


def test_modes_medoid_tie_single_chain_and_scale_zero():
    dist = upper(4, 4, {})                           # every sum equal: the lowest index
    got = same_modes(dist, upper(4, 9, {}), 100, 0.5)
    assert list(got["medoid"]) == [0] and list(got["size"]) == [4]
    dist = upper(4, 50, {(0, 1): 3, (0, 2): 3, (1, 2): 9, (1, 3): 3, (2, 3): 3, (0, 3): 9})
    got = same_modes(dist, upper(4, 50, {}), 100, 0.04)   # a ring: every sum 15
    assert list(got["mode"]) == [0] * 4 and list(got["medoid"]) == [0]
    got = same_modes([[0]], [[0]], 0, 0.1)           # n = 1
    assert list(got["mode"]) == [0] and list(got["flip"]) == [0] and list(got["medoid"]) == [0] and list(got["size"]) == [1]
    got = same_modes(upper(3, 0, {}), upper(3, 0, {}), 0, 0.3)   # scale 0 (N = 1): every e is 0 and links
    assert list(got["mode"]) == [0, 0, 0]
    got = same_modes(upper(2, 1, {}), upper(2, 2, {}), 0, 1.0)   # scale 0 and an e above it
    assert list(got["mode"]) == [0, 1]


def test_modes_random_against_python():
    rng = np.random.RandomState(3)
    for n in (2, 5, 9, 16):
        for thr in (0.0, 0.2, 0.45, 1.0):
            dist, mir = rng.randint(0, 1000, (n, n)), rng.randint(0, 1000, (n, n))
            same_modes(dist.tolist(), mir.tolist(), 1000, thr)


def test_modes_argument_checks():
    lib = sa.lib()
    d, m = np.zeros((2, 2), np.int64), np.zeros((2, 2), np.int64)
    mode, n_modes = np.full(2, 77, np.int32), ctypes.c_int32(77)
    flip, med, size = np.full(2, 77, np.uint8), np.full(2, 77, np.int32), np.full(2, 77, np.int32)
    i32p = ctypes.POINTER(ctypes.c_int32)

    def call(n=2, dist=True, mir=True, scale=10, thr=0.1, want_mode=True):
        return lib.sr_agreement_modes(n, d.ctypes.data_as(I64P) if dist else None, m.ctypes.data_as(I64P) if mir else None,
                                      scale, thr, mode.ctypes.data_as(i32p) if want_mode else None,
                                      flip.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), med.ctypes.data_as(i32p),
                                      size.ctypes.data_as(i32p), ctypes.byref(n_modes))

    for bad in (dict(thr=-0.01), dict(thr=1.0000001), dict(thr=float("nan")), dict(thr=float("inf")), dict(scale=-1),
                dict(n=0), dict(n=-2), dict(dist=False), dict(mir=False), dict(want_mode=False)):
        assert call(**bad) == L.SR_EINVAL, bad
        assert (mode == 77).all() and (flip == 77).all() and (med == 77).all() and (size == 77).all() and n_modes.value == 77
    assert call() == L.SR_OK and n_modes.value == 1
    # flip, medoid, size and n_modes are optional
    assert lib.sr_agreement_modes(2, d.ctypes.data_as(I64P), m.ctypes.data_as(I64P), 10, 0.1, mode.ctypes.data_as(i32p),
                                  None, None, None, None) == L.SR_OK


def raw_dataset(N, M):
    """an sr_dataset of any claimed shape without its matrix: the checks read N and M only"""
    ds = L.sr_dataset()
    ds.N, ds.M = N, M
    return ds


def call(n_sel, count, N=3, M=2, want=("pair_counts", "dist", "dist_mirror"), ds=True, rec=True, out=True):
    """sr_agreement through ctypes; the requested outputs point at small buffers, which no refused call touches."""
    buf32, buf64 = np.zeros(64, np.uint32), np.zeros(64, np.int64)
    r = np.zeros((1, 8, 7), np.int16)
    o = L.sr_agree_out()
    o.scale, o.kernel_ms = -5, -5.0
    for k in want:
        setattr(o, k, buf32.ctypes.data_as(U32P) if k == "pair_counts" else buf64.ctypes.data_as(I64P))
    rc = sa.lib().sr_agreement(ctypes.byref(raw_dataset(N, M)) if ds else None,
                               r.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)) if rec else None, n_sel, count, 0,
                               ctypes.byref(o) if out else None)
    assert not buf32.any() and not buf64.any() and o.scale == -5 and o.kernel_ms == -5.0
    return rc


def test_argument_checks():
    """Every SR_EINVAL case of the definition; none of them reaches the device (this test runs without one)."""
    assert call(1, 8, ds=False) == L.SR_EINVAL
    assert call(1, 8, rec=False) == L.SR_EINVAL
    assert call(1, 8, out=False) == L.SR_EINVAL
    assert call(0, 8) == L.SR_EINVAL                 # n_sel <= 0
    assert call(-1, 8) == L.SR_EINVAL
    assert call(1, 0) == L.SR_EINVAL                 # count < 1
    assert call(1, -3) == L.SR_EINVAL
    assert call(65536, 32768) == L.SR_EINVAL         # n_sel * count = 2^31
    assert call(2, 2 ** 30) == L.SR_EINVAL
    assert call(1, 8, N=0) == L.SR_EINVAL            # N outside 1..32767
    assert call(1, 8, N=-4) == L.SR_EINVAL
    assert call(1, 8, N=32768) == L.SR_EINVAL
    assert sa.lib().sr_session_agreement(None, None, 1, 0, 8, ctypes.byref(L.sr_agree_out())) == L.SR_EINVAL
    # an invalid argument wins over what is unsupported
    assert call(4097, 2 ** 20) == L.SR_EINVAL
    assert call(0, 8, N=32767, want=("pair_counts",)) == L.SR_EINVAL


def test_unsupported():
    """More than 4096 chains, a requested pair_counts beyond 2^28 entries: SR_EUNSUPPORTED before any device call."""
    assert call(4097, 8) == L.SR_EUNSUPPORTED
    assert call(4097, 8, want=()) == L.SR_EUNSUPPORTED
    assert call(1, 8, N=16385, want=("pair_counts",)) == L.SR_EUNSUPPORTED      # N N = 2^28 + 2^15 + 1
    assert call(4, 8, N=8193, want=("pair_counts", "dist")) == L.SR_EUNSUPPORTED
    assert call(4096, 8, N=257, want=("pair_counts",)) == L.SR_EUNSUPPORTED


def test_distances_argument_checks():
    lib = sa.lib()
    pc, d, m, ms = np.zeros((1, 2, 2), np.uint32), np.full(4, 77, np.int64), np.full(4, 77, np.int64), ctypes.c_double(-5.0)

    def dcall(N=2, n_sel=1, counts=True):
        rc = lib.sr_agreement_distances(N, n_sel, pc.ctypes.data_as(U32P) if counts else None, 0, d.ctypes.data_as(I64P),
                                        m.ctypes.data_as(I64P), ctypes.byref(ms))
        assert (d == 77).all() and (m == 77).all() and ms.value == -5.0
        return rc

    assert dcall(counts=False) == L.SR_EINVAL
    assert dcall(n_sel=0) == L.SR_EINVAL and dcall(n_sel=-1) == L.SR_EINVAL
    assert dcall(N=0) == L.SR_EINVAL and dcall(N=32768) == L.SR_EINVAL
    assert dcall(N=0, n_sel=4097) == L.SR_EINVAL
    assert dcall(n_sel=4097) == L.SR_EUNSUPPORTED


def test_host_only_library_exports_and_refuses():
    """The fake-device library (no device layer, so no agreement kernels) still links, exports the four functions,
    answers a valid sr_agreement call with SR_EUNSUPPORTED and an invalid one with SR_EINVAL, and clusters."""
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(sa.__file__)))
    subprocess.check_call(["make", "-s", "-C", pkg, "build/fake/libseriation.so"])
    code = ("import ctypes, numpy as np, seriation_amd as sa\n"
            "from seriation_amd import _lib as L, analysis\n"
            "lib = sa.lib()\n"
            "assert all(hasattr(lib, s) for s in ('sr_agreement', 'sr_session_agreement', 'sr_agreement_distances',"
            " 'sr_agreement_modes'))\n"
            "ds = sa.Dataset.parse(b'3 2\\n1 0\\n1 1\\n0 1\\n')\n"
            "rec = np.zeros((1, 8, 7), np.int16)\n"
            "recp = rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))\n"
            "buf = np.zeros(4, np.int64)\n"
            "out = L.sr_agree_out()\n"
            "out.dist = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))\n"
            "pc = np.zeros((1, 3, 3), np.uint32)\n"
            "print(lib.sr_agreement(ctypes.byref(ds.c), recp, 1, 8, 0, ctypes.byref(out)),"
            " lib.sr_agreement(ctypes.byref(ds.c), recp, 0, 8, 0, ctypes.byref(out)),"
            " lib.sr_agreement_distances(3, 1, pc.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 0, None, None, None),"
            " analysis.chain_modes([[0, 1], [0, 0]], [[0, 9], [0, 0]], 10, 0.1)['n_modes'])\n")
    env = dict(os.environ, SERIATION_LIB=os.path.join(pkg, "build", "fake", "libseriation.so"),
               PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == [str(L.SR_EUNSUPPORTED), str(L.SR_EINVAL), str(L.SR_EUNSUPPORTED),
                                                      "1"], r.stdout + r.stderr


def test_cli_modes_needs_chain_files(capsys):
    from seriation_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["nowhere.txt", "--modes", "--no-save"])
    assert e.value.code == 2 and "--modes" in capsys.readouterr().err


@pytest.mark.parametrize("name", ["hard", "plain"])
def test_known_answers_from_the_oracle(name):
    """The measurement the default threshold rests on, computed again from the oracle's records by the numpy
    definition, clustered by the library."""
    kn = agree_ref.KNOWN[name]
    text = open(G10S10, "rb").read()
    if name == "plain":
        text = text.replace(b"*", b"")
    runs = [oracle_ref.run_chain(text, seed, 300, 200) for seed in kn["seeds"]]
    assert all(o["rc"] == 0 for o in runs)
    N, M = runs[0]["N"], runs[0]["M"]
    res = agree_ref.agreement(np.stack([o["rec_int"] for o in runs]).astype(np.int16), N, M)
    cm = analysis.chain_modes(res["dist"], res["dist_mirror"], res["scale"], kn["threshold"])
    agree_ref.check_known(name, res, cm)
    want = agree_ref.modes(res["dist"], res["dist_mirror"], res["scale"], kn["threshold"])
    assert list(cm["mode"]) == want["mode"] and list(cm["flip"]) == want["flip"] and list(cm["medoid"]) == want["medoid"]
