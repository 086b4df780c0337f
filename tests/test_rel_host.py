"""The host side of the taxon-pair relations: the numpy definition (tests/rel_ref.py) against a brute-force triple
loop, analysis.diversity_curve against np.sort ranks on constructed histograms, and every argument error of
sr_relations, which must be reported before any device call.  CPU only: the counts come from the GPU in
tests/test_gpu_relations.py."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import rel_ref
import seriation_amd as sa
from seriation_amd import _lib as L
from seriation_amd import analysis


def brute(rec, N, M, flips):
    """The definition read literally, one sample, one pair, one position at a time."""
    out = {"orig_before": [[0] * M for _ in range(M)], "ext_before": [[0] * M for _ in range(M)],
           "precedes": [[0] * M for _ in range(M)], "overlap": [[0] * M for _ in range(M)],
           "dur_hist": [[0] * (N + 1) for _ in range(M)], "dur_outside": [0] * M,
           "rich_hist": [[0] * (M + 1) for _ in range(N)]}
    for k, chain in enumerate(rec):
        for row in chain:
            a, b = list(row[:M]), list(row[M:2 * M])
            if flips[k]:
                a, b = [N - v for v in row[M:2 * M]], [N - v for v in row[:M]]
            for i in range(M):
                for j in range(M):
                    out["orig_before"][i][j] += a[i] < a[j]
                    out["ext_before"][i][j] += b[i] < b[j]
                    out["precedes"][i][j] += b[i] <= a[j]
                    out["overlap"][i][j] += max(a[i], a[j]) < min(b[i], b[j])
                d = b[i] - a[i]
                if 0 <= d <= N:
                    out["dur_hist"][i][d] += 1
                else:
                    out["dur_outside"][i] += 1
            for p in range(N):
                out["rich_hist"][p][sum(1 for m in range(M) if a[m] <= p < b[m])] += 1
    return out


def test_ref_matches_brute_force():
    N, M, n_sel, count = 4, 3, 3, 7
    rng = np.random.RandomState(47)
    rec = rng.randint(-2, N + 3, (n_sel, count, 2 * M + N))   # limits outside [0, N] on both sides, a > b rows
    rec[0, 0, 0], rec[1, 2, 5], rec[1, 3, 1] = -32768, 32767, -32768   # chain 1 is reflected: N + 32768
    flips = [0, 1, 0]
    want = brute(rec.tolist(), N, M, flips)
    got = rel_ref.relations(rec.astype(np.int16), N, M, flips)
    assert set(got) == set(rel_ref.KINDS)
    for k in rel_ref.KINDS:
        assert got[k].dtype == np.uint32 and np.array_equal(got[k], np.array(want[k])), k
    T = n_sel * count
    assert (got["rich_hist"].sum(axis=1) == T).all()
    assert (got["dur_hist"].sum(axis=1) + got["dur_outside"] == T).all() and got["dur_outside"].any()
    assert np.array_equal(got["overlap"], got["overlap"].T)
    # the diagonals: empty and non-empty intervals
    assert (np.diag(got["precedes"]) + np.diag(got["overlap"]) == T).all() and np.diag(got["precedes"]).any()
    assert not np.diag(got["orig_before"]).any() and not np.diag(got["ext_before"]).any()
    assert set(rel_ref.relations(rec.astype(np.int16), N, M, flips, kinds=("overlap",))) == {"overlap"}


def sorted_ranks(values, probs):
    """values [T] -> (mean, [quantile per p]) from the sorted samples themselves"""
    v = np.sort(np.asarray(values))
    T = len(v)
    return int(v.sum()) / T, [int(v[min(max(math.ceil(p * float(T)), 1), T) - 1]) for p in probs]


def test_diversity_curve_against_sorted_ranks():
    M = 9
    rng = np.random.RandomState(5)
    probs = (0.0, 0.025, 0.5, 0.51, 0.975, 1.0)
    samples = [rng.randint(0, M + 1, 40), np.full(7, M), np.zeros(3, int), np.array([2, 7, 7, 2]),   # even T: lower median
               rng.randint(3, 6, 1001), np.array([4])]
    hist = np.stack([np.bincount(s, minlength=M + 1) for s in samples]).astype(np.uint32)
    got = analysis.diversity_curve(hist, probs)
    assert got["mean"].dtype == np.float64 and got["quant"].dtype == np.int32 and got["quant"].shape == (len(probs), len(samples))
    for p, s in enumerate(samples):
        mean, q = sorted_ranks(s, probs)
        assert got["mean"][p] == mean and got["quant"][:, p].tolist() == q
        assert got["quant"][0, p] == s.min() and got["quant"][-1, p] == s.max()   # p = 0 and p = 1
    assert analysis.diversity_curve(hist)["quant"].shape == (3, len(samples))
    # and rel_ref's own curve, which never builds a histogram, on records
    N, M2 = 6, 5
    rec = rng.randint(-1, N + 2, (2, 30, 2 * M2 + N)).astype(np.int16)
    want = rel_ref.diversity(rec, N, M2, probs, [1, 0])
    got = analysis.diversity_curve(rel_ref.relations(rec, N, M2, [1, 0], kinds=("rich_hist",))["rich_hist"], probs)
    assert np.array_equal(got["quant"], want["quant"]) and np.array_equal(got["mean"], want["mean"])


def raw_dataset(N, M):
    """an sr_dataset of any claimed shape without its matrix: the checks read N and M only"""
    ds = L.sr_dataset()
    ds.N, ds.M = N, M
    return ds


def call(n_sel, count, N=3, M=2, want=("overlap", "dur_hist", "dur_outside", "rich_hist"), ds=True, rec=True, out=True):
    """sr_relations through ctypes; the requested outputs point at one small buffer, which no refused call touches."""
    buf = np.zeros(64, np.uint32)
    r = np.zeros((1, 8, 7), np.int16)
    o = L.sr_rel_out()
    for k in want:
        setattr(o, k, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    rc = sa.lib().sr_relations(ctypes.byref(raw_dataset(N, M)) if ds else None,
                               r.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)) if rec else None, n_sel, count, 0,
                               ctypes.byref(o) if out else None)
    assert not buf.any()
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
    assert call(1, 8, M=0) == L.SR_EINVAL            # M < 1
    assert call(1, 8, M=-1) == L.SR_EINVAL
    assert sa.lib().sr_session_relations(None, None, 1, 0, 8, ctypes.byref(L.sr_rel_out())) == L.SR_EINVAL
    # an invalid argument wins over an output that is too large
    assert call(0, 8, M=16385, want=("overlap",)) == L.SR_EINVAL


def test_outputs_beyond_one_gib_unsupported():
    """A single requested output larger than 1 GiB: SR_EUNSUPPORTED before any device call, whichever output it
    is."""
    for k in ("orig_before", "ext_before", "precedes", "overlap"):
        assert call(1, 8, N=5, M=16385, want=(k,)) == L.SR_EUNSUPPORTED
    assert call(1, 8, N=32767, M=8193, want=("dur_hist",)) == L.SR_EUNSUPPORTED     # M (N + 1) = 2^28 + 2^15
    assert call(1, 8, N=32767, M=8193, want=("rich_hist",)) == L.SR_EUNSUPPORTED    # N (M + 1) > 2^28
    assert call(1, 8, N=1, M=2 ** 28, want=("rich_hist",)) == L.SR_EUNSUPPORTED
    assert call(1, 8, N=5, M=16385, want=("dur_outside", "overlap")) == L.SR_EUNSUPPORTED


def test_host_only_library_exports_and_refuses():
    """The fake-device library (no device layer, so no relation kernels) still links, exports both functions, and
    answers a valid sr_relations call with SR_EUNSUPPORTED, an invalid one with SR_EINVAL."""
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(sa.__file__)))
    subprocess.check_call(["make", "-s", "-C", pkg, "build/fake/libseriation.so"])
    code = ("import ctypes, numpy as np, seriation_amd as sa\n"
            "from seriation_amd import _lib as L\n"
            "lib = sa.lib()\n"
            "assert all(hasattr(lib, s) for s in ('sr_relations', 'sr_session_relations'))\n"
            "ds = sa.Dataset.parse(b'3 2\\n1 0\\n1 1\\n0 1\\n')\n"
            "rec = np.zeros((1, 8, 7), np.int16)\n"
            "recp = rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))\n"
            "buf = np.zeros(4, np.uint32)\n"
            "out = L.sr_rel_out()\n"
            "out.overlap = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))\n"
            "print(lib.sr_relations(ctypes.byref(ds.c), recp, 1, 8, 0, ctypes.byref(out)),"
            " lib.sr_relations(ctypes.byref(ds.c), recp, 0, 8, 0, ctypes.byref(out)))\n")
    env = dict(os.environ, SERIATION_LIB=os.path.join(pkg, "build", "fake", "libseriation.so"),
               PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == [str(L.SR_EUNSUPPORTED), str(L.SR_EINVAL)], r.stdout + r.stderr


@pytest.mark.parametrize("extra", [[], ["--select", "2", "--no-save"]])
def test_cli_relations_needs_select(capsys, extra):
    from seriation_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["nowhere.txt", "--relations"] + extra)
    assert e.value.code == 2 and "--relations" in capsys.readouterr().err
