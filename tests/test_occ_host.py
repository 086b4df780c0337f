"""Cell occupancy without a GPU: the numpy definition (tests/occ_ref.py) against a literal per-cell, per-sample loop,
the structural identities of its outputs, every argument error of sr_occupancy (reported before any device call, the
outputs untouched), the host-only library's refusal, the Python layer's derived values, and the command line's
argument check."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import occ_ref
import seriation_amd as sa
from seriation_amd import _lib as L
from seriation_amd import analysis


def literal(X, rec):
    """the definition cell by cell and sample by sample, in Python integers"""
    N, M = X.shape
    out = {"alive": np.zeros((N, M), np.int64)}
    for k in occ_ref.KINDS[1:4]:
        out[k] = np.zeros((N, M + 1), np.int64)
    for k in occ_ref.KINDS[4:]:
        out[k] = np.zeros((M, N + 1), np.int64)
    for row in rec.reshape(-1, 2 * M + N).tolist():
        a, b, pi = row[:M], row[M:2 * M], row[2 * M:]
        site = [[0, 0, 0] for _ in range(N)]
        taxon = [[0, 0, 0] for _ in range(M)]
        for n in range(N):
            for m in range(M):
                al, x = a[m] <= pi[n] < b[m], bool(X[n, m])
                out["alive"][n, m] += al
                for i, bit in enumerate((al, al and not x, not al and x)):
                    site[n][i] += bit
                    taxon[m][i] += bit
        for i, name in enumerate(("alive", "f0", "f1")):
            for n in range(N):
                out["site_%s_hist" % name][n, site[n][i]] += 1
            for m in range(M):
                out["taxon_%s_hist" % name][m, taxon[m][i]] += 1
    return out


def tiny(N, M, n_sel, count, seed, full):
    rng = np.random.RandomState(seed)
    X = rng.randint(0, 2, (N, M)).astype(np.uint8)
    W = 2 * M + N
    if full:   # any int16, most entries near [0, N] so that alive cells exist, the extremes placed
        rec = rng.randint(-32768, 32768, (n_sel, count, W))
        near = rng.randint(-2, N + 3, (n_sel, count, W))
        take = rng.randint(0, 4, (n_sel, count, W)) > 0
        rec[take] = near[take]
        rec[0, 0, 0], rec[0, 0, M], rec[0, 0, 2 * M] = -32768, 32767, 32766
        rec[-1, -1, M - 1], rec[-1, -1, W - 1] = 32767, -32768
    else:
        rec = np.empty((n_sel, count, W), np.int64)
        for k in range(n_sel):
            for r in range(count):
                a = rng.randint(0, N + 1, M)
                rec[k, r, :M], rec[k, r, M:2 * M] = a, a + rng.randint(0, N + 1, M) % (N + 1 - a)
                rec[k, r, 2 * M:] = rng.permutation(N)
    return X, rec.astype(np.int16)


CASES = [(1, 1, 1, 1, False), (1, 1, 2, 3, True), (4, 3, 2, 5, False), (3, 5, 2, 4, True), (5, 2, 1, 7, True),
         (6, 7, 3, 3, False)]


@pytest.mark.parametrize("N,M,n_sel,count,full", CASES)
def test_definition_equals_the_literal_loop(N, M, n_sel, count, full):
    X, rec = tiny(N, M, n_sel, count, 11 * N + M, full)
    got, want = occ_ref.occupancy(X, rec), literal(X, rec)
    assert got["total"] == n_sel * count
    for k in occ_ref.KINDS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    if full:
        assert got["alive"][0, 0] >= 1   # a = -32768 <= pi = 32766 < b = 32767


@pytest.mark.parametrize("N,M,n_sel,count,full", CASES)
def test_structural_identities(N, M, n_sel, count, full):
    X, rec = tiny(N, M, n_sel, count, 5 * N + M, full)
    r = occ_ref.occupancy(X, rec)
    T, x, alive = n_sel * count, X.astype(np.int64), r["alive"]
    for k in occ_ref.KINDS[1:]:
        assert (r[k].sum(axis=1) == T).all(), k

    def first_moment(h):
        return (h * np.arange(h.shape[1])[None, :]).sum(axis=1)

    for axis, pre in ((1, "site_"), (0, "taxon_")):
        assert np.array_equal(first_moment(r[pre + "alive_hist"]), alive.sum(axis=axis))
        assert np.array_equal(first_moment(r[pre + "f0_hist"]), ((1 - x) * alive).sum(axis=axis))
        assert np.array_equal(first_moment(r[pre + "f1_hist"]), (x * (T - alive)).sum(axis=axis))


def raw_dataset(N, M):
    """an sr_dataset of any claimed shape without its matrix: the checks read N and M only"""
    ds = L.sr_dataset()
    ds.N, ds.M = N, M
    return ds


def call(n_sel, count, N=3, M=2, want=occ_ref.KINDS, ds=True, rec=True, out=True):
    """sr_occupancy through ctypes; the requested outputs point at one small buffer, which no refused call touches."""
    buf = np.zeros(64, np.uint32)
    r = np.zeros((1, 8, 7), np.int16)
    o = L.sr_occ_out()
    o.kernel_ms = -1.0
    for k in want:
        setattr(o, k, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    rc = sa.lib().sr_occupancy(ctypes.byref(raw_dataset(N, M)) if ds else None,
                               r.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)) if rec else None, n_sel, count, 0,
                               ctypes.byref(o) if out else None)
    assert not buf.any() and o.kernel_ms == -1.0
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
    assert sa.lib().sr_session_occupancy(None, None, 1, 0, 8, ctypes.byref(L.sr_occ_out())) == L.SR_EINVAL
    # an invalid argument wins over a shape that is too large
    assert call(0, 8, N=32767, M=8193) == L.SR_EINVAL


def test_shapes_too_large_unsupported():
    """N M > 2^27, or a requested histogram above 1 GiB: SR_EUNSUPPORTED before any device call."""
    assert call(1, 8, N=32767, M=4097, want=()) == L.SR_EUNSUPPORTED        # N M = 2^27 + 28671, whatever is asked
    assert call(1, 8, N=32767, M=4097, want=("alive",)) == L.SR_EUNSUPPORTED
    assert call(1, 8, N=2, M=2 ** 26 + 1, want=("taxon_f0_hist",)) == L.SR_EUNSUPPORTED
    # a histogram beyond 2^28 entries: under the cell bound none is (N (M + 1) <= 2^27 + 32767, M (N + 1) <= 2^28), so
    # such a shape is past the cell bound too
    for k in occ_ref.KINDS[1:]:
        assert call(1, 8, N=32767, M=8193, want=(k,)) == L.SR_EUNSUPPORTED


def test_host_only_library_exports_and_refuses():
    """The fake-device library (no device layer, so no occupancy kernels) still links, exports both functions, and
    answers a valid sr_occupancy call with SR_EUNSUPPORTED, an invalid one with SR_EINVAL, the outputs untouched."""
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(sa.__file__)))
    subprocess.check_call(["make", "-s", "-C", pkg, "build/fake/libseriation.so"])
    code = ("import ctypes, numpy as np, seriation_amd as sa\n"
            "from seriation_amd import _lib as L\n"
            "lib = sa.lib()\n"
            "assert all(hasattr(lib, s) for s in ('sr_occupancy', 'sr_session_occupancy'))\n"
            "ds = sa.Dataset.parse(b'3 2\\n1 0\\n1 1\\n0 1\\n')\n"
            "rec = np.zeros((1, 8, 7), np.int16)\n"
            "recp = rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))\n"
            "buf = np.zeros(6, np.uint32)\n"
            "out = L.sr_occ_out()\n"
            "out.alive = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))\n"
            "print(lib.sr_occupancy(ctypes.byref(ds.c), recp, 1, 8, 0, ctypes.byref(out)),"
            " lib.sr_occupancy(ctypes.byref(ds.c), recp, 0, 8, 0, ctypes.byref(out)), int(buf.any()))\n")
    env = dict(os.environ, SERIATION_LIB=os.path.join(pkg, "build", "fake", "libseriation.so"),
               PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == [str(L.SR_EUNSUPPORTED), str(L.SR_EINVAL), "0"], r.stdout + r.stderr


def test_derived_values():
    """p_alive, p_false_zero, p_false_one and site_completeness are the stated divisions, NaN where stated."""
    assert analysis.OCC_KINDS == occ_ref.KINDS
    X = np.array([[1, 0, 1], [0, 0, 0], [1, 1, 0], [0, 1, 1]], np.uint8)
    alive = np.array([[7, 0, 3], [2, 7, 1], [0, 0, 5], [0, 0, 0]], np.uint32)   # row 2: found taxa never alive
    T = 7
    got, want = analysis.occupancy_derived(alive, X, T), occ_ref.derived(alive, X, T)
    for k in ("p_alive", "p_false_zero", "p_false_one", "site_completeness"):
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape, k
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        assert np.array_equal(got[k][~np.isnan(want[k])].view(np.uint64), want[k][~np.isnan(want[k])].view(np.uint64)), k
    assert np.array_equal(np.isnan(got["p_false_zero"]), X != 0) and np.array_equal(np.isnan(got["p_false_one"]), X == 0)
    assert got["p_false_one"][0, 0] == 0.0 and got["p_false_one"][2, 0] == 1.0 and got["p_false_zero"][1, 1] == 1.0
    assert got["site_completeness"].tolist()[:3] == [1.0, 0.0, 0.0] and np.isnan(got["site_completeness"][3])
    # the histograms' means and bands are diversity_curve's: the mean is the first moment over T
    r = occ_ref.occupancy(*tiny(4, 3, 2, 5, 3, False))
    dc = analysis.diversity_curve(r["site_f0_hist"], analysis.PROBS)
    x = tiny(4, 3, 2, 5, 3, False)[0].astype(np.int64)
    assert np.array_equal(dc["mean"], ((1 - x) * r["alive"]).sum(axis=1).astype(np.float64) / 10.0)


@pytest.mark.parametrize("extra", [[], ["--select", "2", "--no-save"]])
def test_cli_occupancy_needs_select(capsys, extra):
    from seriation_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["nowhere.txt", "--occupancy"] + extra)
    assert e.value.code == 2 and "--occupancy" in capsys.readouterr().err
