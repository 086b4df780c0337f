"""The host side of the central sampled state: the numpy definition (tests/central_ref.py) against a literal triple
loop and a literal Kendall count, every argument error (reported before any device call, the outputs untouched), the
host-only library, the command line's refusal, and the known answer on the oracle's g10s10 records.  CPU only: counts
and losses come from the GPU in tests/test_gpu_central.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import central_ref
import oracle_ref
import seriation_amd as sa
from seriation_amd import _lib as L

I64P = ctypes.POINTER(ctypes.c_int64)
I32P = ctypes.POINTER(ctypes.c_int32)
U32P = ctypes.POINTER(ctypes.c_uint32)
I16P = ctypes.POINTER(ctypes.c_int16)
G10S10 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datasets", "g10s10.txt")


def test_ref_matches_triple_loop():
    N, M, n_sel, count = 4, 2, 3, 7
    rng = np.random.RandomState(12)
    rec = rng.randint(-3, 8, (n_sel, count, 2 * M + N))   # few values: many ties, limits on both sides of [0, N]
    rec[0, 0, 2 * M], rec[0, 0, 2 * M + 1], rec[1, 3, 2 * M + 3], rec[2, 6, 2 * M] = -32768, 32767, 32767, -32768
    rec[2, 5, 2 * M:] = 32767                             # a row of ties at the extreme
    rec[0, 1, 0], rec[0, 1, M], rec[1, 2, 1], rec[1, 2, M + 1] = -32768, 32767, 32767, -32768   # limits at the extremes
    rec = rec.astype(np.int16)
    flips = [0, 1, 0]
    rows = []   # (a', b', pi') of every row as Python ints
    for k in range(n_sel):
        for row in rec[k].tolist():
            a, b, pi = row[:M], row[M:2 * M], row[2 * M:]
            if flips[k]:
                a, b, pi = [N - v for v in row[M:2 * M]], [N - v for v in row[:M]], [N - 1 - v for v in pi]
            rows.append((a, b, pi))
    C = [[sum(pi[i] < pi[j] for _a, _b, pi in rows) for j in range(N)] for i in range(N)]
    ol = [sum((pi[i] < pi[j]) * C[j][i] + (pi[i] > pi[j]) * C[i][j] for i in range(N) for j in range(i + 1, N))
          for _a, _b, pi in rows]

    def clamp(v):
        return min(max(v, 0), N)

    ll = [sum(abs(clamp(a[m]) - clamp(sa_[m])) + abs(clamp(b[m]) - clamp(sb[m])) for sa_, sb, _p in rows for m in range(M))
          for a, b, _pi in rows]
    keys = [(ol[r], ll[r], r // count, r % count) for r in range(n_sel * count)]
    got = central_ref.central(rec, N, M, flips)
    assert got["pair_counts"].dtype == np.uint32 and np.array_equal(got["pair_counts"], np.array(C))
    assert got["order_loss"].dtype == np.int64 and np.array_equal(got["order_loss"].ravel(), np.array(ol))
    assert got["limit_loss"].dtype == np.int64 and np.array_equal(got["limit_loss"].ravel(), np.array(ll))
    assert got["central"] == min(keys)[2:]
    assert list(got["best"]) == [min(x for x in keys if x[2] == k)[3] for k in range(n_sel)]
    a, b, pi = rows[got["central"][0] * count + got["central"][1]]
    assert got["state"]["a"].tolist() == a and got["state"]["b"].tolist() == b and got["state"]["pi"].tolist() == pi
    assert got["scale"] == n_sel * count * 6
    pc = got["pair_counts"].astype(np.int64)
    assert not np.diag(pc).any() and (pc + pc.T < n_sel * count).any()   # the ties
    assert max(max(abs(v) for v in a + b) for a, b, _p in rows) > 32767   # a reflected extreme left int16's range


def test_order_loss_is_the_sum_of_kendall_distances():
    """Permutation rows, one chain flagged: a row's order loss is the number of discordant pairs between it and every
    row, counted literally."""
    N, M, n_sel, count = 7, 3, 3, 11
    rng = np.random.RandomState(3)
    rec = np.empty((n_sel, count, 2 * M + N), np.int16)
    rec[:, :, :2 * M] = rng.randint(0, N + 1, (n_sel, count, 2 * M))
    for k in range(n_sel):
        for t in range(count):
            rec[k, t, 2 * M:] = rng.permutation(N)
    flips = [0, 0, 1]
    _a, _b, pi = central_ref.oriented(rec, N, M, flips)
    P = pi.tolist()

    def kendall(x, y):
        return sum((x[i] < x[j]) != (y[i] < y[j]) for i in range(N) for j in range(i + 1, N))

    want = np.array([sum(kendall(x, y) for y in P) for x in P]).reshape(n_sel, count)
    got = central_ref.central(rec, N, M, flips)
    assert np.array_equal(got["order_loss"], want)
    C = got["pair_counts"].astype(np.int64)
    assert got["order_loss"].sum() == 2 * np.triu(C * C.T, 1).sum()
    assert not np.array_equal(central_ref.central(rec, N, M)["order_loss"], want)   # the flag matters


def raw_dataset(N, M):
    """an sr_dataset of any claimed shape without its matrix: the checks read N and M only"""
    ds = L.sr_dataset()
    ds.N, ds.M = N, M
    return ds


OUTS = ("order_loss", "limit_loss", "pair_counts", "best", "state")


def call(n_sel, count, N=3, M=2, want=OUTS, ds=True, rec=True, out=True):
    """sr_central through ctypes; the requested outputs point at small buffers, which no refused call touches."""
    bufs = {"order_loss": np.full(64, 77, np.int64), "limit_loss": np.full(64, 77, np.int64),
            "pair_counts": np.full(64, 77, np.uint32), "best": np.full(64, 77, np.int32), "state": np.full(64, 77, np.int32)}
    types = {"order_loss": I64P, "limit_loss": I64P, "pair_counts": U32P, "best": I32P, "state": I32P}
    r = np.zeros((1, 8, 7), np.int16)
    o = L.sr_central_out()
    o.central_chain, o.central_row, o.scale, o.kernel_ms = -5, -5, -5, -5.0
    for k in want:
        setattr(o, k, bufs[k].ctypes.data_as(types[k]))
    rc = sa.lib().sr_central(ctypes.byref(raw_dataset(N, M)) if ds else None, r.ctypes.data_as(I16P) if rec else None,
                             n_sel, count, 0, ctypes.byref(o) if out else None)
    assert all((b == 77).all() for b in bufs.values())
    assert (o.central_chain, o.central_row, o.scale, o.kernel_ms) == (-5, -5, -5, -5.0)
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
    assert call(65536, 32768) == L.SR_EINVAL         # T = 2^31
    assert call(2, 2 ** 30) == L.SR_EINVAL
    assert call(1, 8, N=0) == L.SR_EINVAL            # N outside 1..32767
    assert call(1, 8, N=-4) == L.SR_EINVAL
    assert call(1, 8, N=32768) == L.SR_EINVAL
    assert call(1, 8, M=0) == L.SR_EINVAL            # M < 1
    assert call(1, 8, M=-2) == L.SR_EINVAL
    # 2 M N T >= 2^62: 2 * 2^30 * 2^14 * 2^17 = 2^62 exactly, and shapes whose product does not fit 64 bits
    assert call(2 ** 9, 2 ** 8, N=2 ** 14, M=2 ** 30, want=()) == L.SR_EINVAL
    assert call(2 ** 8, 2 ** 8, N=2 ** 15 - 1, M=2 ** 31 - 1, want=()) == L.SR_EINVAL
    assert call(32767, 65536, N=32767, M=2 ** 31 - 1) == L.SR_EINVAL
    assert sa.lib().sr_session_central(None, None, 1, 0, 8, ctypes.byref(L.sr_central_out())) == L.SR_EINVAL
    # an invalid argument wins over what is unsupported
    assert call(0, 8, N=32767, want=("pair_counts",)) == L.SR_EINVAL
    assert call(1, 8, N=16385, M=0, want=("pair_counts",)) == L.SR_EINVAL


def test_unsupported():
    """A requested pair_counts above 1 GiB: SR_EUNSUPPORTED before any device call; not asked for, the shape is fine
    (and reaches the device layer, which this build has: not called here)."""
    assert call(1, 8, N=16385, want=("pair_counts",)) == L.SR_EUNSUPPORTED      # N N = 2^28 + 2^15 + 1
    assert call(4, 8, N=32767, want=OUTS) == L.SR_EUNSUPPORTED


def test_order_loss_argument_checks():
    lib = sa.lib()
    r, ag = np.zeros((1, 8, 7), np.int16), np.zeros((3, 3), np.uint32)
    loss, ms = np.full(64, 77, np.int64), ctypes.c_double(-5.0)

    def ocall(n_sel=1, count=8, N=3, M=2, ds=True, rec=True, against=True, out=True):
        rc = lib.sr_order_loss(ctypes.byref(raw_dataset(N, M)) if ds else None, r.ctypes.data_as(I16P) if rec else None,
                               n_sel, count, None, ag.ctypes.data_as(U32P) if against else None, 0,
                               loss.ctypes.data_as(I64P) if out else None, ctypes.byref(ms))
        assert (loss == 77).all() and ms.value == -5.0
        return rc

    for bad in (dict(ds=False), dict(rec=False), dict(against=False), dict(out=False), dict(n_sel=0), dict(n_sel=-1),
                dict(count=0), dict(count=-3), dict(n_sel=65536, count=32768), dict(N=0), dict(N=32768), dict(M=0)):
        assert ocall(**bad) == L.SR_EINVAL, bad


def test_host_only_library_exports_and_refuses():
    """The fake-device library (no device layer, so no central kernels) still links, exports the three functions and
    answers valid calls with SR_EUNSUPPORTED and an invalid one with SR_EINVAL."""
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(sa.__file__)))
    subprocess.check_call(["make", "-s", "-C", pkg, "build/fake/libseriation.so"])
    code = ("import ctypes, numpy as np, seriation_amd as sa\n"
            "from seriation_amd import _lib as L\n"
            "lib = sa.lib()\n"
            "assert all(hasattr(lib, s) for s in ('sr_central', 'sr_session_central', 'sr_order_loss'))\n"
            "ds = sa.Dataset.parse(b'3 2\\n1 0\\n1 1\\n0 1\\n')\n"
            "rec = np.zeros((1, 8, 7), np.int16)\n"
            "recp = rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))\n"
            "buf = np.zeros(8, np.int64)\n"
            "out = L.sr_central_out()\n"
            "out.order_loss = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))\n"
            "ag = np.zeros((3, 3), np.uint32)\n"
            "print(lib.sr_central(ctypes.byref(ds.c), recp, 1, 8, 0, ctypes.byref(out)),"
            " lib.sr_central(ctypes.byref(ds.c), recp, 0, 8, 0, ctypes.byref(out)),"
            " lib.sr_order_loss(ctypes.byref(ds.c), recp, 1, 8, None, ag.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 0,"
            " buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None))\n")
    env = dict(os.environ, SERIATION_LIB=os.path.join(pkg, "build", "fake", "libseriation.so"),
               PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == [str(L.SR_EUNSUPPORTED), str(L.SR_EINVAL), str(L.SR_EUNSUPPORTED)], \
        r.stdout + r.stderr


@pytest.mark.parametrize("argv", [["--central"], ["--central", "--select", "2", "--no-save"]])
def test_cli_central_needs_select_and_chain_files(capsys, argv):
    from seriation_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["nowhere.txt"] + argv)
    assert e.value.code == 2 and "--central" in capsys.readouterr().err


def test_known_answer_from_the_oracle():
    """The central row of three short chains on g10s10, computed from the oracle's records by the numpy definition,
    against the values pinned when the test was written."""
    kn = central_ref.KNOWN
    text = open(G10S10, "rb").read()
    runs = [oracle_ref.run_chain(text, seed, 0, kn["calls"]) for seed in kn["seeds"]]
    assert all(o["rc"] == 0 for o in runs)
    N, M = runs[0]["N"], runs[0]["M"]
    res = central_ref.central(np.stack([o["rec_int"] for o in runs]).astype(np.int16), N, M)
    check_known(res)
    # the central row is a state the sampler produced: a permutation with a <= b in every taxon
    assert sorted(res["state"]["pi"].tolist()) == list(range(N)) and (res["state"]["a"] <= res["state"]["b"]).all()


def check_known(res):
    kn = central_ref.KNOWN
    ck, ct = res["central"]
    assert (ck, ct) == kn["central"] and list(res["best"]) == kn["best"] and res["scale"] == kn["scale"]
    assert int(res["order_loss"][ck][ct]) == kn["order_loss"] and int(res["limit_loss"][ck][ct]) == kn["limit_loss"]
