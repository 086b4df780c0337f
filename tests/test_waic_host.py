"""The host side of WAIC: the numpy definition (tests/waic_ref.py) against a literal per-cell, per-sample loop,
sr_waic_reduce and analysis.waic_compare against the sequential definitions, every argument error of sr_waic, which
must be reported before any kernel runs, and analysis.read_chain_cd.  CPU only: the pointwise terms come from the GPU
in tests/test_gpu_waic.py."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import seriation_amd as sa
import waic_ref
from seriation_amd import _lib as L
from seriation_amd import analysis

_DBLP = ctypes.POINTER(ctypes.c_double)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def brute(X, rec, cd, manycd):
    """The definition read literally, one cell and one sample at a time: lppd, ll_mean, pwaic as nested lists."""
    N, M = len(X), len(X[0])
    n_sel, count = len(rec), len(rec[0])
    T = n_sel * count

    def terms(k, r, m):
        row = cd[k][r]
        c, d = (row[m], row[M + m]) if manycd else (row[0], row[1])
        ec, ed = math.exp(c), math.exp(d)
        return [1.0 - ec, ed, 1.0 - ed, ec], [math.log(1.0 - ec), d, math.log(1.0 - ed), c]

    def idx(k, r, n, m):
        row = rec[k][r]
        alive = row[m] <= row[2 * M + n] < row[M + m]
        return (2 if alive else 3) if X[n][m] else (1 if alive else 0)

    def total(f, n, m):
        tot = 0.0
        for k in range(n_sel):
            s = 0.0
            for r in range(count):
                s += f(k, r, n, m)
            tot += s
        return tot

    lppd, mean, pw = ([[0.0] * M for _ in range(N)] for _ in range(3))
    for n in range(N):
        for m in range(M):
            sp = total(lambda k, r, n, m: terms(k, r, m)[0][idx(k, r, n, m)], n, m)
            sl = total(lambda k, r, n, m: terms(k, r, m)[1][idx(k, r, n, m)], n, m)
            mu = sl / float(T)
            v = total(lambda k, r, n, m: (terms(k, r, m)[1][idx(k, r, n, m)] - mu) * (terms(k, r, m)[1][idx(k, r, n, m)] - mu),
                      n, m)
            lppd[n][m], mean[n][m], pw[n][m] = math.log(sp / float(T)), mu, v / float(T - 1)
    return lppd, mean, pw


@pytest.mark.parametrize("manycd", [False, True])
def test_ref_matches_brute_force(manycd):
    N, M, n_sel, count = 4, 3, 3, 7
    rng = np.random.RandomState(11 + manycd)
    X = rng.randint(0, 2, (N, M))
    rec = rng.randint(-1, N + 2, (n_sel, count, 2 * M + N))
    rec[0, 0, 0], rec[1, 2, M + 1], rec[2, 3, 2 * M] = -32768, 32767, 32767
    cd = -rng.uniform(0.05, 7.0, (n_sel, count, 2 * M if manycd else 3))
    lppd, mean, pw = brute(X.tolist(), rec.tolist(), cd.tolist(), manycd)
    got = waic_ref.waic(X, rec.astype(np.int16), cd, manycd)
    assert np.array_equal(bits(got["lppd"]), bits(lppd))
    assert np.array_equal(bits(got["ll_mean"]), bits(mean))
    assert np.array_equal(bits(got["pwaic"]), bits(pw))
    assert (got["pwaic"] > 0).all() and (got["lppd"] >= got["ll_mean"] - 1e-12).all()
    # the reduction, by loops
    e = [[a - b for a, b in zip(ra, rb)] for ra, rb in zip(lppd, pw)]
    tot = 0.0
    for row in e:
        for v in row:
            tot += v
    assert bits(got["elpd_waic"]) == bits(tot) and bits(got["waic"]) == bits(-2.0 * tot)
    for n in range(N):
        s = 0.0
        for m in range(M):
            s += e[n][m]
        assert bits(got["site_elpd"][n]) == bits(s)
    for m in range(M):
        s = 0.0
        for n in range(N):
            s += e[n][m]
        assert bits(got["taxon_elpd"][m]) == bits(s)


def c_reduce(lppd, pwaic, site=True, taxon=True):
    lppd, pwaic = np.ascontiguousarray(lppd, np.float64), np.ascontiguousarray(pwaic, np.float64)
    N, M = lppd.shape
    out = L.sr_waic_out()
    se, te = np.full(N, 7.0), np.full(M, 7.0)
    if site:
        out.site_elpd = se.ctypes.data_as(_DBLP)
    if taxon:
        out.taxon_elpd = te.ctypes.data_as(_DBLP)
    rc = sa.lib().sr_waic_reduce(N, M, lppd.ctypes.data_as(_DBLP), pwaic.ctypes.data_as(_DBLP), ctypes.byref(out))
    assert rc == L.SR_OK
    return out, se, te


def test_reduce_against_sequential_definition():
    rng = np.random.RandomState(3)
    for N, M in ((1, 1), (1, 5), (6, 1), (7, 9), (40, 33)):
        lppd = -rng.uniform(1e-3, 9.0, (N, M)) * 10.0 ** rng.randint(-3, 3, (N, M))
        pwaic = rng.uniform(0.0, 0.8, (N, M))
        out, se, te = c_reduce(lppd, pwaic)
        e = (lppd - pwaic).reshape(-1).tolist()
        sl = sp = tot = 0.0
        for a, b, v in zip(lppd.reshape(-1).tolist(), pwaic.reshape(-1).tolist(), e):
            sl += a
            sp += b
            tot += v
        me, q = tot / float(N * M), 0.0
        for v in e:
            q += (v - me) * (v - me)
        assert bits(out.lppd_sum) == bits(sl) and bits(out.p_waic) == bits(sp) and bits(out.elpd) == bits(tot)
        assert bits(out.waic) == bits(-2.0 * tot) and out.n_high == int((pwaic > 0.4).sum())
        if N * M == 1:
            assert math.isnan(out.se)
        else:
            assert bits(out.se) == bits(math.sqrt(float(N * M) * (q / float(N * M - 1))))
        want = waic_ref.reduce(lppd, pwaic)
        for k, v in (("elpd_waic", out.elpd), ("se", out.se), ("p_waic", out.p_waic), ("lppd_sum", out.lppd_sum),
                     ("waic", out.waic)):
            assert bits(want[k]) == bits(v), k
        assert want["n_high"] == out.n_high
        assert np.array_equal(bits(se), bits(want["site_elpd"])) and np.array_equal(bits(te), bits(want["taxon_elpd"]))
        # the optional outputs are left alone when not asked for
        out2, se2, te2 = c_reduce(lppd, pwaic, site=False, taxon=False)
        assert (se2 == 7.0).all() and (te2 == 7.0).all() and bits(out2.elpd) == bits(tot)
    lib = sa.lib()
    one = np.zeros(1)
    o = L.sr_waic_out()
    p = one.ctypes.data_as(_DBLP)
    assert lib.sr_waic_reduce(1, 1, None, p, ctypes.byref(o)) == L.SR_EINVAL
    assert lib.sr_waic_reduce(1, 1, p, None, ctypes.byref(o)) == L.SR_EINVAL
    assert lib.sr_waic_reduce(1, 1, p, p, None) == L.SR_EINVAL
    assert lib.sr_waic_reduce(0, 1, p, p, ctypes.byref(o)) == L.SR_EINVAL
    assert lib.sr_waic_reduce(1, 0, p, p, ctypes.byref(o)) == L.SR_EINVAL


def test_compare_against_sequential_definition():
    rng = np.random.RandomState(8)
    for shape in ((1, 1), (3, 4), (25, 31)):
        a = {"elpd": -rng.uniform(0.01, 5.0, shape)}
        b = {"elpd": -rng.uniform(0.01, 5.0, shape)}
        got, want = analysis.waic_compare(a, b), waic_ref.compare(a, b)
        assert set(got) == {"elpd_diff", "se_diff"}
        assert bits(got["elpd_diff"]) == bits(want["elpd_diff"])
        if shape == (1, 1):
            assert math.isnan(got["se_diff"]) and math.isnan(want["se_diff"])
        else:
            assert bits(got["se_diff"]) == bits(want["se_diff"]) and got["se_diff"] > 0
        back = analysis.waic_compare(b, a)
        assert bits(back["elpd_diff"]) == bits(-want["elpd_diff"])
    assert analysis.waic_compare(a, a) == {"elpd_diff": 0.0, "se_diff": 0.0}
    with pytest.raises(AssertionError):
        analysis.waic_compare({"elpd": np.zeros((2, 3))}, {"elpd": np.zeros((3, 2))})


def call(n_sel, count, N=3, M=2, manycd=0, cd=None, ds=True, rec=True, cdp=True, out=True, X=True):
    """sr_waic through ctypes on a dataset of any claimed shape (the checks before the rates read N and M only);
    every output points at a small buffer, which no refused call touches.  cd: the values of the first row."""
    buf = np.full(16, 5.0)
    r = np.zeros((1, 8, 7), np.int16)
    r[:, :, 2:4] = 3
    x = np.zeros(6, np.uint8)
    rates = np.full((8, 4 if manycd else 3), -1.0)
    if cd is not None:
        rates[0, :len(cd)] = cd
    d = L.sr_dataset()
    d.N, d.M = N, M
    if X:
        d.X = x.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    o = L.sr_waic_out()
    for k in ("lppd", "ll_mean", "pwaic", "site_elpd", "taxon_elpd"):
        setattr(o, k, buf.ctypes.data_as(_DBLP))
    o.elpd = o.kernel_ms = 5.0
    rc = sa.lib().sr_waic(ctypes.byref(d) if ds else None, r.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)) if rec else None,
                          rates.ctypes.data_as(_DBLP) if cdp else None, manycd, n_sel, count, 0,
                          ctypes.byref(o) if out else None)
    if rc != L.SR_OK:
        assert (buf == 5.0).all() and o.elpd == 5.0 and o.kernel_ms == 5.0
    return rc


def accepted():
    """what a call whose arguments are in order returns: the device's answer"""
    return L.SR_OK if sa.lib().sr_device_count() > 0 else L.SR_EDEVICE


def test_argument_checks():
    """Every SR_EINVAL case of the definition; none of them reaches the device (this test runs without one)."""
    assert call(1, 8, ds=False) == L.SR_EINVAL
    assert call(1, 8, rec=False) == L.SR_EINVAL
    assert call(1, 8, cdp=False) == L.SR_EINVAL
    assert call(1, 8, out=False) == L.SR_EINVAL
    assert call(1, 8, X=False) == L.SR_EINVAL
    assert call(0, 8) == L.SR_EINVAL                 # n_sel <= 0
    assert call(-1, 8) == L.SR_EINVAL
    assert call(1, 0) == L.SR_EINVAL                 # count < 1
    assert call(1, -3) == L.SR_EINVAL
    assert call(1, 1) == L.SR_EINVAL                 # T < 2
    assert call(65536, 32768) == L.SR_EINVAL         # T = 2^31
    assert call(2, 2 ** 30) == L.SR_EINVAL
    assert call(1, 8, N=0) == L.SR_EINVAL            # N outside 1..32767
    assert call(1, 8, N=-4) == L.SR_EINVAL
    assert call(1, 8, N=32768) == L.SR_EINVAL
    assert call(1, 8, M=0) == L.SR_EINVAL            # M < 1
    assert call(1, 8, M=-1) == L.SR_EINVAL
    assert sa.lib().sr_session_waic(None, None, 1, 0, 8, ctypes.byref(L.sr_waic_out())) == L.SR_EINVAL
    # an invalid argument wins over a matrix that is too large
    assert call(0, 8, N=1, M=2 ** 27 + 1) == L.SR_EINVAL


def test_cells_beyond_limit_unsupported():
    assert call(1, 8, N=1, M=2 ** 27 + 1) == L.SR_EUNSUPPORTED
    assert call(1, 8, N=32767, M=4097) == L.SR_EUNSUPPORTED      # 32767 * 4097 > 2^27
    assert call(1, 8, N=2 ** 14, M=2 ** 13 + 1) == L.SR_EUNSUPPORTED


LO, HI = -700.0, -2.0 ** -50


@pytest.mark.parametrize("manycd", [0, 1])
def test_rate_domain(manycd):
    """c, d in [-700, -2^-50]: the edges are accepted (the call goes on to the device), everything just outside,
    +0.0, NaN and the infinities are refused, in either slot and, manycd, in any taxon's."""
    slots = range(4) if manycd else range(2)
    for edge in (LO, HI):
        for j in slots:
            cd = [-1.0] * len(slots)
            cd[j] = edge
            assert call(1, 8, manycd=manycd, cd=cd) == accepted()
    bad = (np.nextafter(LO, -np.inf), np.nextafter(HI, 0.0), -0.0, 0.0, 1e-300, 1.0, float("nan"), float("inf"),
           float("-inf"), -1e308)
    for v in bad:
        for j in slots:
            cd = [-1.0] * len(slots)
            cd[j] = v
            assert call(1, 8, manycd=manycd, cd=cd) == L.SR_EINVAL, (v, j)
    if not manycd:   # the loglik entry is not read
        for v in (0.0, float("nan"), float("inf"), 12.5):
            assert call(1, 8, cd=[-1.0, -1.0, v]) == accepted()


def test_rate_domain_last_row():
    """a bad value in the last row that is read is found; one beyond the rows that are read is not looked at"""
    buf = np.full(16, 5.0)
    r = np.zeros((2, 4, 7), np.int16)
    ds = sa.Dataset(np.zeros((3, 2), np.uint8), np.zeros(3, bool))
    rates = np.full((2, 4, 3), -1.0)
    rates[1, 3, 1] = 0.5
    o = L.sr_waic_out()
    o.lppd = buf.ctypes.data_as(_DBLP)
    args = (ctypes.byref(ds.c), r.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), rates.ctypes.data_as(_DBLP), 0)
    assert sa.lib().sr_waic(*args, 2, 4, 0, ctypes.byref(o)) == L.SR_EINVAL and (buf == 5.0).all()
    assert sa.lib().sr_waic(*args, 1, 4, 0, ctypes.byref(o)) == accepted()


def test_host_only_library_exports_and_refuses():
    """The fake-device library (no device layer, so no WAIC kernels) still links, exports the three functions,
    answers a valid sr_waic call with SR_EUNSUPPORTED and an invalid one with SR_EINVAL, and reduces."""
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(sa.__file__)))
    subprocess.check_call(["make", "-s", "-C", pkg, "build/fake/libseriation.so"])
    code = ("import ctypes, numpy as np, seriation_amd as sa\n"
            "from seriation_amd import _lib as L\n"
            "lib = sa.lib()\n"
            "assert all(hasattr(lib, s) for s in ('sr_waic', 'sr_session_waic', 'sr_waic_reduce'))\n"
            "ds = sa.Dataset.parse(b'3 2\\n1 0\\n1 1\\n0 1\\n')\n"
            "rec = np.zeros((1, 8, 7), np.int16)\n"
            "recp = rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))\n"
            "cd = np.full((1, 8, 3), -1.0)\n"
            "cdp = cd.ctypes.data_as(ctypes.POINTER(ctypes.c_double))\n"
            "out = L.sr_waic_out()\n"
            "print(lib.sr_waic(ctypes.byref(ds.c), recp, cdp, 0, 1, 8, 0, ctypes.byref(out)),"
            " lib.sr_waic(ctypes.byref(ds.c), recp, cdp, 0, 0, 8, 0, ctypes.byref(out)),"
            " lib.sr_waic_reduce(1, 3, cdp, cdp, ctypes.byref(out)), out.elpd)\n")
    env = dict(os.environ, SERIATION_LIB=os.path.join(pkg, "build", "fake", "libseriation.so"),
               PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == [str(L.SR_EUNSUPPORTED), str(L.SR_EINVAL), "0", "0.0"], \
        r.stdout + r.stderr


def test_read_chain_cd(tmp_path):
    """fields 3, 4 and 5 of chain_data.csv: the log of the first token (shared rates) or of all M tokens"""
    M = 3
    lines = {4: ["1 2 3 ,4 5 6 ,0 1 ,0.01000000000000 0.02000000000000 0.03000000000000 ,"
                 "0.30000000000000 0.40000000000000 0.50000000000000 ,-123.45600000000000\n",
                 "1 2 3 ,4 5 6 ,1 0 ,0.00100000000000 0.09990000000000 0.05000000000000 ,"
                 "0.79999999999999 0.20000000000000 0.25000000000000 ,-99.00000000000000\n"],
             11: ["0 0 0 ,2 2 2 ,0 1 ,0.05000000000000 0.05000000000000 0.05000000000000 ,"
                  "0.60000000000000 0.60000000000000 0.60000000000000 ,-7.50000000000000\n",
                  "0 0 0 ,2 2 2 ,0 1 ,0.07000000000000 0.07000000000000 0.07000000000000 ,"
                  "0.45000000000000 0.45000000000000 0.45000000000000 ,-8.25000000000000\n"]}
    for chain, rows in lines.items():
        d = tmp_path / "Chains" / ("chain_%02d" % chain)
        d.mkdir(parents=True)
        (d / "chain_data.csv").write_text("".join(rows))
    shared = analysis.read_chain_cd(str(tmp_path), [11, 4], M)
    assert shared.shape == (2, 2, 3) and shared.dtype == np.float64
    want = [[[math.log(0.05), math.log(0.6), -7.5], [math.log(0.07), math.log(0.45), -8.25]],
            [[math.log(0.01), math.log(0.3), -123.456], [math.log(0.001), math.log(0.79999999999999), -99.0]]]
    assert np.array_equal(bits(shared), bits(want))
    many = analysis.read_chain_cd(str(tmp_path), [4], M, manycd=True)
    assert many.shape == (1, 2, 2 * M)
    want = [[[math.log(v) for v in (0.01, 0.02, 0.03, 0.3, 0.4, 0.5)],
             [math.log(v) for v in (0.001, 0.0999, 0.05, 0.79999999999999, 0.2, 0.25)]]]
    assert np.array_equal(bits(many), bits(want))


@pytest.mark.parametrize("extra", [[], ["--select", "2", "--no-save"]])
def test_cli_waic_needs_select(capsys, extra):
    from seriation_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["nowhere.txt", "--waic"] + extra)
    assert e.value.code == 2 and "--waic" in capsys.readouterr().err
