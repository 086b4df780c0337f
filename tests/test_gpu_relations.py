"""GPU taxon-pair relations, durations and richness (csrc/sr_rel.hip): every count equal to the numpy definition in
tests/rel_ref.py (np.array_equal) at the shapes where the kernels can go wrong, the constructed extremes, the
reflection identities, the optional outputs, the session form (records in HBM) equal to the host-record form and
leaving the session untouched, and the command line's diversity.csv and taxon_pairs.csv."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rel_ref
import seriation_amd as sa
from seriation_amd import _lib as L
from seriation_amd import analysis, launcher

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DS = os.path.join(ROOT, "tests", "golden", "datasets")
PKG = os.path.join(ROOT, "seriation-in-paleontological-data-using-mcmc_amd")
PAIRS = ("orig_before", "ext_before", "precedes", "overlap")


def dataset(N, M):
    return sa.Dataset(np.zeros((N, M), np.uint8), np.zeros(N, bool))


def records(kind, N, M, n_sel, count):
    """[n_sel][count][2M+N] int16 (the idea of tests/test_gpu_marginals.py's generators).  real: every taxon's
    interval wanders as an autocorrelated centre and half-width, clipped to [0, N], so a <= b, some intervals empty;
    full: any int16 with, from column to column, none, a third, two thirds or all of the entries drawn from [0, N]
    instead (a > b rows, differences far outside [0, N]), the int16 extremes placed, and the last taxon given
    limits whose difference always lies in [0, N]."""
    rng = np.random.RandomState(1000 * N + 10 * M + count)
    W = 2 * M + N
    out = np.empty((n_sel, count, W), np.int64)
    out[:, :, 2 * M:] = np.arange(N)   # pi: never read
    if kind == "full":
        x = rng.randint(-32768, 32768, (n_sel, count, 2 * M))
        x[(x >= 0) & (x <= N)] = -1   # in-range values only where they are put
        inr = rng.randint(0, N + 1, (n_sel, count, 2 * M))
        take = rng.randint(0, 3, (n_sel, count, 2 * M)) < (np.arange(2 * M) % 4)[None, None, :]
        x[take] = inr[take]
        x[0, 0, 1], x[0, 1, M] = -32768, 32767   # reflected: N + 32768 and N - 32767
        x[:, :, M - 1] = rng.randint(0, N + 1, (n_sel, count))
        x[:, :, 2 * M - 1] = x[:, :, M - 1] + rng.randint(0, N + 1, (n_sel, count)) % (N + 1 - x[:, :, M - 1])
        out[:, :, :2 * M] = x
        return out.astype(np.int16)
    e = rng.standard_normal((n_sel, count, 2 * M))
    z = np.empty_like(e)
    z[:, 0] = e[:, 0] / 0.6
    for t in range(1, count):
        z[:, t] = 0.8 * z[:, t - 1] + e[:, t]
    centre = rng.uniform(0, N, M)[None, None, :] + z[:, :, :M] * N / 16.0
    half = np.abs(z[:, :, M:]) * N / 12.0
    out[:, :, :M] = np.clip(np.rint(centre - half), 0, N)
    out[:, :, M:2 * M] = np.clip(np.rint(centre + half), 0, N)
    return out.astype(np.int16)


_REC, _REF = {}, {}


def rec_of(kind, N, M, n_sel, count):
    key = (kind, N, M, n_sel, count)
    if key not in _REC:
        _REC[key] = records(kind, N, M, n_sel, count)
        _REC[key].setflags(write=False)
    return _REC[key]


def ref_of(kind, N, M, n_sel, count, flips, kinds=rel_ref.KINDS):
    key = (kind, N, M, n_sel, count, tuple(flips) if flips else None, kinds)
    if key not in _REF:
        _REF[key] = rel_ref.relations(rec_of(kind, N, M, n_sel, count), N, M, flips, kinds)
    return _REF[key]


def check(res, want, N, M, T, kinds=rel_ref.KINDS):
    shapes = {"dur_hist": (M, N + 1), "dur_outside": (M,), "rich_hist": (N, M + 1)}
    assert set(res) == set(kinds) | {"total", "kernel_ms"}
    for k in kinds:
        assert res[k].dtype == np.uint32 and res[k].shape == shapes.get(k, (M, M)), k
        assert np.array_equal(res[k], want[k]), k
    assert res["total"] == T and res["kernel_ms"] > 0


# kind, N, M, n_sel, count, flips
CASES = [
    pytest.param("real", 5, 1, 1, 1, None, id="one-taxon-one-sample"),
    pytest.param("full", 5, 3, 2, 17, None, id="full-int16"),
    pytest.param("full", 5, 3, 2, 17, [1, 0], id="full-int16-flipped"),
    pytest.param("real", 64, 64, 2, 65, None, id="exactly-one-tile"),
    pytest.param("real", 64, 65, 2, 65, None, id="one-column-over"),
    pytest.param("real", 40, 200, 2, 33, None, id="ragged-tiles"),
    pytest.param("real", 124, 139, 3, 100, [0, 1, 0], id="g10s10-shape-flipped-middle"),
    pytest.param("real", 8, 600, 1, 1100, None, id="stream-pieces-chunk-tails"),
    pytest.param("real", 3000, 4, 2, 50, None, id="long-difference-array"),
    pytest.param("real", 6, 3000, 2, 20, None, id="narrowed-richness-tile"),
    pytest.param("real", 1, 2, 1, 9, None, id="single-position"),
]


@pytest.mark.parametrize("kind,N,M,n_sel,count,flips", CASES)
def test_relations_equal_definition(kind, N, M, n_sel, count, flips):
    rec = rec_of(kind, N, M, n_sel, count)
    res = analysis.relations_from_records(dataset(N, M), rec, flips=flips)
    want = ref_of(kind, N, M, n_sel, count, flips)
    check(res, want, N, M, n_sel * count)
    T = n_sel * count
    assert (res["rich_hist"].sum(axis=1) == T).all() and (res["dur_hist"].sum(axis=1) + res["dur_outside"] == T).all()
    if kind == "full":   # the case does hold what it is for
        assert (want["dur_outside"] > 0).any() and (want["dur_outside"] == 0).any()
        a, b = rel_ref.limits(rec, N, M, flips)
        assert (a > b).any()
        if flips:   # the reflection leaves the int16 range
            assert b.max() == N + 32768 and a.min() == N - 32767


def test_bins_beyond_lds():
    """M + 1 bins of one position no longer fit a workgroup's LDS: the richness kernel counts straight into the
    device histogram.  (No pair matrices at this M: they are asked for at M <= 3000 above.)"""
    N, M, kinds = 2, 41000, ("dur_hist", "dur_outside", "rich_hist")
    rng = np.random.RandomState(7)
    rec = np.zeros((1, 3, 2 * M + N), np.int16)
    rec[:, :, :M] = rng.randint(0, N + 1, (1, 3, M))
    rec[:, :, M:2 * M] = rng.randint(0, N + 1, (1, 3, M))
    res = analysis.relations_from_records(dataset(N, M), rec, kinds=kinds)
    check(res, rel_ref.relations(rec, N, M, None, kinds), N, M, 3, kinds)


def test_constructed_extremes():
    N, M, n_sel, count = 7, 70, 2, 40
    T = n_sel * count
    rec = np.zeros((n_sel, count, 2 * M + N), np.int16)
    rec[:, :, M:2 * M] = N   # every taxon alive everywhere
    res = analysis.relations_from_records(dataset(N, M), rec)
    assert (res["rich_hist"][:, M] == T).all() and res["rich_hist"].sum() == N * T
    assert (res["overlap"] == T).all() and not res["precedes"].any()
    assert (res["dur_hist"][:, N] == T).all() and not res["dur_outside"].any()
    rec[:, :, :M] = np.arange(M) % (N + 1)   # every interval empty: b = a
    rec[:, :, M:2 * M] = rec[:, :, :M]
    res = analysis.relations_from_records(dataset(N, M), rec, flips=[0, 1])
    assert (res["rich_hist"][:, 0] == T).all() and res["rich_hist"].sum() == N * T
    assert (np.diag(res["precedes"]) == T).all() and not res["overlap"].any()
    assert (res["dur_hist"][:, 0] == T).all()


def test_reflection_identities():
    """GPU against GPU: every chain flipped."""
    N, M, n_sel, count = 124, 139, 3, 100
    ds, rec = dataset(N, M), rec_of("real", N, M, n_sel, count)
    plain = analysis.relations_from_records(ds, rec)
    flipped = analysis.relations_from_records(ds, rec, flips=[1, 1, 1])
    assert np.array_equal(flipped["orig_before"], plain["ext_before"].T)
    assert np.array_equal(flipped["ext_before"], plain["orig_before"].T)
    assert np.array_equal(flipped["precedes"], plain["precedes"].T)
    assert np.array_equal(flipped["overlap"], plain["overlap"])
    assert np.array_equal(flipped["dur_hist"], plain["dur_hist"])
    assert np.array_equal(flipped["dur_outside"], plain["dur_outside"])
    assert np.array_equal(flipped["rich_hist"], plain["rich_hist"][::-1])
    assert not np.array_equal(plain["precedes"], plain["precedes"].T)   # the identities are not trivially true
    assert not np.array_equal(plain["rich_hist"], plain["rich_hist"][::-1])


def test_optional_outputs():
    N, M, n_sel, count, flips = 40, 200, 2, 33, [0, 1]
    ds, rec = dataset(N, M), rec_of("real", N, M, n_sel, count)
    full = analysis.relations_from_records(ds, rec, flips=flips)
    for kinds in (("overlap",), ("rich_hist",), ("dur_outside",)):
        one = analysis.relations_from_records(ds, rec, flips=flips, kinds=kinds)
        assert set(one) == set(kinds) | {"total", "kernel_ms"}
        assert np.array_equal(one[kinds[0]], full[kinds[0]]) and one["kernel_ms"] > 0


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def test_session_form():
    ds = sa.Dataset.parse(open(os.path.join(DS, "g10s10.txt"), "rb").read())
    seeds, sel, flips = [5, 9, 13, 21], [2, 0, 3], [0, 0, 1]

    def sampled(s):
        s.run(5)
        s.reset_records()
        s.run(40, save=True)

    with sa.Session(ds, seeds, calls_per_launch=40) as s, sa.Session(ds, seeds, calls_per_launch=40) as plain:
        sampled(s)
        sampled(plain)
        ab0, cdl0 = s.fetch_records()
        res = analysis.relations_from_session(s, sel, first=4, count=36, flips=flips)
        ab1, cdl1 = s.fetch_records()
        assert np.array_equal(ab0, ab1) and np.array_equal(bits(cdl0), bits(cdl1))
        host = analysis.relations_from_records(ds, ab0[sel, 4:40], flips=flips)
        want = rel_ref.relations(ab0[sel, 4:40], ds.N, ds.M, flips)
        check(res, want, ds.N, ds.M, 3 * 36)
        check(host, want, ds.N, ds.M, 3 * 36)
        assert not res["dur_outside"].any() and (res["rich_hist"].sum(axis=1) == 3 * 36).all()
        # errors: rows beyond the buffered records, a chain index out of range, no rows
        for bad in (dict(chains=sel, first=5, count=36), dict(chains=[0, 4], first=0, count=40),
                    dict(chains=[-1], first=0, count=40), dict(chains=sel, first=0, count=0),
                    dict(chains=sel, first=-1, count=4), dict(chains=[], first=0, count=4)):
            with pytest.raises(sa.SrError) as e:
                analysis.relations_from_session(s, **bad)
            assert e.value.code == L.SR_EINVAL
        s.run(3, save=False)
        plain.run(3, save=False)
        for c in range(len(seeds)):
            x, y = s.state(c), plain.state(c)
            for k in ("a", "b", "pi", "counts"):
                assert np.array_equal(x[k], y[k])
            assert np.array_equal(bits([x["c"], x["d"], x["loglik"]]), bits([y["c"], y["d"], y["loglik"]]))


def test_cli_relations(tmp_path):
    """python -m seriation_amd --select 2 --relations: Chains/diversity.csv and Chains/taxon_pairs.csv hold the
    definition's numbers for the chosen chains' chain_data.csv rows."""
    path = os.path.join(DS, "g2s2.txt")
    r = subprocess.run([sys.executable, "-m", "seriation_amd", path, "--chains", "4", "--burnin", "5", "--samples", "20",
                        "--seed-base", "1", "--root", str(tmp_path), "--select", "2", "--relations"], cwd=PKG,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ds = sa.Dataset.load(path)
    chosen = launcher.choose_chains(2, str(tmp_path))
    assert ("selected: " + " ".join(str(k) for k in chosen)) in r.stdout and 1 <= len(chosen) <= 2
    rec = analysis.read_chain_rows(str(tmp_path), chosen, ds.N, ds.M)
    assert rec.shape == (len(chosen), 20, 2 * ds.M + ds.N)
    flips = analysis.chain_orientation(rec[:, :, 2 * ds.M:].astype(np.int64).sum(axis=1))
    want = rel_ref.relations(rec, ds.N, ds.M, flips)
    dc = analysis.diversity_curve(want["rich_hist"], analysis.PROBS)
    lines = (tmp_path / "Chains" / "diversity.csv").read_text().splitlines()
    assert lines[0] == "position,mean,q0.025,q0.5,q0.975" and len(lines) == 1 + ds.N
    for p, line in enumerate(lines[1:]):
        f = line.split(",")
        assert int(f[0]) == p and float(f[1]) == dc["mean"][p] and f[1] == repr(float(dc["mean"][p]))
        assert [int(v) for v in f[2:]] == dc["quant"][:, p].tolist()
    lines = (tmp_path / "Chains" / "taxon_pairs.csv").read_text().splitlines()
    assert lines[0] == "i,j,orig_ij,orig_ji,ext_ij,ext_ji,prec_ij,prec_ji,overlap"
    pairs = [(i, j) for i in range(ds.M) for j in range(i + 1, ds.M)]
    assert len(lines) == 1 + len(pairs)
    ob, eb, pr, ov = (want[k] for k in PAIRS)
    for (i, j), line in zip(pairs, lines[1:]):
        assert [int(v) for v in line.split(",")] == [i, j, ob[i, j], ob[j, i], eb[i, j], eb[j, i], pr[i, j], pr[j, i],
                                                     ov[i, j]]
