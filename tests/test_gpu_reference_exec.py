"""GPU sessions against chains the reference sampler itself computed (tests/golden/reference_exec.json).

The fixture holds per-call digests written by the reference's unmodified mcmc.c executing
(tests/golden/make_golden_ref.py; tests/test_reference_exec.py keeps it current where the reference is present).
Every case runs a Session of the fixture's seed and compares the state after mcmc_randomize and every call's
a / b / pi digest and c / d / loglik bits with it -- no oracle in the loop, only the fixture is read.

Each case runs on the default kernel (compiled for the shape; manycd sessions have generic kernels only, so their
default leg is the generic 1024-thread kernel) and with SR_F_GENERIC_KERNEL; the 64 x 64 case, the wave and LDS
boundary shape, also with its columns in HBM.  The split plan (two workgroups per chain) cannot be forced at
that shape -- the planner splits only chains of more than 128 taxa -- so it is left out."""
import numpy as np
import pytest

import ref_exec as R
import seriation_amd as sa

pytestmark = pytest.mark.gpu

_FX = R.load_fixture()
CASES = _FX["cases"]
_IDS = ["%s-seed%d%s" % (c["name"], c["seed"], "-manycd" if c["manycd"] else "") for c in CASES]
_DS = {}


def _dataset(c):
    key = c.get("dataset") or tuple(sorted(c["generator"].items()))
    if key not in _DS:
        _DS[key] = sa.Dataset.parse(R.case_text(c.get("dataset") or c["generator"]), maxs=0)
    return _DS[key]


def _check(c, **kw):
    ds = _dataset(c)
    assert (ds.N, ds.M) == (c["N"], c["M"])
    calls, M = c["calls"], c["M"]
    with sa.Session(ds, [c["seed"]], calls_per_launch=calls, manycd=c["manycd"], **kw) as s:
        kind = (s.specialized, s.variant, s.kernel)
        st = s.state(0)
        s.run(calls, save=True)
        ab, cdl = s.fetch_records()
        cv = s.fetch_cd_vectors() if c["manycd"] else None
    init = np.concatenate([st["a"], st["b"], st["pi"]])
    assert R.record_digest(init) == c["init_sha256"], "the state after mcmc_randomize"
    assert [float(v).hex() for v in (st["c"], st["d"], st["loglik"])] == c["init_cdl_hex"]
    got = [R.record_digest(r) for r in ab[0]]
    bad = [k for k in range(calls) if got[k] != c["sha256"][k]]
    assert not bad, "a / b / pi differ from the reference first at call %d of %d" % (bad[0], calls)
    hexes = [[float(v).hex() for v in r] for r in cdl[0]]
    bad = [k for k in range(calls) if hexes[k] != c["cdl_hex"][k]]
    assert not bad, "c / d / loglik differ first at call %d: %s, the reference %s" % (bad[0], hexes[bad[0]],
                                                                                      c["cdl_hex"][bad[0]])
    if c["manycd"]:
        got = [R.cd_digest(r[:M], r[M:]) for r in cv[0]]
        bad = [k for k in range(calls) if got[k] != c["cd_sha256"][k]]
        assert not bad, "per-taxon c, d differ first at call %d" % bad[0]
    return kind


def test_fixture_is_the_reference_s():
    """The file says where it comes from, and holds the cases this module expects."""
    p = _FX["provenance"]
    assert "ref_driver" in p["program"] and "-ffp-contract=off" in p["compile"] and len(p["mcmc_c_sha256"]) == 64
    want = [(n, s, mc, calls) for n, _, seeds, mcs, calls in R.FIXTURE_CASES for mc in mcs for s in seeds]
    assert [(c["name"], c["seed"], c["manycd"], c["calls"]) for c in CASES] == want
    for c in CASES:
        assert len(c["sha256"]) == len(c["cdl_hex"]) == c["calls"] and len(set(c["sha256"])) > c["calls"] // 2


@pytest.mark.parametrize("c", CASES, ids=_IDS)
def test_default_kernel_equals_reference(c):
    specialized, variant, kernel = _check(c)
    assert specialized == (not c["manycd"]) and kernel == "single" and variant == "lds"


@pytest.mark.parametrize("c", CASES, ids=_IDS)
def test_generic_kernel_equals_reference(c):
    specialized, variant, kernel = _check(c, generic=True)
    assert not specialized and kernel == "single"


@pytest.mark.parametrize("c", [c for c in CASES if c["name"] == "64x64"], ids=["64x64-hbm"])
def test_hbm_columns_equal_reference(c):
    specialized, variant, kernel = _check(c, columns="hbm")
    assert variant == "hbm" and kernel == "single"
