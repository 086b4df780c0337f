"""The reference sampler itself, executing, against the oracle (CPU, no tolerance anywhere).

Every parity claim of the suite ends at oracle/om_mcmc.c, a hand transcription of the reference's mcmc.c.  Here
the reference's unmodified source runs (oracle/_ref/mcmc_ref and ref_driver: oracle/Makefile builds them over the
GSL stand-in oracle/ref/gsl/ where the reference tree is present) and every byte it writes and every bit of its
state is compared with the oracle's: the CLI's five files, the state after mcmc_randomize and after every
mcmc_sample call (manycd 0 and 1, hard sites, zero columns, the Johnk beta branch, the smallest shape), the
committed fixture tests/golden/chains.json re-derived from the reference's output, and the Gibbs pick
(mcmc_auxa / mcmc_logtop / mcmc_randompick) on the certification tests' boundary inputs.

What this does not pin: the stand-in forwards the generator and the distributions to oracle/om_gsl.h, so GSL's
own gamma / ziggurat stream is still compared with nothing here.  The reference's exp / log are this machine's
libm, so om_exp / om_log (oracle/om_libm.h) are checked against it on every value the chains pass through.

The reference runs (child processes) overlap on a small thread pool; the file takes about a minute of wall time
on eight cores.  Times of 10 mcmc_sample calls of ref_driver (-O1) per golden dataset, measured once: g10s10
0.19 s, g5s5 0.36 s, g10s2 0.41 s, synth_256x512 0.81 s, g2s2 0.89 s; the reference CLI's fixed 1000 + 1000 calls
take 15 s on g10s10, the smallest, which is therefore the CLI test's dataset."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import cert_cases
import oracle_ref
import ref_exec as R
from test_gpu_edge import _all_ones_text, make_text

pytestmark = pytest.mark.skipif(not R.have_ref(), reason=R.SKIP_REASON)

GOLDEN = ["g10s10.txt", "g5s5.txt", "g10s2.txt", "synth_256x512.txt", "g2s2.txt"]
SEEDS = [1, 2, 3, 4]
CALLS = 50

# The inputs the GPU edge tests construct (tests/test_gpu_edge.py), as dataset text both programs read:
# hard sites nh = 1, N / 2, N - 1; all-zero columns; the all-ones matrix whose counts f1a = t0a = 0 send
# mcmc_samplebeta into gsl_ran_beta's Johnk branch; and 2 x 1, the smallest shape that runs (N = 1 is refused:
# test_one_site_aborts_in_the_reference).
SYNTH = {
    "nh1": make_text(24, 17, 1, seed=24017),
    "nh-half": make_text(24, 17, 12, seed=24017),
    "nh-n-1": make_text(24, 17, 23, seed=24017),
    "zero-columns": make_text(20, 12, 3, seed=20012, zero_cols=5),
    "johnk": _all_ones_text(40, 24, {5, 17, 30}),
    "smallest": b"2 1\n1\n0\n",
}
SYNTH_CALLS = 200

CLI_RUNS = [(seed, idx, None) for seed in (0, 1, 255) for idx in ("3", "12")] + [(1, "3", "mt19937")]
CLI_FILES = ["taxa.csv", "sites.csv", "hard_sites.csv", "exp_data.csv", "chain_data.csv"]


def _chains_json():
    with open(os.path.join(R.ROOT, "tests", "golden", "chains.json")) as fh:
        return json.load(fh)


def _run_cli(exe, seed, idx, rng_type, root):
    d = os.path.join(root, "%s-%d-%s-%s" % (os.path.basename(exe), seed, idx, rng_type))
    os.makedirs(os.path.join(d, "Chains", "chain_%02d" % int(idx)))
    env = dict(os.environ, GSL_RNG_SEED=str(seed))
    env.pop("GSL_RNG_TYPE", None)
    if rng_type:
        env["GSL_RNG_TYPE"] = rng_type
    p = subprocess.run([exe, idx], input=R.golden_text("g10s10.txt"), cwd=d, env=env, capture_output=True, timeout=900)
    files = {}
    for f in CLI_FILES:
        with open(os.path.join(d, "Chains", "chain_%02d" % int(idx), f), "rb") as fh:
            files[f] = fh.read()
    return p.returncode, p.stdout, p.stderr, files


def _oracle(text, seed, manycd, calls):
    return oracle_ref.run_chain(text, seed, 0, calls, maxs=0, want_init=True, manycd=manycd)


def _oracle_job(text, seed, manycd, calls):
    return R.submit(("oracle", hash(text), seed, manycd, calls), _oracle, text, seed, manycd, calls)


@pytest.fixture(scope="module", autouse=True)
def farm(tmp_path_factory):
    """Queue every run of the file at once (longest first), so the slow ones overlap with everything else."""
    root = str(tmp_path_factory.mktemp("cli"))
    for seed, idx, ty in CLI_RUNS:
        for exe in (R.CLI, R.ORACLE_CLI):
            R.submit(("cli", exe, seed, idx, ty), _run_cli, exe, seed, idx, ty, root)
    for name in reversed(GOLDEN):
        for seed in SEEDS:
            for mc in (0, 1):
                R.driver_job(R.golden_text(name), seed, mc, 0, CALLS)
                _oracle_job(R.golden_text(name), seed, mc, CALLS)
    for c in _chains_json()["cases"]:
        R.driver_job(R.golden_text(c["dataset"]), c["seed"], 0, 0, c["calls"])
    for text in SYNTH.values():
        for mc in (0, 1):
            R.driver_job(text, 3, mc, 0, SYNTH_CALLS)
    return root


def _same_states(o, q, manycd, what):
    """Every integer and every double bit of the initial state and of each call: o the reference, q the oracle."""
    assert o["rc"] == 0 and o["consistent"] == 0, (what, o["rc"], o["stderr"][-300:])
    assert q["rc"] == 0, what
    np.testing.assert_array_equal(o["init"], q["init"], err_msg="%s: state after mcmc_randomize" % what)
    assert np.array_equal(o["init_cdl"].view(np.uint64), q["init_cdl"].view(np.uint64)), what
    np.testing.assert_array_equal(o["rec_int"], q["rec_int"], err_msg="%s: a, b, pi per call" % what)
    same = (o["rec_dbl"].view(np.uint64) == q["rec_dbl"].view(np.uint64)).all(axis=1)
    assert same.all(), "%s: c[0] / d[0] / loglik first differ at call %d" % (what, int(np.argmin(same)))
    if manycd:
        cd = np.concatenate([o["rec_c"], o["rec_d"]], axis=1)
        assert np.array_equal(cd.view(np.uint64), q["rec_cdv"].view(np.uint64)), "%s: per-taxon c, d" % what
    else:   # one c, one d: every taxon holds the same bits
        assert (o["rec_c"].view(np.uint64) == o["rec_c"].view(np.uint64)[:, :1]).all(), what
        assert (o["rec_d"].view(np.uint64) == o["rec_d"].view(np.uint64)[:, :1]).all(), what
    assert o["words"] == q["words"], "%s: generator words drawn" % what


# ------------------------------------------------------------------------------------------------ the CLI's bytes
@pytest.mark.parametrize("seed,idx,rng_type", CLI_RUNS, ids=["seed%d-chain%s%s" % (s, i, "-type" if t else "")
                                                              for s, i, t in CLI_RUNS])
def test_cli_files_byte_identical(farm, seed, idx, rng_type):
    """`mcmc <chain_index> < g10s10` (1000 + 1000 calls): the five files of Chains/chain_NN byte for byte, the exit
    status and stdout; index 12 takes the reference's two-digit branch, seed 0 GSL's 4357; with GSL_RNG_TYPE set,
    stderr as well (gsl_rng_env_setup's two lines and everything the run prints)."""
    rc_r, out_r, err_r, f_r = R.submit(("cli", R.CLI, seed, idx, rng_type), None).result()
    rc_o, out_o, err_o, f_o = R.submit(("cli", R.ORACLE_CLI, seed, idx, rng_type), None).result()
    assert rc_r == 0 and rc_o == 0, (rc_r, rc_o, err_r[-300:], err_o[-300:])
    for f in CLI_FILES:
        assert f_r[f] == f_o[f], "%s differs (reference %d bytes, oracle %d)" % (f, len(f_r[f]), len(f_o[f]))
    assert len(f_r["chain_data.csv"].splitlines()) == 1000
    assert out_r == out_o
    if rng_type:
        assert err_r == err_o and b"GSL_RNG_TYPE=mt19937" in err_r and b"GSL_RNG_SEED=1" in err_r


# ------------------------------------------------------------------------------------------- the state per call
@pytest.mark.parametrize("manycd", [0, 1])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", GOLDEN)
def test_state_per_call_golden_datasets(name, seed, manycd):
    text = R.golden_text(name)
    o = R.driver_job(text, seed, manycd, 0, CALLS).result()
    q = _oracle_job(text, seed, manycd, CALLS).result()
    _same_states(o, q, manycd, "%s seed %d manycd %d" % (name, seed, manycd))
    if manycd:
        assert len(np.unique(o["rec_c"][-1])) > 1   # the taxa do carry their own c


@pytest.mark.parametrize("manycd", [0, 1])
@pytest.mark.parametrize("name", list(SYNTH))
def test_state_per_call_edge_inputs(name, manycd):
    text = SYNTH[name]
    o = R.driver_job(text, 3, manycd, 0, SYNTH_CALLS).result()
    q = _oracle(text, 3, manycd, SYNTH_CALLS)
    _same_states(o, q, manycd, "%s manycd %d" % (name, manycd))
    moved = (o["rec_int"][1:] != o["rec_int"][:-1]).any(axis=1).sum()
    if name == "johnk":       # the branch is the one meant: t0a = f1a = 0 when the first sweep draws c
        assert (o["counts"][0, [0, 3]] == 0).all()
    if name == "nh-n-1":      # one free site among 23 ordered ones: pi3 never proposes, the others still move it
        assert o["N"] - 23 < 2
    if name != "smallest":
        assert moved > SYNTH_CALLS // 4, "%s: the chain barely moves (%d of %d calls)" % (name, moved, SYNTH_CALLS)


def test_one_site_aborts_in_the_reference():
    """N = 1, the smallest shape the parser accepts, cannot run: the reference asks gsl_rng_uniform_int for a
    number below N - 1 = 0, which GSL refuses through its error handler (abort).  The product refuses the shape
    before it runs (sr_session_create: N < 2); 2 x 1 is the smallest case above."""
    o = R.run_driver(b"1 1\n1\n", 1, 0, 0, 1)
    assert o["rc"] == -6 and "gsl_rng_uniform_int" in o["stderr"], o


# ---------------------------------------------------------------------------- the committed fixture re-derived
def test_chains_json_is_what_the_reference_computes():
    """tests/golden/chains.json (written by the oracle; the whole GPU suite leans on it) recomputed from the
    reference's states in the format its note documents: the digests, the hex doubles, the words drawn and the
    exp_data sums (compute_exp_data / print_exp_data: libm exp, divisor 1000)."""
    for c in _chains_json()["cases"]:
        o = R.driver_job(R.golden_text(c["dataset"]), c["seed"], 0, 0, c["calls"]).result()
        what = "%s seed %d" % (c["dataset"], c["seed"])
        assert o["rc"] == 0 and (o["N"], o["M"]) == (c["N"], c["M"]), what
        assert R.record_digest(o["init"]) == c["init_sha256"], what
        assert [float(v).hex() for v in o["init_cdl"]] == c["init_cdl_hex"], what
        assert [R.record_digest(r) for r in o["rec_int"]] == c["sha256"], what
        assert [[float(v).hex() for v in r] for r in o["rec_dbl"]] == c["cdl_hex"], what
        ls = cs = ds = 0.0
        for cc, dd, ll in o["rec_dbl"]:
            ls += -float(ll)
            cs += math.exp(cc)
            ds += math.exp(dd)
        assert [(v / 1000).hex() for v in (ls, cs, ds)] == c["exp_hex"], what
        assert o["words"] == c["rng_words"], what


def test_reference_exec_fixture_is_current():
    """tests/golden/reference_exec.json (the GPU tests' ground truth) equals what the reference computes now."""
    now, held = R.build_fixture(), R.load_fixture()
    assert now["cases"] == held["cases"]
    assert now["note"] == held["note"] and now["provenance"]["compile"] == held["provenance"]["compile"]
    if "mcmc_c_sha256" in now["provenance"]:
        assert now["provenance"]["mcmc_c_sha256"] == held["provenance"]["mcmc_c_sha256"]


# ------------------------------------------------------------------------------------------------ the Gibbs pick
def _unit_cases():
    """(x, o, c, d, u, entry or None): cert_cases' column families -- random, tail (clamped mass), steep, rise at
    N = 3000 (the trimmed windows) -- with u on the oracle's CDF boundaries, one ulp either side, and 0, 1/2, 1-."""
    rng = np.random.default_rng(20240)
    grid = cert_cases.cd_grid()
    cases, k = [], 0
    for kind, N, blocks in (("random", 200, 4), ("tail", 200, 3), ("steep", 200, 4), ("rise", 3000, 2)):
        for _ in range(blocks):
            c, d = grid[(7 * k + 3) % len(grid)]
            k += 1
            col, rev, o, L = cert_cases.gibbs_block_columns(kind, N, rng)
            x = cert_cases.walk_bits(col, N, rev, L)
            for u in (0.0, 0.5, float(np.nextafter(1.0, 0.0))):
                cases.append((x, o, c, d, u, None))
            for i in cert_cases._boundaries(x, o, c, d, rng.integers(0, L, 2)):
                ub = oracle_ref.auxa_boundary(x, o, c, d, i)
                if 0.0 < ub < 1.0:
                    for u in (cert_cases._step(ub, -1), ub, cert_cases._step(ub, 1)):
                        cases.append((x, o, c, d, u, i))
    return cases


def test_gibbs_pick_and_probabilities_bitwise():
    cases = _unit_cases()
    assert 300 <= len(cases) <= 900, len(cases)
    got = R.run_unit([R.unit_line(x, o, c, d, u) for x, o, c, d, u, _ in cases])
    assert len(got) == len(cases)
    on_boundary = 0
    for n, ((x, o, c, d, u, i), (pick, counts, q)) in enumerate(zip(cases, got)):
        want, p = oracle_ref.auxa_pick(x, o, c, d, u, want_p=True)
        assert pick == want, "case %d: the reference picks %d, the oracle %d (u = %r)" % (n, pick, want, u)
        assert np.array_equal(q.view(np.uint64), p.view(np.uint64)), "case %d: probabilities differ" % n
        col = np.asarray(x[min(o, pick):max(o, pick)])
        ones, zeros = int(col.sum()), int(len(col) - col.sum())
        sign = 1 if pick > o else -1   # mcmc_auxa's count changes at the pick
        assert counts.tolist() == [sign * zeros, -sign * zeros, -sign * ones, sign * ones], n
        if i is not None:
            on_boundary += 1
    # the boundaries are the reference's own: at ub the pick lies beyond entry i, one ulp below it does not
    for n in range(len(cases) - 2):
        if cases[n][5] is not None and cases[n + 1][5] == cases[n][5] and cases[n + 2][5] == cases[n][5] \
                and cases[n][4] < cases[n + 1][4] < cases[n + 2][4]:
            i = cases[n][5]
            assert got[n][0] <= i < got[n + 1][0] and got[n + 2][0] > i, (n, i, got[n][0], got[n + 1][0])
    assert on_boundary >= 200


# ------------------------------------------------------------------------------------------ optimisation level
def test_O0_build_equals_O1():
    """The committed recipe compiles the reference at -O1; the same source at -O0 prints the same bytes (g10s10,
    50 calls), so nothing the tests see depends on the optimiser."""
    if R.reference_source() is None:
        pytest.skip("the reference source is absent: oracle/_ref/O0/ref_driver cannot be built here")
    subprocess.check_call(["make", "-s", "-C", R.ORACLE_DIR, "_ref/O0/ref_driver"])
    outs = []
    for exe in (R.DRIVER, R.DRIVER_O0):
        p = subprocess.run([exe, "chain", "0", "0", str(CALLS)], input=R.golden_text("g10s10.txt"), capture_output=True,
                           env=dict(os.environ, GSL_RNG_SEED="1"), timeout=600)
        assert p.returncode == 0
        outs.append(p.stdout)
    assert outs[0] == outs[1] and outs[0].count(b"state ") == CALLS + 1
