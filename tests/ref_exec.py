"""The reference sampler executing (oracle/_ref/, built by oracle/Makefile where the reference tree is present)
-- TEST INFRASTRUCTURE.

Helpers shared by tests/test_reference_exec.py (CPU: the reference against the oracle),
tests/golden/make_golden_ref.py (writes tests/golden/reference_exec.json from the reference's own output) and
tests/test_gpu_reference_exec.py (GPU: sessions against that fixture; it uses only the case list, the dataset
generator and the digests from here, never the binaries)."""
import concurrent.futures
import hashlib
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
REF_DIR = os.path.join(ORACLE_DIR, "_ref")
DRIVER = os.path.join(REF_DIR, "ref_driver")
DRIVER_O0 = os.path.join(REF_DIR, "O0", "ref_driver")
CLI = os.path.join(REF_DIR, "mcmc_ref")
ORACLE_CLI = os.path.join(ORACLE_DIR, "build", "mcmc_oracle")
FLAGS = os.path.join(REF_DIR, "flags.txt")
DATASETS = os.path.join(ROOT, "tests", "golden", "datasets")
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_exec.json")
SKIP_REASON = "oracle/_ref/ref_driver is not built (the reference tree is absent: make -C oracle REFERENCE=<its path>)"


def have_ref():
    return os.path.exists(DRIVER) and os.path.exists(CLI)


def reference_source():
    """Path of the reference's mcmc.c (REFERENCE as oracle/Makefile reads it), or None where it is absent."""
    p = os.path.join(os.environ.get("REFERENCE", "/root/reference"), "C_Implementation", "mcmc.c")
    return p if os.path.exists(p) else None


def golden_text(name):
    with open(os.path.join(DATASETS, name), "rb") as fh:
        return fh.read()


def synth_text(N, M, nh, seed, ones=0.45, noise=0.02, zero_cols=1):
    """A dataset in the reference's text format from a seed (numpy's frozen RandomState stream): each taxon a run
    of sites filled with ones at density `ones`, stray ones at `noise` elsewhere, `zero_cols` all-zero columns and
    `nh` hard sites ("*" after the row)."""
    rng = np.random.RandomState(seed)
    X = np.zeros((N, M), np.uint8)
    for m in range(M):
        lo = rng.randint(0, N)
        hi = min(N, lo + rng.randint(1, max(2, N // 2) + 1))
        col = (rng.random_sample(N) < noise).astype(np.uint8)
        col[lo:hi] = (rng.random_sample(hi - lo) < ones).astype(np.uint8)
        X[:, m] = col
    X[:, rng.choice(M, size=min(zero_cols, M), replace=False)] = 0
    hard = np.zeros(N, bool)
    hard[rng.choice(N, size=nh, replace=False)] = True
    lines = ["%d %d" % (N, M)] + [" ".join(str(v) for v in X[i]) + (" *" if hard[i] else "") for i in range(N)]
    return ("\n".join(lines) + "\n").encode()


# ------------------------------------------------------------------------------------------- running the driver
def _bits(tokens):
    return np.array([int(t, 16) for t in tokens], np.uint64).view(np.float64)


def parse_states(out):
    """ref_driver chain's stdout -> dict(init, rec: lists of state dicts; words; consistent).  A state: a, b, pi
    (int32), c, d (float64 [M], from their bit patterns), loglik, counts (t0a f0a t1a f1a)."""
    states, words, consistent = [], None, None
    cur = None
    for line in out.split("\n"):
        f = line.split()
        if not f:
            continue
        k = f[0]
        if k == "state":
            cur = {"tag": f[1]}
            states.append(cur)
        elif k in ("a", "b", "pi"):
            cur[k] = np.array(f[1:], np.int32)
        elif k in ("c", "d"):
            cur[k] = _bits(f[1:])
        elif k == "loglik":
            cur[k] = _bits(f[1:])[0]
        elif k == "counts":
            cur[k] = np.array(f[1:], np.int32)
        elif k == "words":
            words = int(f[1])
        elif k == "consistent":
            consistent = int(f[1])
    return states, words, consistent


def run_driver(text, seed, manycd, tb, ts, exe=None, env_extra=None):
    """One ref_driver chain run.  Returns dict(rc, stderr, N, M, init (2M+N int32: a, b, pi), init_c, init_d [M],
    init_cdl [3], rec_int [ts, 2M+N], rec_c, rec_d [ts, M], rec_dbl [ts, 3] (c[0], d[0], loglik), counts [ts + 1, 4]
    (row 0 the initial state's), words, consistent) -- the layout of oracle_ref.run_chain."""
    env = dict(os.environ, GSL_RNG_SEED=str(seed))
    env.pop("GSL_RNG_TYPE", None)
    env.update(env_extra or {})
    p = subprocess.run([exe or DRIVER, "chain", str(int(manycd)), str(tb), str(ts)], input=text, capture_output=True,
                       env=env, timeout=600)
    out = dict(rc=p.returncode, stderr=p.stderr.decode(errors="replace"))
    if p.returncode not in (0, 1):
        return out
    states, words, consistent = parse_states(p.stdout.decode())
    assert len(states) == ts + 1 and states[0]["tag"] == "init", (len(states), ts)
    s0, rec = states[0], states[1:]
    M, N = len(s0["a"]), len(s0["pi"])
    cat = lambda s: np.concatenate([s["a"], s["b"], s["pi"]])
    out.update(N=N, M=M, init=cat(s0), init_c=s0["c"], init_d=s0["d"],
               init_cdl=np.array([s0["c"][0], s0["d"][0], s0["loglik"]]),
               rec_int=np.array([cat(s) for s in rec], np.int32).reshape(ts, 2 * M + N),
               rec_c=np.array([s["c"] for s in rec]).reshape(ts, M), rec_d=np.array([s["d"] for s in rec]).reshape(ts, M),
               rec_dbl=np.array([[s["c"][0], s["d"][0], s["loglik"]] for s in rec]).reshape(ts, 3),
               counts=np.array([s["counts"] for s in states], np.int32), words=words, consistent=consistent)
    return out


def run_unit(lines):
    """ref_driver unit over case lines (see unit_line); returns [(pick, counts [4], q float64 [L + 1])]."""
    p = subprocess.run([DRIVER, "unit"], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stderr[-500:])
    res = []
    for line in p.stdout.decode().split("\n"):
        f = line.split()
        if f:
            assert f[0] == "pick" and f[2] == "counts" and f[7] == "q"
            res.append((int(f[1]), np.array(f[3:7], np.int32), _bits(f[8:])))
    return res


def hexbits(v):
    return "%016x" % int(np.array([v], np.float64).view(np.uint64)[0])


def unit_line(x, o, c, d, u):
    return "%d %d %s %s %s %s" % (len(x), o, hexbits(c), hexbits(d), hexbits(u), " ".join(str(int(b)) for b in x))


_POOL = None
_JOBS = {}


def submit(key, fn, *args, **kw):
    """Run fn(*args) once per key on a small pool of worker threads (the work is in child processes): the
    reference at a faithful optimisation level is slow, its runs are independent, so they overlap."""
    global _POOL
    if _POOL is None:
        _POOL = concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1)))
    if key not in _JOBS:
        _JOBS[key] = _POOL.submit(fn, *args, **kw)
    return _JOBS[key]


def driver_job(text, seed, manycd, tb, ts, exe=None):
    key = ("chain", hashlib.sha1(text).hexdigest(), seed, int(manycd), tb, ts, exe)
    return submit(key, run_driver, text, seed, manycd, tb, ts, exe)


# ------------------------------------------------------------------------------------------------ the fixture
def record_digest(rec_int):
    """SHA-256 of a state's a || b || pi (int32 little endian), as tests/golden/chains.json."""
    return hashlib.sha256(np.ascontiguousarray(rec_int, dtype="<i4").tobytes()).hexdigest()


def cd_digest(c, d):
    """SHA-256 of every taxon's c then d (float64 little endian): the per-taxon rates of a manycd state."""
    return hashlib.sha256(np.concatenate([c, d]).astype("<f8").tobytes()).hexdigest()


# name, dataset file or generator parameters of synth_text, seeds, manycd values, calls
FIXTURE_CASES = [
    ("g10s10", "g10s10.txt", [0, 1, 255], [0, 1], 50),
    ("24x17-nh5", dict(N=24, M=17, nh=5, seed=2417), [3], [0, 1], 200),
    ("24x17-nh23", dict(N=24, M=17, nh=23, seed=2418), [3], [0], 200),
    ("64x64", dict(N=64, M=64, nh=4, seed=6464), [5], [0], 100),
]


def case_text(src):
    return golden_text(src) if isinstance(src, str) else synth_text(**src)


def fixture_record(name, src, seed, manycd, calls, o):
    """One fixture case from a run's states (o: run_driver's layout, or the same fields from a GPU session)."""
    rec = {"name": name, "seed": seed, "manycd": manycd, "calls": calls, "N": int(o["N"]), "M": int(o["M"]),
           ("dataset" if isinstance(src, str) else "generator"): src,
           "init_sha256": record_digest(o["init"]),
           "init_cdl_hex": [float(v).hex() for v in o["init_cdl"]],
           "sha256": [record_digest(r) for r in o["rec_int"]],
           "cdl_hex": [[float(v).hex() for v in r] for r in o["rec_dbl"]]}
    if manycd:
        rec["cd_sha256"] = [cd_digest(c, d) for c, d in zip(o["rec_c"], o["rec_d"])]
    return rec


def build_fixture():
    """The fixture's content from the reference executing now (every case one ref_driver run, tb = 0)."""
    jobs = [(name, src, s, mc, calls, driver_job(case_text(src), s, mc, 0, calls))
            for name, src, seeds, mcs, calls in FIXTURE_CASES for mc in mcs for s in seeds]
    cases = []
    for name, src, s, mc, calls, job in jobs:
        o = job.result()
        assert o["rc"] == 0 and o["consistent"] == 0, (name, s, mc, o["rc"], o["stderr"][-300:])
        cases.append(fixture_record(name, src, s, mc, calls, o))
    with open(FLAGS) as fh:
        flags = fh.read().strip()
    prov = {"program": "oracle/ref/ref_driver.c chain <manycd> 0 <calls> over the reference's C_Implementation/mcmc.c "
                       "and the GSL stand-in oracle/ref/gsl/ (generator and distributions: oracle/om_gsl.h)",
            "compile": flags, "seed": "GSL_RNG_SEED (0 -> 4357)"}
    src = reference_source()
    if src:
        with open(src, "rb") as fh:
            prov["mcmc_c_sha256"] = hashlib.sha256(fh.read()).hexdigest()
    return {"note": "the reference sampler's own per-call states: sha256(a||b||pi int32le), c[0]/d[0]/loglik hex; "
                    "cd_sha256 (manycd): sha256(c[0..M) || d[0..M) float64le); init_*: the state after mcmc_randomize; "
                    "tb=0, mcmc_sample's 10 sweeps per call; generator: tests/ref_exec.py synth_text",
            "provenance": prov, "cases": cases}


def load_fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)
