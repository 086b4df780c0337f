#!/usr/bin/env python3
"""Posterior predictive check kernels (csrc/sr_ppc.hip): the selected chains x 1000 saved samples of g10s10
(124 x 139) and of the synthetic 256 x 512 workload, read straight from a session's record buffer in HBM
(sr_session_ppc), shared rates, every output asked for.

    python tools/bench_ppc.py [--samples 1000] [--chains 8] [--reps 1] [--thin 1] [--no-host]
                              [--out profiles/ppc_bench.json]

Prints one JSON line: per dataset the kernel ms (HIP events around the table, main and tally kernels of every batch;
best of 5 calls after a warm-up), the replicate cells drawn per second (N M T reps / kernel time), the record bytes
read per replicate pass, the wall time of the whole call, and as the comparison the wall time of the numpy definition
of tests/ppc_ref.py on the same inputs on the same machine (records and rates fetched to the host first).  The two
results are compared integer for integer.  --no-host leaves the comparison out.

--thin: sweeps per saved sample; the records' content does not change what the kernels do, so the default keeps the
sampling short.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seriation-in-paleontological-data-using-mcmc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ARRAYS = ("taxon_gt", "taxon_eq", "taxon_sum_obs", "taxon_sum_rep", "site_gt", "site_eq", "site_sum_rep", "total_obs",
          "total_rep", "total_gt", "total_eq")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--thin", type=int, default=1)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    args = ap.parse_args()
    import numpy as np
    import ppc_ref
    import seriation_amd as sa
    from seriation_amd import analysis

    rows = []
    for name in ("g10s10", "synth_256x512"):
        ds = sa.Dataset.load(os.path.join(ROOT, "tests", "golden", "datasets", name + ".txt"))
        N, M = ds.N, ds.M
        X = np.ctypeslib.as_array(ds.c.X, (N * M,)).reshape(N, M)
        sel = list(range(args.chains))
        with sa.Session(ds, list(range(1, args.chains + 1)), calls_per_launch=args.samples,
                        sweeps_per_call=args.thin) as s:
            s.run(args.samples, save=True)
            s.sync()
            analysis.ppc_from_session(s, [0], count=1)   # warm-up: loads the code object
            best = None
            for _ in range(5):
                t0 = time.perf_counter()
                r = analysis.ppc_from_session(s, sel, seed=args.seed, reps=args.reps, totals=True)
                wall = time.perf_counter() - t0
                if best is None or r["kernel_ms"] < best[0]["kernel_ms"]:
                    best = (r, wall)
            r, wall = best
            T = args.chains * args.samples
            row = {"dataset": name, "N": N, "M": M, "chains": args.chains, "samples": T, "reps": args.reps,
                   "kernel_ms": r["kernel_ms"], "cells": N * M * T * args.reps,
                   "cells_per_s": N * M * T * args.reps / (r["kernel_ms"] / 1e3),
                   "record_bytes": T * (2 * M + N) * 2, "call_wall_s": wall,
                   "p_total": [float(v) for v in r["p_total"]],
                   "taxa_f0_outside_95": int(((r["p_taxon"][3] < 0.025) | (r["p_taxon"][3] > 0.975)).sum())}
            if not args.no_host:
                t0 = time.perf_counter()
                got = [s.fetch_chain_records(c) for c in sel]
                ab, cd = np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
                t1 = time.perf_counter()
                want = ppc_ref.ppc(X, ab, cd, False, args.seed, args.reps)
                t2 = time.perf_counter()
                row.update({"host_fetch_s": t1 - t0, "host_numpy_s": t2 - t1, "host_over_gpu_wall": (t2 - t0) / wall,
                            "equal_to_numpy": bool(all(np.array_equal(r[k].astype(np.int64), want[k]) for k in ARRAYS))})
            rows.append(row)
            print("bench_ppc: %s" % json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps({"workload": "%d chains x %d samples (%d sweeps apart), %d replicate(s) per sample, shared rates, "
                                   "records in HBM; one run on one GPU" % (args.chains, args.samples, args.thin, args.reps),
                       "runs": rows})
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if all(r.get("equal_to_numpy", True) for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
