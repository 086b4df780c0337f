#!/usr/bin/env python3
"""Convergence-diagnostics kernel (csrc/sr_diag.hip) at the flagship scale: 8 and 100 selected chains x 1000 saved
samples of the synthetic 256x512 workload (1280 integer columns), read straight from a session's record buffer in
HBM (sr_session_diagnostics), all lags (max_lag 0 = 499) and max_lag 100.

    python tools/bench_diag.py [--samples 1000] [--chains 100]

Prints one JSON line: per configuration the summed kernel ms (HIP events; the moments are computed in batches of
chains), the integer multiply-adds the lagged products need (algorithmic: sequences x columns x sum over lags of
h - k) and their rate, and the wall time of the whole call (kernels, moment copies to the host, the exact
128-bit host reduction).  Nothing is judged: there is no earlier implementation to compare with.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seriation-in-paleontological-data-using-mcmc_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--chains", type=int, default=100)
    args = ap.parse_args()
    import numpy as np
    import seriation_amd as sa
    from seriation_amd import analysis
    ds = sa.Dataset.load(os.path.join(ROOT, "tests", "golden", "datasets", "synth_256x512.txt"))
    W = 2 * ds.M + ds.N
    h = args.samples // 2
    rows = []
    with sa.Session(ds, list(range(1, args.chains + 1)), calls_per_launch=args.samples) as s:
        s.run(args.samples, save=True)
        s.sync()
        analysis.diagnostics_from_session(s, [0], max_lag=1)   # warm-up: loads the code object
        for n_sel in sorted({min(8, args.chains), args.chains}):
            for max_lag in (0, 100):
                lags = h - 1 if max_lag == 0 else max_lag
                t0 = time.perf_counter()
                r = analysis.diagnostics_from_session(s, list(range(n_sel)), max_lag=max_lag)
                wall = time.perf_counter() - t0
                macs = 2 * n_sel * W * ((lags + 1) * h - lags * (lags + 1) // 2)
                rows.append({"chains": n_sel, "max_lag": max_lag, "lags": lags, "kernel_ms": r["kernel_ms"],
                             "multiply_adds": macs, "multiply_adds_per_s": macs / (r["kernel_ms"] / 1e3),
                             "call_wall_s": wall,
                             "max_rhat_pi": float(np.nanmax(r["rhat"]["pi"])), "min_ess_pi": float(np.nanmin(r["ess"]["pi"]))})
    print(json.dumps({"workload": "synthetic 256x512 (%d integer columns), %d samples per chain, records in HBM"
                                  % (W, args.samples), "runs": rows}), flush=True)


if __name__ == "__main__":
    main()
