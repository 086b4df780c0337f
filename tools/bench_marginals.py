#!/usr/bin/env python3
"""Posterior-marginals kernels (csrc/sr_marg.hip) at the flagship scale: 8 and 100 selected chains x 1000 saved
samples of the synthetic 256x512 workload (1280 integer columns, 257 bins each), read straight from a session's
record buffer in HBM (sr_session_marginals).

    python tools/bench_marginals.py [--samples 1000] [--chains 100] [--out profiles/marginals_bench.json]

Prints one JSON line: per configuration the kernel ms (HIP events: histogram and summary kernels with the clearing
of the device histogram), the bytes the records hold (n_sel x count x W x 2) and the rate they were read at, the
wall time of the whole call, and as the comparison the wall time of the path a user had before on the same
machine: fetch_records to the host plus the numpy of tests/marg_ref.py.  The two results are compared for equality.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seriation-in-paleontological-data-using-mcmc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--chains", type=int, default=100)
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    args = ap.parse_args()
    import numpy as np
    import marg_ref
    import seriation_amd as sa
    from seriation_amd import analysis
    ds = sa.Dataset.load(os.path.join(ROOT, "tests", "golden", "datasets", "synth_256x512.txt"))
    W = 2 * ds.M + ds.N
    rows = []
    with sa.Session(ds, list(range(1, args.chains + 1)), calls_per_launch=args.samples) as s:
        s.run(args.samples, save=True)
        s.sync()
        analysis.marginals_from_session(s, [0])   # warm-up: loads the code object
        for n_sel in sorted({min(8, args.chains), args.chains}):
            sel = list(range(n_sel))
            best = None
            for _ in range(5):
                t0 = time.perf_counter()
                r = analysis.marginals_from_session(s, sel)
                wall = time.perf_counter() - t0
                if best is None or r["kernel_ms"] < best[0]["kernel_ms"]:
                    best = (r, wall)
            r, wall = best
            t0 = time.perf_counter()
            ab = np.stack([s.fetch_chain_records(c)[0] for c in sel])   # the chosen chains only
            t1 = time.perf_counter()
            want = marg_ref.marginals(ab, ds.N, ds.M, analysis.PROBS)
            t2 = time.perf_counter()
            equal = (np.array_equal(marg_ref.flat(r, "quant"), want["quant"])
                     and np.array_equal(marg_ref.flat(r, "mode"), want["mode"])
                     and marg_ref.same_mean(marg_ref.flat(r, "mean"), want["mean"])
                     and np.array_equal(r["pi_sum"], want["pi_sum"]))
            nbytes = n_sel * args.samples * W * 2
            rows.append({"chains": n_sel, "kernel_ms": r["kernel_ms"], "record_bytes": nbytes,
                         "record_bytes_per_s": nbytes / (r["kernel_ms"] / 1e3), "call_wall_s": wall,
                         "host_fetch_s": t1 - t0, "host_numpy_s": t2 - t1, "host_path_wall_s": t2 - t0,
                         "host_over_gpu_wall": (t2 - t0) / wall, "equal_to_numpy": bool(equal)})
    line = json.dumps({"workload": "synthetic 256x512 (%d integer columns, %d bins), %d samples per chain, records in HBM"
                                   % (W, ds.N + 1, args.samples), "runs": rows})
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if all(r["equal_to_numpy"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
