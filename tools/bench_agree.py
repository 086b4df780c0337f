#!/usr/bin/env python3
"""Chain-agreement kernels (csrc/sr_agree.hip) at the flagship scale: 100 chains x 1000 saved samples of the synthetic
256x512 workload (32640 site pairs per chain, 100 x 100 chain pairs), read straight from a session's record buffer in
HBM (sr_session_agreement).

    python tools/bench_agree.py [--samples 1000] [--chains 100] [--out profiles/agree_bench.json]

Prints one JSON line: the kernel ms (HIP events: the clearing of the device buffers, the pair-count kernel and the
distance kernel of every band), the compares it stands for (chains x samples x N^2) and their rate, the wall time of
the whole call, and as the baseline the wall time of the numpy definition (tests/agree_ref.py) on the same records,
fetched to the host first.  The two results are compared for equality.  Nothing is asserted about speed.
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
    import agree_ref
    import seriation_amd as sa
    from seriation_amd import analysis
    ds = sa.Dataset.load(os.path.join(ROOT, "tests", "golden", "datasets", "synth_256x512.txt"))
    with sa.Session(ds, list(range(1, args.chains + 1)), calls_per_launch=args.samples) as s:
        s.run(args.samples, save=True)
        s.sync()
        analysis.agreement_from_session(s, [0])   # warm-up: loads the code object
        sel = list(range(args.chains))
        best = None
        for _ in range(5):
            t0 = time.perf_counter()
            r = analysis.agreement_from_session(s, sel)
            wall = time.perf_counter() - t0
            if best is None or r["kernel_ms"] < best[0]["kernel_ms"]:
                best = (r, wall)
        r, wall = best
        t0 = time.perf_counter()
        ab = np.stack([s.fetch_chain_records(c)[0] for c in sel])
        t1 = time.perf_counter()
        want = agree_ref.agreement(ab, ds.N, ds.M)
        t2 = time.perf_counter()
    equal = (np.array_equal(r["dist"], want["dist"]) and np.array_equal(r["dist_mirror"], want["dist_mirror"])
             and r["scale"] == want["scale"])
    compares = args.chains * args.samples * ds.N * ds.N
    row = {"chains": args.chains, "samples": args.samples, "kernel_ms": r["kernel_ms"], "compares": compares,
           "compares_per_s": compares / (r["kernel_ms"] / 1e3), "call_wall_s": wall, "host_fetch_s": t1 - t0,
           "host_numpy_s": t2 - t1, "host_path_wall_s": t2 - t0, "host_over_gpu_wall": (t2 - t0) / wall,
           "equal_to_numpy": bool(equal)}
    line = json.dumps({"workload": "synthetic 256x512 (%d sites: %d site pairs), %d chains x %d samples, records in HBM"
                                   % (ds.N, ds.N * (ds.N - 1) // 2, args.chains, args.samples), "run": row})
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
