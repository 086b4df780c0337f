#!/usr/bin/env python3
"""Central-state kernels (csrc/sr_central.hip) at the flagship scale: 8 chains x 1000 saved samples of the synthetic
256x512 workload (8000 records x 32640 site pairs, 1024 limit columns), and as the yardstick the chain-agreement
kernels (csrc/sr_agree.hip), which do the same N^2 T / 2 comparison work, in the same process on the same records
(both through their host-record forms; the upload is outside either kernel time).

    python tools/bench_central.py [--samples 1000] [--chains 8] [--out profiles/central_bench.json]

Prints one JSON line: the kernel ms of central (HIP events: the clearing of the device buffers, the pooled pair-count
and order-loss kernels of every band, the histogram, table and look-up kernels of every column batch) and of
agreement (best of 5 each), their ratio, the order-loss kernel alone (sr_order_loss against the pooled counts), the
device name, and whether central's outputs equal the numpy definition (tests/central_ref.py).  Nothing is asserted about speed.
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
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    import central_ref
    import seriation_amd as sa
    from seriation_amd import analysis
    ds = sa.Dataset.load(os.path.join(ROOT, "tests", "golden", "datasets", "synth_256x512.txt"))
    with sa.Session(ds, list(range(1, args.chains + 1)), calls_per_launch=args.samples) as s:
        s.run(args.samples, save=True)
        s.sync()
        ab = np.ascontiguousarray(np.stack([s.fetch_chain_records(c)[0] for c in range(args.chains)]))
    analysis.central_from_records(ds, ab[:1, :64])   # warm-up: loads the code objects
    analysis.agreement_from_records(ds, ab[:1, :64])
    best = {}
    for name, fn in (("central", analysis.central_from_records), ("agreement", analysis.agreement_from_records)):
        for _ in range(5):
            t0 = time.perf_counter()
            r = fn(ds, ab)
            wall = time.perf_counter() - t0
            if name not in best or r["kernel_ms"] < best[name][0]["kernel_ms"]:
                best[name] = (r, wall)
    r, wall = best["central"]
    pooled = analysis.central_from_records(ds, ab, pair_counts=True)["pair_counts"]
    loss_ms = min(analysis.order_loss(ds, ab, pooled)["kernel_ms"] for _ in range(5))   # the order-loss kernel alone
    t0 = time.perf_counter()
    want = central_ref.central(ab, ds.N, ds.M)
    numpy_s = time.perf_counter() - t0
    equal = (np.array_equal(r["order_loss"], want["order_loss"]) and np.array_equal(r["limit_loss"], want["limit_loss"])
             and r["central"] == want["central"] and np.array_equal(r["best"], want["best"])
             and all(np.array_equal(r["state"][k], want["state"][k]) for k in ("a", "b", "pi")))
    ck, ct = r["central"]
    compares = args.chains * args.samples * ds.N * ds.N
    row = {"chains": args.chains, "samples": args.samples, "central_kernel_ms": r["kernel_ms"],
           "order_loss_kernel_ms": loss_ms, "agreement_kernel_ms": best["agreement"][0]["kernel_ms"],
           "central_over_agreement": r["kernel_ms"] / best["agreement"][0]["kernel_ms"],
           "compares": compares, "central_call_wall_s": wall, "agreement_call_wall_s": best["agreement"][1],
           "host_numpy_s": numpy_s, "central": [ck, ct],
           "expected_kendall": int(r["order_loss"][ck, ct]) / r["scale"], "equal_to_numpy": bool(equal)}
    line = json.dumps({"workload": "synthetic 256x512 (%d sites: %d site pairs, %d limit columns), %d chains x %d samples, "
                                   "records from host memory" % (ds.N, ds.N * (ds.N - 1) // 2, 2 * ds.M, args.chains,
                                                                 args.samples),
                       "device": torch.cuda.get_device_name(0),
                       "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), "run": row})
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
