#!/usr/bin/env python3
"""Relation kernels (csrc/sr_rel.hip) at the flagship scale: 8 and 100 selected chains x 1000 saved samples of the
synthetic 256x512 workload (512 taxa: 262144 ordered pairs, 257 duration bins, 256 positions x 513 richness bins),
read straight from a session's record buffer in HBM (sr_session_relations), every output requested.

    python tools/bench_relations.py [--samples 1000] [--chains 100] [--repeats 7] [--out profiles/relations_bench.json]

Prints one JSON line: per configuration the kernel ms (HIP events around the three kernels and the clearing of their
device outputs) and the wall time of the whole call, each as median, minimum and maximum over the repeats after one
warm-up call, the pair comparisons per second the kernel time amounts to (4 predicates x M^2 pairs x samples), and
as the comparison the wall time of the path a user had before on the same machine: fetch_records to the host plus
the numpy of tests/rel_ref.py (three repeats at 8 chains; once at the larger selection, where one run takes
minutes).  The two results are compared for equality.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seriation-in-paleontological-data-using-mcmc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "repeats": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--chains", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    args = ap.parse_args()
    import numpy as np
    import rel_ref
    import seriation_amd as sa
    from seriation_amd import analysis
    ds = sa.Dataset.load(os.path.join(ROOT, "tests", "golden", "datasets", "synth_256x512.txt"))
    rows = []
    with sa.Session(ds, list(range(1, args.chains + 1)), calls_per_launch=args.samples) as s:
        s.run(args.samples, save=True)
        s.sync()
        analysis.relations_from_session(s, [0])   # warm-up: loads the code object
        for n_sel in sorted({min(8, args.chains), args.chains}):
            sel = list(range(n_sel))
            analysis.relations_from_session(s, sel)   # warm-up at this shape
            kms, walls = [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                r = analysis.relations_from_session(s, sel)
                walls.append(time.perf_counter() - t0)
                kms.append(r["kernel_ms"])
            print("# %d chains: gpu kernel %.3f ms, call %.4f s (medians)" % (n_sel, statistics.median(kms),
                                                                              statistics.median(walls)), flush=True)
            fetch, numpy_s = [], []
            for _ in range(3 if n_sel <= 8 else 1):
                t0 = time.perf_counter()
                ab = np.stack([s.fetch_chain_records(c)[0] for c in sel])   # the chosen chains only
                t1 = time.perf_counter()
                want = {}
                for k in rel_ref.KINDS:   # (kind by kind: a line of output per stage of a run of minutes)
                    want.update(rel_ref.relations(ab, ds.N, ds.M, None, (k,)))
                    print("# %d chains: numpy %s after %.1f s" % (n_sel, k, time.perf_counter() - t1), flush=True)
                t2 = time.perf_counter()
                fetch.append(t1 - t0)
                numpy_s.append(t2 - t1)
            equal = all(np.array_equal(r[k], want[k]) for k in rel_ref.KINDS)
            host = [f + n for f, n in zip(fetch, numpy_s)]
            compares = 4.0 * ds.M * ds.M * n_sel * args.samples
            rows.append({"chains": n_sel, "kernel_ms": spread(kms), "call_wall_s": spread(walls),
                         "pair_compares_per_s": compares / (statistics.median(kms) / 1e3),
                         "host_fetch_s": spread(fetch), "host_numpy_s": spread(numpy_s), "host_path_wall_s": spread(host),
                         "host_over_gpu_wall": statistics.median(host) / statistics.median(walls),
                         "equal_to_numpy": bool(equal)})
    line = json.dumps({"workload": "synthetic 256x512 (%d taxa, %d positions), %d samples per chain, records in HBM, "
                                   "all seven outputs" % (ds.M, ds.N, args.samples), "runs": rows})
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if all(r["equal_to_numpy"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
