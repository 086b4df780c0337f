#!/usr/bin/env python3
"""Cell occupancy kernels (csrc/sr_occ.hip): 8 and 100 chains x 1000 saved samples of the synthetic 256 x 512
workload, read straight from a session's record buffer in HBM (sr_session_occupancy), every output asked for.

    python tools/bench_occ.py [--samples 1000] [--chains 8,100] [--thin 1] [--no-host]
                              [--out profiles/occ_bench.json]

Prints one JSON line: per selection the kernel ms (HIP events around the cell kernel and the two margin launches;
best of 5 calls after a warm-up), the same for the cell counts alone and for the six histograms alone, the alive
predicates per second (N M T over the cell kernel's time), the record bytes of the selection, the wall time of the
whole call, and as the comparison the wall time of the numpy definition of tests/occ_ref.py on the same records on
the same machine (fetched to the host first).  The two results are compared integer for integer.  --no-host leaves
the comparison out.

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--chains", default="8,100")
    ap.add_argument("--thin", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    args = ap.parse_args()
    import numpy as np
    import occ_ref
    import seriation_amd as sa
    from seriation_amd import analysis

    ds = sa.Dataset.load(os.path.join(ROOT, "tests", "golden", "datasets", "synth_256x512.txt"))
    N, M = ds.N, ds.M
    X = np.ctypeslib.as_array(ds.c.X, (N * M,)).reshape(N, M)
    sels = [int(c) for c in args.chains.split(",")]
    rows = []
    with sa.Session(ds, list(range(1, max(sels) + 1)), calls_per_launch=args.samples, sweeps_per_call=args.thin) as s:
        s.run(args.samples, save=True)
        s.sync()
        analysis.occupancy_from_session(s, [0], count=1)   # warm-up: loads the code object

        def best_of(sel, kinds):
            best = None
            for _ in range(5):
                t0 = time.perf_counter()
                r = analysis.occupancy_from_session(s, sel, kinds=kinds)
                wall = time.perf_counter() - t0
                if best is None or r["kernel_ms"] < best[0]["kernel_ms"]:
                    best = (r, wall)
            return best

        for n in sels:
            sel = list(range(n))
            T = n * args.samples
            r, wall = best_of(sel, analysis.OCC_KINDS)
            cells_ms = best_of(sel, ("alive",))[0]["kernel_ms"]
            hists_ms = best_of(sel, analysis.OCC_KINDS[1:])[0]["kernel_ms"]
            row = {"dataset": "synth_256x512", "N": N, "M": M, "chains": n, "samples": T, "kernel_ms": r["kernel_ms"],
                   "kernel_ms_alive_only": cells_ms, "kernel_ms_histograms_only": hists_ms,
                   "predicates": N * M * T, "cell_predicates_per_s": N * M * T / (cells_ms / 1e3),
                   "record_bytes": T * (2 * M + N) * 2, "call_wall_s": wall}
            if not args.no_host:
                t0 = time.perf_counter()
                ab = np.stack([s.fetch_chain_records(c)[0] for c in sel])
                t1 = time.perf_counter()
                want = occ_ref.occupancy(X, ab)
                t2 = time.perf_counter()
                row.update({"host_fetch_s": t1 - t0, "host_numpy_s": t2 - t1, "host_over_gpu_wall": (t2 - t0) / wall,
                            "equal_to_numpy": bool(all(np.array_equal(r[k].astype(np.int64), want[k])
                                                       for k in occ_ref.KINDS))})
            rows.append(row)
            print("bench_occ: %s" % json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps({"workload": "chains x %d samples (%d sweeps apart) of 256 x 512, every output, records in HBM; "
                                   "one run on one GPU" % (args.samples, args.thin), "runs": rows})
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if all(r.get("equal_to_numpy", True) for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
