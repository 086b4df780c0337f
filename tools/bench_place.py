#!/usr/bin/env python3
"""Placement kernels (csrc/sr_place.hip): 8 and 100 chains x 1000 saved samples of the synthetic 256 x 512 workload,
read straight from a session's record buffer in HBM (sr_session_placement), with Q = 1, 16 and 256 query rows (the
dataset's own first rows), shared rates and per-taxon rates (manycd).

    python tools/bench_place.py [--samples 1000] [--chains 8,100] [--queries 1,16,256] [--thin 1] [--no-host]
                                [--budget 16384] [--out profiles/place_bench.json]

Prints one JSON line: per configuration the kernel ms (HIP events around every batch's kernels, summed; best of 3
calls after a warm-up), the likelihood terms per second (T Q N M over that time), the record bytes of the selection
and the wall time of the whole call.

The comparison is the numpy definition of tests/place_ref.py on the same machine.  It performs the same T Q N M
sequential f64 adds in numpy passes, hours at the larger configurations, so it is run on a leading part of the
selection: the first chains and rows that hold at most --budget query-samples (chains x rows x Q; every chain of the
selection where that leaves at least one row each, else the first budget / Q chains, two at least).  The GPU is run
again on exactly that part and pos, site, lse and lpd are compared bit for bit; the JSON states the part
(compared_chains, compared_rows), the numpy seconds it took and those seconds scaled to the whole selection
(host_numpy_s_scaled, an extrapolation, not a measurement).  --no-host leaves the comparison out.

--thin: sweeps per saved sample; the records' content does not change what the kernels do, so the default keeps the
sampling short.
"""
import argparse
import ctypes
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
    ap.add_argument("--queries", default="1,16,256")
    ap.add_argument("--thin", type=int, default=1)
    ap.add_argument("--budget", type=int, default=16384)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    args = ap.parse_args()
    import numpy as np
    import place_ref
    import seriation_amd as sa
    from seriation_amd import _lib as L
    from seriation_amd import analysis

    ds = sa.Dataset.load(os.path.join(ROOT, "tests", "golden", "datasets", "synth_256x512.txt"))
    N, M = ds.N, ds.M
    X = np.ctypeslib.as_array(ds.c.X, (N * M,)).reshape(N, M)
    sels = [int(c) for c in args.chains.split(",")]
    qs = [int(q) for q in args.queries.split(",")]
    rows = []
    for manycd in (0, 1):
        with sa.Session(ds, list(range(1, max(sels) + 1)), calls_per_launch=args.samples, sweeps_per_call=args.thin,
                        manycd=manycd) as s:
            s.run(args.samples, save=True)
            s.sync()
            analysis.placement_from_session(s, [0], X[:1], count=1)   # warm-up: loads the code object
            for n in sels:
                sel = list(range(n))
                T = n * args.samples
                for Q in qs:
                    Y = np.ascontiguousarray(X[:Q], np.uint8)
                    best = None
                    for _ in range(3):
                        t0 = time.perf_counter()
                        r = analysis.placement_from_session(s, sel, Y)
                        wall = time.perf_counter() - t0
                        if best is None or r["kernel_ms"] < best[0]["kernel_ms"]:
                            best = (r, wall)
                    r, wall = best
                    row = {"dataset": "synth_256x512", "N": N, "M": M, "rates": "manycd" if manycd else "shared",
                           "chains": n, "samples": T, "queries": Q, "kernel_ms": r["kernel_ms"],
                           "terms": T * Q * N * M, "terms_per_s": T * Q * N * M / (r["kernel_ms"] / 1e3),
                           "record_bytes": T * (2 * M + N) * 2, "call_wall_s": wall,
                           "pos_row_sum_max_err": float(np.abs(r["pos"].sum(axis=1) - 1.0).max())}
                    if not args.no_host:
                        nc = n if n * Q <= args.budget else min(n, max(2, args.budget // Q))
                        nr = max(1, min(args.samples, args.budget // (Q * nc)))
                        part = sel[:nc]
                        g = analysis.placement_from_session(s, part, Y, count=nr, lse=True)
                        t0 = time.perf_counter()
                        fetched = [s.fetch_chain_records(c, 0, nr) for c in part]
                        ab = np.stack([f[0] for f in fetched])
                        if manycd:
                            cv = np.zeros((s.n, nr, 2 * M))
                            sa.core._check(L.lib().sr_session_fetch_cd_vectors(
                                s.h, 0, nr, cv.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "fetch_cd_vectors")
                            cd = cv[part]
                        else:
                            cd = np.stack([f[1] for f in fetched])
                        t1 = time.perf_counter()
                        want = place_ref.placement(N, ab, cd, Y, bool(manycd))
                        t2 = time.perf_counter()
                        row.update({"compared_chains": nc, "compared_rows": nr,
                                    "compared_whole_selection": nc == n and nr == args.samples, "host_fetch_s": t1 - t0,
                                    "host_numpy_s": t2 - t1, "host_numpy_s_scaled": (t2 - t1) * T / (nc * nr),
                                    "equal_to_numpy": bool(all(np.array_equal(g[k].view(np.uint64),
                                                                              want[k].view(np.uint64))
                                                               for k in ("pos", "site", "lse", "lpd")))})
                    rows.append(row)
                    print("bench_place: %s" % json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps({"workload": "chains x %d samples (%d sweeps apart) of 256 x 512, Q of the dataset's own rows as "
                                   "queries, records in HBM; one run on one GPU; equal_to_numpy is over the leading "
                                   "compared_chains x compared_rows samples, on which the GPU was run again"
                                   % (args.samples, args.thin), "runs": rows})
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if all(r.get("equal_to_numpy", True) for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
