#!/usr/bin/env python3
"""WAIC kernels (csrc/sr_waic.hip) at the flagship scale: 8 and 100 selected chains x 1000 saved samples of the
synthetic 256x512 workload, read straight from a session's record buffer in HBM (sr_session_waic), with shared rates
and with per-taxon rates (manycd).

    python tools/bench_waic.py [--samples 1000] [--chains 100] [--thin 1] [--host-sites 0]
                               [--out profiles/waic_bench.json]

Prints one JSON line: per configuration the kernel ms (HIP events around the table, pass, combine and finish
kernels of every batch; best of 5 calls after a warm-up), the algorithmic bytes computed from the shapes and the
rate they stand for, the wall time of the whole call, and as the comparison the wall time of the path a user had
before on the same machine: the records and rates fetched to the host plus the numpy of tests/waic_ref.py.  The two
results are compared bit for bit.

Algorithmic bytes: with T = chains x samples, W = 2M + N, Mt = 1 (shared rates) or M, each of the two passes reads
every record row once (T W 2 bytes) and the rates once (T 2 Mt 8), writes the table once (T Mt 64) and reads it once
(64 bytes a row in the first pass, the 32 of l[4] in the second), and the pointwise sums are read and written once
per chain and pass (16 N M bytes for Sp and Sl, 8 N M for V, each way).  Every tile of 16 sites stages the rows and
the table again, from L2 where they fit: the bytes that move on the chip are up to N / 16 times these.

--thin: sweeps per saved sample; the records' content does not change what the kernels do, so the default keeps the
sampling short.  --host-sites K (0 = all): for more than 8 chains the numpy reference is run over the first K sites
only (the cells are independent, so those cells' pointwise results are compared bit for bit, the scalars are not);
its time is reported as measured, with the number of sites it covers.
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
    ap.add_argument("--thin", type=int, default=1)
    ap.add_argument("--host-sites", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    args = ap.parse_args()
    import numpy as np
    import seriation_amd as sa
    import waic_ref
    from seriation_amd import analysis

    def bits(x):
        return np.ascontiguousarray(x, np.float64).view(np.uint64)

    ds = sa.Dataset.load(os.path.join(ROOT, "tests", "golden", "datasets", "synth_256x512.txt"))
    N, M = ds.N, ds.M
    X = np.ctypeslib.as_array(ds.c.X, (N * M,)).reshape(N, M)
    W = 2 * M + N
    rows = []
    for manycd in (0, 1):
        Mt = M if manycd else 1
        with sa.Session(ds, list(range(1, args.chains + 1)), calls_per_launch=args.samples, sweeps_per_call=args.thin,
                        manycd=manycd) as s:
            s.run(args.samples, save=True)
            s.sync()
            analysis.waic_from_session(s, [0])   # warm-up: loads the code object
            for n_sel in sorted({min(8, args.chains), args.chains}):
                sel = list(range(n_sel))
                best = None
                for _ in range(5):
                    t0 = time.perf_counter()
                    r = analysis.waic_from_session(s, sel)
                    wall = time.perf_counter() - t0
                    if best is None or r["kernel_ms"] < best[0]["kernel_ms"]:
                        best = (r, wall)
                r, wall = best
                t0 = time.perf_counter()
                got = [s.fetch_chain_records(c) for c in sel]   # the chosen chains only
                ab = np.stack([g[0] for g in got])
                cd = s.fetch_cd_vectors()[sel] if manycd else np.stack([g[1] for g in got])
                t1 = time.perf_counter()
                K = args.host_sites if (args.host_sites and n_sel > 8) else N
                if K < N:
                    sub = np.concatenate([ab[:, :, :2 * M], ab[:, :, 2 * M:2 * M + K]], axis=2)
                    want = waic_ref.waic(X[:K], sub, cd, bool(manycd))
                    keys = ("lppd", "ll_mean", "pwaic")
                else:
                    want = waic_ref.waic(X, ab, cd, bool(manycd))
                    keys = ("lppd", "ll_mean", "pwaic", "elpd", "site_elpd", "taxon_elpd", "elpd_waic", "se", "p_waic",
                            "lppd_sum", "waic")
                t2 = time.perf_counter()
                equal = all(np.array_equal(bits(r[k][:K] if K < N else r[k]), bits(want[k])) for k in keys)
                T = n_sel * args.samples
                rec_b, cd_b, tab_b, nm = T * W * 2, T * 2 * Mt * 8, T * Mt * 64, N * M
                nbytes = 2 * rec_b + 2 * cd_b + 2 * tab_b + tab_b + tab_b // 2 + n_sel * (2 * 16 * nm + 2 * 8 * nm)
                rows.append({"manycd": manycd, "chains": n_sel, "samples": T, "kernel_ms": r["kernel_ms"],
                             "record_bytes": rec_b, "table_bytes": tab_b, "algorithmic_bytes": nbytes,
                             "algorithmic_bytes_per_s": nbytes / (r["kernel_ms"] / 1e3),
                             "cell_terms_per_s": 2.0 * nm * T / (r["kernel_ms"] / 1e3), "call_wall_s": wall,
                             "host_fetch_s": t1 - t0, "host_numpy_s": t2 - t1, "host_numpy_sites": K,
                             "host_path_wall_s": t2 - t0, "host_over_gpu_wall": (t2 - t0) / wall,
                             "elpd_waic": r["elpd_waic"], "p_waic": r["p_waic"], "n_high": r["n_high"],
                             "bit_equal_to_numpy": bool(equal)})
                print("bench_waic: %s" % json.dumps(rows[-1]), file=sys.stderr, flush=True)
    line = json.dumps({"workload": "synthetic 256x512 (%d cells), %d samples per chain (%d sweeps apart), records in HBM; "
                                   "one run on one GPU" % (N * M, args.samples, args.thin), "runs": rows})
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if all(r["bit_equal_to_numpy"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
