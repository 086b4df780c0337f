#!/usr/bin/env python3
"""PSIS-LOO kernels (csrc/sr_loo.hip) at the flagship scale: 8 and 100 selected chains x 1000 saved samples of the
synthetic 256x512 workload, read straight from a session's record buffer in HBM (sr_session_loo), with shared rates
and with per-taxon rates (manycd).

    python tools/bench_loo.py [--samples 1000] [--chains 100] [--thin 1] [--host-sites 2]
                              [--out profiles/loo_bench.json]

Prints one JSON line: per configuration the kernel ms (HIP events around the kernels of every batch; best of 5 calls
after a warm-up) split into the sum, the selection and the finish phase, the tail length and the number of cell
batches, the algorithmic bytes computed from the shapes, the wall time of the whole call, sr_session_waic's kernel ms
on the same records, and as the comparison the wall time of the path a user has without the kernels on the same
machine: the records and rates fetched to the host plus the numpy of tests/loo_ref.py over the first --host-sites
sites (the cells are independent, so those cells' pointwise results are compared bit for bit; the scalars are not).
Its time is reported as measured, with the number of sites it covers.

Algorithmic bytes: with T = chains x samples, W = 2M + N, Mt = 1 (shared rates) or M, n the tail length and B the
number of cell batches (the heaps of a batch fit SR_LOO_SCRATCH): the sum phase reads every record row once (T W 2
bytes) and the rates once (T 2 Mt 8), writes the table once and reads it once (T Mt 64 each), and reads and writes the
two partial sums once per chain (32 N M bytes each way); the selection reads the rows and the rates and writes the
table B times more and reads the table's ratios (T Mt 32) as often, and clears the heaps once ((n + 1) 8 N M); the
finish reads every heap m + 2 times ((m + 2) (n + 1) 8 N M, m = 30 + isqrt(n)) and writes it once in the sort.  The
pushes into the heaps depend on the data and are not counted; every tile of 16 sites stages the rows and the table
again, from L2 where they fit.

--thin: sweeps per saved sample; the records' content changes how often the selection pushes, so the default keeps
the sampler's own consecutive samples.
"""
import argparse
import ctypes
import json
import math
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
    ap.add_argument("--host-sites", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    args = ap.parse_args()
    import numpy as np
    import loo_ref
    import seriation_amd as sa
    from seriation_amd import _lib as L
    from seriation_amd import analysis

    def bits(x):
        return np.ascontiguousarray(x, np.float64).view(np.uint64)

    def loo_call(s, sel):
        """analysis.loo_from_session, keeping the struct for its phase times"""
        ch = (ctypes.c_int32 * len(sel))(*sel)
        out, arrs = analysis._loo_outs(s.ds.N, s.ds.M, True)
        t0 = time.perf_counter()
        rc = L.lib().sr_session_loo(s.h, ch, len(sel), 0, args.samples, ctypes.byref(out))
        wall = time.perf_counter() - t0
        if rc != L.SR_OK:
            raise sa.SrError(rc, "sr_session_loo")
        return out, arrs, wall

    ds = sa.Dataset.load(os.path.join(ROOT, "tests", "golden", "datasets", "synth_256x512.txt"))
    N, M = ds.N, ds.M
    X = np.ctypeslib.as_array(ds.c.X, (N * M,)).reshape(N, M)
    W = 2 * M + N
    K = max(1, min(args.host_sites, N))
    scratch = int(os.environ.get("SR_LOO_SCRATCH", "0")) or 256 << 20
    tiles = ((M + 63) // 64) * ((N + 15) // 16)
    rows = []
    for manycd in (0, 1):
        Mt = M if manycd else 1
        with sa.Session(ds, list(range(1, args.chains + 1)), calls_per_launch=args.samples, sweeps_per_call=args.thin,
                        manycd=manycd) as s:
            s.run(args.samples, save=True)
            s.sync()
            loo_call(s, [0])   # warm-up: loads the code object
            analysis.waic_from_session(s, [0])
            for n_sel in sorted({min(8, args.chains), args.chains}):
                sel = list(range(n_sel))
                best = None
                for _ in range(5):
                    out, arrs, wall = loo_call(s, sel)
                    if best is None or out.kernel_ms < best[0].kernel_ms:
                        best = (out, arrs, wall)
                out, arrs, wall = best
                waic_ms = min(analysis.waic_from_session(s, sel, pointwise=False)["kernel_ms"] for _ in range(3))
                t0 = time.perf_counter()
                got = [s.fetch_chain_records(c) for c in sel]   # the chosen chains only
                ab = np.stack([g[0] for g in got])
                cd = s.fetch_cd_vectors()[sel] if manycd else np.stack([g[1] for g in got])
                t1 = time.perf_counter()
                sub = np.concatenate([ab[:, :, :2 * M], ab[:, :, 2 * M:2 * M + K]], axis=2)
                want = loo_ref.loo(X[:K], sub, cd, bool(manycd))
                t2 = time.perf_counter()
                equal = all(np.array_equal(bits(arrs[k][:K]), bits(want[k])) for k in ("elpd", "pareto_k", "lppd", "p_loo_cell"))
                T = n_sel * args.samples
                n = int(out.tail_len)
                m = 30 + math.isqrt(n)
                tb = max(1, min(tiles, scratch // (1024 * (n + 1) * 8)))
                B = (tiles + tb - 1) // tb
                rec_b, cd_b, tab_b, nm = T * W * 2, T * 2 * Mt * 8, T * Mt * 64, N * M
                nbytes = ((1 + B) * (rec_b + cd_b + tab_b) + tab_b + B * tab_b // 2 + n_sel * 64 * nm
                          + (n + 1) * 8 * nm * (1 + m + 2 + 1))
                rows.append({"manycd": manycd, "chains": n_sel, "samples": T, "tail_len": n, "cell_batches": B,
                             "kernel_ms": out.kernel_ms, "sum_ms": out.phase_ms[0], "select_ms": out.phase_ms[1],
                             "finish_ms": out.phase_ms[2], "waic_kernel_ms": waic_ms,
                             "record_bytes": rec_b, "table_bytes": tab_b, "algorithmic_bytes": nbytes,
                             "algorithmic_bytes_per_s": nbytes / (out.kernel_ms / 1e3),
                             "cell_samples_per_s": float(nm) * T / (out.kernel_ms / 1e3),
                             "fit_logs_per_s": float(nm) * (m + 1) * n / (out.phase_ms[2] / 1e3),
                             "call_wall_s": wall, "host_fetch_s": t1 - t0, "host_numpy_s": t2 - t1,
                             "host_numpy_sites": K, "host_path_wall_s": t2 - t0,
                             "elpd_loo": out.elpd, "p_loo": out.p_loo, "n_k": [int(v) for v in out.n_k],
                             "bit_equal_to_numpy": bool(equal)})
                print("bench_loo: %s" % json.dumps(rows[-1]), file=sys.stderr, flush=True)
    line = json.dumps({"workload": "synthetic 256x512 (%d cells), %d samples per chain (%d sweeps apart), records in HBM; "
                                   "one run on one GPU" % (N * M, args.samples, args.thin), "runs": rows})
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if all(r["bit_equal_to_numpy"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
