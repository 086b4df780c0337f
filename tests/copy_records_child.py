"""Child process of tests/test_gpu_summaries.py: sr_session_copy_chain_records into torch tensors on the GPU.
A process of its own because torch has to initialise the GPU before the library does, as in bench.py; the suite's
process has long opened it through the library.  A g10s10 session of 4 chains with 40 saved rows (buffer of 100);
every destination is one row longer than the copy and filled with a guard value.  Prints one JSON line:
{"cases": {name: [failed checks]}, "refusals": [...]} -- empty lists when all is well."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seriation-in-paleontological-data-using-mcmc_amd"))
import seriation_amd as sa  # noqa: E402
from seriation_amd import _lib as L  # noqa: E402

AB_GUARD, CD_GUARD = -21846, -7.25e300
# chain, first, count, which arrays ("cdl": dev_ab_pi = NULL, "ab": dev_cdl = NULL), on torch's stream?
CASES = [(2, 3, 36, "both", False), (0, 0, 40, "both", False), (3, 39, 1, "both", False), (1, 17, 0, "both", False),
         (1, 40, 0, "both", False), (2, 3, 36, "cdl", False), (0, 5, 35, "ab", False), (3, 1, 38, "both", True)]
REFUSED = [(-1, 0, 1), (4, 0, 1), (0, -1, 1), (0, 0, -1), (0, 0, 41), (0, 1, 40), (0, 40, 1), (0, 41, 0)]


def case_name(c):
    return "chain%d-first%d-count%d-%s%s" % (c[0], c[1], c[2], c[3], "-torch-stream" if c[4] else "")


def guarded(rows, W):
    dev = torch.device("cuda", 0)
    ab = torch.full((rows + 1, W), AB_GUARD, dtype=torch.int16, device=dev)
    cd = torch.full((rows + 1, 3), CD_GUARD, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()   # the fills run on torch's stream, the copies on the session's
    return ab, cd


def main():
    torch.cuda.set_device(0)
    ds = sa.Dataset.load(os.path.join(ROOT, "tests", "golden", "datasets", "g10s10.txt"))
    W = 2 * ds.M + ds.N
    out = {"cases": {}, "refusals": []}
    with sa.Session(ds, [1, 2, 3, 4]) as s:
        s.run(2)
        s.run(40, save=True)
        s.sync()
        for case in CASES:
            chain, first, count, which, on_torch = case
            bad = []
            if on_torch:   # as bench.py: the session launches on torch's current stream
                s.set_stream(torch.cuda.current_stream().cuda_stream)
            ab, cd = guarded(count, W)
            n = s.copy_chain_records(chain, ab.data_ptr() if which != "cdl" else 0,
                                     cd.data_ptr() if which != "ab" else 0, first=first, count=count)
            if n != count:
                bad.append("returned %d" % n)
            if on_torch:
                torch.cuda.current_stream().synchronize()
            else:
                s.sync()
            got_ab, got_cd = ab.cpu().numpy(), cd.cpu().numpy()
            want_ab, want_cd = s.fetch_chain_records(chain, first, count)
            if count and which == "both":   # real rows, not a copy of nothing
                if not (np.sort(want_ab[:, 2 * ds.M:], axis=1) == np.arange(ds.N)).all() or not (want_cd[:, 2] < 0).all():
                    bad.append("fetched rows are no records")
            if which == "cdl":
                want_ab = np.full((count, W), AB_GUARD, np.int16)
            if which == "ab":
                want_cd = np.full((count, 3), CD_GUARD, np.float64)
            if got_ab[:count].tobytes() != want_ab.tobytes():
                bad.append("ab_pi bytes differ")
            if got_cd[:count].tobytes() != want_cd.tobytes():
                bad.append("cdl bytes differ")
            if not (got_ab[count:] == AB_GUARD).all() or not (got_cd[count:] == CD_GUARD).all():
                bad.append("guard row written")
            out["cases"][case_name(case)] = bad
        # a chain outside the session, a negative first or count, rows past the saved ones: SR_EINVAL, nothing written
        ab, cd = guarded(40, W)
        for chain, first, count in REFUSED:
            try:
                s.copy_chain_records(chain, ab.data_ptr(), cd.data_ptr(), first=first, count=count)
                out["refusals"].append("not refused: %r" % ((chain, first, count),))
            except L.SrError as e:
                if e.code != L.SR_EINVAL:
                    out["refusals"].append("code %d: %r" % (e.code, (chain, first, count)))
        torch.cuda.synchronize()
        s.sync()
        if not (ab.cpu().numpy() == AB_GUARD).all() or not (cd.cpu().numpy() == CD_GUARD).all():
            out["refusals"].append("a refused copy wrote")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
