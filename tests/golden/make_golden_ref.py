#!/usr/bin/env python3
"""Regenerate tests/golden/reference_exec.json (TEST INFRASTRUCTURE): per-call digests of chains the REFERENCE
sampler itself computed, the ground truth of tests/test_gpu_reference_exec.py.

Unlike chains.json (written by the oracle, tests/golden/make_golden.py), every number here comes from the
reference's unmodified mcmc.c executing under oracle/_ref/ref_driver (oracle/Makefile builds it where the reference
tree is present; see oracle/ref/ref_driver.c).  The cases, the dataset generator and the record format live in
tests/ref_exec.py; the file records the compile line and the SHA-256 of the mcmc.c it was built from.

    make -C oracle && python tests/golden/make_golden_ref.py

tests/test_reference_exec.py regenerates the same content in memory and checks it equals the committed file.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_exec  # noqa: E402


def main():
    if not ref_exec.have_ref():
        sys.exit(ref_exec.SKIP_REASON)
    fx = ref_exec.build_fixture()
    with open(ref_exec.FIXTURE, "w") as fh:
        json.dump(fx, fh, indent=0)
        fh.write("\n")
    print("wrote %d cases, %d bytes" % (len(fx["cases"]), os.path.getsize(ref_exec.FIXTURE)))


if __name__ == "__main__":
    main()
