"""Records tests/golden/wgrad_bits.npz (checked by tests/test_wgrad_bits_gpu.py): for every case of tests/wgrad_bits_cases.py and
each of its four ways (set / accumulate, at once / deferred) the SHA-256 of dw's bytes, its f64 sum and its absolute maximum.
Needs the GPU.

    python tools/gen_golden_wgrad_bits.py --lib LIB

LIB is a build of the commit whose bits are to be pinned: a refactoring of csrc/wgrad.hip and its headers records from its PARENT
(a checkout of it, built with the Makefile's OBJDIR= / LIB= overrides) and must pass unchanged -- the file is never re-recorded
from the code under test.  Every case runs on memory poisoned with either value of tests/alloc_poison.py; if the two runs differ in
one bit, or a deferred reduction differs from the immediate one, nothing is written: the kernels promise fixed summation orders.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "wgrad_bits.npz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="library whose bits are recorded (a build of the parent commit)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import tools.diaglib as D
    lib = D.use(a.lib)
    import wgrad_bits_cases as B
    rows, unstable = [], []
    for name in B.NAMES:
        one, two = B.run(name, "nan"), B.run(name, "big")
        unstable += [k for (k, d1), (_, d2) in zip(one, two) if d1[0] != d2[0]]
        by_way = dict(one)
        unstable += [f"{name}/{w}_deferred != {w}" for w in B.WAYS[:2] if by_way[f"{name}/{w}_deferred"][0] != by_way[f"{name}/{w}"][0]]
        rows += one
        print(f"{name}: sum {one[0][1][1]:.17g}, absmax {one[0][1][2]:.9g}", flush=True)
    if unstable:
        sys.exit("runs differ, nothing written: " + ", ".join(unstable))
    np.savez_compressed(a.out, name=np.array([k for k, _ in rows]), sha256=np.array([d[0] for _, d in rows]),
                        sum=np.array([d[1] for _, d in rows], dtype=np.float64),
                        absmax=np.array([d[2] for _, d in rows], dtype=np.float64))
    print(f"wrote {a.out}: {len(rows)} rows from {lib}, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
