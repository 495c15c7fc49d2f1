"""Records tests/golden/medicalnet_bits.npz (checked by tests/test_medicalnet_bits_gpu.py): for every output tensor of the cases in
tests/medicalnet_bits_cases.py the SHA-256 of its bytes, its f64 sum and its absolute maximum.  Needs the GPU.

    python tools/gen_golden_medicalnet_bits.py --lib LIB

LIB is a build of the commit whose bits are to be pinned: a refactoring of csrc/medicalnet*.hip records from its PARENT and must
pass unchanged -- the file is never re-recorded from the code under test.  Every case runs twice, on memory poisoned with either
value of tests/alloc_poison.py; if the two runs differ in one bit nothing is written: the kernels promise fixed reduction orders.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "medicalnet_bits.npz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="library whose bits are recorded (a build of the parent commit)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import tools.diaglib as D
    lib = D.use(a.lib)
    import medicalnet_bits_cases as B
    first, second = B.Cases("nan"), B.Cases("big")
    rows, unstable = [], []
    for name in B.CASES:
        one, two = B.run(name, first), B.run(name, second)
        unstable += [k for (k, d1), (_, d2) in zip(one, two) if d1[0] != d2[0]]
        rows += one
        print(f"{name}: {len(one)} tensors")
    if unstable:
        sys.exit("two runs differ, nothing written: " + ", ".join(unstable))
    np.savez_compressed(a.out, name=np.array([k for k, _ in rows]), sha256=np.array([d[0] for _, d in rows]),
                        sum=np.array([d[1] for _, d in rows], dtype=np.float64),
                        absmax=np.array([d[2] for _, d in rows], dtype=np.float64))
    print(f"wrote {a.out}: {len(rows)} tensors from {lib}, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
