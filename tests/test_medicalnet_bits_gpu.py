"""Bit pin of the MedicalNet kernels (csrc/medicalnet.hip, csrc/medicalnet_bwd.hip, csrc/medicalnet_common.h): every output tensor of
the cases in tests/medicalnet_bits_cases.py has the SHA-256 that tools/gen_golden_medicalnet_bits.py recorded in
tests/golden/medicalnet_bits.npz from the commit BEFORE the kernels' shared code moved into one header.  No tolerance: the MFMA
sequence per accumulator and every reduction order are part of what these kernels promise (graph replays and repeated backward
passes are compared with torch.equal elsewhere).  A deliberate change of the arithmetic re-records the file from the new code's
parent-to-be and says so; a refactoring never does.
"""
import os

import numpy as np
import pytest

import medicalnet_bits_cases as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "medicalnet_bits.npz"))
    return {str(k): (str(h), float(s), float(m)) for k, h, s, m in zip(z["name"], z["sha256"], z["sum"], z["absmax"])}


@pytest.fixture(scope="module")
def cases(hip):
    return B.Cases("nan")


def test_the_table_holds_exactly_the_cases(golden):
    assert sorted({k.split("/")[0] for k in golden}) == sorted(B.CASES)


@pytest.mark.parametrize("name", B.CASES)
def test_bits_equal_the_recorded_ones(cases, golden, name):
    got = B.run(name, cases)
    assert [k for k, _ in got] == [k for k in golden if k.startswith(name + "/")]
    moved = []
    for k, (sha, total, absmax) in got:
        want = golden[k]
        print(f"{k}: sum {total:.17g} (recorded {want[1]:.17g}), absmax {absmax:.9g} (recorded {want[2]:.9g})")
        if sha != want[0]:
            moved.append(f"{k}: sum {total:.17g} recorded {want[1]:.17g}, absmax {absmax:.9g} recorded {want[2]:.9g}")
    assert not moved, "bits moved:\n  " + "\n  ".join(moved)
