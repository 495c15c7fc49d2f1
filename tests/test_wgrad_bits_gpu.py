"""Bit pin of the weight-gradient kernels (csrc/wgrad.hip and its wgrad_*.h headers): dw of every case in tests/wgrad_bits_cases.py
has the SHA-256 that tools/gen_golden_wgrad_bits.py recorded in tests/golden/wgrad_bits.npz from the commit BEFORE the source was
split by kernel family.  No tolerance: the MFMA sequence per accumulator, the order in which waves and slabs are added and the
scatter into the torch layout are what these kernels promise (deferred and immediate reductions, graph replays and side-stream
launches are compared with torch.equal elsewhere).  A deliberate change of the arithmetic re-records the file from the new code's
parent-to-be and says so; a refactoring never does.
"""
import os

import numpy as np
import pytest

import wgrad_bits_cases as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "wgrad_bits.npz"))
    return {str(k): (str(h), float(s), float(m)) for k, h, s, m in zip(z["name"], z["sha256"], z["sum"], z["absmax"])}


def test_the_table_holds_exactly_the_cases(golden):
    assert list(golden) == [f"{name}/{way}" for name in B.NAMES for way in B.WAYS]


@pytest.mark.parametrize("name", B.NAMES)
def test_bits_equal_the_recorded_ones(hip, golden, name):
    got = B.run(name)
    assert [k for k, _ in got] == [k for k in golden if k.startswith(name + "/")]
    moved = []
    for k, (sha, total, absmax) in got:
        want = golden[k]
        print(f"{k}: sum {total:.17g} (recorded {want[1]:.17g}), absmax {absmax:.9g} (recorded {want[2]:.9g})")
        if sha != want[0]:
            moved.append(f"{k}: sum {total:.17g} recorded {want[1]:.17g}, absmax {absmax:.9g} recorded {want[2]:.9g}")
    assert not moved, "bits moved:\n  " + "\n  ".join(moved)
    by_way = dict(got)
    for way in B.WAYS[:2]:
        assert by_way[f"{name}/{way}_deferred"][0] == by_way[f"{name}/{way}"][0], f"deferred {way} differs from the immediate one"
