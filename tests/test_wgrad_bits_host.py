"""Every case of the weight-gradient bit pin (tests/wgrad_bits_cases.py) lands on the plan kind and slab count its row names, and
the list as a whole reaches every kind.  No GPU: the planner is host code and reads no memory behind the descriptor's pointers.
The slab count, with the rules of make_reduce_job, fixes the reduction form each row's comment states."""
import ctypes as C

import pytest

import wgrad_bits_cases as B


@pytest.fixture(scope="module")
def lib():
    from unet_bssfp_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", B.NAMES)
def test_case_lands_on_its_kernel(lib, name):
    c = B.case(name)
    d = c.desc()
    ws = lib.mi355_conv_wgrad_workspace(C.byref(d))
    assert ws > 0 and ws % c.slab_bytes(d) == 0
    assert (lib.mi355_conv_wgrad_plan_kind(C.byref(d)), ws // c.slab_bytes(d)) == (c.kind, c.nslabs)


def test_the_cases_reach_every_kind():
    assert {B.Case(row).kind for row in B.CASES} == {B.GENERIC, B.TILE, B.MARCH, B.POINTWISE, B.MARCH2}
    assert len(set(B.NAMES)) == len(B.NAMES)
