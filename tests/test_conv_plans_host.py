"""The convolution planners answer what tests/golden/conv_plans.npz recorded (no GPU: both planners are host code).

For every forward descriptor: plan id, d-segment length, both outputs of mi355_conv_num_tiles and the split-K workspace; for
every weight-gradient descriptor: plan kind and slab workspace (which fixes the slab count, so the splits and segments).
A descriptor the planner refuses is pinned as refused.  The descriptors are the sweeps of tests/conv_plan_cases.py plus the
real ones of a training step per audit configuration (rows in the table).  tools/gen_golden_conv_plans.py records the table;
a change that is not meant to move a plan must pass against the table of its parent commit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_plan_cases as P  # noqa: E402

# halo tile shapes the planner can produce (the shape comment of csrc/conv_api.hip)
HALO_SHAPES = {0, 1, 2, 4, 5, 6, 9, 10, 11, 12, 13, 14}
GATHER_KS = {1, 2, 3, 4}


@pytest.fixture(scope="module")
def lib():
    from unet_bssfp_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "conv_plans.npz"))


def _same(got, want, names, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)       # one result per descriptor: no row skipped
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} rows differ; first row {bad[0]} ({names}): got {got[bad[0]]}, pinned {want[bad[0]]}"


def _plans(ops, rows):
    return [ops.decode_plan_id(int(p)) for p in np.unique(rows[:, 0]) if p > 0]


def _halo_shapes(ops, rows):
    return {p.shape for p in _plans(ops, rows) if p.halo}


def test_forward_plans_match_the_table(lib, golden):
    from unet_bssfp_amd import _lib, ops
    assert list(golden["fwd_columns"]) == P.columns(_lib.ConvDesc)      # the rows still mean the same fields
    real = [P.unflatten(_lib.ConvDesc, r) for r in golden["fwd_real_desc"]]
    assert len(real) > 0 and all(P.flatten(d) == list(r) for d, r in zip(real, golden["fwd_real_desc"]))
    got_real, got_sweep = P.table(lib, P.query_fwd, real, 5), P.table(lib, P.query_fwd, P.fwd_sweep(), 5)
    _same(got_sweep, golden["fwd_sweep"], P.FWD_RESULTS, "forward sweep")
    _same(got_real, golden["fwd_real"], P.FWD_RESULTS, "forward descriptors of the training steps")
    # the table leaves nothing out: every family, split-K on and off, refusals, and the real rows are all accepted
    assert (got_real[:, 0] > 0).all()
    both = np.concatenate([got_sweep, got_real])
    assert _halo_shapes(ops, both) == HALO_SHAPES
    assert {p.ks for p in _plans(ops, both) if not p.halo} == GATHER_KS
    assert (both[:, 0] == P.REJECTED).any()
    accepted = both[both[:, 0] > 0]
    assert (accepted[:, 4] > 0).any() and (accepted[:, 4] == 0).any()           # split-K on and off
    # the real steps reach the families the audit demands of them
    real_shapes = _halo_shapes(ops, got_real)
    assert {ops.SHAPE_MARCH, ops.SHAPE_MARCHG, ops.SHAPE_MARCH2} <= real_shapes and real_shapes & set(ops.SHAPES_LOWG)


def test_weight_gradient_plans_match_the_table(lib, golden):
    from unet_bssfp_amd import _lib
    assert list(golden["wgrad_columns"]) == P.columns(_lib.WgradDesc)
    real = [P.unflatten(_lib.WgradDesc, r) for r in golden["wgrad_real_desc"]]
    assert len(real) > 0 and all(P.flatten(d) == list(r) for d, r in zip(real, golden["wgrad_real_desc"]))
    got_real, got_sweep = P.table(lib, P.query_wgrad, real, 2), P.table(lib, P.query_wgrad, P.wgrad_sweep(), 2)
    _same(got_sweep, golden["wgrad_sweep"], P.WGRAD_RESULTS, "weight-gradient sweep")
    _same(got_real, golden["wgrad_real"], P.WGRAD_RESULTS, "weight-gradient descriptors of the training steps")
    assert (got_real[:, 0] >= 0).all()
    assert set(np.unique(got_sweep[:, 0])) == {P.REJECTED, 0, 1, 2, 3, 4}
    assert {1, 2, 3, 4} <= set(np.unique(got_real[:, 0]))
