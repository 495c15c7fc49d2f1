"""Preprocessing, host side: the gradient table, the kernels' per-voxel arithmetic compiled with g++ (plain and
under the address / undefined-behaviour sanitizers, as a stand-alone program), the argument checks of every new entry point
and the range bookkeeping.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import preprocess_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENTRY_POINTS = ("mi355_dtifit", "mi355_channel_minmax", "mi355_bssfp_workspace_bytes", "mi355_bssfp_phase_sums",
                "mi355_bssfp_phase_correct", "mi355_bssfp_assemble", "mi355_normalize_channels")


# ------------------------------------------------------------------------------------------------------------ gradient table
def _seven():
    """b = 0 once, then b = 1000 along x, y, z and the three face diagonals: the design matrix by hand"""
    r = np.sqrt(0.5)
    bvals = np.array([0, 1000, 1000, 1000, 1000, 1000, 1000.0])
    bvecs = np.array([[0, 1, 0, 0, r, r, 0], [0, 0, 1, 0, r, 0, r], [0, 0, 0, 1, 0, r, r]])
    design = np.array([[0, 0, 0, 0, 0, 0, 1],
                       [-1000, 0, 0, 0, 0, 0, 1],
                       [0, 0, 0, -1000, 0, 0, 1],
                       [0, 0, 0, 0, 0, -1000, 1],
                       [-500, -1000, 0, -500, 0, 0, 1],
                       [-500, 0, -1000, 0, 0, -500, 1],
                       [0, 0, 0, -500, -1000, -500, 1.0]])
    return bvals, bvecs, design


def test_gradient_table_hand_written_case():
    from unet_bssfp_amd import preprocess as P
    bvals, bvecs, design = _seven()
    t = P.gradient_table(bvals, bvecs)
    assert t.n == 7 and t.design.dtype == np.float64 and t.design.shape == (7, 7) and t.pinv.shape == (7, 7)
    np.testing.assert_allclose(t.design, design, rtol=0, atol=1e-12)
    np.testing.assert_allclose(t.pinv @ t.design, np.eye(7), rtol=0, atol=1e-9)
    np.testing.assert_allclose(t.design, R.design_matrix(bvals, bvecs), rtol=0, atol=0)
    # the model: a known tensor and S0 come back from exact signals
    beta = np.array([1.7e-3, 1e-4, -2e-4, 0.9e-3, 3e-4, 0.6e-3, np.log(800.0)])
    np.testing.assert_allclose(t.pinv @ (t.design @ beta), beta, rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(P.gradient_table(bvals, bvecs.T).design, design, atol=1e-12)      # N x 3 is taken too


def test_gradient_table_reads_fsl_text(tmp_path):
    from unet_bssfp_amd import preprocess as P
    b, g = R.scheme(13)
    np.savetxt(tmp_path / "dwi.bval", b[None], fmt="%g")
    np.savetxt(tmp_path / "dwi.bvec", g, fmt="%.17g")
    t = P.gradient_table(str(tmp_path / "dwi.bval"), tmp_path / "dwi.bvec")
    np.testing.assert_array_equal(t.design, R.design_matrix(b, g))
    assert t.n == 13 and t.pinv.shape == (7, 13)


def test_gradient_table_value_errors():
    from unet_bssfp_amd import preprocess as P
    b, g = R.scheme(13)
    with pytest.raises(ValueError, match="7 .. 512"):
        P.gradient_table(b[:6], g[:, :6])
    b513, g513 = R.scheme(513)
    with pytest.raises(ValueError, match="7 .. 512"):
        P.gradient_table(b513, g513)
    P.gradient_table(*R.scheme(512))
    with pytest.raises(ValueError, match="rank"):
        P.gradient_table(np.full(13, 1000.0), np.where(b > 0, g, [[1.0], [0.0], [0.0]]))   # one shell, no b = 0: S0 is free
    with pytest.raises(ValueError, match="rank"):
        P.gradient_table(b, np.repeat(g[:, -1:], 13, 1))              # one direction
    with pytest.raises(ValueError, match="b-vectors"):
        P.gradient_table(b, g[:, :12])
    with pytest.raises(ValueError, match="finite"):
        P.gradient_table(np.where(np.arange(13) == 3, np.nan, b), g)


# -------------------------------------------------------------------------------------------------- core arithmetic on the host
def _build(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-O2", *flags, "-o", str(exe), os.path.join(HERE, "host_dtifit_check.cpp"), "-lm"])
    return exe


def _run_host(exe, tmp_path, case, raw):
    s = case["dwi"].astype(np.float64)
    np.concatenate([case["design"].ravel(), case["pinv"].ravel(), s.ravel(), raw]).tofile(tmp_path / "in.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0",UBSAN_OPTIONS="halt_on_error=1")
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(case["nvox"]), str(case["n"]),
                           str(len(raw))], env=env)
    o = np.fromfile(tmp_path / "out.bin")
    nv = case["nvox"]
    return o[:7 * nv].reshape(nv, 7), o[7 * nv:14 * nv].reshape(nv, 7), o[14 * nv:15 * nv] != 0, o[15 * nv:]


def _check_host(got, case, raw):
    ols, wls, fell, ph = got
    assert np.all(np.abs(ols - case["ols"]) <= case["ols_bound"])
    np.testing.assert_array_equal(fell, case["fallback"])
    assert np.all(np.abs(wls - case["wls"]) <= R.wls_bound(case)[None, :]), np.abs(wls - case["wls"]).max(0) / R.wls_bound(case)
    np.testing.assert_array_equal(wls[fell], ols[fell])                 # the fallback IS the OLS solution
    np.testing.assert_array_equal(ph, R.phase(raw))                     # three separately rounded operations: bit for bit


@pytest.mark.parametrize("n,bad", [(7, False), (13, True), (64, True), (512, False)])
def test_core_arithmetic_on_host_matches_restatement(tmp_path, n, bad):
    """csrc/dtifit_core.h is plain C++: the SAME per-voxel code the HIP kernels run, compiled with g++"""
    case = R.fit_case((5, 7, 9), n, bad)
    assert bad == bool(case["fallback"].any())
    raw = np.arange(0, 4096, 5, dtype=np.float64)
    _check_host(_run_host(_build(tmp_path, "hdf", []), tmp_path, case, raw), case, raw)


def test_core_arithmetic_on_host_under_sanitizers(tmp_path):
    """the same stand-alone program with -fsanitize=address,undefined: a finding aborts it (non-zero exit)"""
    case = R.fit_case((5, 7, 9), 13, True)
    raw = np.arange(0, 4096, 64, dtype=np.float64)
    exe = _build(tmp_path, "hdf_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    _check_host(_run_host(exe, tmp_path, case, raw), case, raw)


# ------------------------------------------------------------------------------------------------------------ argument checks
def test_entry_points_are_declared_built_and_exported():
    from unet_bssfp_amd import _lib
    make = open(os.path.join(ROOT, "unet_bssfp_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bdtifit\.hip\b", make, flags=re.M) and re.search(r"^SRCS :=.*\bprep\.hip\b", make, flags=re.M)
    header = open(_lib.HEADER_PATH).read()
    assert "#define MI355_DTIFIT_MAX_MEAS 512" in header and _lib.H["DTIFIT_MAX_MEAS"] == 512
    assert len(_lib._structs) == 12                                          # the feature adds no struct
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_argument_checks_before_any_launch():
    """bad arguments return MI355_ERR_ARG with a message; nothing is launched (there is no GPU here, and the pointers are
    small integers that no kernel could touch)"""
    from unet_bssfp_amd import _lib
    lib, E = _lib.load(), _lib.H["ERR_ARG"]
    err = lambda: lib.mi355_last_error()                                  # noqa: E731
    p = 4096                                                              # a non-null "device pointer"
    fit = lambda **k: lib.mi355_dtifit(*[{**dict(dwi=p, nvox=10, n=13, ms=10, vs=1, design=p, pinv=p, method=0, mask=None,   # noqa: E731
                                                 tensor=p, dt=0, ocs=10, ovs=1, s0=None, norm=None, stream=None), **k}[a]
                                         for a in ("dwi", "nvox", "n", "ms", "vs", "design", "pinv", "method", "mask", "tensor",
                                                   "dt", "ocs", "ovs", "s0", "norm", "stream")])
    for n in (6, 0, -1, 513):
        assert fit(n=n) == E and b"7 .. 512" in err()
    for k in ("dwi", "design", "pinv", "tensor"):
        assert fit(**{k: None}) == E and b"null" in err()
    for k in ("ms", "vs", "ocs", "ovs"):
        assert fit(**{k: 0}) == E and b"strides" in err()
        assert fit(**{k: -3}) == E and b"strides" in err()
    assert fit(method=2) == E and b"method" in err()
    assert fit(dt=1) == E and b"dtype" in err()
    assert fit(nvox=-1) == E and b"voxel count" in err()
    import ctypes as C
    assert fit(norm=(C.c_double * 12)(*([0.0, 1.0] * 5 + [2.0, 2.0]))) == E and b"range 5" in err()
    assert fit(nvox=0) == 0                                               # nothing to do is not an error

    assert lib.mi355_channel_minmax(None, 6, 10, None, p, None) == E and b"null" in err()
    assert lib.mi355_channel_minmax(p, 6, 10, None, None, None) == E and b"null" in err()
    assert lib.mi355_channel_minmax(p, 0, 10, None, p, None) == E and b"channel count" in err()
    assert lib.mi355_channel_minmax(p, 6, -1, None, p, None) == E and b"voxel count" in err()

    assert lib.mi355_bssfp_workspace_bytes(0, 10) == E and lib.mi355_bssfp_workspace_bytes(17, 10) == E
    assert lib.mi355_bssfp_workspace_bytes(12, -1) == E
    assert lib.mi355_bssfp_workspace_bytes(12, 1) == 12 * 16
    ws = lib.mi355_bssfp_workspace_bytes(12, 96 * 128 * 128)
    assert ws > 0 and ws % 16 == 0
    for cyc in (0, 17):
        assert lib.mi355_bssfp_phase_sums(p, p, cyc, 10, p, 1 << 20, p, None) == E and b"1 .. 16" in err()
        assert lib.mi355_bssfp_phase_correct(p, p, cyc, 10, p, p, p, None) == E and b"1 .. 16" in err()
        assert lib.mi355_bssfp_assemble(p, p, cyc, 10, None, 0.0, 1.0, 0.0, 1.0, -1, p, None) == E and b"1 .. 16" in err()
    for i in (0, 1, 4, 6):
        a = [p, p, 12, 10, p, 1 << 20, p, None]
        a[i] = None
        assert lib.mi355_bssfp_phase_sums(*a) == E and b"null" in err()
    assert lib.mi355_bssfp_phase_sums(p, p, 12, 10, p, 8, p, None) == E and b"workspace" in err()
    assert lib.mi355_bssfp_phase_sums(p, p, 12, 10, p + 4, 1 << 20, p, None) == E and b"workspace" in err()
    assert lib.mi355_bssfp_phase_sums(p, p, 12, 0, p, 1 << 20, p, None) == E and b"voxel count" in err()
    for i in (0, 1, 4, 5, 6):
        a = [p, p, 12, 10, p, p, p, None]
        a[i] = None
        assert lib.mi355_bssfp_phase_correct(*a) == E and b"null" in err()
    for i in (0, 1, 10):
        a = [p, p, 12, 10, None, 0.0, 1.0, 0.0, 1.0, -1, p, None]
        a[i] = None
        assert lib.mi355_bssfp_assemble(*a) == E and b"null" in err()
    assert lib.mi355_bssfp_assemble(p, p, 12, 10, None, 0.0, 1.0, 0.0, 1.0, 12, p, None) == E and b"repeat_cycle" in err()
    assert lib.mi355_bssfp_assemble(p, p, 12, 10, None, 0.0, 1.0, 0.0, 1.0, -2, p, None) == E and b"repeat_cycle" in err()
    assert lib.mi355_bssfp_assemble(p, p, 12, 10, None, 1.0, 1.0, 0.0, 1.0, -1, p, None) == E and b"range" in err()

    cmap, rng = (C.c_int32 * 6)(*[0] * 6), (C.c_double * 12)(*[0.0, 1.0] * 6)
    far = p + (1 << 20)
    norm = lambda *a: lib.mi355_normalize_channels(*a, None)               # noqa: E731
    assert norm(None, 1, cmap, rng, 6, 10, None, far) == E and b"null" in err()
    assert norm(p, 1, None, rng, 6, 10, None, far) == E and b"null" in err()
    assert norm(p, 1, cmap, None, 6, 10, None, far) == E and b"null" in err()
    assert norm(p, 1, cmap, rng, 6, 10, None, None) == E and b"null" in err()
    assert norm(p, 1, cmap, rng, 0, 10, None, far) == E and b"1 .. 32" in err()
    assert norm(p, 1, cmap, rng, 33, 10, None, far) == E and b"1 .. 32" in err()
    assert norm(p, 1, (C.c_int32 * 6)(0, 0, 1, 0, 0, 0), rng, 6, 10, None, far) == E and b"source channel" in err()
    assert norm(p, 1, cmap, (C.c_double * 12)(*[1.0, 0.0] * 6), 6, 10, None, far) == E and b"range 0" in err()
    assert norm(p, 1, cmap, rng, 6, 10, None, p + 8) == E and b"overlaps" in err()


def test_wrappers_raise_on_cpu_tensors():
    from unet_bssfp_amd import _lib, preprocess as P
    t = P.gradient_table(*R.scheme(13))
    x = torch.ones(13, 2, 2, 2)
    with pytest.raises(_lib.Mi355Error, match="GPU only"):
        P.fit_tensor(x, t)
    with pytest.raises(_lib.Mi355Error, match="GPU only"):
        P.phase_sums(x, x)
    with pytest.raises(_lib.Mi355Error, match="GPU only"):
        P.phase_correct(x, x)
    with pytest.raises(_lib.Mi355Error, match="GPU only"):
        P.assemble_bssfp(x, x, None, (0, 1), (0, 1))
    with pytest.raises(_lib.Mi355Error, match="GPU only"):
        P.assemble_t1w(x[0], None, (0, 1))
    with pytest.raises(_lib.Mi355Error, match="GPU only"):
        P.normalize_tensor(x, (0, 1))
    with pytest.raises(_lib.Mi355Error, match="GPU only"):
        P.RangeAccumulator(6, device="cpu")


# -------------------------------------------------------------------------------------------------------------------- ranges
def test_range_grouping():
    from unet_bssfp_amd import preprocess as P
    per = np.array([[0.1, 2.0], [-0.5, 0.4], [-0.3, 0.6], [0.2, 1.5], [-0.7, 0.1], [0.05, 1.9]])
    merged = P.RangeAccumulator.merge(per, P.TENSOR_GROUPS)
    np.testing.assert_array_equal(merged[[0, 3, 5]], [[0.05, 2.0]] * 3)            # diagonal elements
    np.testing.assert_array_equal(merged[[1, 2, 4]], [[-0.7, 0.6]] * 3)            # off-diagonal elements
    even, odd = P.bssfp_groups(24)
    assert even == tuple(range(0, 24, 2)) and odd == tuple(range(1, 24, 2))
    per24 = np.stack([np.arange(24.0), np.arange(24.0) + 100], 1)
    m24 = P.RangeAccumulator.merge(per24, (even, odd))
    np.testing.assert_array_equal(m24[0::2], [[0.0, 122.0]] * 12)
    np.testing.assert_array_equal(m24[1::2], [[1.0, 123.0]] * 12)
    np.testing.assert_array_equal(P.RangeAccumulator.merge(per, ()), per)           # no group: every channel its own
    for bad in (((0, 1), (1, 2)), ((0, 6),), ((),), ((-1,),)):
        with pytest.raises(ValueError, match="groups"):
            P.RangeAccumulator._check_groups(bad, 6)


def test_rescale_args_round_trip(tmp_path):
    from unet_bssfp_amd import augment, preprocess as P
    r = np.array([[0.05, 2.0], [-0.7, 0.6], [-0.7, 0.6], [0.05, 2.0], [-0.7, 0.6], [0.05, 2.0]]) * (1.0 / 3.0)
    P.write_rescale_args(tmp_path / "rescale_args_dwi.txt", r)
    min_v, max_v = np.loadtxt(tmp_path / "rescale_args_dwi.txt")                    # the reference's reading (src/eval.py:51-52)
    np.testing.assert_array_equal(min_v, r[:, 0])
    np.testing.assert_array_equal(max_v, r[:, 1])
    back = P.read_rescale_args(tmp_path / "rescale_args_dwi.txt")
    np.testing.assert_array_equal(back, r)                                          # %.17g: bit for bit
    np.testing.assert_array_equal(augment.check_tensor_rescale(back), r)
    P.write_rescale_args(tmp_path / "one.txt", (1.0 / 7.0, 3.5))
    min_v, max_v = np.loadtxt(tmp_path / "one.txt")
    assert (float(min_v), float(max_v)) == (1.0 / 7.0, 3.5)
    np.testing.assert_array_equal(P.read_rescale_args(tmp_path / "one.txt"), [[1.0 / 7.0, 3.5]])


def test_phase_flip_cap_of_the_chosen_seeds():
    """the assembled-phase test leaves out voxels with |phase| > pi - 1e-4 and caps them at 1e-3 of the voxels: the fixed
    cases stay under the cap (uniform phases give about 3e-5)"""
    for p in (12, 3):
        mag, raw, mask = R.bssfp_case(p, (17, 16, 33))
        re, im = R.phase_correct(mag, raw)
        for rep in (None, 1):
            _, pha = R.assemble(re.astype(np.float32), im.astype(np.float32), mask, (0.0, 1.0), (-np.pi, np.pi), rep)
            assert np.mean(np.abs(pha) > np.pi - 1e-4) <= 1e-3
