"""Regridding kernels on the GPU against the f64 numpy restatement tests/regrid_ref.py: the B-spline
prefilter, the three interpolation orders on every shared case, the properties that need no restatement, unwritten memory,
the extent limits and the files-to-files pipeline with files on grids of their own.  Every test prints its measured figure
before it asserts (run with -s to see them)."""
import json

import numpy as np
import pytest
import torch

from tests import preprocess_ref as PR
from tests import regrid_ref as R
from tests.alloc_poison import poisoned

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
EPS32 = 2.0 ** -24                      # 2^-24 |ref|: between half an f32 ulp of ref and a whole one, by where ref sits in its
                                        # binade -- an upper bound of the half ulp that the one rounding of the store costs
INTERP = {0: "nearest", 1: "linear", 3: "bspline"}
_ID = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)        # noqa: E731

# The coefficient bound is K_COEF 2^-53 27 max|x|.  K_COEF cannot be derived exactly (the recursion's error constant depends
# on the fma contraction the compiler picks): the largest ratio |kernel - restatement| / (2^-53 27 max|x|) measured on the
# MI355X was MEASURED_COEF_RATIO = 4.952 (the 512-long lines of test_extent_limits; over the five shapes of
# test_coefficients_against_restatement 0.762, 4.788, 3.058, 3.333 and 4.353); K_COEF is 4 x that = 19.8, rounded up to a
# power of two.
MEASURED_COEF_RATIO = 4.952
K_COEF = 32.0


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)              # a copy: the shared cases are read-only


def _f32_slack(ref):
    """an upper bound of half an f32 ulp of ref (see EPS32), with the smallest subnormal for ref = 0"""
    return EPS32 * np.abs(ref) * (1 + 1e-6) + 2.0 ** -149


def _coef_bound(xmax):
    return K_COEF * R.EPS64 * R.PREFILTER_GAIN * xmax


# ------------------------------------------------------------------------------------------------------------- prefilter
@pytest.mark.parametrize("src", [s for s, _ in R.PAIRS], ids=_ID)
def test_coefficients_against_restatement(hip, src):
    """f64 coefficients of a 3-channel volume within K_COEF 2^-53 27 max|x| of the restatement (K_COEF: see the top of the
    file).  Measured on the MI355X: ratios 0.762 (1 x 5 x 7), 4.788 (2 x 3 x 9), 3.058 (5 x 7 x 9), 3.333 (17 x 16 x 33) and 4.353
    (3 x 4 x 130); 4.952 on the 512-long lines of test_extent_limits.  K_COEF = 32."""
    from unet_bssfp_amd import preprocess as P
    k = R.case(src, src, "identity")
    got = P.bspline_coefficients(_dev(k["x"]))
    assert got.dtype == F64 and tuple(got.shape) == k["x"].shape
    ratio = np.abs(got.cpu().numpy() - k["coef"]).max() / (R.EPS64 * R.PREFILTER_GAIN * k["xmax"])
    print(f"coefficients {src}: max |kernel - restatement| / (2^-53 27 max|x|) = {ratio:.4f} (K_COEF = {K_COEF})")
    assert ratio <= K_COEF


# --------------------------------------------------------------------------------------------------------------- regrid
def _check_regrid(src, dst, name, order, channels):
    from unet_bssfp_amd import preprocess as P
    k = R.case(src, dst, name, channels)
    keep = ~(k["boundary"] | k["tie"]) if order == 0 else ~k["boundary"]
    assert keep.mean() >= 0.99 and (k["inside"] & keep).any()
    ref = np.asarray(k[order])
    bound = _f32_slack(ref) + (_coef_bound(k["xmax"]) if order == 3 else 8 * R.EPS64 * k["xmax"])
    x, worst = _dev(k["x"]), 0.0
    for fill in R.FILLS:
        got = P.regrid(x, k["m"], dst, INTERP[order], fill)
        assert got.dtype == F32 and tuple(got.shape) == (channels,) + tuple(dst)
        got = got.cpu().numpy()
        outside = ~k["inside"] & keep
        assert np.all(got[:, outside] == np.float32(fill))                # bit for bit (-0.0 is not a fill of the cases)
        on = k["inside"] & keep
        err = np.abs(got.astype(np.float64) - ref)[:, on]
        worst = max(worst, float(np.max(err / bound[:, on])))
        assert np.all(err <= bound[:, on]), worst
    return worst, k


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("src,dst,name", R.CASES + R.EXACT_CASES, ids=_ID)
def test_regrid_against_restatement(hip, src, dst, name, order):
    """orders 1 and 3 on every pair x matrix case and on the exact cases, C in {1, 3}, fill in {0, -1.5}.  Order 1: within half
    an f32 ulp of the reference plus 8 f64 ulps of max|x|.  Order 3: half an f32 ulp plus the coefficient bound.  Outside
    voxels equal the fill bit for bit."""
    worst = max(_check_regrid(src, dst, name, order, c)[0] for c in (1, 3))
    print(f"order {order} {src}->{dst} {name}: max error / bound = {worst:.4f}")


@pytest.mark.parametrize("src,dst,name", R.NEAREST_CASES + R.EXACT_CASES, ids=_ID)
def test_regrid_nearest_against_restatement(hip, src, dst, name):
    """order 0 where no coordinate lies within the tolerance of a rounding tie: the reference is an input sample, so the
    result equals it bit for bit"""
    from unet_bssfp_amd import preprocess as P
    for c in (1, 3):
        worst, k = _check_regrid(src, dst, name, 0, c)
        got = P.regrid(_dev(k["x"]), k["m"], dst, "nearest", 0.0).cpu().numpy()
        on = k["inside"] & ~(k["boundary"] | k["tie"])
        np.testing.assert_array_equal(got[:, on], np.asarray(k[0])[:, on].astype(np.float32))
    print(f"order 0 {src}->{dst} {name}: max error / bound = {worst:.4f}; inside voxels bit-identical to the gathered input")


# --------------------------------------------------------------------------------- properties that need no restatement
@pytest.mark.parametrize("shape,shift", [(s, (0, 0, 0)) for s in R.IDENTITY_SHAPES] + [(s, R.SHIFT) for s in R.SHIFT_SHAPES], ids=_ID)
def test_identity_and_integer_translation_return_the_input(hip, shape, shift):
    """orders 0 and 1 return the (shifted) input bit for bit; order 3 returns it within the coefficient bound plus half an f32
    ulp: the prefilter inverts the sampling.  Voxels shifted in from outside hold the fill."""
    from unet_bssfp_amd import preprocess as P
    x = _dev(R.volume(3, shape))
    xmax = float(x.abs().max())
    m = np.concatenate([np.eye(3), np.asarray(shift, np.float64)[:, None]], 1)
    idx = torch.meshgrid(*[torch.arange(n, device=DEV) + t for n, t in zip(shape, shift)], indexing="ij")
    ins = torch.stack([(i >= 0) & (i < n) for i, n in zip(idx, shape)]).all(0)
    want = torch.where(ins, x[:, idx[0].clamp(0, shape[0] - 1), idx[1].clamp(0, shape[1] - 1), idx[2].clamp(0, shape[2] - 1)],
                       torch.tensor(-1.5, device=DEV))
    for how in ("nearest", "linear"):
        assert torch.equal(P.regrid(x, m, shape, how, -1.5), want)
    got = P.regrid(x, m, shape, "bspline", -1.5)
    assert torch.equal(got[:, ~ins], want[:, ~ins])
    err = (got.double() - want.double()).abs()
    bound = _coef_bound(xmax) + EPS32 * want.double().abs() * (1 + 1e-6)
    print(f"bspline {shape} shift {shift}: max |regrid - input| / bound = {float((err / bound)[:, ins].max()):.4f}")
    assert bool((err <= bound)[:, ins].all())
    coef = P.bspline_coefficients(x)                                     # the coefficients may be computed once and reused
    assert torch.equal(P.regrid(coef, m, shape, "bspline", -1.5), got)


def test_linear_agrees_with_rigid_resample(hip):
    """order 1 at equal shapes with the ``rot`` matrix against augment.rigid_resample, which computes the coordinates in f32;
    both clamp the corners.  Bound 2^-20 max|x| on voxels inside for both.  The matrix is rounded to f32 for both, the extents
    stay below 32 (a coordinate carries at most 1.5 ulps of 2^-19 from its three f32 fmas) and the volume is smooth: its
    gradient, summed over the axes, is at most 0.15 per voxel at max|x| = 4, so the coordinate error moves the value by
    0.15 * 1.5 * 2^-19 = 0.11 * 2^-20 max|x|; the f32 lerps of rigid_resample add at most six roundings of 2^-22 = 0.4 * 2^-20
    max|x|."""
    from unet_bssfp_amd import augment as A, preprocess as P
    shape = (16, 16, 24)
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    x = np.stack([3.0 + np.sin(0.06 * g[0] + 0.05 * g[1] * (1 - 2 * (k % 2)) + 0.04 * g[2] + k) for k in range(3)]).astype(np.float32)
    m = R.matrix("rot", shape, shape).astype(np.float32).astype(np.float64)
    s = R.coordinates(m, shape)
    n = np.asarray(shape, np.float64).reshape(3, 1, 1, 1)
    both = np.all((s >= -0.5 + 1e-3) & (s < n - 0.5 - 1e-3), axis=0)     # inside for the f32 coordinates too
    assert both.mean() >= 0.14
    got = P.regrid(_dev(x), m, shape, "linear", 0.0).cpu().numpy().astype(np.float64)
    other = A.rigid_resample(_dev(x), m, fill=0.0).cpu().numpy().astype(np.float64)
    xmax = float(np.abs(x).max())
    err = np.abs(got - other)[:, both].max()
    print(f"linear vs rigid_resample {shape}: max difference / (2^-20 max|x|) = {err / (2.0 ** -20 * xmax):.4f}")
    assert err <= 2.0 ** -20 * xmax


# ------------------------------------------------------------------------------------------------------ unwritten memory
@pytest.mark.parametrize("src,dst", [R.PAIRS[0], R.PAIRS[3]], ids=_ID)
def test_every_output_element_is_written(hip, src, dst):
    """NaN-poisoned ``out=`` and coefficient buffers, and every allocation of the wrappers under the poison: the results are
    finite and identical to the unpoisoned ones"""
    from unet_bssfp_amd import preprocess as P
    x, m = _dev(R.volume(3, src)), R.matrix("rot", src, dst)
    plain = {how: P.regrid(x, m, dst, how, -1.5) for how in INTERP.values()}
    plain_coef = P.bspline_coefficients(x)
    with poisoned("nan") as stats:
        coef = torch.empty(x.shape, dtype=F64, device=DEV)
        assert bool(torch.isnan(coef).all())
        assert P.bspline_coefficients(x, out=coef) is coef
        assert bool(torch.isfinite(coef).all()) and torch.equal(coef, plain_coef)
        for how in INTERP.values():
            out = torch.empty((3,) + tuple(dst), dtype=F32, device=DEV)
            assert bool(torch.isnan(out).all())
            assert P.regrid(x, m, dst, how, -1.5, out=out) is out
            assert bool(torch.isfinite(out).all()) and torch.equal(out, plain[how])
            assert torch.equal(P.regrid(x, m, dst, how, -1.5), plain[how])
        out = torch.empty((3,) + tuple(dst), dtype=F32, device=DEV)
        assert torch.equal(P.regrid(coef, m, dst, "bspline", -1.5, out=out), plain["bspline"])
    assert stats.filled >= 5


# ---------------------------------------------------------------------------------------------------------------- limits
def test_extent_limits(hip):
    """an extent of 513 raises before any launch; 512 along W runs: (2, 2, 512) -> (2, 2, 64) against the restatement"""
    from unet_bssfp_amd import _lib, preprocess as P
    for shape in ((1, 2, 2, 513), (1, 2, 513, 2), (1, 513, 2, 2)):
        with pytest.raises(_lib.Mi355Error, match="exceed 512"):
            P.bspline_coefficients(torch.zeros(shape, device=DEV))
        with pytest.raises(_lib.Mi355Error, match="exceed 512"):
            P.regrid(torch.zeros(shape, device=DEV), np.eye(4), (2, 2, 2), "bspline")
    src, dst = (2, 2, 512), (2, 2, 64)
    k = R.case(src, dst, "down", 1)
    coef = P.bspline_coefficients(_dev(k["x"]))
    ratio = np.abs(coef.cpu().numpy() - k["coef"]).max() / (R.EPS64 * R.PREFILTER_GAIN * k["xmax"])
    got = P.regrid(coef, k["m"], dst, "bspline").cpu().numpy().astype(np.float64)
    ref = np.asarray(k[3])
    on = k["inside"] & ~k["boundary"]
    worst = np.max((np.abs(got - ref) / (_f32_slack(ref) + _coef_bound(k["xmax"])))[:, on])
    print(f"extent 512: coefficient ratio {ratio:.4f} (K_COEF = {K_COEF}), regrid error / bound = {worst:.4f}")
    assert ratio <= K_COEF and worst <= 1.0 and on.all()


# -------------------------------------------------------------------------------------------------------------- pipeline
FINE, COARSE, N_DWI, CYCLES = (20, 24, 16), (10, 12, 8), 7, 3
A_FINE = np.eye(4)
A_COARSE = np.array([[2.0, 0, 0, 0.5], [0, 2.0, 0, 0.5], [0, 0, 2.0, 0.5], [0, 0, 0, 1.0]])     # the same field of view


def _subject(tmp_path, tag, grid, affine, scale=1.0):
    """T1w, mask and bSSFP on ``grid``; the DWI series (N = 7) on the 2.0-spaced 10 x 12 x 8 grid"""
    from unet_bssfp_amd import nifti
    case = PR.fit_case(COARSE, N_DWI)
    mag, raw, _ = PR.bssfp_case(CYCLES, grid)
    rng = np.random.default_rng(91)
    g = np.meshgrid(*[np.linspace(-1, 1, n) for n in grid], indexing="ij")
    mask = ((g[0] ** 2 + g[1] ** 2 + g[2] ** 2) < 0.8).astype(np.uint8)
    t1 = (1500.0 + 1200.0 * np.sin(3 * g[0] + 2 * g[1] - g[2]) + rng.uniform(0, 300, grid)).astype(np.float32)
    np.savetxt(tmp_path / "dwi.bval", case["bvals"][None], fmt="%.17g")
    np.savetxt(tmp_path / "dwi.bvec", case["bvecs"], fmt="%.17g")
    f = {"sub": tag, "ses": "1", "bval": str(tmp_path / "dwi.bval"), "bvec": str(tmp_path / "dwi.bvec")}
    arrays = {"dwi": (case["dwi"].reshape(COARSE + (N_DWI,)), A_COARSE), "mask": (mask, affine), "t1w": (t1 * np.float32(scale), affine),
              "bssfp_mag": (np.moveaxis(mag, 0, -1) * np.float32(scale), affine), "bssfp_phase": (np.moveaxis(raw, 0, -1), affine)}
    for key, (arr, aff) in arrays.items():
        f[key] = str(tmp_path / f"sub-{tag}_{key}.nii.gz")
        nifti.save(np.ascontiguousarray(arr), f[key], aff)
    return f, {k: v[0] for k, v in arrays.items()}


def _written(path):
    from unet_bssfp_amd import nifti
    return nifti.load(path)


def _cl(t):
    return np.ascontiguousarray(t.movedim(0, -1).cpu().numpy())


@pytest.mark.parametrize("how", ["linear", "bspline"])
def test_pipeline_regrids_onto_the_dwi_grid(hip, tmp_path, how):
    """T1w, mask and bSSFP on a 1.0-spaced 20 x 24 x 16 grid, the DWI on the 2.0-spaced 10 x 12 x 8 grid: with the ``regrid``
    option the written volumes have the DWI shape and affine, equal the public functions composed by hand bit for bit, and lie
    in [0, 1] (pass 1 regrids too, so a cubic undershoot is inside the range).  Through the command line as well."""
    from unet_bssfp_amd import preprocess as P
    opts = {"interpolation": how, "fill": 0.0}
    f, arr = _subject(tmp_path, "01", FINE, A_FINE)
    f2, arr2 = _subject(tmp_path, "02", FINE, A_FINE, scale=0.5)
    acc = P.make_accumulators(CYCLES, DEV)
    for s in (f, f2):
        P.accumulate_subject(s, acc, device=DEV, regrid=opts)
    ranges = P.ranges_of(acc)
    entry = P.preprocess_subject(f, ranges, str(tmp_path / "out"), device=DEV, regrid=opts)
    # by hand
    m = P.index_matrix(A_FINE, A_COARSE)
    np.testing.assert_array_equal(m, np.concatenate([2 * np.eye(3), np.full((3, 1), 0.5)], 1))
    mask = (P.regrid(_dev((arr["mask"] != 0).astype(np.float32))[None], m, COARSE, "nearest")[0] != 0).to(torch.uint8)
    assert 0.2 < float(mask.float().mean()) < 0.8
    t1 = P.regrid(_dev(arr["t1w"])[None], m, COARSE, how, 0.0)
    re, im = P.phase_correct(_dev(np.moveaxis(arr["bssfp_mag"], -1, 0)), _dev(np.moveaxis(arr["bssfp_phase"], -1, 0)))
    assert tuple(re.shape) == (CYCLES,) + FINE                            # corrected on the native grid ...
    re, im = P.regrid(re, m, COARSE, how, 0.0), P.regrid(im, m, COARSE, how, 0.0)     # ... and only then regridded
    want = {"t1w": P.assemble_t1w(t1, mask, ranges["t1w"]),
            "pc-bssfp": P.assemble_bssfp(re, im, mask, ranges["bssfp-mag"], ranges["bssfp-phase"]),
            "bssfp": P.assemble_bssfp(re, im, mask, ranges["bssfp-mag"], ranges["bssfp-phase"], repeat_cycle=0)}
    for name, t in want.items():
        data, affine = _written(entry[name])
        assert data.shape == COARSE + (t.shape[0],) and data.dtype == np.float32
        np.testing.assert_array_equal(affine, A_COARSE)
        np.testing.assert_array_equal(data, _cl(t))
        print(f"pipeline {how} {name}: written range [{data.min():.6f}, {data.max():.6f}]")
        assert data.min() >= 0.0 and data.max() <= 1.0
    data, affine = _written(entry["dwi-tensor"])
    assert data.shape == COARSE + (6,) and np.array_equal(affine, A_COARSE) and data.min() >= 0.0 and data.max() <= 1.0
    if how == "bspline":
        # the command line: the manifest key
        (tmp_path / "manifest.json").write_text(json.dumps({"subjects": [f, f2], "out_dir": str(tmp_path / "cli"), "device": DEV,
                                                            "cycles": CYCLES, "regrid": opts}))
        assert P.main([str(tmp_path / "manifest.json")]) == 0
        made = json.loads((tmp_path / "cli" / "train_manifest.json").read_text())
        for name in want:
            np.testing.assert_array_equal(_written(made["train"][0][name])[0], _written(entry[name])[0])


def test_pipeline_co_registration_matrix(hip, tmp_path):
    """``files["xfm"]["t1w"]``: a world translation by (2, -4, 0) mm is an index shift of (2, -4, 0) fine voxels"""
    from unet_bssfp_amd import preprocess as P
    f, arr = _subject(tmp_path, "01", FINE, A_FINE)
    xfm = np.eye(4)
    xfm[:3, 3] = (2.0, -4.0, 0.0)
    np.savetxt(tmp_path / "t1w_xfm.txt", xfm, fmt="%.17g")
    f["xfm"] = {"t1w": str(tmp_path / "t1w_xfm.txt")}
    sub = P._load_subject(f, DEV, ("linear", 0.0))
    m = P.index_matrix(A_FINE, A_COARSE, xfm)
    np.testing.assert_array_equal(m[:, 3], [2.5, -3.5, 0.5])
    assert torch.equal(sub["t1"], P.regrid(_dev(arr["t1w"])[None], m, COARSE, "linear")[0])
    assert bool((sub["t1"][:, :2] == 0).all()) and tuple(sub["t1"].shape) == COARSE      # shifted in from outside: the fill
    from unet_bssfp_amd import nifti
    moved = dict(f, bssfp_phase=str(tmp_path / "moved_phase.nii.gz"))        # a phase file off the magnitude's grid
    nifti.save(np.ascontiguousarray(arr["bssfp_phase"]), moved["bssfp_phase"], A_COARSE)
    with pytest.raises(ValueError, match="grid of bssfp_mag"):
        P._load_subject(moved, DEV, ("linear", 0.0))
    with pytest.raises(ValueError, match="4 x 4"):
        np.savetxt(tmp_path / "bad.txt", np.eye(3))
        P._load_subject(dict(f, xfm={"t1w": str(tmp_path / "bad.txt")}), DEV, ("linear", 0.0))


def test_pipeline_without_the_option_is_unchanged(hip, tmp_path):
    """same-grid files and no ``regrid`` key: the bytes of the functions composed by hand, as before the option existed; the
    key on same-grid files changes nothing either; mismatched shapes without the key raise"""
    from unet_bssfp_amd import preprocess as P
    f, arr = _subject(tmp_path, "01", COARSE, A_COARSE)
    acc = P.make_accumulators(CYCLES, DEV)
    P.accumulate_subject(f, acc, device=DEV)
    ranges = P.ranges_of(acc)
    entry = P.preprocess_subject(f, ranges, str(tmp_path / "plain"), device=DEV)
    mask = _dev((arr["mask"] != 0).astype(np.uint8))
    re, im = P.phase_correct(_dev(np.moveaxis(arr["bssfp_mag"], -1, 0)), _dev(np.moveaxis(arr["bssfp_phase"], -1, 0)))
    table = P.gradient_table(f["bval"], f["bvec"])
    want = {"dwi-tensor": P.fit_tensor(_dev(arr["dwi"]), table, "ols", mask, norm=ranges["dwi-tensor"], channels_first=False),
            "t1w": P.assemble_t1w(_dev(arr["t1w"]), mask, ranges["t1w"]),
            "pc-bssfp": P.assemble_bssfp(re, im, mask, ranges["bssfp-mag"], ranges["bssfp-phase"]),
            "bssfp": P.assemble_bssfp(re, im, mask, ranges["bssfp-mag"], ranges["bssfp-phase"], repeat_cycle=0)}
    acc2 = P.make_accumulators(CYCLES, DEV)
    P.accumulate_subject(f, acc2, device=DEV, regrid={"interpolation": "bspline"})
    for key in acc:
        assert torch.equal(acc[key].buffer, acc2[key].buffer)
    keyed = P.preprocess_subject(f, ranges, str(tmp_path / "keyed"), device=DEV, regrid={"interpolation": "bspline"})
    for name, t in want.items():
        data, affine = _written(entry[name])
        np.testing.assert_array_equal(data, _cl(t))
        np.testing.assert_array_equal(affine, A_COARSE)
        np.testing.assert_array_equal(_written(keyed[name])[0], data)
    fine, _ = _subject(tmp_path, "03", FINE, A_FINE)
    with pytest.raises(ValueError, match="does not match"):
        P.preprocess_subject(fine, ranges, str(tmp_path / "bad"), device=DEV)
    with pytest.raises(ValueError, match="does not match"):
        P.accumulate_subject(fine, P.make_accumulators(CYCLES, DEV), device=DEV)
