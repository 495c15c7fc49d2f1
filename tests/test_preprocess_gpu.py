"""Preprocessing kernels on the GPU against the f64 numpy restatement tests/preprocess_ref.py: the tensor fit
(OLS / WLS, every layout, masks, fused normalisation, bad signals, unwritten memory), the dataset ranges, the bSSFP phase
correction and channel assembly, the T1w copy and the files-to-files pipeline.  Every test prints its measured figure before
it asserts (run with -s to see them)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import preprocess_ref as R
from tests.alloc_poison import poisoned

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
EPS32 = 2.0 ** -24                      # half an f32 ulp, relative


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)              # a copy: the shared cases are read-only


def _series(case, layout="cf"):
    """the (nvox, n) f32 series as a device tensor: 'cf' = (n, *grid), 'nifti' = (*grid, n)"""
    d = case["dwi"].reshape(case["grid"] + (case["n"],))
    return _dev(np.moveaxis(d, -1, 0)) if layout == "cf" else _dev(d)


def _table(case):
    from unet_bssfp_amd import preprocess as P
    return P.gradient_table(case["bvals"], case["bvecs"])


def _flat(t):
    """(6, *grid) device tensor -> (nvox, 6) f64 numpy"""
    return t.detach().cpu().numpy().reshape(6, -1).T.astype(np.float64)


def _f32_slack(ref):
    return EPS32 * np.abs(ref) * (1 + 1e-6) + 2.0 ** -149


CASES = [(g, n) for g in R.GRIDS for n in R.MEAS]


# ----------------------------------------------------------------------------------------------------------------- the fit
@pytest.mark.parametrize("grid,n", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fit_ols_against_restatement(hip, grid, n):
    """f64 output within 2 (N + 4) 2^-53 sum_i |P_ji| |y_i| per component; f32 output adds half an f32 ulp of the value;
    S0 = exp(beta_7) within S0 (bound_7 + 4 ulp)"""
    from unet_bssfp_amd import preprocess as P
    case = R.fit_case(grid, n)
    dwi, table = _series(case), _table(case)
    t64, s64 = P.fit_tensor(dwi, table, "ols", dtype=F64, return_s0=True)
    t32, s32 = P.fit_tensor(dwi, table, "ols", dtype=F32, return_s0=True)
    ref, bound = case["ols"], case["ols_bound"]
    e64 = np.abs(_flat(t64) - ref[:, :6])
    e32 = np.abs(_flat(t32) - ref[:, :6])
    print(f"ols {grid} N={n}: f64 error / bound = {np.max(e64 / bound[:, :6]):.3f}, f32 = {np.max(e32 / (bound[:, :6] + _f32_slack(ref[:, :6]))):.3f}")
    assert np.all(e64 <= bound[:, :6])
    assert np.all(e32 <= bound[:, :6] + _f32_slack(ref[:, :6]))
    s0_ref = np.exp(ref[:, 6])
    s0_bound = s0_ref * (bound[:, 6] + 4 * R.EPS64)
    assert np.all(np.abs(s64.cpu().numpy().reshape(-1) - s0_ref) <= s0_bound)
    assert np.all(np.abs(s32.cpu().numpy().reshape(-1).astype(np.float64) - s0_ref) <= s0_bound + _f32_slack(s0_ref))


@pytest.mark.parametrize("grid,n", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fit_wls_against_restatement(hip, grid, n):
    """no derivable bound: the kernel lies within 4 x the largest difference, per component, between the restatement's two
    solutions of the case (Cholesky on the normal equations, lstsq on sqrt(W) A)"""
    from unet_bssfp_amd import preprocess as P
    case = R.fit_case(grid, n)
    got = _flat(P.fit_tensor(_series(case), _table(case), "wls", dtype=F64))
    err, bound = np.abs(got - case["wls"][:, :6]).max(0), R.wls_bound(case)[:6]
    print(f"wls {grid} N={n}: max error per component / (4 x reference spread) = {np.array2string(err / bound, precision=3)}; "
          f"largest relative error {np.max(np.abs(got - case['wls'][:, :6]) / np.abs(case['wls'][:, :6]).max(0)):.2e}")
    assert not case["fallback"].any()
    assert np.all(err <= bound)


@pytest.mark.parametrize("grid,n", [((1, 1, 1), 13), ((5, 7, 9), 13), ((5, 7, 9), 64), ((17, 16, 33), 13)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fit_bad_signals(hip, grid, n):
    """signals <= 0: y = 0 in OLS, weight 0 in WLS; a voxel with fewer than 7 positive signals takes the OLS solution"""
    from unet_bssfp_amd import preprocess as P
    case = R.fit_case(grid, n, True)
    dwi, table = _series(case), _table(case)
    assert (case["dwi"] <= 0).any() and case["fallback"].any() and (grid == (1, 1, 1) or not case["fallback"].all())
    ols = _flat(P.fit_tensor(dwi, table, "ols", dtype=F64))
    wls = _flat(P.fit_tensor(dwi, table, "wls", dtype=F64))
    assert np.all(np.abs(ols - case["ols"][:, :6]) <= case["ols_bound"][:, :6])
    err, bound = np.abs(wls - case["wls"][:, :6]).max(0), R.wls_bound(case)[:6]
    fb = case["fallback"]
    if (~fb).any():
        print(f"bad signals {grid} N={n}: wls error / bound = {np.array2string(err / bound, precision=3)}")
    print(f"bad signals {grid} N={n}: {int(fb.sum())} of {case['nvox']} voxels fall back")
    np.testing.assert_array_equal(wls[fb], ols[fb])                     # the fallback is the OLS solution, bit for bit
    assert np.all(np.abs(wls - case["wls"][:, :6])[fb] <= case["ols_bound"][:, :6][fb])
    assert np.all(np.abs(wls - case["wls"][:, :6])[~fb] <= bound[None, :])


@pytest.mark.parametrize("method", ["ols", "wls"])
@pytest.mark.parametrize("n", [13, 64])
def test_fit_round_trip(hip, method, n):
    """a random positive-definite tensor field and S0, several b = 0 rows, S_i = S0 exp(-b g^T D g): both methods recover
    D and S0 (bound: preprocess_ref.roundtrip_bound, from the f32 rounding of the series and the solver's conditioning)"""
    from unet_bssfp_amd import preprocess as P
    case = R.fit_case((5, 7, 9), n)
    assert (case["bvals"] == 0).sum() >= 2
    t, s0 = P.fit_tensor(_series(case), _table(case), method, dtype=F64, return_s0=True)
    bound = R.roundtrip_bound(case, method)
    err = np.abs(_flat(t) - case["d6"])
    rel_s0 = np.abs(s0.cpu().numpy().reshape(-1) / case["s0"] - 1)
    print(f"round trip {method} N={n}: max |D - D_true| = {err.max():.3e} (bound {bound[:, :6].max():.3e}, ratio "
          f"{np.max(err / bound[:, :6]):.3f}); max relative S0 error {rel_s0.max():.3e}")
    assert np.all(err <= bound[:, :6])
    assert np.all(rel_s0 <= 2 * bound[:, 6] + 8 * R.EPS64)              # exp(d) - 1 <= 2 d for small d


@pytest.mark.parametrize("method", ["ols", "wls"])
@pytest.mark.parametrize("grid", [(5, 7, 9), (17, 16, 33)], ids=lambda g: "x".join(map(str, g)))
def test_fit_layouts_mask_and_fused_normalisation(hip, method, grid):
    """both input layouts, both output layouts, f32 and f64, mask on and off, and the fused normalisation: one set of bits.
    (17 x 16 x 33 channel-first takes the 16-byte loads in OLS, 5 x 7 x 9 and the interleaved series the 4-byte ones.)"""
    from unet_bssfp_amd import preprocess as P
    case = R.fit_case(grid, 13)
    table = _table(case)
    cf, nii = _series(case, "cf"), _series(case, "nifti")
    base = P.fit_tensor(cf, table, method, dtype=F64)
    base_np = base.cpu().numpy()
    mask_np = (np.random.default_rng(5).random(grid) < 0.6).astype(np.uint8)
    mask = _dev(mask_np)
    for dwi, first in ((cf, True), (nii, False)):
        for dt in (F64, F32):
            want = base_np.astype(np.float64 if dt == F64 else np.float32)
            for out_first in (True, False):
                for m in (None, mask):
                    got = P.fit_tensor(dwi, table, method, mask=m, channels_first=first, out_channels_first=out_first, dtype=dt)
                    got = got.cpu().numpy() if out_first else np.moveaxis(got.cpu().numpy(), -1, 0)
                    np.testing.assert_array_equal(got, want if m is None else np.where(mask_np[None] != 0, want, 0))
    # fused normalisation == the unfused f64 result normalised in f64, after the same rounding
    lo = base_np.reshape(6, -1).min(1) - 1e-4
    norm = np.stack([lo, base_np.reshape(6, -1).max(1) + 2e-4], 1)
    want = R.normalize(base_np, norm[:, 0].reshape(6, 1, 1, 1), norm[:, 1].reshape(6, 1, 1, 1))
    for dt, npdt in ((F64, np.float64), (F32, np.float32)):
        fused = P.fit_tensor(nii, table, method, mask=mask, norm=norm, channels_first=False, dtype=dt).cpu().numpy()
        np.testing.assert_array_equal(fused, np.where(mask_np[None] != 0, want, 0).astype(npdt))
    # and the unfused call: normalize_tensor of the f32 tensor is ((double)x - min) / (max - min), rounded once
    t32 = P.fit_tensor(cf, table, method, dtype=F32)
    unfused = P.normalize_tensor(t32, norm, mask).cpu().numpy()
    want32 = R.normalize(t32.cpu().numpy().astype(np.float64), norm[:, 0].reshape(6, 1, 1, 1), norm[:, 1].reshape(6, 1, 1, 1))
    np.testing.assert_array_equal(unfused, np.where(mask_np[None] != 0, want32, 0).astype(np.float32))


def test_fit_vector_loads_with_a_partial_last_group(hip):
    """OLS through the C ABI with a measurement stride padded to 16 bytes: 315 voxels = 78 groups of four and a tail of 3"""
    from unet_bssfp_amd import _lib, preprocess as P
    case = R.fit_case((5, 7, 9), 13)
    nvox, n, ms = case["nvox"], 13, 316
    padded = np.full((n, ms), np.nan, np.float32)
    padded[:, :nvox] = case["dwi"].T
    dwi, out = _dev(padded), torch.full((6, nvox + 5), -7.0, dtype=F64, device=DEV)
    design, pinv = _table(case).on(DEV)
    _lib.check(hip.mi355_dtifit(dwi.data_ptr(), nvox, n, ms, 1, design.data_ptr(), pinv.data_ptr(), 0, None, out.data_ptr(), 2,
                                nvox + 5, 1, None, None, torch.cuda.current_stream().cuda_stream))
    want = P.fit_tensor(_series(case), _table(case), "ols", dtype=F64).reshape(6, -1)
    assert torch.equal(out[:, :nvox], want) and bool((out[:, nvox:] == -7.0).all())      # nothing past the last voxel


@pytest.mark.parametrize("method", ["ols", "wls"])
def test_fit_writes_every_output_element(hip, method):
    """outputs allocated under the NaN poison, a mask, S0 and both output layouts: every element is finite afterwards"""
    from unet_bssfp_amd import preprocess as P
    case = R.fit_case((5, 7, 9), 13, True)
    dwi, table, grid = _series(case), _table(case), case["grid"]
    mask = _dev((np.random.default_rng(6).random(grid) < 0.5).astype(np.uint8))
    with poisoned("nan") as stats:
        for out_first in (True, False):
            for dt in (F32, F64):
                out = torch.empty((6,) + grid if out_first else grid + (6,), dtype=dt, device=DEV)
                s0 = torch.empty(grid, dtype=dt, device=DEV)
                assert bool(torch.isnan(out).all()) and bool(torch.isnan(s0).all())
                t, s = P.fit_tensor(dwi, table, method, mask=mask, out_channels_first=out_first, dtype=dt, out=out, out_s0=s0)
                assert t is out and s is s0
                assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(s0).all())
                off = (mask == 0)
                assert bool((s0[off] == 0).all()) and bool(((out if out_first else out.movedim(-1, 0))[:, off] == 0).all())
    assert stats.filled >= 8


# ------------------------------------------------------------------------------------------------------------------ ranges
@pytest.mark.parametrize("grid", R.GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_ranges_bit_exact_over_two_subjects(hip, grid):
    from unet_bssfp_amd import preprocess as P
    rng = np.random.default_rng(11 + int(np.prod(grid)))
    subjects = [(rng.standard_normal((6,) + grid).astype(np.float32) * s, (rng.random(grid) < p).astype(np.uint8))
                for s, p in ((1.0, 0.7), (3.0, 0.4))]
    if grid == (1, 1, 1):
        subjects = [(x, np.ones(grid, np.uint8)) for x, _ in subjects]
    acc = P.RangeAccumulator(6, P.TENSOR_GROUPS, DEV)
    want = None
    for x, m in subjects:
        acc.update(_dev(x), _dev(m))
        want = R.channel_minmax(x, m, want)
    np.testing.assert_array_equal(acc.buffer.cpu().numpy(), want)        # f32 bits
    np.testing.assert_array_equal(acc.ranges(), P.RangeAccumulator.merge(want.astype(np.float64), P.TENSOR_GROUPS))
    assert len(acc.group_ranges()) == 2
    # no mask = every voxel; an unaligned view takes the 4-byte loads
    acc2 = P.RangeAccumulator(6, (), DEV)
    acc2.update(_dev(subjects[0][0]))
    np.testing.assert_array_equal(acc2.buffer.cpu().numpy(), R.channel_minmax(subjects[0][0]))


def test_ranges_empty_mask_leaves_the_initial_values(hip):
    from unet_bssfp_amd import preprocess as P
    acc = P.RangeAccumulator(3, (), DEV)
    x = _dev(np.random.default_rng(1).standard_normal((3, 5, 7, 9)).astype(np.float32))
    acc.update(x, torch.zeros((5, 7, 9), dtype=torch.uint8, device=DEV))
    np.testing.assert_array_equal(acc.buffer.cpu().numpy(), [[np.inf, -np.inf]] * 3)
    acc.update(torch.full((3, 5, 7, 9), float("nan"), device=DEV))        # NaN values are skipped
    np.testing.assert_array_equal(acc.buffer.cpu().numpy(), [[np.inf, -np.inf]] * 3)


# ------------------------------------------------------------------------------------------------------------------- bSSFP
@pytest.mark.parametrize("grid", R.GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_bssfp_phase_sums_and_correction(hip, grid):
    """per-cycle complex sums within n_vox 2^-53 sum |term| of numpy's f64 sum and bit-identical over two runs; corrected
    re / im within 2^-22 of the magnitude (f32 output rounding)"""
    from unet_bssfp_amd import preprocess as P
    mag, raw, _ = R.bssfp_case(12, grid)
    dm, dr = _dev(mag), _dev(raw)
    s1, s2 = P.phase_sums(dm, dr), P.phase_sums(dm, dr)
    assert torch.equal(s1, s2)
    want, abs_sum = R.phase_sums(mag, raw)
    nvox = int(np.prod(grid))
    err, bound = np.abs(s1.cpu().numpy() - want), nvox * R.EPS64 * abs_sum[:, None]
    print(f"phase sums {grid}: error / (n_vox 2^-53 sum|term|) = {np.max(err / bound):.4f}")
    assert np.all(err <= bound)
    re, im = P.phase_correct(dm, dr)
    wre, wim = R.phase_correct(mag, raw)
    tol = 2.0 ** -22 * mag.astype(np.float64)
    e = np.maximum(np.abs(re.cpu().numpy() - wre), np.abs(im.cpu().numpy() - wim))
    print(f"corrected re / im {grid}: max error / magnitude = {np.max(e / np.maximum(mag, 1e-30)):.3e} (bound {2.0 ** -22:.3e})")
    assert np.all(e <= tol)


@pytest.mark.parametrize("p", [12, 3])
@pytest.mark.parametrize("repeat", [None, 1])
def test_bssfp_assembled_channels(hip, p, repeat):
    """channel 2i = normalised |z_i|, 2i + 1 = normalised atan2(im_i, re_i), masked voxels 0.  Magnitudes within f32 rounding;
    phases too, leaving out voxels where the restatement's |phase| > pi - 1e-4 (a 2 pi flip there is either side's choice):
    at most 1e-3 of the voxels"""
    from unet_bssfp_amd import preprocess as P
    grid = (17, 16, 33)
    mag, raw, mask = R.bssfp_case(p, grid)
    re, im = P.phase_correct(_dev(mag), _dev(raw))
    mag_range, pha_range = (0.0, 1024.0), (-np.pi, np.pi)
    got = P.assemble_bssfp(re, im, _dev(mask), mag_range, pha_range, repeat_cycle=repeat).cpu().numpy().astype(np.float64)
    assert got.shape == (2 * p,) + grid
    want, pha = R.assemble(re.cpu().numpy(), im.cpu().numpy(), mask, mag_range, pha_range, repeat)
    on = mask != 0
    assert np.all(got[:, ~on] == 0)
    slack = 8 * R.EPS64
    e_mag = np.abs(got[0::2] - want[0::2])[:, on]
    assert np.all(e_mag <= _f32_slack(want[0::2][:, on]) + slack)
    keep = (np.abs(pha) <= np.pi - 1e-4) & on[None]
    left_out = 1.0 - keep[:, on].mean()
    e_pha = np.abs(got[1::2] - want[1::2])
    print(f"assembled P={p} repeat={repeat}: magnitude error / bound = {np.max(e_mag / (_f32_slack(want[0::2][:, on]) + slack)):.3f}, "
          f"phase = {np.max(e_pha[keep] / (_f32_slack(want[1::2][keep]) + slack)):.3f}, {left_out:.2e} of the voxels left out")
    assert left_out <= 1e-3
    assert np.all(e_pha[keep] <= _f32_slack(want[1::2][keep]) + slack)
    if repeat is not None:
        for i in range(1, p):
            np.testing.assert_array_equal(got[2 * i:2 * i + 2], got[0:2])
    # ranges (0, 1) give the raw values: what the range pass accumulates
    raw_out = P.assemble_bssfp(re, im, None, (0.0, 1.0), (0.0, 1.0)).cpu().numpy()
    want_raw = R.assemble(re.cpu().numpy(), im.cpu().numpy(), None, (0.0, 1.0), (0.0, 1.0))[0]
    assert np.all(np.abs(raw_out[0::2] - want_raw[0::2]) <= _f32_slack(want_raw[0::2]) + 8 * R.EPS64 * want_raw[0::2])


# --------------------------------------------------------------------------------------------------------------------- T1w
@pytest.mark.parametrize("grid", R.GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_t1w_and_normalised_copy(hip, grid):
    """((double)x - min) / (max - min) rounded once, 0 outside the mask: equal to numpy bit for bit"""
    from unet_bssfp_amd import preprocess as P
    rng = np.random.default_rng(21 + int(np.prod(grid)))
    t1 = rng.uniform(0, 3000, grid).astype(np.float32)
    mask = (rng.random(grid) < 0.7).astype(np.uint8)
    got = P.assemble_t1w(_dev(t1), _dev(mask), (1.5, 2987.25)).cpu().numpy()
    want = np.where(mask != 0, R.normalize(t1, 1.5, 2987.25), 0).astype(np.float32)
    assert got.shape == (6,) + grid
    for c in range(6):
        np.testing.assert_array_equal(got[c], want)
    x = rng.standard_normal((5,) + grid).astype(np.float32)
    ranges = np.stack([np.linspace(-4, -3, 5), np.linspace(3, 5, 5)], 1)
    got = P.normalize_tensor(_dev(x), ranges).cpu().numpy()
    np.testing.assert_array_equal(got, R.normalize(x, ranges[:, 0].reshape(5, 1, 1, 1), ranges[:, 1].reshape(5, 1, 1, 1)).astype(np.float32))
    with poisoned("nan"):
        out = torch.empty((6,) + grid, dtype=F32, device=DEV)
        P.assemble_t1w(_dev(t1), _dev(mask), (1.5, 2987.25), out=out)
        assert bool(torch.isfinite(out).all())


# ---------------------------------------------------------------------------------------------------------------- pipeline
def test_pipeline_files_to_files(hip, tmp_path):
    """two synthetic subjects (16^3, N = 13): range pass, output pass, data.subjects_from_nifti loads the files, and the
    written normalised tensor gives the synthetic field's FA through eval.calc_scalar_maps(min_v, max_v)"""
    from oracle import dti_ref
    from unet_bssfp_amd import data, eval as E, nifti, preprocess as P
    grid, n = (16, 16, 16), 13
    case = R.fit_case(grid, n)
    mag, raw, mask0 = R.bssfp_case(12, grid)
    rng = np.random.default_rng(77)
    np.savetxt(tmp_path / "dwi.bval", case["bvals"][None], fmt="%.17g")
    np.savetxt(tmp_path / "dwi.bvec", case["bvecs"], fmt="%.17g")
    subjects, masks = [], []
    for i, scale in enumerate((1.0, 0.5)):
        m = mask0 if i == 0 else (rng.random(grid) < 0.5).astype(np.uint8)
        masks.append(m)
        f = {"sub": f"{i + 1:02d}", "ses": "1", "bval": str(tmp_path / "dwi.bval"), "bvec": str(tmp_path / "dwi.bvec")}
        for key, arr in (("dwi", (case["dwi"] * np.float32(scale)).reshape(grid + (n,))), ("mask", m),
                         ("bssfp_mag", np.moveaxis(mag, 0, -1) * np.float32(scale)), ("bssfp_phase", np.moveaxis(raw, 0, -1)),
                         ("t1w", rng.uniform(0, 3000, grid).astype(np.float32))):
            f[key] = str(tmp_path / f"sub-{i}_{key}.nii.gz")
            nifti.save(np.ascontiguousarray(arr), f[key])
        subjects.append(f)
    acc = P.make_accumulators(12, DEV, tensor_groups=((0, 1, 2, 3, 4, 5),))      # one group: eval takes one (min_v, max_v)
    for f in subjects:
        P.accumulate_subject(f, acc, device=DEV)
    ranges = P.ranges_of(acc)
    assert set(ranges) == set(P.RANGE_KEYS)
    assert np.all(ranges["dwi-tensor"] == ranges["dwi-tensor"][0])
    min_v, max_v = ranges["dwi-tensor"][0]                                       # the accumulated range, one f32 ulp wider
    (lo, hi), = acc["dwi-tensor"].group_ranges()
    assert min_v == np.nextafter(np.float32(lo), np.float32(-np.inf)) and max_v == np.nextafter(np.float32(hi), np.float32(np.inf))
    out_dir = tmp_path / "out"
    entries = [P.preprocess_subject(f, ranges, str(out_dir), device=DEV) for f in subjects]
    want_fa = dti_ref.scalar_maps(case["d6"])["fa"].reshape(grid)
    for f, entry, m in zip(subjects, entries, masks):
        assert set(entry) == {"dwi-tensor", "pc-bssfp", "bssfp", "t1w"} and all(os.path.exists(p) for p in entry.values())
        sub = data.subjects_from_nifti(entry, DEV)
        assert {k: tuple(v["data"].shape) for k, v in sub.items()} == {"dwi-tensor": (6,) + grid, "pc-bssfp": (24,) + grid,
                                                                        "bssfp": (24,) + grid, "t1w": (6,) + grid}
        for v in sub.values():
            t = v["data"]
            assert t.dtype == F32 and float(t.min()) >= 0.0 and float(t.max()) <= 1.0 and bool((t[:, _dev(m) == 0] == 0).all())
        assert torch.equal(sub["bssfp"]["data"][2:4], sub["pc-bssfp"]["data"][0:2])
        fa = E.calc_scalar_maps(sub["dwi-tensor"]["data"], min_v, max_v, channels_first=True)["fa"].cpu().numpy().astype(np.float64)
        # FA is Lipschitz in D with constant <= sqrt(6) / |D|_F; D carries the fit's round-trip bound and the f32 rounding
        # of the stored normalised value (2^-24 of the range); on top, the f32 tolerance of the DTI kernel's own test
        d_err = R.roundtrip_bound(case, "ols")[:, :6] + EPS32 * (max_v - min_v)
        full = case["d6"][:, [0, 1, 2, 1, 3, 4, 2, 4, 5]]
        tol = 2e-6 + np.sqrt(6.0) * np.sqrt((d_err[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]] ** 2).sum(1)) / np.sqrt((full ** 2).sum(1))
        on = m != 0
        err = np.abs(fa - want_fa)[on]
        print(f"pipeline sub-{f['sub']}: max FA error {err.max():.3e} (tolerance >= {tol.min():.3e})")
        assert np.all(err <= tol.reshape(grid)[on])
    np.testing.assert_array_equal(P.read_rescale_args(_save(acc, tmp_path)), acc["dwi-tensor"].ranges())
    # the command line: both passes from a manifest, diagonal / off-diagonal groups, the second subject held out for validation
    import json
    cli_dir = tmp_path / "cli"
    (tmp_path / "manifest.json").write_text(json.dumps({"subjects": subjects, "out_dir": str(cli_dir), "device": DEV, "val": [1]}))
    assert P.main([str(tmp_path / "manifest.json")]) == 0
    made = json.loads((cli_dir / "train_manifest.json").read_text())
    assert len(made["train"]) == 1 and len(made["val"]) == 1 and set(made["train"][0]) == set(entries[0])
    rescale = P.read_rescale_args(cli_dir / "rescale_args_dwi-tensor.txt")
    np.testing.assert_array_equal(rescale, np.asarray(made["tensor_rescale"]))
    assert np.all(rescale[[0, 3, 5]] == rescale[0]) and np.all(rescale[[1, 2, 4]] == rescale[1]) and not np.all(rescale[0] == rescale[1])
    for key in ("bssfp-mag", "bssfp-phase", "t1w"):
        assert P.read_rescale_args(cli_dir / f"rescale_args_{key}.txt").shape == (1, 2)
    # the bSSFP and T1w volumes do not depend on the tensor's grouping: the same bits as the calls above
    for name in ("pc-bssfp", "bssfp", "t1w"):
        np.testing.assert_array_equal(nifti.load(made["val"][0][name])[0], nifti.load(entries[1][name])[0])
    t = data.subjects_from_nifti({"dwi-tensor": made["train"][0]["dwi-tensor"]}, DEV)["dwi-tensor"]["data"]
    assert float(t.min()) >= 0.0 and float(t.max()) <= 1.0


def _save(acc, tmp_path):
    path = tmp_path / "rescale_args_dwi.txt"
    acc["dwi-tensor"].save(path)
    return path
