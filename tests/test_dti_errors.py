"""DTI relative-error table (eval.error_table): the numpy oracle against the golden of the reference's own
functions, the shared per-voxel header compiled on the host against the oracle (CPU), the HIP kernel
against golden and oracle, determinism, evaluate_subject and host-side argument errors (GPU)."""
import csv
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dti_errors_ref as ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "dti_errors.npz")
CASES = ("c1", "c2", "c3")


def _case(g, c):
    mm = g[f"{c}_minmax"]
    min_v, max_v = (None, None) if mm.size == 0 else (float(mm[0]), float(mm[1]))
    return g[f"{c}_pred"], g[f"{c}_target"], g[f"{c}_mask"], g[f"{c}_probseg"], min_v, max_v


def _assert_close(got, want, rtol, atol=0.0, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ"
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=rtol, atol=atol, err_msg=what)


# ------------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize("case", CASES)
def test_oracle_reproduces_reference_golden(case):
    g = np.load(GOLD)
    pred, target, mask, ps, min_v, max_v = _case(g, case)
    table, maps = ref.error_table(pred, target, mask, ps, min_v, max_v)
    _assert_close(table, g[f"{case}_table"], 1e-12, what="table")
    _assert_close(maps, g[f"{case}_maps"], 1e-12, what="maps")


def test_golden_pins_the_edge_cases():
    g = np.load(GOLD)
    assert np.isfinite(g["c1_table"]).all()
    assert np.isnan(g["c2_table"][:, :10]).all() and np.isfinite(g["c2_table"][:, 10:]).all()
    assert np.isnan(g["c3_table"][1]).all() and np.isfinite(g["c3_table"][[0, 2]]).all()
    pred, target, mask, ps, _, _ = _case(g, "c1")
    inside = mask.astype(np.uint8) > 0
    assert ((target == 0) & (pred != 0) & inside[..., None]).any()              # inf -> 0
    assert (np.all(pred == target, -1) & inside).any()
    assert (np.all(pred == 0, -1) & ~inside).any()                              # NaN outside the mask -> 0
    assert ((mask > 0) & ~inside).any()                                         # 0.5 -> uint8 0
    p = ps.astype(np.float64)[inside]
    assert ((p > 0.9e-5) & (p <= 1e-5)).any() and ((p > 1e-5) & (p < 1.1e-5)).any()


def _host_check(tmp_path, pred, target, mask, ps, min_v=None, max_v=None):
    exe = tmp_path / "hdec"
    if not exe.exists():
        subprocess.check_call(["g++", "-O2", "-o", str(exe), os.path.join(HERE, "host_dti_errors_check.cpp"), "-lm"])
    n, nroi = mask.size, ps.shape[-1]
    with open(tmp_path / "in.bin", "wb") as fh:
        for a in (pred, target, ps):
            np.ascontiguousarray(a, np.float64).tofile(fh)
        np.ascontiguousarray(mask.astype(np.uint8)).tofile(fh)
    scale, offset = (1.0, 0.0) if min_v is None else (abs(max_v - min_v), min_v)
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(n), str(nroi),
                           repr(scale), repr(offset)])
    out = np.fromfile(tmp_path / "out.bin")
    maps = np.moveaxis(out[:12 * n].reshape(n, 12), -1, 0).reshape((12,) + mask.shape)
    return out[12 * n:].reshape(nroi, 12), maps


def test_core_header_on_host_matches_oracle(tmp_path):
    """csrc/dti_errors_core.h is plain C++: the per-voxel code the kernel runs, compiled with g++ -- on the golden
    subjects and on random SPD / indefinite tensors with random masks, against the oracle (LAPACK)."""
    g = np.load(GOLD)
    for c in CASES:
        pred, target, mask, ps, min_v, max_v = _case(g, c)
        table, maps = _host_check(tmp_path, pred, target, mask, ps, min_v, max_v)
        _assert_close(maps[:6], g[f"{c}_maps"][:6], 0, what=f"{c} components")              # same f64 formula
        _assert_close(maps[6:], g[f"{c}_maps"][6:], 1e-11, 1e-11, what=f"{c} maps")
        _assert_close(table, g[f"{c}_table"], 1e-12, what=f"{c} table")
    rng = np.random.default_rng(7)
    for seed, (shape, nroi, norm) in enumerate((((40, 50), 3, False), ((30, 70), 4, True), ((1, 999), 1, False))):
        pred, target, mask, ps, min_v, max_v = ref.synthetic_case(shape, nroi, seed=seed, normalised=norm)
        mask = (rng.random(shape) < 0.8).astype(np.uint8)
        table, maps = _host_check(tmp_path, pred, target, mask, ps, min_v, max_v)
        want_t, want_m = ref.error_table(pred, target, mask, ps, min_v, max_v)
        _assert_close(maps[:6], want_m[:6], 0, what="components")
        _assert_close(maps[6:10], want_m[6:10], 1e-9, 1e-12, what="md fa ad rd")   # eigen-accuracy / |t|
        _assert_close(maps[10:], want_m[10:], 0, 1e-9, what="angles")
        _assert_close(table, want_t, 1e-11, what="table")


def test_library_rejects_bad_arguments_without_gpu():
    from unet_bssfp_amd import _lib
    lib = _lib.load()
    assert lib.mi355_dti_errors_workspace_bytes(0, 3) == 39 * 8
    assert lib.mi355_dti_errors_workspace_bytes(1 << 30, 3) == 2048 * 39 * 8
    assert lib.mi355_dti_errors_workspace_bytes(100, 5) == -1
    ws = ctypes.create_string_buffer(64)
    rc = lib.mi355_dti_errors(1, 1, 0, 1, 6, 1, 1, 0, 1, 5, 10, 5, 1.0, 0.0, ctypes.addressof(ws), 64, 1, None, None)
    assert rc < 0 and b"tissue maps" in lib.mi355_last_error()
    rc = lib.mi355_dti_errors(1, 1, 1, 1, 6, 1, 1, 0, 1, 3, 10, 3, 1.0, 0.0, ctypes.addressof(ws), 64, 1, None, None)
    assert rc < 0 and b"dtype" in lib.mi355_last_error()
    rc = lib.mi355_dti_errors(1, 1, 0, 1, 6, 1, 1, 0, 1, 3, 10, 3, 1.0, 0.0, ctypes.addressof(ws), 8, 1, None, None)
    assert rc < 0 and b"workspace" in lib.mi355_last_error()


def test_error_rows_and_csv_without_gpu(tmp_path):
    from unet_bssfp_amd import eval as E, _lib
    assert E.ERROR_COLUMNS == ref.COLUMNS
    table = torch.arange(36, dtype=torch.float64).reshape(3, 12) / 7
    table[1, 3] = float("nan")
    rows = E.error_rows(table, "bssfp", "p1", "01", "1")
    assert [r["roi"] for r in rows] == ["CSF", "GM", "WM"] and rows[2]["fa"] == 31 / 7
    path = tmp_path / "errors.csv"
    E.write_error_csv(rows, str(path))
    with open(path) as fh:
        back = list(csv.DictReader(fh))
    assert list(back[0]) == ["modality", "pred_id", "sub", "ses", "roi", *E.ERROR_COLUMNS]
    assert float(back[2]["fa"]) == 31 / 7 and back[1]["dyy"] == "nan" and back[0]["sub"] == "01"
    with pytest.raises(ValueError):
        E.error_rows(table[:2], "bssfp", "p1", "01", "1")
    x = torch.zeros(2, 2, 2, 6)
    with pytest.raises(_lib.Mi355Error):                                          # no CPU fallback
        E.error_table(x, x, torch.ones(2, 2, 2), torch.ones(2, 2, 2, 3))


# ------------------------------------------------------------------------------------------------ GPU

def _cf(a):
    """(..., k) -> (k, ...)"""
    return np.ascontiguousarray(np.moveaxis(a, -1, 0))


def _run(pred, target, mask, ps, min_v, max_v, dtype, channels_first, ps_dtype=None):
    from unet_bssfp_amd import eval as E
    ps_dtype = ps_dtype or dtype
    if channels_first:
        pred, target, ps = _cf(pred), _cf(target), _cf(ps)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)   # noqa: E731
    table, maps = E.error_table(t(pred, dtype), t(target, dtype), torch.from_numpy(np.ascontiguousarray(mask)).cuda(),
                                t(ps, ps_dtype), min_v, max_v, channels_first=channels_first, return_maps=True)
    assert table.dtype == torch.float64 and all(m.dtype == dtype for m in maps.values())
    return table.cpu().numpy(), np.stack([maps[k].double().cpu().numpy() for k in E.ERROR_COLUMNS])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("channels_first", [False, True])
def test_gpu_matches_reference_golden(case, dtype, channels_first):
    g = np.load(GOLD)
    pred, target, mask, ps, min_v, max_v = _case(g, case)
    table, maps = _run(pred, target, mask, ps, min_v, max_v, dtype, channels_first, ps_dtype=torch.float32)
    _assert_close(table, g[f"{case}_table"], 1e-11, what="table")
    if dtype == torch.float64:
        _assert_close(maps[:6], g[f"{case}_maps"][:6], 0, what="components")
        _assert_close(maps[6:], g[f"{case}_maps"][6:], 1e-11, 1e-11, what="maps")
    else:
        _assert_close(maps, g[f"{case}_maps"].astype(np.float32), 1e-6, 1e-6, what="f32 maps")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 257), (64, 64, 64)])
@pytest.mark.parametrize("nroi,normalised", [(1, False), (3, True), (4, False), (4, True)])
def test_gpu_matches_oracle(shape, nroi, normalised):
    pred, target, mask, ps, min_v, max_v = ref.synthetic_case(shape, nroi, seed=sum(shape) + nroi, normalised=normalised)
    want_t, want_m = ref.error_table(pred, target, mask, ps, min_v, max_v)
    table, maps = _run(pred, target, mask, ps.astype(np.float64), min_v, max_v, torch.float64, False)
    _assert_close(maps[:6], want_m[:6], 0, what="components")
    _assert_close(maps[6:10], want_m[6:10], 1e-9, 1e-12, what="md fa ad rd")   # eigen-accuracy / |t|
    _assert_close(maps[10:], want_m[10:], 0, 1e-9, what="angles")
    _assert_close(table, want_t, 1e-11, what="table")
    t32, _ = _run(pred, target, mask, ps, min_v, max_v, torch.float32, True)        # f32 inputs are these values
    _assert_close(t32, want_t, 1e-11, what="f32 channels-first table")


@pytest.mark.gpu
def test_gpu_deterministic_and_maps_do_not_change_the_table():
    from unet_bssfp_amd import eval as E
    pred, target, mask, ps, min_v, max_v = ref.synthetic_case((48, 40, 36), 3, seed=3, normalised=True)
    args = [torch.from_numpy(a).cuda() for a in (pred, target, mask, ps)]
    a = E.error_table(*args, min_v=min_v, max_v=max_v)
    b = E.error_table(*args, min_v=min_v, max_v=max_v)
    c, maps = E.error_table(*args, min_v=min_v, max_v=max_v, return_maps=True)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert set(maps) == set(E.ERROR_COLUMNS) and maps["fa"].shape == (48, 40, 36)
    fmask = torch.from_numpy(mask.astype(np.float32) * 1.5).cuda()                  # float mask: uint8 truncation
    assert torch.equal(E.error_table(args[0], args[1], fmask, args[3], min_v=min_v, max_v=max_v), a)
    empty = E.error_table(torch.zeros(0, 6, device="cuda"), torch.zeros(0, 6, device="cuda"),
                          torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(0, 3, device="cuda"))
    assert empty.shape == (3, 12) and torch.isnan(empty).all()


@pytest.mark.gpu
def test_gpu_evaluate_subject_is_predict_volume_then_error_table():
    from unet_bssfp_amd import eval as E, nn as N
    from unet_bssfp_amd.inference import predict_volume
    torch.manual_seed(0)
    gen = N.Generator("bssfp").cuda().eval()
    g = torch.Generator().manual_seed(4)
    x = torch.rand(24, 32, 32, 48, generator=g).cuda()
    target = torch.rand(6, 32, 32, 48, generator=g).cuda()
    mask = (torch.rand(32, 32, 48, generator=g) < 0.7).to(torch.uint8).cuda()
    ps = torch.rand(3, 32, 32, 48, generator=g).cuda()
    got = E.evaluate_subject(gen, x, target, mask, ps, patch_size=32, batch_size=2, min_v=-1e-3, max_v=3e-3)
    with torch.no_grad():
        pred = predict_volume(gen, x, 32, 0, 2, "crop")
    want = E.error_table(pred, target, mask, ps, -1e-3, 3e-3, channels_first=True)
    assert got.shape == (3, 12) and torch.equal(got.isnan(), want.isnan())
    assert torch.equal(got.nan_to_num(), want.nan_to_num())


@pytest.mark.gpu
def test_gpu_host_errors():
    from unet_bssfp_amd import eval as E, _lib
    t = torch.rand(4, 5, 6, 6, device="cuda", dtype=torch.float64)
    m = torch.ones(4, 5, 6, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.Mi355Error, match="tissue maps"):
        E.error_table(t, t, m, torch.rand(4, 5, 6, 5, device="cuda"))
    with pytest.raises(ValueError):
        E.error_table(t, t, m[:3], torch.rand(4, 5, 6, 3, device="cuda"))
    with pytest.raises(ValueError):
        E.error_table(t, t, m, torch.rand(4, 5, 6, 3, device="cuda"), channels_first=True)
    with pytest.raises(_lib.Mi355Error):
        E.error_table(t, t.cpu(), m, torch.rand(4, 5, 6, 3, device="cuda"))
    with pytest.raises(_lib.Mi355Error):
        E.error_table(t.half(), t.half(), m, torch.rand(4, 5, 6, 3, device="cuda"))
    with pytest.raises(_lib.Mi355Error):
        E.error_table(t, t.float(), m, torch.rand(4, 5, 6, 3, device="cuda"))
    with pytest.raises(ValueError):
        E.error_table(t, t, m, torch.rand(4, 5, 6, 3, device="cuda"), min_v=0.0)
