"""Host mathematics of RandomMotion (unet_bssfp_amd.augment) against the literal f64 restatement of
tests/motion_ref.py, the host plan of a patch queue that carries the stage, and the resources of csrc/motion.hip from its
ISA.  No GPU needed.  TorchIO and SimpleITK are absent: these tests pin the project's reading, parity with TorchIO itself
is unpinned."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import motion_ref as R
from unet_bssfp_amd import augment as A
from unet_bssfp_amd import data as Q

EPS = np.finfo(np.float64).eps


def _moved_copies(shape, k, seed):
    """K + 1 arbitrary real volumes: the band identity holds for any real x_k, moved copies of one volume or not"""
    return list(np.random.default_rng(seed).random((k + 1,) + tuple(shape)))


def _times(k, kind, rng):
    step = 1.0 / (k + 1)
    t = (np.arange(1, k + 1) * step + rng.uniform(-0.3 * step, 0.3 * step, k)).astype(np.float32)
    if kind == "none_above_half":
        t = (t * 0.45).astype(np.float32)
    elif kind == "empty_band" and k > 1:
        t[1] = t[0]                                                   # two equal bin limits: the second image owns nothing
    return t


@pytest.mark.parametrize("shape", [(5, 6, 7), (6, 5, 8), (4, 7, 12), (3, 4, 33)])
def test_band_sum_equals_the_fft_composite(shape):
    n = shape[2]
    worst, imag = 0.0, 0.0
    for k in range(1, 5):
        for kind in ("plain", "none_above_half", "empty_band"):
            rng = np.random.default_rng(100 * k + len(kind))
            times = _times(k, kind, rng)
            images = _moved_copies(shape, k, k + n)
            want = R.composite(images, times, return_complex=True)
            bands = A.motion_bands(times, n)
            got = sum(np.tensordot(images[im], A.motion_band_matrix(n, first, last), axes=([2], [1])) for im, first, last in bands)
            # f64 rounding of an N-term product per image and of the 3-D transforms: a few ulp of the data range
            bound = 8 * n * EPS * max(np.abs(v).max() for v in images)
            worst = max(worst, np.abs(got - want.real).max() / bound)
            imag = max(imag, np.abs(want.imag).max())
            assert np.abs(got - want.real).max() <= bound, (k, kind)
            # the bands tile [0, N): the circulants sum to the identity
            total = sum(A.motion_band_matrix(n, first, last) for _, first, last in bands)
            assert np.abs(total - np.eye(n)).max() <= 4 * n * EPS
            assert sorted((f, l) for _, f, l in bands)[0][0] == 0 and max(l for _, _, l in bands) == n
            assert all(l > f for _, f, l in bands)
            if kind == "empty_band" and k > 1:
                assert len(bands) == k
            if kind == "none_above_half":
                assert bands[-1][0] == 0 and bands[-1][2] == n and not (times > 0.5).any()   # sort_spectra: image 0 <-> image K
    assert imag > 0.05                                                # real() discards something: not an approximation
    print(f"band identity {shape}: worst err / bound = {worst:.3g}, largest discarded imaginary part {imag:.3g}")


def test_motion_bands_apply_the_sort_spectra_swap():
    assert A.motion_bands(np.array([0.3, 0.7], np.float32), 10) == [(1, 0, 3), (0, 3, 7), (2, 7, 10)]
    assert A.motion_bands(np.array([0.6], np.float32), 9) == [(0, 0, 5), (1, 5, 9)]          # j = 0: no swap
    assert A.motion_bands(np.array([0.2, 0.4], np.float32), 10) == [(2, 0, 2), (1, 2, 4), (0, 4, 10)]
    assert A.motion_bands(np.array([0.25, 0.26, 0.8], np.float32), 8) == [(2, 0, 2), (0, 2, 6), (3, 6, 8)]
    c = A.motion_band_matrix(8, 2, 6)
    i = np.arange(8)
    assert c.dtype == np.float64 and np.array_equal(c, c[:, 0][(i[:, None] - i[None, :]) % 8])


CASES = [
    ("both", [[3.0, -7.5, 9.0], [-10.0, 4.0, 0.5]], [[2.0, -9.0, 5.5], [10.0, -0.25, 3.0]]),
    ("zero_rotation", [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], [[2.0, -9.0, 5.5], [10.0, -0.25, 3.0]]),
    ("zero_translation", [[3.0, -7.5, 9.0], [-10.0, 4.0, 0.5]], [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]),
    ("one_pure_translation", [[0.0, 0.0, 0.0]], [[1.0, 2.0, 3.0]]),
    ("tiny_rotation", [[1e-7, 0.0, -2e-7]], [[1.0, 2.0, 3.0]]),
    ("large", [[60.0, -45.0, 80.0], [20.0, 30.0, -70.0], [5.0, 5.0, 5.0]], [[30.0, -20.0, 10.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]),
]


@pytest.mark.parametrize("name,degrees,translation", CASES)
@pytest.mark.parametrize("shape", [(96, 128, 128), (9, 11, 13)])
def test_motion_matrices_equal_the_scipy_route(shape, name, degrees, translation):
    got = A.motion_matrices(degrees, translation, shape)
    want = R.matrices(degrees, translation, shape)
    k = len(degrees)
    assert got.shape == (k + 1, 4, 4) and got.dtype == np.float64
    # logm / expm of scipy are backward stable to a few hundred eps of the matrix norm; the entries reach |shape| (the
    # rotation about the centre shows in the translation column)
    scale = max(1.0, np.abs(want).max())
    assert np.abs(got - want).max() <= 2000 * EPS * scale, np.abs(got - want).max()
    assert np.array_equal(got[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (k + 1, 1)))
    for m in got:                                                     # rigid
        assert np.abs(m[:3, :3] @ m[:3, :3].T - np.eye(3)).max() <= 64 * EPS
    assert np.abs(got[1] - A.euler_index_matrix(degrees[0], translation[0], shape)).max() > 1e-3 or name == "tiny_rotation"
    assert np.abs(A.euler_index_matrix(degrees[0], translation[0], shape) - R.euler(degrees[0], translation[0], shape)).max() <= 64 * EPS * scale


def test_all_zero_parameters_give_identities_and_no_effect():
    for k in (1, 2, 4):
        z = np.zeros((k, 3))
        assert np.array_equal(A.motion_matrices(z, z, (5, 6, 7)), np.tile(np.eye(4), (k + 1, 1, 1)))
        assert not A.RandomMotion.has_effect(A.MotionParams(np.full(k, 0.5, np.float32), z, z))
    assert A.RandomMotion.has_effect(A.MotionParams(np.array([0.5], np.float32), np.zeros((1, 3)), np.array([[0, 1e-3, 0]])))
    assert A.RandomMotion.has_effect(A.MotionParams(np.array([0.5], np.float32), np.array([[0, 0, 1e-3]]), np.zeros((1, 3))))
    x = np.random.default_rng(0).random((2, 5, 6, 7))
    assert np.array_equal(R.motion(x, [0.4, 0.7], np.zeros((2, 3)), np.zeros((2, 3))), x)
    # and the restatement agrees that identical copies composite to the input
    assert np.abs(R.composite([x[0]] * 3, np.array([0.4, 0.7], np.float32)) - x[0]).max() <= 64 * EPS
    with pytest.raises(ValueError):
        A.motion_matrices([[0.0, 0.0, 180.0]], [[0.0, 0.0, 0.0]], (5, 6, 7))


def test_resample_restatement_on_cases_with_a_known_answer():
    """pins the restatement itself (tests/motion_ref.py, the yardstick of the GPU tests), not the package: shifts and a
    quarter-voxel offset whose answers are known in closed form; the package's side of it, that the same matrices reach
    the device as their first three rows rounded to f32 once, is checked on ``_rigid_rows``"""
    shift34 = np.eye(4)[:3] + np.array([[0, 0, 0, 0.1], [0, 0, 0, 0], [0, 0, 0, 1.0]])
    rows = A._rigid_rows(np.vstack([shift34, [0, 0, 0, 1]]))
    assert rows.dtype == np.float32 and rows.shape == (12,) and np.array_equal(rows, A._rigid_rows(shift34))
    assert np.array_equal(rows.reshape(3, 4), shift34.astype(np.float32))
    with pytest.raises(ValueError):
        A._rigid_rows(np.eye(3))
    x = np.random.default_rng(1).random((2, 4, 5, 6)) - 0.3
    assert np.array_equal(R.resample(x, np.eye(4)), x)
    shift = np.eye(4)
    shift[2, 3] = 1.0                                                 # reads one voxel further along W
    y = R.resample(x, shift)
    assert np.array_equal(y[..., :5], x[..., 1:])
    assert np.array_equal(y[..., 5], np.broadcast_to(x.min(axis=(1, 2, 3))[:, None, None], (2, 4, 5)))   # s = 6 >= 5.5: fill
    half = np.eye(4)
    half[0, 3] = 0.25
    y = R.resample(x, half)
    assert np.abs(y[:, :3] - (0.75 * x[:, :3] + 0.25 * x[:, 1:])).max() <= 4 * EPS
    assert np.abs(y[:, 3] - x[:, 3]).max() <= 4 * EPS                 # 3.25 < 3.5: inside, both neighbours clamp to 3
    assert np.array_equal(R.resample(x, shift, fill=7.0)[..., 5], np.full((2, 4, 5), 7.0))


# ---- the stage object ---------------------------------------------------------------------------------------------------

def test_sample_replays_from_a_seed_in_the_documented_order():
    for k in (1, 2, 3, 7):
        mo = A.RandomMotion(degrees=(-4, 9), translation=6, num_transforms=k)
        torch.manual_seed(11 + k)
        got = mo.sample()
        torch.manual_seed(11 + k)
        degrees = torch.FloatTensor(k, 3).uniform_(-4, 9)
        translation = torch.FloatTensor(k, 3).uniform_(-6, 6)
        step = 1 / (k + 1)
        times = torch.arange(0, 1, step)[1:] + torch.FloatTensor(k).uniform_(-0.3 * step, 0.3 * step)
        assert isinstance(got, A.MotionParams)
        assert np.array_equal(got.degrees, degrees.numpy()) and np.array_equal(got.translation, translation.numpy())
        assert np.array_equal(got.times, times.numpy()) and got.times.dtype == np.float32 and got.times.shape == (k,)
        assert (np.diff(got.times) > 0).all() and got.times[0] > 0 and got.times[-1] < 1
        assert (got.degrees >= -4).all() and (got.degrees <= 9).all() and (np.abs(got.translation) <= 6).all()
        assert A.RandomMotion.has_effect(got)


def test_constructor_ranges_as_torchio_parses_them():
    mo = A.RandomMotion()
    assert mo.degrees_range == (-10.0, 10.0) and mo.translation_range == (-10.0, 10.0)
    assert mo.num_transforms == 2 and mo.image_interpolation == "linear" and mo.p == 1.0 and mo.per_image
    mo = A.RandomMotion(degrees=(2, 5), translation=3, num_transforms=4, p=0.1)
    assert mo.degrees_range == (2.0, 5.0) and mo.translation_range == (-3.0, 3.0) and mo.num_transforms == 4 and mo.p == 0.1
    with pytest.raises(NotImplementedError):
        A.RandomMotion(image_interpolation="nearest")
    with pytest.raises(NotImplementedError):
        A.RandomMotion(image_interpolation="bspline")
    with pytest.raises(ValueError):
        A.RandomMotion(num_transforms=0)
    # ranges that could compose to a rotation near a half turn are refused here, not in the load that draws one
    for bad in (180, 56, (-60, 10), (0, 90)):
        with pytest.raises(ValueError, match="half turn"):
            A.RandomMotion(degrees=bad)
    worst = A.RandomMotion(degrees=55)
    for signs in ((1, 1, 1), (1, -1, 1), (-1, -1, -1), (1, 1, -1)):               # the corners of the admitted range
        d = 55.0 * np.array([signs, signs])
        assert np.isfinite(A.motion_matrices(d, np.zeros((2, 3)), (9, 11, 13))).all()
    assert worst.degrees_range == (-55.0, 55.0)
    from unet_bssfp_amd import _lib
    with pytest.raises(_lib.Mi355Error):
        A.RandomMotion()(torch.zeros(1, 4, 4, 4))                     # GPU only, like the others
    with pytest.raises(_lib.Mi355Error):
        A.rigid_resample(torch.zeros(1, 4, 4, 4), np.eye(4))


def test_reference_full_transform_lists_the_seven():
    tr = A.reference_full_transform()
    assert [type(t) for t in tr] == [A.RandomMotion, A.RandomGhosting, A.RandomSpike, A.RandomBiasField, A.RandomBlur,
                                     A.RandomNoise, A.RandomGamma]
    assert all(t.p == 0.1 for t in tr)
    assert tr[0].degrees_range == (-10.0, 10.0) and tr[0].translation_range == (-10.0, 10.0) and tr[0].num_transforms == 2
    assert [type(t) for t in tr[1:]] == [type(t) for t in A.reference_training_transform()]
    assert tr[2].intensity_range == (0.01, 0.1) and tr[4].std_range == (0.01, 0.1) and tr[5].std_range == (0.01, 0.1)


# ---- host plan ----------------------------------------------------------------------------------------------------------

def _queue(n=4, lo=0.0, transform=None, **kw):
    g = torch.Generator().manual_seed(0)
    subs = [{"bssfp": {"data": torch.rand(24, 3, 3, 3, generator=g) + lo},
             "dwi-tensor": {"data": torch.rand(6, 3, 3, 3, generator=g) + lo}} for _ in range(n)]
    kw.setdefault("target_shape", (3, 3, 3))
    kw.setdefault("sampler", Q.UniformSampler(2))
    return Q.PatchQueue(subs, "bssfp", transform=transform, **kw)


def _seven(p):
    tr = A.reference_full_transform()
    for t in tr:
        t.p = p
    return tr


def test_queue_draws_one_motion_set_per_augmented_image_and_replays():
    q = _queue(2, transform=_seven(1.0), max_length=1, samples_per_volume=1)
    for pl in q.next_plan(12):
        assert [type(t) for t, _ in pl.load.stages] == [type(t) for t in q.transform]
        t, params = pl.load.stages[0]
        assert list(params) == ["bssfp", "dwi-tensor"] and all(isinstance(v, A.MotionParams) for v in params.values())
        assert not np.array_equal(params["bssfp"].degrees, params["dwi-tensor"].degrees)
        torch.manual_seed(pl.load.seed)                               # the chain: decision, then one set per image in order
        assert torch.rand(1).item() < 1.0
        for name in ("bssfp", "dwi-tensor"):
            want = t.sample()
            assert all(np.array_equal(a, b) for a, b in zip(params[name], want))
        # the spike that follows a fired motion cannot take the DC shortcut
        assert [p.path for s, p in pl.load.stages if isinstance(s, A.RandomSpike)] == ["dft"]
    q = _queue(2, transform=_seven(0.0), max_length=1, samples_per_volume=1)
    assert all(pl.load.stages == () for pl in q.next_plan(12))
    # a kept image that is the modality itself is not drawn twice
    q = _queue(2, transform=[A.RandomMotion()], keep={"bssfp": "bssfp_orig"})
    assert list(q.next_plan(1)[0].load.stages[0][1]) == ["bssfp"]


def test_the_plan_does_not_depend_on_augmented_target():
    """next_plan knows nothing of the flag: two queues of one seed, one gathered with and one without it, plan alike"""
    a, b = (_queue(3, transform=_seven(0.5), seed=9) for _ in range(2))
    assert "augmented_target" not in Q.PatchQueue.next_plan.__code__.co_varnames
    for _ in range(6):
        pa, pb = a.next_plan(5), b.next_plan(5)
        assert [(p.load.subject, p.load.seed, p.origin) for p in pa] == [(p.load.subject, p.load.seed, p.origin) for p in pb]
        for x, y in zip(pa, pb):
            for (t1, p1), (t2, p2) in zip(x.load.stages, y.load.stages):
                assert type(t1) is type(t2)
                if isinstance(t1, A.RandomMotion):
                    assert list(p1) == list(p2) == ["bssfp", "dwi-tensor"]
                    assert all(np.array_equal(u, v) for n in p1 for u, v in zip(p1[n], p2[n]))


def test_split_stages_stages_a_fired_motion_and_drops_an_all_zero_one():
    mo, gh, sp, bias, blur, noise, gamma = A.reference_full_transform()
    live = A.MotionParams(np.array([0.3, 0.7], np.float32), np.ones((2, 3)), np.zeros((2, 3)))
    dead = A.MotionParams(np.array([0.3, 0.7], np.float32), np.zeros((2, 3)), np.zeros((2, 3)))
    coef = np.zeros(20, np.float32)
    stages = ((mo, {"bssfp": live, "dwi-tensor": live}), (bias, coef), (gamma, 1.1))
    staged, fused = Q.PatchQueue.split_stages(Q.SubjectLoad(0, 0, 0, 0, stages))
    assert [t for t, _ in staged] == [mo] and [t for t, _ in fused] == [bias, gamma]
    stages = ((mo, {"bssfp": dead, "dwi-tensor": dead}), (bias, coef), (gamma, 1.1))
    staged, fused = Q.PatchQueue.split_stages(Q.SubjectLoad(0, 0, 0, 0, stages))
    assert staged == () and [t for t, _ in fused] == [bias, gamma]
    stages = ((mo, {"bssfp": dead, "dwi-tensor": live}), (gamma, 1.1))            # one image moves: the stage stays
    staged, fused = Q.PatchQueue.split_stages(Q.SubjectLoad(0, 0, 0, 0, stages))
    assert [t for t, _ in staged] == [mo] and [t for t, _ in fused] == [gamma]
    stages = ((bias, coef), (mo, {"bssfp": live, "dwi-tensor": live}), (gh, (5, 1, 0.7)), (noise, (0.0, 0.05, 1)))
    staged, fused = Q.PatchQueue.split_stages(Q.SubjectLoad(0, 0, 0, 0, stages))
    assert [t for t, _ in staged] == [bias, mo, gh] and [t for t, _ in fused] == [noise]


def test_what_motion_cannot_do_is_refused_at_construction():
    with pytest.raises(ValueError, match="exceeds 128"):
        _queue(2, transform=[A.RandomMotion()], target_shape=(3, 3, 160), sampler=Q.UniformSampler(2))
    with pytest.raises(ValueError, match="exceeds 128"):
        _queue(2, transform=A.reference_full_transform(), target_shape=(3, 3, 160), sampler=Q.UniformSampler(2))
    _queue(2, transform=[A.RandomMotion()], target_shape=(160, 160, 128), sampler=Q.UniformSampler(2))   # only W is limited
    with pytest.raises(ValueError, match="transforms per image"):
        _queue(2, transform=[A.RandomMotion(num_transforms=8)])
    _queue(2, transform=[A.RandomMotion(num_transforms=7)])
    with pytest.raises(TypeError):
        _queue(2, transform=[A.RandomMotion(), A.RandomMotion()])
    with pytest.raises(TypeError, match="RandomMotion"):
        _queue(2, transform=[object()])
    assert [type(t) for t in _queue(2).transform] == [A.RandomBiasField, A.RandomNoise, A.RandomGamma]   # the default stays


def test_seven_stages_fire_at_rate_p():
    q = _queue(2, transform=A.reference_full_transform(), max_length=1, samples_per_volume=1, seed=3)
    loads = [pl.load for pl in q.next_plan(3000)]
    tol = 4.5 * np.sqrt(0.1 * 0.9 / 3000)
    for t in q.transform:
        rate = np.mean([any(s[0] is t for s in l.stages) for l in loads])
        assert abs(rate - 0.1) < tol, (type(t).__name__, rate)


# ---- the kernels' resources ----------------------------------------------------------------------------------------------

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unet_bssfp_amd", "csrc")


def test_motion_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """every shipped instantiation of csrc/motion.hip: 0 bytes of scratch, no spilled register, at most 64 KB of LDS"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "motion.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-Wno-unused-function",
                    "-Wno-unused-variable", os.path.join(CSRC, "motion.hip"), "-o", str(out)], check=True, capture_output=True)
    isa = out.read_text()
    names = re.findall(r"\.name:\s+(\S*kernel\S*)", isa)
    assert sum("resample_kernel" in n for n in names) == 2 and sum("motion_kernel" in n for n in names) == 1
    scratch = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", isa)]
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", isa)]
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", isa)]
    assert len(scratch) == len(names) == 3 and set(scratch) == {0} and set(spills) == {0}
    assert max(lds) <= 65536
    body = "\n".join(l for l in isa.splitlines() if not l.lstrip().startswith((".", ";", "//")))
    assert "atomic" not in body
    # the band sum reads its wave-uniform matrix rows through the scalar cache, as axis_apply_kernel does: per chunk of 8
    # rows 8 x s_load_dwordx4 (4 values of j each) feeding v_pk_fma_f32 from SGPRs, no wide vector load of a uniform
    # address, and no SGPR spilled to VGPR lanes (the row addresses are not kept across the image loop)
    sgpr_spills = [int(v) for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", isa)]
    assert len(sgpr_spills) == 3 and set(sgpr_spills) == {0}
    start = isa.index("motion_kernel")
    fused = isa[start:isa.index("s_endpgm", start)]
    assert fused.count("s_load_dwordx4") >= 32 and "v_pk_fma_f32" in fused
    assert "global_load_dwordx4" not in fused and "v_readlane" not in fused and "v_writelane" not in fused
    loops = re.split(r"^\.LBB\d+_\d+:", fused, flags=re.M)
    band = [b for b in loops if b.count("s_load_dwordx4") == 8]
    assert len(band) >= 4                                              # one vectorised j loop per chunk
    for b in band:
        assert b.count("v_pk_fma_f32") >= 16 and "global_load" not in b and "ds_read" in b


def test_motion_source_is_built_declared_and_bound():
    from unet_bssfp_amd import _lib
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bmotion\.hip\b", make, flags=re.M)
    header = open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "mi355_unet.h")).read()
    assert "#define MI355_MOTION_MAX_IMAGES 8" in header and A.MOTION_MAX_IMAGES == 8
    for name in ("mi355_rigid_resample", "mi355_aug_motion"):
        assert name in _lib.EXPORTED_SYMBOLS and re.search(rf"\b{name}\s*\(", header)
    lib = _lib.load()
    # argument validation happens on the host before any launch
    z = np.zeros(12 * 9, np.float32)
    assert lib.mi355_aug_motion(None, None, 1, 2, 2, 2, 1, None, None, None, None) == -1
    assert lib.mi355_aug_motion(1, 2, 1, 2, 2, 2, 9, z.ctypes.data, 3, 4, None) == -2 and b"exceed 8" in lib.mi355_last_error()
    assert lib.mi355_aug_motion(1, 2, 1, 2, 2, 160, 2, z.ctypes.data, 3, 4, None) == -2 and b"exceeds 128" in lib.mi355_last_error()
    z[5] = np.nan
    assert lib.mi355_rigid_resample(1, 2, 1, 2, 2, 2, z.ctypes.data, None, 0.0, None) == -1
    assert b"not finite" in lib.mi355_last_error()
    assert lib.mi355_rigid_resample(1, 1, 1, 2, 2, 2, z.ctypes.data, None, 0.0, None) == -1      # in place
