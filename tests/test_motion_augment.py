"""The rigid trilinear resampler and RandomMotion on the device (csrc/motion.hip, unet_bssfp_amd.augment) against the f64
restatement of tests/motion_ref.py, and the patch queue that stages the seven-stage transform (unet_bssfp_amd.data), bit
for bit against the chained path.  Every bound is derived from the f32 format, none is fitted: u = 2^-24,
gamma_n = n u / (1 - n u) bounds an n-term chain of roundings.

Resampler.  The device computes a source coordinate with three fmas in f32 from the integer output index, the
restatement in f64 from the same (or, for the whole stage, the unrounded) matrix:
    e_a <= gamma_4 (sum_b |m_ab| i_b + |t_a|)                     coordinate error along axis a, in voxels
    value error <= sum_a e_a (max - min of the channel) + 9 u max|x|
(trilinear interpolation is 1-Lipschitz per axis in units of neighbour differences; three nested lerps, each a
subtraction (u |b - a| <= 2 u max|x|) and an fma (u max|x|), 3 u max|x| per level).  A voxel whose f64 source coordinate
lies within e_a of the inside / outside surface may flip to or from the fill value and is left out; the share of such
voxels is capped (1e-4 of the voxels, 5e-3 of the lines along W of the whole stage: two orders of magnitude above what
the f64 reading alone leaves out for draws from the reference's ranges, 1.3e-6 and 4.1e-4), and the cap is a condition
that is asserted, so that an input which maps a whole voxel plane onto the surface fails loudly.  TorchIO is absent: parity with TorchIO itself stays unpinned."""
import gc

import numpy as np
import pytest
import torch

import motion_ref as R
from unet_bssfp_amd import augment as A
from unet_bssfp_amd import data as Q

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
BIG = (96, 128, 128)


def gamma(n):
    return n * U / (1 - n * U)


def _ulp(ref):
    return np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def _draw(seed, degrees=10, translation=10, k=2):
    torch.manual_seed(seed)
    return A.RandomMotion(degrees=degrees, translation=translation, num_transforms=k).sample()


def _volume(c, shape, lo, seed):
    return torch.rand((c,) + tuple(shape), generator=torch.Generator().manual_seed(seed)) + lo


def _coordinate_bound(m, shape):
    """e_a per output voxel, (3, D, H, W)"""
    m = np.abs(np.asarray(m, dtype=np.float64))
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"))
    return gamma(4) * (np.tensordot(m[:3, :3], grid, axes=([1], [0])) + m[:3, 3][:, None, None, None])


def _left_out(m, shape, e):
    """voxels whose inside / outside status the coordinate error can change: neither surely inside nor surely outside"""
    s = R.source_coordinates(m, shape)
    n = np.array(shape, dtype=np.float64)[:, None, None, None]
    surely_in = ((s >= -0.5 + e) & (s < n - 0.5 - e)).all(0)
    surely_out = ((s < -0.5 - e) | (s >= n - 0.5 + e)).any(0)
    outside = ~((s >= -0.5) & (s < n - 0.5)).all(0)
    return ~(surely_in | surely_out), outside


def _value_bound(x64, e):
    """(C, D, H, W): sum_a e_a (max - min of the channel) + 9 u max|x|"""
    rng = (x64.max(axis=(1, 2, 3)) - x64.min(axis=(1, 2, 3)))[:, None, None, None]
    return e.sum(0)[None] * rng + 9 * U * np.abs(x64).max(axis=(1, 2, 3))[:, None, None, None]


def _pick_small_draw(shape, start, k=2):
    """a draw, scaled to a small volume, for which the f64 reading alone leaves no voxel out"""
    for seed in range(start, start + 50):
        p = _draw(seed, degrees=10, translation=1.5, k=k)
        ms = A.motion_matrices(p.degrees, p.translation, shape).astype(np.float32).astype(np.float64)
        if not any(_left_out(m, shape, _coordinate_bound(m, shape))[0].any() for m in ms):
            return p
    raise AssertionError("no draw without a voxel on the surface among 50")


CASES = [(24, BIG, 0.0), (6, BIG, -0.4), (6, (9, 11, 13), 0.0), (24, (7, 13, 11), -0.4)]


# ---- the resampler ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c,shape,lo", CASES)
def test_rigid_resample_against_the_restatement(hip, c, shape, lo):
    big = shape == BIG
    x = _volume(c, shape, lo, seed=c + shape[0])
    xd, x64 = x.to(DEV), x.double().numpy()
    p = _draw(3 + c) if big else _pick_small_draw(shape, 40 + c)
    ms = A.motion_matrices(p.degrees, p.translation, shape)
    for k, m in enumerate(ms):
        m32 = m.astype(np.float32).astype(np.float64)                 # the SAME f32-rounded matrix on both sides
        got = A.rigid_resample(xd, m).cpu().double().numpy()
        want = R.resample(x64, m32)
        e = _coordinate_bound(m32, shape)
        skip, outside = _left_out(m32, shape, e)
        share, out_share = skip.mean(), outside.mean()
        ratio = np.abs(got - want) / (_value_bound(x64, e) + _ulp(want))
        worst = float(ratio[:, ~skip].max())
        print(f"rigid_resample C={c} {shape} image {k}: max e_a {e.max():.3g} voxel, left out {share:.3g}, outside "
              f"{out_share:.3g}, worst err / bound = {worst:.3f}")
        if big:
            assert share <= 1e-4, share
            assert out_share > 0.01                                   # the fill path is exercised
        else:
            assert not skip.any()
        assert worst <= 1.0
        # outside voxels hold the channel minimum exactly
        sure = outside & ~skip
        assert np.array_equal(got[:, sure], np.broadcast_to(x64.min(axis=(1, 2, 3))[:, None], (c, int(sure.sum()))))
    # a given fill value instead of the channel minimum; the identity is exact
    got = A.rigid_resample(xd, ms[1], fill=-7.5).cpu().double().numpy()
    want = R.resample(x64, ms[1].astype(np.float32).astype(np.float64), fill=-7.5)
    e = _coordinate_bound(ms[1], shape)
    skip, outside = _left_out(ms[1].astype(np.float32).astype(np.float64), shape, e)
    assert (got[:, outside & ~skip] == -7.5).all()
    assert (np.abs(got - want) <= _value_bound(x64, e) + _ulp(want))[:, ~skip].all()
    assert torch.equal(A.rigid_resample(xd, np.eye(4)), xd)


# ---- the stage ---------------------------------------------------------------------------------------------------------------

def _stage_reference(x64, p):
    """(want, bound, lines left out) of RandomMotion.apply from the f64 reading: the resample bound carried through the
    band sum, sum_k sum_j |C_k[i][j]| bound_kj + gamma_{(K+1) N} sum_k sum_j |C_k[i][j] x_k[j]| + ulp"""
    shape = x64.shape[1:]
    n, k = shape[2], len(p.times)
    ms = R.matrices(p.degrees, p.translation, shape)
    images = [R.resample(x64, m) for m in ms]                         # motion_ref.motion, with the moved copies kept
    want = np.stack([R.composite([im[ch] for im in images], p.times) for ch in range(x64.shape[0])])
    bound = np.zeros_like(x64)
    skip = np.zeros(shape[:2], dtype=bool)
    for image, first, last in R.band_limits(p.times, n):               # the restatement's own bands, not the package's
        if last <= first:
            continue                                                  # an empty band contributes nothing
        cabs = R.band_response(n, first, last)
        e = _coordinate_bound(ms[image], shape)
        bound += np.einsum("ij,cdhj->cdhi", cabs, _value_bound(x64, e) + gamma((k + 1) * n) * np.abs(images[image]))
        skip |= _left_out(ms[image], shape, e)[0].any(2)
    return want, bound + _ulp(want), skip


@pytest.mark.parametrize("c,shape,lo", CASES)
def test_motion_apply_against_the_restatement_and_the_chained_form(hip, c, shape, lo):
    big = shape == BIG
    x = _volume(c, shape, lo, seed=2 * c + shape[1])
    xd, x64 = x.to(DEV), x.double().numpy()
    mo = A.RandomMotion()
    p = _draw(5 + c) if big else _pick_small_draw(shape, 60 + c)
    got = mo.apply(xd, p)
    want, bound, skip = _stage_reference(x64, p)
    share = skip.mean()
    ratio = np.abs(got.cpu().double().numpy() - want) / bound
    worst = float(ratio[:, ~skip].max())
    print(f"motion C={c} {shape}: lines left out {share:.3g}, worst err / bound = {worst:.3f}, "
          f"changed by {np.abs(want - x64).max():.3g}, minimum {want.min():.3g}")
    if big:
        assert share <= 5e-3, share
    else:
        assert not skip.any()
    assert worst <= 1.0
    assert np.abs(want - x64).max() > 0.05                            # the artefact is not the identity
    # fused against chained: inside the sum of both bounds.  The chained form's own bound is no larger than the fused one's:
    # per image (gamma_N + u) sum|C x| for the pass, then K roundings of partial sums no larger than sum_k sum|C_k x_k|,
    # and N + 1 + K <= (K + 1) N
    chained = mo.apply_chained(xd, p).cpu().double().numpy()
    assert (np.abs(chained - want) <= bound)[:, ~skip].all()
    assert (np.abs(chained - got.cpu().double().numpy()) <= 2 * bound)[:, ~skip].all()
    assert mo.apply(xd, tuple(p)).equal(got)                          # a plain tuple is accepted; the launch is deterministic


def test_motion_identity_image_counts_and_extent_limits(hip):
    from unet_bssfp_amd import _lib
    x = torch.rand(3, 6, 9, 12, device=DEV)
    mo = A.RandomMotion()
    for k in (1, 2, 7):
        z = np.zeros((k, 3), np.float32)
        assert mo.apply(x, A.MotionParams(_draw(k, k=k).times, z, z)) is x
    for k in (1, 7):                                                  # the smallest and the largest image count
        p = _pick_small_draw(tuple(x.shape[1:]), 20 + k, k=k)
        got = mo.apply(x, p).cpu().double().numpy()
        want, bound, skip = _stage_reference(x.cpu().double().numpy(), p)
        assert not skip.any() and (np.abs(got - want) <= bound).all()
    with pytest.raises(_lib.Mi355Error, match="exceed"):
        mo.apply(x, _draw(1, k=8))
    with pytest.raises(_lib.Mi355Error, match="exceeds 128"):
        mo.apply(torch.zeros(1, 2, 2, 160, device=DEV), _draw(1))
    rows = np.zeros(12 * 9, np.float32)
    rc = hip.mi355_aug_motion(x.data_ptr(), x.data_ptr() + 4096, *x.shape, 9, rows.ctypes.data, x.data_ptr(), x.data_ptr(), None)
    assert rc == -2 and b"exceed 8" in hip.mi355_last_error()
    y = mo(x)                                                         # sample + apply, and the subject-dict form
    assert y.shape == x.shape and not torch.equal(y, x)
    torch.manual_seed(5)
    d = mo({"a": {"data": x}, "b": {"data": x}, "other": 3})
    assert not torch.equal(d["a"]["data"], d["b"]["data"]) and d["other"] == 3       # one parameter set per image
    torch.manual_seed(5)
    assert torch.rand(1).item() < 1.0
    assert torch.equal(mo.apply(x, mo.sample()), d["a"]["data"]) and torch.equal(mo.apply(x, mo.sample()), d["b"]["data"])
    assert A.RandomMotion(p=0.0)(x) is x


# ---- the patch queue ------------------------------------------------------------------------------------------------------

def _subjects(n, extents, seed=0, lo=-0.3):
    g = torch.Generator().manual_seed(seed)
    return [{"bssfp": {"data": (torch.rand((24,) + tuple(extents[i % len(extents)]), generator=g) + lo).to(DEV)},
             "dwi-tensor": {"data": (torch.rand((6,) + tuple(extents[i % len(extents)]), generator=g) + lo).to(DEV)}}
            for i in range(n)]


def _chained(q, plan, name, augmented):
    """extract_patches(chain(crop_or_pad(raw))) patch by patch, with the augmentation objects and the recorded parameters"""
    from unet_bssfp_amd.inference import extract_patches
    out = []
    for p in plan:
        x = A.crop_or_pad(q._by_index[p.load.subject][name]["data"], q.target_shape, q.padding_value)
        if augmented:
            for t, params in p.load.stages:
                x = t.apply(x, params[name] if isinstance(t, A.RandomMotion) else params)
        loc = np.array([list(p.origin) + [o + s for o, s in zip(p.origin, q.patch_size)]])
        out.append(extract_patches(x, loc, q.patch_size))
    return torch.cat(out)


def _check_batch(q, plan, batch, augmented_target):
    assert torch.equal(batch["bssfp"]["data"], _chained(q, plan, "bssfp", True))
    assert torch.equal(batch["dwi-tensor_orig"]["data"], _chained(q, plan, "dwi-tensor", False))
    assert ("dwi-tensor" in batch) == augmented_target
    if augmented_target:
        assert torch.equal(batch["dwi-tensor"]["data"], _chained(q, plan, "dwi-tensor", True))


def _forced(p=1.0):
    tr = A.reference_full_transform()
    for t in tr:
        t.p = p
    tr[4].std_range = (0.5, 1.5)                                      # a blur that does blur
    return tr


@pytest.mark.parametrize("patch", [(8, 12, 16), (8, 12, 13)])        # the two kernels of the gather: 16-byte rows or not
@pytest.mark.parametrize("augmented_target", [True, False])
def test_queue_with_seven_forced_stages_equals_the_chained_path(hip, patch, augmented_target):
    target = (20, 24, 32)
    extents = [(23, 19, 32), (20, 24, 32), (17, 27, 37)]               # crop D + pad H; the target; pad D + crop H, W
    subs = _subjects(5, extents, seed=8)

    def queue():
        return Q.PatchQueue(subs, "bssfp", max_length=4, samples_per_volume=2, sampler=Q.UniformSampler(patch),
                            target_shape=target, transform=_forced(), seed=13)
    q, twin = queue(), queue()
    _check_batch(q, twin.next_plan(2), q.next_batch(2, augmented_target=augmented_target), augmented_target)
    for bs in (3, 6, 5):                                              # fills of 4 patches: every batch straddles fills
        batch = q.next_batch(bs, augmented_target=augmented_target)
        plan = twin.next_plan(bs)
        assert len({p.load.fill for p in plan}) > 1
        for p in plan:
            staged, fused = Q.PatchQueue.split_stages(p.load)
            assert [type(t) for t, _ in staged] == [A.RandomMotion, A.RandomGhosting, A.RandomSpike, A.RandomBiasField, A.RandomBlur]
            assert [type(t) for t, _ in fused] == [A.RandomNoise, A.RandomGamma]
            assert [pp.path for t, pp in staged if isinstance(t, A.RandomSpike)] == ["dft"]
        _check_batch(q, plan, batch, augmented_target)
    assert all(set(e[1]) == ({"bssfp", "dwi-tensor"} if augmented_target else {"bssfp"}) for e in q._staged.values())


def test_queue_with_motion_only_stages_each_image_with_its_own_set(hip):
    target, patch = (20, 24, 32), (8, 12, 16)
    subs = _subjects(3, [(23, 19, 32), (20, 24, 32)], seed=9, lo=0.0)
    q = Q.PatchQueue(subs, "bssfp", sampler=Q.UniformSampler(patch), target_shape=target, transform=[A.RandomMotion()], seed=1)
    plan = q.next_plan(8)
    batch = q.gather(plan, augmented_target=True)
    _check_batch(q, plan, batch, True)
    assert float(batch["bssfp"]["data"].min()) < 0 <= float(batch["dwi-tensor_orig"]["data"].min())   # motion is not sign-preserving


def test_seven_stage_queue_never_synchronises_and_releases_staging(hip):
    target, patch = (20, 24, 32), (8, 12, 16)
    extents = [(23, 19, 32), (20, 24, 32), (17, 27, 37)]
    subs = _subjects(8, extents, seed=6)

    def queue(p):
        return Q.PatchQueue(subs, "bssfp", max_length=4, samples_per_volume=2, sampler=Q.UniformSampler(patch),
                            target_shape=target, transform=_forced(p), seed=21)
    q, twin = queue(0.5), queue(0.5)
    q.next_batch(2), twin.next_plan(2)                                # first use uploads the DFT matrices
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        batches = [(bs, q.next_batch(bs, augmented_target=True)) for bs in (3, 6, 5, 7)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    moved = 0
    for bs, batch in batches:
        plan = twin.next_plan(bs)
        moved += sum(any(isinstance(t, A.RandomMotion) for t, _ in Q.PatchQueue.split_stages(p.load)[0]) for p in plan)
        _check_batch(q, plan, batch, True)
    assert moved > 2
    q = queue(1.0)                                                    # every fill: 2 loads = one batch of 4

    def run(fills):
        while q.fill_count < fills:
            q.next_batch(4, augmented_target=True)
        while q._patches:
            q.next_batch(len(q._patches), augmented_target=True)
        gc.collect()
        torch.cuda.synchronize()
        return torch.cuda.memory_stats()["requested_bytes.all.current"]   # bytes the live tensors asked for (see 8.9)
    after4 = run(4)
    assert len(q._staged) <= 2
    assert run(40) == after4


def test_seven_stage_queue_feeds_a_graphed_training_step(hip):
    import unet_bssfp_amd as M
    from unet_bssfp_amd.functional import DropoutState
    from unet_bssfp_amd.gan import GraphedTrainingStep, bSSFPToDWITensorModel, synthetic_batch

    torch.manual_seed(4)
    DropoutState.reset()
    gen, discr = M.Generator("bssfp", dropout=0.05), M.Discriminator("bssfp")
    model = bSSFPToDWITensorModel("bssfp", gen=gen.to(DEV), discr=discr.to(DEV)).train()
    M.set_compute_dtype(model, M.compute_dtype_from_name("bf16"))
    subs = _subjects(3, [(96, 128, 128), (90, 120, 128)], seed=2, lo=0.0)

    def queue():
        tr = A.reference_full_transform()
        for t in tr:
            t.p = 0.5                                                 # the reference's stages, firing often enough to see
        return Q.PatchQueue(subs, "bssfp", transform=tr, seed=17)      # the reference's 96 x 128 x 128 target, 64^3 patches
    q, twin = queue(), queue()
    gs = GraphedTrainingStep(model, synthetic_batch(8, 64, seed=1, device=DEV), warmup=2)
    static = gs.instances[0][0]
    moved = 0
    for _ in range(4):
        q.next_batch(8, out=static)
        moved += sum(any(isinstance(t, A.RandomMotion) for t, _ in Q.PatchQueue.split_stages(l)[0]) for l, _ in q._staged.values())
        want = twin.next_batch(8)
        assert torch.equal(static["bssfp"]["data"], want["bssfp"]["data"])
        assert torch.equal(static["dwi-tensor_orig"]["data"], want["dwi-tensor_orig"]["data"])
        gs(0)
        logs = torch.stack([v.reshape(()).float() for v in model.last_logs.values()])
        assert torch.isfinite(logs).all()
    assert moved > 0
