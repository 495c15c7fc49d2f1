"""RandomFlip and RandomAffine on the device (csrc/spatial.hip, unet_bssfp_amd.augment.affine_resample) and in the patch
queue (unet_bssfp_amd.data), DESIGN.md 8.17.  Flips and the identity are pinned bit for bit; an affine is compared with the
f64 restatement of tests/spatial_ref.py on the SAME f32-rounded matrix under the bound that tests/test_motion_augment.py
derives for the resampler, which is general in |m_ab| (u = 2^-24, gamma_n = n u / (1 - n u)):
    e_a <= gamma_4 (sum_b |m_ab| i_b + |t_a|)                    coordinate error along axis a, in voxels
    value error <= sum_a e_a (max - min of the channel) + 9 u max|x|
(the channel being the cropped / padded volume, padding included).  Draws are picked so that the f64 reading leaves NO
voxel within e_a of the inside / outside surface; that is a condition and it is asserted.  A tensor image adds, for
component i of n' = T6 n + t6 (T6 and t6 rounded to f32 once, six fmas):
    sum_j |T6_ij| bound_j + gamma_7 sum_j |T6_ij| |n_j| + u |t6_i|
plus 1e-12 sum_j |n_j| for the distance between the package's f64 map and the restatement's rotation, which
tests/test_spatial_host.py pins.  The queue is compared bit for bit with the chained path
extract_patches(chain(affine_resample(crop_or_pad(raw)))).  TorchIO is absent: parity with it stays unpinned."""
import gc
import itertools

import numpy as np
import pytest
import torch

import spatial_ref as S
import test_motion_augment as TM
from alloc_poison import run_scenario
from unet_bssfp_amd import augment as A
from unet_bssfp_amd import data as Q

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
TARGET = (20, 24, 32)
EXTENTS = [(23, 19, 32), (20, 24, 32), (17, 27, 37)]                  # crop D + pad H; the target; pad D + crop H, W
VOLUMES = [(6, (9, 11, 13)), (24, (7, 13, 12))]
PATCHES = [(8, 12, 16), (8, 12, 13)]                                  # 16-byte rows or the per-voxel form
SUBSETS = [s for n in range(4) for s in itertools.combinations(range(3), n)]
RESCALE = np.array([[-0.5, 2.5], [-1.0, 1.0], [-1.5, 0.5], [0.0, 3.0], [-0.75, 1.25], [0.25, 2.0]])


def _volume(c, shape, lo, seed):
    return torch.rand((c,) + tuple(shape), generator=torch.Generator().manual_seed(seed)) + lo


def _draw_affine(seed, **kw):
    torch.manual_seed(seed)
    return A.RandomAffine(**{"scales": 0.1, "degrees": 10, "translation": 1.5, **kw}).sample()


def _rounded(m):
    return np.asarray(m, dtype=np.float64).astype(np.float32).astype(np.float64)


def pick_affine(shape, start, **kw):
    """a draw whose f64 reading leaves no voxel of ``shape`` on the inside / outside surface, as ``_pick_small_draw``
    picks one, and some voxel outside (the fill is exercised)"""
    for seed in range(start, start + 50):
        p = _draw_affine(seed, **kw)
        m = _rounded(A.affine_index_matrix(*p, shape))
        skip, outside = TM._left_out(m, shape, TM._coordinate_bound(m, shape))
        if not skip.any() and outside.any():
            return p
    raise AssertionError("no draw without a voxel on the surface among 50")


def _sample_bound(x64, m32, shape):
    """(bound (C, D, H, W), outside (D, H, W)) of a resample of the padded f64 volume; asserts the surface condition"""
    e = TM._coordinate_bound(m32, shape)
    skip, outside = TM._left_out(m32, shape, e)
    assert not skip.any()
    return TM._value_bound(x64, e), outside


def _tensor_map(m, rescale):
    """(|T6|, |t6|) from the restatement: the reorientation of the basis vectors"""
    rot = S.rotation_of(m)
    zero = S.reorient(np.zeros((6, 1)), rot, rescale)
    cols = S.reorient(np.eye(6), rot, rescale) - zero
    return np.abs(cols), np.abs(zero[:, 0])


def _tensor_bound(sampled, bound, m, rescale):
    t6, t = _tensor_map(m, rescale)
    mix = lambda v: np.einsum("ij,jdhw->idhw", t6, v)
    return mix(bound) + TM.gamma(7) * mix(np.abs(sampled)) + U * t[:, None, None, None] + 1e-12 * np.abs(sampled).sum(0)[None]


def _check_against_restatement(got, x64, m, fill, what, tensor=False, rescale=None):
    """``got`` against the f64 reading of the padded volume ``x64`` through the f32-rounded ``m``; -> share outside"""
    shape = x64.shape[1:]
    m32 = _rounded(m)
    want, sampled = S.spatial(x64, m32, fill, tensor, rescale, rotation_from=m)
    bound, outside = _sample_bound(x64, m32, shape)
    bound = bound + TM._ulp(sampled)
    if tensor:
        bound = np.where(outside[None], bound, _tensor_bound(sampled, bound, m, rescale))
    got = got.cpu().double().numpy()
    worst = float((np.abs(got - want) / bound).max())
    print(f"{what}: outside {outside.mean():.3g}, changed by {np.abs(want - x64).max():.3g}, worst err / bound = {worst:.3f}")
    assert worst <= 1.0
    fills = x64.min(axis=(1, 2, 3)) if fill is None else np.full(len(x64), fill)
    assert np.array_equal(got[:, outside], np.broadcast_to(fills[:, None], (len(x64), int(outside.sum()))))
    return outside.mean()


# ---- 1. identity and flips, bit for bit ---------------------------------------------------------------------------------

@pytest.mark.parametrize("c,shape", VOLUMES)
def test_identity_and_flips_are_exact(hip, c, shape):
    x = _volume(c, shape, -0.4, seed=c).to(DEV)
    assert torch.equal(A.affine_resample(x, np.eye(4)), x)
    assert torch.equal(A.affine_resample(x, np.eye(4), fill=-3.0), x)
    for axes in SUBSETS:
        want = torch.flip(x, [1 + a for a in axes]) if axes else x
        assert torch.equal(A.affine_resample(x, A.flip_index_matrix(axes, shape)), want), axes
        got = A.RandomFlip(axes=(0, 1, 2)).apply(x, axes)
        assert torch.equal(got, want) and (axes or got is x)
    assert A.RandomFlip(p=0.0)(x) is x
    torch.manual_seed(1)
    d = A.RandomFlip(axes=(0, 1, 2), flip_probability=1.0)({"a": {"data": x}, "b": {"data": x}, "other": 3})
    assert torch.equal(d["a"]["data"], torch.flip(x, [1, 2, 3])) and torch.equal(d["b"]["data"], d["a"]["data"]) and d["other"] == 3


def test_flips_of_a_tensor_image_carry_the_sign_pattern(hip):
    shape = VOLUMES[0][1]
    x = _volume(6, shape, -0.4, seed=3).to(DEV)
    for axes in SUBSETS:
        sigma = [-1.0 if a in axes else 1.0 for a in range(3)]
        signs = torch.tensor([sigma[a] * sigma[b] for a, b in A.TENSOR_COMPONENTS], device=DEV)[:, None, None, None]
        flipped = torch.flip(x, [1 + a for a in axes]) if axes else x
        got = A.affine_resample(x, A.flip_index_matrix(axes, shape), tensor_rescale=None)
        assert torch.equal(got, signs * flipped), axes
        assert torch.equal(A.affine_resample(x, A.flip_index_matrix(axes, shape)), flipped)        # no tensor image: no signs
    sub = {"t": {"data": x}, "s": {"data": x}}
    d = A.RandomFlip(axes=(1,), flip_probability=1.0)(sub, tensor_images={"t": None})
    assert torch.equal(d["s"]["data"], torch.flip(x, [2]))
    assert torch.equal(d["t"]["data"], torch.tensor([1.0, -1, 1, 1, -1, 1], device=DEV)[:, None, None, None] * torch.flip(x, [2]))
    with pytest.raises(ValueError, match="6 channels"):
        A.affine_resample(x[:5], np.eye(4), tensor_rescale=None)
    with pytest.raises(Exception, match="not finite"):
        A.affine_resample(x, np.full((4, 4), np.nan))


def _subjects(n, extents=EXTENTS, seed=0, lo=-0.3):
    g = torch.Generator().manual_seed(seed)
    return [{"bssfp": {"data": (torch.rand((24,) + tuple(extents[i % len(extents)]), generator=g) + lo).to(DEV)},
             "dwi-tensor": {"data": (torch.rand((6,) + tuple(extents[i % len(extents)]), generator=g) + lo).to(DEV)}}
            for i in range(n)]


def _plan(q, stage, params, origins):
    """one load per subject of the queue with ``stage`` fired with ``params``, and a patch of it at each origin"""
    loads = [Q.SubjectLoad(i, 0, 0, 0, (), ((stage, params),)) for i in q.indices]
    return [Q.PlannedPatch(load, o) for load in loads for o in origins]


def _slices(origin, patch):
    return (slice(None),) + tuple(slice(o, o + p) for o, p in zip(origin, patch))


@pytest.mark.parametrize("patch", PATCHES)
def test_flips_in_the_gather_read_the_cropped_and_padded_volume_exactly(hip, patch):
    subs = _subjects(3, seed=4)
    fl = A.RandomFlip(axes=(0, 1, 2))
    q = Q.PatchQueue(subs, "bssfp", sampler=Q.UniformSampler(patch), target_shape=TARGET, transform=[], spatial=[fl],
                     padding_value=0.25)
    origins = [(0, 0, 0), tuple(t - p for t, p in zip(TARGET, patch)), (5, 7, 9)]
    for axes in SUBSETS[1:]:
        plan = _plan(q, fl, axes, origins)
        batch = q.gather(plan, augmented_target=True)
        sigma = [-1.0 if a in axes else 1.0 for a in range(3)]
        signs = torch.tensor([sigma[a] * sigma[b] for a, b in A.TENSOR_COMPONENTS], device=DEV)[:, None, None, None]
        for b, p in enumerate(plan):
            raw = subs[p.load.subject]
            for name, src, sign in (("bssfp", "bssfp", 1.0), ("dwi-tensor_orig", "dwi-tensor", signs), ("dwi-tensor", "dwi-tensor", signs)):
                want = torch.flip(A.crop_or_pad(raw[src]["data"], TARGET, 0.25), [1 + a for a in axes])
                assert torch.equal(batch[name]["data"][b], (sign * want)[_slices(p.origin, patch)]), (axes, b, name)


# ---- 2. affine against the restatement -------------------------------------------------------------------------------------

@pytest.mark.parametrize("c,shape", VOLUMES)
def test_affine_resample_against_the_restatement(hip, c, shape):
    x = _volume(c, shape, -0.4, seed=2 * c)
    xd, x64 = x.to(DEV), x.double().numpy()
    p = pick_affine(shape, 10 + c)
    m = A.affine_index_matrix(*p, shape)
    assert _check_against_restatement(A.affine_resample(xd, m), x64, m, None, f"affine C={c} {shape} minimum") > 0
    _check_against_restatement(A.affine_resample(xd, m, fill=-7.5), x64, m, -7.5, f"affine C={c} {shape} fill -7.5")
    af = A.RandomAffine(default_pad_value=-7.5)
    assert torch.equal(af.apply(xd, p), A.affine_resample(xd, m, fill=-7.5))
    assert torch.equal(A.RandomAffine().apply(xd, p), A.affine_resample(xd, m))
    assert af.apply(xd, A.AffineParams(np.ones(3), np.zeros(3), np.zeros(3))) is xd
    # a flip and an affine composed: one resample through the product
    both = A.compose_index_matrices([A.flip_index_matrix((0, 2), shape), m])
    _check_against_restatement(A.affine_resample(xd, both), x64, both, None, f"flip . affine C={c} {shape}")


@pytest.mark.parametrize("patch", PATCHES)
def test_affine_in_the_gather_against_the_restatement_of_the_padded_volume(hip, patch):
    subs = _subjects(3, seed=5)
    p = pick_affine(TARGET, 30)
    m = A.affine_index_matrix(*p, TARGET)
    origins = [(0, 0, 0), tuple(t - q for t, q in zip(TARGET, patch)), (5, 7, 9)]
    for pad_value, fill in ((-0.5, "minimum"), (0.25, 1.5)):             # the padding is the minimum of a padded channel
        af = A.RandomAffine(default_pad_value=fill)
        q = Q.PatchQueue(subs, "bssfp", sampler=Q.UniformSampler(patch), target_shape=TARGET, transform=[], spatial=[af],
                         padding_value=pad_value, tensor_images={})
        plan = _plan(q, af, p, origins)
        batch = q.gather(plan)
        for i, sub in enumerate(subs):
            for name, src in (("bssfp", "bssfp"), ("dwi-tensor_orig", "dwi-tensor")):
                x64 = S.crop_or_pad(sub[src]["data"].cpu().double().numpy(), TARGET, pad_value)
                # the patches of the subject pasted into a volume of the restatement's own values
                want, _ = S.spatial(x64, _rounded(m), None if fill == "minimum" else fill)
                got = torch.from_numpy(want).float().to(DEV)
                for b, pl in enumerate(plan):
                    if pl.load.subject == i:
                        got[_slices(pl.origin, patch)] = batch[name]["data"][b]
                _check_against_restatement(got, x64, m, None if fill == "minimum" else fill,
                                           f"gather {name} raw {tuple(sub[src]['data'].shape[1:])} pad {pad_value}")


# ---- 3. the tensor image ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["rotation", "scale", "rescale"])
def test_tensor_image_against_the_restatement(hip, kind):
    shape = VOLUMES[0][1]
    x = _volume(6, shape, -0.4, seed=7)
    xd, x64 = x.to(DEV), x.double().numpy()
    if kind == "rotation":
        p = pick_affine(shape, 50, scales=0.0, degrees=25)
    else:
        p = pick_affine(shape, 60, scales=0.3, degrees=15)
    rescale = RESCALE if kind == "rescale" else None
    m = A.affine_index_matrix(*p, shape)
    t6, t = A.tensor_reorientation(m, rescale)
    assert np.abs(t6 - np.eye(6)).max() > 0.05 and (kind == "rescale") == bool(t.any())
    got = A.affine_resample(xd, m, tensor_rescale=rescale)
    assert _check_against_restatement(got, x64, m, None, f"tensor {kind}", tensor=True, rescale=rescale) > 0
    assert torch.equal(A.RandomAffine().apply(xd, p, tensor_rescale=rescale), got)
    plain = A.affine_resample(xd, m)
    assert not torch.equal(plain, got)


# ---- 4. the queue equals the chained path, bit for bit -------------------------------------------------------------------------

def _chained(q, plan, name, augmented):
    """extract_patches(chain(affine_resample(crop_or_pad(raw)))) patch by patch, from the recorded parameters"""
    from unet_bssfp_amd.inference import extract_patches
    out = []
    for p in plan:
        x = A.crop_or_pad(q._by_index[p.load.subject][name]["data"], q.target_shape, q.padding_value)
        live = [(t, params) for t, params in p.load.spatial if t.has_effect(params)]
        if live:
            m = S.chain([t.matrix(params, q.target_shape) for t, params in live])
            fills = [t.fill for t, _ in live if isinstance(t, A.RandomAffine)]
            x = A.affine_resample(x, m, fills[0] if fills else 0.0, q.tensor_images.get(name, A.NOT_A_TENSOR))
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


def _setup(mode):
    """(transform, spatial, tensor_images) of a queue"""
    if mode == "fused":                                               # spatial + local stages only: nothing is staged
        return ([A.RandomBiasField(), A.RandomNoise(std=(0.01, 0.1)), A.RandomGamma()],
                [A.RandomFlip(axes=(0, 1, 2), flip_probability=0.7), A.RandomAffine(translation=2)], None)
    tr = TM._forced(1.0 if mode == "staged" else 0.5)
    if mode == "staged":                                              # spatial + all seven stages
        return tr, [A.RandomAffine(translation=2, default_pad_value=-1.5), A.RandomFlip(axes=(0, 1, 2))], {"dwi-tensor": RESCALE}
    return tr, [A.RandomFlip(axes=(0, 2), p=0.5), A.RandomAffine(translation=2, p=0.5)], None       # mixed batches


@pytest.mark.parametrize("patch", PATCHES)
@pytest.mark.parametrize("augmented_target", [True, False])
@pytest.mark.parametrize("mode", ["fused", "staged", "mixed"])
def test_queue_with_spatial_stages_equals_the_chained_path(hip, mode, patch, augmented_target):
    subs = _subjects(7, seed=8)

    def queue():
        tr, sp, tensors = _setup(mode)
        return Q.PatchQueue(subs, "bssfp", max_length=4, samples_per_volume=2, sampler=Q.UniformSampler(patch),
                            target_shape=TARGET, transform=tr, spatial=sp, tensor_images=tensors, seed=13)
    q, twin = queue(), queue()
    moved = still = 0
    for bs in (2, 3, 6, 5, 12):                                       # fills of 4 patches: the later batches straddle fills
        batch = q.next_batch(bs, augmented_target=augmented_target)
        plan = twin.next_plan(bs)
        loads = {id(p.load): p.load for p in plan}
        if bs > 2:
            assert len({l.fill for l in loads.values()}) > 1
        if bs == 12:
            assert len(loads) > 4                                     # more loads than one launch takes: chunked
        for load in loads.values():
            staged, fused = Q.PatchQueue.split_stages(load)
            assert mode != "fused" or (not staged and len(fused) == 3)
            assert mode != "staged" or (len(staged) == 5 and len(fused) == 2)
            moved += twin.spatial_transform(load) is not None
            still += twin.spatial_transform(load) is None
        _check_batch(q, plan, batch, augmented_target)
    assert moved > 2 and (mode != "mixed" or still > 2)
    if mode == "fused":
        assert not q._staged
    if mode == "staged":
        assert all(set(e[1]) == ({"bssfp", "dwi-tensor"} if augmented_target else {"bssfp"}) for e in q._staged.values())


# ---- 5. ineffective stages change nothing ------------------------------------------------------------------------------------

@pytest.mark.parametrize("patch", PATCHES)
def test_stages_without_effect_change_nothing(hip, patch):
    subs = _subjects(4, seed=9)

    def queue(**kw):
        tr = A.reference_augmentation()
        for t in tr:
            t.p = 0.6
        return Q.PatchQueue(subs, "bssfp", max_length=4, samples_per_volume=2, sampler=Q.UniformSampler(patch),
                            target_shape=TARGET, transform=tr, seed=3, **kw)
    plain = queue()
    still = queue(spatial=[A.RandomFlip(axes=(0, 1, 2), flip_probability=0.0), A.RandomAffine(scales=0, degrees=0, translation=0)])
    for bs in (3, 6, 5):
        a, b = plain.next_batch(bs, augmented_target=True), still.next_batch(bs, augmented_target=True)
        assert sorted(a) == sorted(b)
        for name in ("bssfp", "dwi-tensor_orig", "dwi-tensor"):
            assert torch.equal(a[name]["data"], b[name]["data"])
        assert torch.equal(a["location"], b["location"])
    assert all(len(l.spatial) == 2 and still.spatial_transform(l) is None for l in still.last_fill)


# ---- 6. no synchronisation, no staging ---------------------------------------------------------------------------------------

def test_spatial_queue_never_synchronises_and_stages_nothing(hip):
    subs = _subjects(8, seed=6)

    def queue():
        tr, sp, _ = _setup("fused")
        return Q.PatchQueue(subs, "bssfp", max_length=4, samples_per_volume=2, sampler=Q.UniformSampler(PATCHES[0]),
                            target_shape=TARGET, transform=tr, spatial=sp, seed=21)
    q, twin = queue(), queue()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        batches = [(bs, q.next_batch(bs, augmented_target=True)) for bs in (3, 6, 5, 7)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for bs, batch in batches:
        _check_batch(q, twin.next_plan(bs), batch, True)
    assert not q._staged
    q = queue()

    def run(fills):
        while q.fill_count < fills:
            q.next_batch(4, augmented_target=True)
            assert not q._staged
        while q._patches:
            q.next_batch(len(q._patches), augmented_target=True)
        gc.collect()
        torch.cuda.synchronize()
        return torch.cuda.memory_stats()["requested_bytes.all.current"]
    after4 = run(4)
    assert run(40) == after4


# ---- every output voxel is written ---------------------------------------------------------------------------------------------

def test_results_do_not_depend_on_fresh_memory(hip):
    def scenario():
        torch.manual_seed(0)
        x = torch.rand(6, 9, 11, 13, generator=torch.Generator().manual_seed(1)).to(DEV)
        m = A.affine_index_matrix((1.1, 0.9, 1.05), (8, -5, 12), (1, 0.5, -1), x.shape[1:])
        out = {"affine": A.affine_resample(x, m), "tensor": A.affine_resample(x, m, fill=0.0, tensor_rescale=RESCALE)}
        tr, sp, _ = _setup("fused")
        q = Q.PatchQueue(_subjects(3, seed=2), "bssfp", sampler=Q.UniformSampler(PATCHES[1]), target_shape=TARGET,
                         transform=tr, spatial=sp, seed=1)
        batch = q.next_batch(6, augmented_target=True)
        out.update({name: v["data"] for name, v in batch.items() if isinstance(v, dict)})
        return out
    run_scenario(scenario, sync=torch.cuda.synchronize)
