"""Host side of the spatial stages of the patch feed (unet_bssfp_amd.augment, unet_bssfp_amd.data): the
index-space matrices and the tensor reorientation against the independent restatement of tests/spatial_ref.py, the plan of
a queue with spatial stages, and every refusal.  No GPU.  TorchIO is absent: parity with it stays unpinned."""
import numpy as np
import pytest
import torch

import spatial_ref as S
from unet_bssfp_amd import augment as A
from unet_bssfp_amd import data as Q

SHAPE = (20, 24, 32)


def _rng(seed):
    return np.random.default_rng(seed)


def _random_tensors(seed, n=50):
    """(6, n) components of symmetric positive definite matrices with well separated eigenvalues"""
    g = _rng(seed)
    q = np.linalg.qr(g.normal(size=(n, 3, 3)))[0]
    lam = np.sort(g.uniform(0.2, 3.0, size=(n, 3)))
    d = q @ (lam[:, :, None] * np.swapaxes(q, 1, 2))
    return S.components_of(d), d


# ---- matrices ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axes", [(), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)])
def test_flip_matrix_matches_the_restatement_and_is_exact_in_f32(axes):
    m = A.flip_index_matrix(axes, SHAPE)
    assert np.array_equal(m, S.flip(axes, SHAPE))
    assert np.array_equal(m.astype(np.float32).astype(np.float64), m)
    i = np.array([3, 5, 7, 1.0])
    assert np.array_equal((m @ i)[:3], [SHAPE[a] - 1 - i[a] if a in axes else i[a] for a in range(3)])
    assert A.RandomFlip.matrix(axes, SHAPE) is not None and np.array_equal(A.RandomFlip.matrix(axes, SHAPE), m)


def test_affine_matrix_matches_the_restatement():
    g = _rng(1)
    for _ in range(20):
        s, d, t = g.uniform(0.7, 1.4, 3), g.uniform(-40, 40, 3), g.uniform(-5, 5, 3)
        got = A.affine_index_matrix(s, d, t, SHAPE)
        assert np.abs(got - S.affine(s, d, t, SHAPE)).max() <= 1e-12
        assert np.array_equal(A.RandomAffine.matrix(A.AffineParams(s, d, t), SHAPE), got)
    # s > 1 zooms in: the output voxels read a smaller part of the input, about the centre of the grid
    m = A.affine_index_matrix((2, 2, 2), (0, 0, 0), (0, 0, 0), SHAPE)
    c = (np.array(SHAPE) - 1) / 2
    assert np.allclose(m @ np.append(c, 1), np.append(c, 1)) and np.allclose((m @ [0, 0, 0, 1])[:3], c / 2)
    # a translation moves the point that is read
    assert np.allclose(A.affine_index_matrix((1, 1, 1), (0, 0, 0), (1, -2, 3), SHAPE)[:3, 3], [1, -2, 3])


def test_the_affine_without_effect_is_the_identity_and_is_dropped():
    assert np.array_equal(A.affine_index_matrix((1, 1, 1), (0, 0, 0), (0, 0, 0), SHAPE), np.eye(4))
    none = A.AffineParams(np.ones(3), np.zeros(3), np.zeros(3))
    assert not A.RandomAffine.has_effect(none) and not A.RandomFlip.has_effect(())
    assert A.RandomAffine.has_effect(none._replace(translation=np.array([0, 0, 1e-3]))) and A.RandomFlip.has_effect((2,))
    load = Q.SubjectLoad(0, 0, 0, 0, (), ((A.RandomFlip(), ()), (A.RandomAffine(), none)))
    assert _queue().spatial_transform(load) is None


def test_composition_follows_list_order():
    g = _rng(2)
    m1 = A.flip_index_matrix((0, 2), SHAPE)
    m2 = A.affine_index_matrix(g.uniform(0.8, 1.2, 3), g.uniform(-20, 20, 3), g.uniform(-3, 3, 3), SHAPE)
    got = A.compose_index_matrices([m1, m2])
    assert np.abs(got - S.chain([S.flip((0, 2), SHAPE), m2])).max() <= 1e-12
    assert np.abs(got - m1 @ m2).max() == 0 and np.abs(got - m2 @ m1).max() > 1
    # resampling twice, in list order, reads where the product says
    i = np.array([4, 9, 13, 1.0])
    assert np.allclose(got @ i, m1 @ (m2 @ i))
    params = A.AffineParams(np.array([1.1, 0.9, 1.0]), np.array([5.0, -3, 8]), np.array([1.0, 0, -2]))
    fl, af = A.RandomFlip((0, 1, 2)), A.RandomAffine(default_pad_value=-2)
    q = _queue(spatial=[fl, af])
    m, fill = q.spatial_transform(Q.SubjectLoad(0, 0, 0, 0, (), ((fl, (1,)), (af, params))))
    assert fill == -2.0 and np.abs(m - S.chain([S.flip((1,), SHAPE), S.affine(*params, SHAPE)])).max() <= 1e-12
    m, fill = q.spatial_transform(Q.SubjectLoad(0, 0, 0, 0, (), ((fl, (1,)),)))
    assert fill == 0.0 and np.array_equal(m, S.flip((1,), SHAPE))
    assert q.spatial_transform(Q.SubjectLoad(0, 0, 0, 0, (), ((A.RandomAffine(), params),)))[1] is None   # 'minimum'


# ---- tensor map ------------------------------------------------------------------------------------------------------------

def _cases():
    g = _rng(3)
    out = []
    for _ in range(6):                                                # rotations
        out.append(("rotation", A.affine_index_matrix((1, 1, 1), g.uniform(-60, 60, 3), g.uniform(-3, 3, 3), SHAPE)))
    for axes in [(0,), (1, 2), (0, 1, 2)]:                            # reflections, alone and with a rotation
        out.append(("reflection", A.flip_index_matrix(axes, SHAPE)))
        out.append(("reflection", A.flip_index_matrix(axes, SHAPE) @ out[0][1]))
    for _ in range(4):                                                # anisotropic scales
        out.append(("scale", A.affine_index_matrix(g.uniform(0.6, 1.6, 3), g.uniform(-30, 30, 3), (0, 0, 0), SHAPE)))
    return out


@pytest.mark.parametrize("kind,m", _cases())
def test_tensor_map_is_r_d_rt(kind, m):
    t6, t = A.tensor_reorientation(m)
    assert not t.any()
    rot = S.rotation_of(m)
    assert np.abs(rot @ rot.T - np.eye(3)).max() <= 1e-12              # the polar factor is orthogonal
    assert np.sign(np.linalg.det(rot)) == np.sign(np.linalg.det(m[:3, :3]))   # a reflection stays a reflection
    if kind != "scale":
        assert np.abs(rot - np.linalg.inv(m[:3, :3])).max() <= 1e-12  # nothing but the rotation / reflection itself
    n6, d = _random_tensors(7)
    got = t6 @ n6
    want = S.components_of(rot @ d @ rot.T)
    assert np.abs(got - want).max() <= 1e-12
    assert np.abs(np.linalg.eigvalsh(S.tensor_of(got)) - np.linalg.eigvalsh(d)).max() <= 1e-12
    assert np.abs(got - S.reorient(n6, rot)).max() <= 1e-12


def test_pure_flips_only_change_the_signs_of_the_off_diagonal():
    for axes in [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]:
        sigma = [-1.0 if a in axes else 1.0 for a in range(3)]
        t6, t = A.tensor_reorientation(A.flip_index_matrix(axes, SHAPE))
        assert np.array_equal(t6, np.diag([sigma[a] * sigma[b] for a, b in A.TENSOR_COMPONENTS])) and not t.any()


def test_tensor_map_with_a_rescale_acts_on_normalised_values():
    g = _rng(4)
    rescale = np.stack([g.uniform(-2, -0.5, 6), g.uniform(1, 3, 6)], axis=1)
    rescale[3] = rescale[3][::-1]                                     # |max - min| is what counts
    n6, _ = _random_tensors(9)
    n6 = S.normalise(n6, rescale)
    for kind, m in _cases():
        t6, t = A.tensor_reorientation(m, rescale)
        got = t6 @ n6 + t[:, None]
        rot = S.rotation_of(m)
        want_d = S.components_of(rot @ S.tensor_of(S.denormalise(n6, rescale)) @ rot.T)
        assert np.abs(S.denormalise(got, rescale) - want_d).max() <= 1e-12
        assert np.abs(got - S.reorient(n6, rot, rescale)).max() <= 1e-12
    with pytest.raises(ValueError, match=r"\(6, 2\)"):
        A.tensor_reorientation(np.eye(4), np.zeros((6, 3)))
    with pytest.raises(ValueError, match="min != max"):
        A.tensor_reorientation(np.eye(4), np.zeros((6, 2)))


# ---- sampling ---------------------------------------------------------------------------------------------------------------

def test_sampling_order_and_ranges():
    torch.manual_seed(3)
    fl = A.RandomFlip(axes=(2, 0, 1), flip_probability=0.5)
    got = fl.sample()
    torch.manual_seed(3)
    assert got == tuple(a for a in (2, 0, 1) if torch.rand(1).item() < 0.5)       # one rand per listed axis, in order
    assert A.RandomFlip(axes=(0, 1, 2), flip_probability=1.0).sample() == (0, 1, 2)
    assert A.RandomFlip(axes=1, flip_probability=0.0).sample() == ()
    af = A.RandomAffine(scales=0.2, degrees=(-5, 15), translation=4)
    torch.manual_seed(5)
    p = af.sample()
    torch.manual_seed(5)
    r = [torch.rand(3, dtype=torch.float64).numpy() for _ in range(3)]            # scales, degrees, translation
    assert af.scales_range == (1 - 0.2, 1 + 0.2) and af.degrees_range == (-5.0, 15.0) and af.translation_range == (-4.0, 4.0)
    for got, u, (lo, hi) in zip(p, r, (af.scales_range, af.degrees_range, af.translation_range)):
        assert np.array_equal(got, u * (hi - lo) + lo)
    torch.manual_seed(5)
    iso = A.RandomAffine(scales=0.2, isotropic=True).sample()
    assert np.array_equal(iso.scales, np.full(3, p.scales[0])) and np.array_equal(iso.translation, np.zeros(3))
    assert A.RandomAffine().fill is None and A.RandomAffine(default_pad_value=3).fill == 3.0
    assert A.RandomAffine(scales=(0.5, 2.0)).scales_range == (0.5, 2.0)


# ---- plans -------------------------------------------------------------------------------------------------------------------

def _queue(n=5, **kw):
    subs = [{"bssfp": {"data": torch.zeros(24, 1, 1, 1)}, "dwi-tensor": {"data": torch.zeros(6, 1, 1, 1)}} for _ in range(n)]
    kw.setdefault("target_shape", SHAPE)
    kw.setdefault("sampler", Q.UniformSampler((8, 12, 16)))
    kw.setdefault("transform", A.reference_full_transform())
    return Q.PatchQueue(subs, "bssfp", **kw)


def _both():
    return [A.RandomFlip(axes=(0, 1, 2), p=0.7), A.RandomAffine(p=0.6, translation=2, default_pad_value=0.5)]


def test_a_plan_with_spatial_stages_equals_the_plan_without_them():
    a, b = _queue(seed=11), _queue(seed=11, spatial=_both())
    fired = 0
    for _ in range(3):                                                # three epochs
        pa, pb = a.next_plan(len(a)), b.next_plan(len(b))
        for x, y in zip(pa, pb):
            assert x.origin == y.origin and x.load.spatial == ()
            assert x.load[:4] == y.load[:4]                           # subject, epoch, fill, seed
            assert _drawn(x.load.stages) == _drawn(y.load.stages)
            fired += len(y.load.spatial)
    assert fired > 40
    assert torch.equal(a._gen.get_state(), b._gen.get_state())        # the queue's generator never saw a spatial draw
    assert Q.SubjectLoad._fields[-1] == "spatial" and Q.SubjectLoad(0, 0, 0, 0, ()).spatial == ()


def _drawn(stages):
    """the stages that fired and their parameters, without the identity of the transform objects"""
    return repr([(type(t).__name__, p) for t, p in stages])


def test_the_spatial_draws_come_from_the_seed_of_the_load():
    stages = _both()
    q = _queue(seed=2, spatial=stages, transform=[])
    for pl in q.next_plan(16):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(pl.load.seed + 1)
            want = []
            for t in stages:
                if torch.rand(1).item() < t.p:
                    want.append((t, t.sample()))
        assert _drawn(pl.load.spatial) == _drawn(want)


def test_no_spatial_stage_draws_nothing():
    before = torch.random.get_rng_state()
    for spatial in (None, []):
        q = _queue(seed=5, spatial=spatial, transform=[])
        assert q.spatial == [] and q._draw_spatial(7) == ()
        assert all(pl.load.spatial == () for pl in q.next_plan(40))
    assert torch.equal(before, torch.random.get_rng_state())          # the global generator is left as it was
    q = _queue(seed=5, spatial=_both(), transform=[])
    q.next_plan(40)
    assert torch.equal(before, torch.random.get_rng_state())


def test_a_resumed_queue_repeats_its_spatial_draws():
    a = _queue(seed=9, spatial=_both())
    a.next_plan(len(a))
    state = a.state_dict()
    assert set(state) == {"generator", "epoch", "fill_count"}          # no new state
    b = _queue(seed=1234, spatial=_both())
    b.load_state_dict(state)
    pa, pb = a.next_plan(2 * len(a)), b.next_plan(2 * len(b))
    for x, y in zip(pa, pb):
        assert (x.origin, x.load[:4], _drawn(x.load.spatial)) == (y.origin, y.load[:4], _drawn(y.load.spatial))
    assert sum(len(p.load.spatial) for p in pa) > 20


# ---- refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals_of_the_stages():
    with pytest.raises(NotImplementedError, match="linear"):
        A.RandomAffine(image_interpolation="nearest")
    with pytest.raises(NotImplementedError, match="linear"):
        A.RandomAffine(image_interpolation="bspline")
    for center in ("origin", "mass"):
        with pytest.raises(NotImplementedError, match="image"):
            A.RandomAffine(center=center)
    for pad in ("mean", "otsu"):
        with pytest.raises(NotImplementedError, match="minimum"):
            A.RandomAffine(default_pad_value=pad)
    for pad in (None, float("nan"), (1, 2)):
        with pytest.raises(ValueError, match="minimum"):
            A.RandomAffine(default_pad_value=pad)
    with pytest.raises(ValueError, match="scale"):
        A.RandomAffine(scales=1.0)                                    # (0, 2): a scale of 0 has no inverse
    with pytest.raises(ValueError, match="positive"):
        A.affine_index_matrix((1, 0, 1), (0, 0, 0), (0, 0, 0), SHAPE)
    for axes in (3, (0, 0), (), ("LR",)):
        with pytest.raises(ValueError, match="axes"):
            A.RandomFlip(axes=axes)
    with pytest.raises(ValueError, match="flip_probability"):
        A.RandomFlip(flip_probability=1.5)
    with pytest.raises(ValueError, match="axes"):
        A.flip_index_matrix((3,), SHAPE)


def test_refusals_of_the_queue():
    with pytest.raises(TypeError, match="two RandomFlip"):
        _queue(spatial=[A.RandomFlip(0), A.RandomFlip(1)])
    with pytest.raises(TypeError, match="two RandomAffine"):
        _queue(spatial=[A.RandomAffine(), A.RandomFlip(1), A.RandomAffine()])
    with pytest.raises(TypeError, match="no spatial stage"):
        _queue(spatial=[A.RandomGamma()])
    with pytest.raises(TypeError, match="cannot be fused"):
        _queue(transform=[A.RandomFlip()])                            # a spatial stage inside the keep= Compose breaks the pair
    # a tensor image without 6 channels
    with pytest.raises(ValueError, match="24 channels"):
        _queue(spatial=[A.RandomFlip()], tensor_images={"bssfp": None})
    with pytest.raises(ValueError, match="not among the images"):
        _queue(spatial=[A.RandomFlip()], tensor_images={"fa": None})
    with pytest.raises(ValueError, match=r"\(6, 2\)"):
        _queue(spatial=[A.RandomFlip()], tensor_images={"dwi-tensor": np.zeros((2, 6))})
    q = _queue(spatial=[A.RandomFlip()])
    assert list(q.tensor_images) == ["dwi-tensor"] and q.tensor_images["dwi-tensor"] is None
    assert _queue(spatial=[A.RandomFlip()], tensor_images={}).tensor_images == {}
    # a fifth image
    subs = [{k: {"data": torch.zeros(6, 1, 1, 1)} for k in ("bssfp", "dwi-tensor", "fa")}]
    q = Q.PatchQueue(subs, "bssfp", target_shape=SHAPE, sampler=Q.UniformSampler(8), spatial=[A.RandomFlip()],
                     keep={"dwi-tensor": "dwi-tensor_orig", "fa": "fa_orig"})
    assert len(q._images(False)) == 3
    with pytest.raises(ValueError, match="at most 4 images"):
        q._images(True)


# ---- the manifest ------------------------------------------------------------------------------------------------------------

def test_manifest_keys_build_the_stages(tmp_path):
    from unet_bssfp_amd.train import spatial_from_manifest
    assert spatial_from_manifest({"modality": "bssfp"}) == {}
    rescale = [[-0.5, 2.5], [-1.0, 1.0], [-1.5, 0.5], [0.0, 3.0], [-0.75, 1.25], [0.25, 2.0]]
    path = tmp_path / "rescale_args_dwi.txt"
    np.savetxt(path, np.array(rescale))
    for given in (rescale, str(path)):
        kw = spatial_from_manifest({"spatial": [{"type": "RandomFlip", "axes": [0, 1, 2]},
                                                {"type": "RandomAffine", "degrees": 10, "scales": 0.1, "p": 0.5}],
                                    "tensor_rescale": given})
        fl, af = kw["spatial"]
        assert type(fl) is A.RandomFlip and fl.axes == (0, 1, 2) and fl.flip_probability == 0.5
        assert type(af) is A.RandomAffine and af.degrees_range == (-10.0, 10.0) and af.p == 0.5 and af.fill is None
        assert np.array_equal(kw["tensor_images"]["dwi-tensor"], np.array(rescale))
        q = _queue(**kw)
        assert q.spatial == [fl, af] and q.tensor_images["dwi-tensor"].shape == (6, 2)
    with pytest.raises(ValueError, match="unknown type"):
        spatial_from_manifest({"spatial": [{"type": "RandomElasticDeformation"}]})
    with pytest.raises(NotImplementedError, match="linear"):
        spatial_from_manifest({"spatial": [{"type": "RandomAffine", "image_interpolation": "bspline"}]})
