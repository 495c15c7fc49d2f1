"""RandomGhosting / RandomSpike / RandomBlur on the device (csrc/kspace.hip, unet_bssfp_amd.augment) against the f64
restatements of tests/kspace_ref.py, and the patch queue that stages them (unet_bssfp_amd.data), bit for bit against the
chained path.  Every bound is derived from the f32 format: gamma_N = N u / (1 - N u), u = 2^-24, is the bound of an N-term
fma chain.  TorchIO is absent: parity with TorchIO itself stays unpinned."""
import gc

import numpy as np
import pytest
import torch

import kspace_ref as K
from unet_bssfp_amd import augment as A
from unet_bssfp_amd import data as Q

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
E_TRIG = 1e-6 + 3 * U     # phase fraction rounded to f32 (2 pi u), sincospif (2 ulp), the wave's own fma and scaling


def gamma(n):
    return n * U / (1 - n * U)


def _ulp(ref):
    return np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def _einsum(m, x, axis):
    """f64 on the host: sum_j m[i][j] x[c][..j..] along spatial axis `axis` of (C, D, H, W)"""
    spec = ["ij,cjhw->cihw", "ij,cdjw->cdiw", "ij,cdhj->cdhi"][axis]
    return torch.einsum(spec, m, x)


# ---- the primitive ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(24, 96, 128, 128), (6, 128, 96, 96), (6, 7, 96, 13), (24, 5, 9, 128)])
def test_axis_apply_against_f64_einsum(hip, shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.rand(shape, generator=g) - 0.3
    xd = x.to(DEV)
    x64 = x.double()
    for axis in range(3):
        n = shape[1 + axis]
        m = (torch.rand(n, n, generator=g) - 0.5).float()
        got = A.axis_apply(xd, m.to(DEV), axis).cpu().double()
        want = _einsum(m.double(), x64, axis)
        bound = gamma(n) * _einsum(m.double().abs(), x64.abs(), axis).numpy() + _ulp(want.numpy())
        ratio = float(((got - want).abs().numpy() / bound).max())
        print(f"axis_apply {shape} axis {axis} N {n}: worst err / bound = {ratio:.3f}")
        assert ratio <= 1.0


def test_axis_apply_rejects_what_it_does_not_do(hip):
    from unet_bssfp_amd import _lib
    x = torch.zeros(1, 2, 2, 130, device=DEV)
    with pytest.raises(_lib.Mi355Error, match="exceeds 128"):
        A.axis_apply(x, torch.zeros(130, 130, device=DEV), 2)
    with pytest.raises(ValueError):
        A.axis_apply(x, torch.zeros(3, 3, device=DEV), 0)
    rc = hip.mi355_axis_apply(x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 2, 2, 130, 0, None)
    assert rc < 0 and b"in-place" in hip.mi355_last_error()


def test_complex_passes_reproduce_fftn_and_its_maximum(hip):
    """the three DFT passes (W real -> complex, H, D) against numpy, and the reducing last pass against the same data"""
    shape = (3, 10, 12, 9)
    x = torch.rand(shape, generator=torch.Generator().manual_seed(0)) - 0.5
    xd = x.to(DEV)
    planes = {n: tuple(t.to(DEV) for t in (torch.from_numpy(A.dft_matrix(n).real.astype(np.float32)),
                                            torch.from_numpy(A.dft_matrix(n).imag.astype(np.float32)))) for n in shape[1:]}
    re, im = xd, None
    for axis in (2, 1, 0):
        mr, mi = planes[shape[1 + axis]]
        outr, outi = torch.empty_like(xd), torch.empty_like(xd)
        rc = hip.mi355_axis_apply_complex(re.data_ptr(), None if im is None else im.data_ptr(), mr.data_ptr(), mi.data_ptr(),
                                          outr.data_ptr(), outi.data_ptr(), *shape, axis, None)
        assert rc == 0, hip.mi355_last_error()
        re, im = outr, outi
    want = np.fft.fftn(x.double().numpy(), axes=(1, 2, 3))
    sabs = x.double().abs().sum((1, 2, 3)).numpy()[:, None, None, None]
    bound = (sum(gamma(2 * n) + U for n in shape[1:])) * sabs * np.sqrt(2)     # complex: 2 N terms per sum
    assert (np.abs(re.cpu().numpy() - want.real) <= bound).all() and (np.abs(im.cpu().numpy() - want.imag) <= bound).all()
    m = A.spectrum_max_device(xd).cpu().numpy()
    for c in range(shape[0]):
        ref = A.spectrum_max(x[c].double().numpy())
        assert abs(m[c, 0] - ref.real) <= bound[c, 0, 0, 0] and abs(m[c, 1] - ref.imag) <= bound[c, 0, 0, 0]
    sm = A.channel_sum_min(xd).cpu().numpy()
    assert np.allclose(sm[:, 0], x.double().sum((1, 2, 3)).numpy(), rtol=0, atol=1e-9)
    assert np.array_equal(sm[:, 1], x.amin((1, 2, 3)).double().numpy())


# ---- the stages -----------------------------------------------------------------------------------------------------------

SHAPES = [(6, 96, 128, 128), (3, 9, 20, 14)]


@pytest.mark.parametrize("shape", SHAPES)
def test_ghosting_against_the_restatement(hip, shape):
    x = torch.rand(shape, generator=torch.Generator().manual_seed(1))
    xd = x.to(DEV)
    gh = A.RandomGhosting()
    for axis, n, intensity in ((0, 4, 0.73), (1, 7, 1.0), (2, 10, 0.5)):
        got = gh.apply(xd, (n, axis, intensity)).cpu().double().numpy()
        n_axis = shape[1 + axis]
        g = A.ghosting_matrix(n_axis, n, intensity)
        sabs = _einsum(torch.from_numpy(np.abs(g)), x.double().abs(), axis).numpy()
        worst = 0.0
        for c in range(shape[0]):
            want = K.ghosting(x[c].double().numpy(), n, axis, intensity)
            bound = (gamma(n_axis) + U) * sabs[c] + _ulp(want)       # one pass; + u: the matrix is rounded to f32 once
            worst = max(worst, float((np.abs(got[c] - want) / bound).max()))
        print(f"ghosting {shape} axis {axis}: worst err / bound = {worst:.3f}")
        assert worst <= 1.0
    assert gh.apply(xd, (0, 1, 0.7)) is xd and gh.apply(xd, (5, 1, 0.0)) is xd
    y = gh(xd)                                                         # sample + apply, and the subject-dict form
    assert y.shape == xd.shape and not torch.equal(y, xd)
    torch.manual_seed(5)
    d = gh({"a": {"data": xd}, "b": {"data": xd[:2]}, "other": 3})
    assert torch.equal(d["a"]["data"][:2], d["b"]["data"]) and d["other"] == 3


@pytest.mark.parametrize("shape", SHAPES)
def test_blur_against_scipy(hip, shape):
    x = torch.rand(shape, generator=torch.Generator().manual_seed(2)) - 0.3
    xd = x.to(DEV)
    for sigmas in ((0.6, 1.5, 0.9), (1.2, 0.1, 2.0)):                 # the second skips H
        got = A.RandomBlur().apply(xd, sigmas).cpu().double().numpy()
        # per element, built from the one-pass bound: pass p adds (gamma_N + u) sum|B||y| + ulp (u: the matrix is rounded
        # to f32 once), and the error of the earlier passes goes through B itself (its entries are non-negative)
        y, bound = x.double(), torch.zeros(shape, dtype=torch.float64)
        for axis, sigma in enumerate(sigmas):
            b = A.blur_matrix(shape[1 + axis], sigma)
            if b is None:
                continue
            b = torch.from_numpy(b)
            step = (gamma(shape[1 + axis]) + U) * _einsum(b, y.abs(), axis)
            y = _einsum(b, y, axis)
            bound = _einsum(b, bound, axis) + step + torch.from_numpy(_ulp(y.numpy()))
        want = np.stack([K.blur(x[c].double().numpy(), sigmas) for c in range(shape[0])])
        assert np.abs(y.numpy() - want).max() <= 64 * np.finfo(np.float64).eps   # the matrices are scipy's filter
        worst = float((np.abs(got - want) / bound.numpy()).max())
        print(f"blur {shape} sigmas {sigmas}: worst err / bound = {worst:.3f}")
        assert worst <= 1.0
        assert float(np.abs(got - x.double().numpy()).max()) > 0.05


def test_blur_with_the_reference_arguments_returns_its_input_and_launches_nothing(hip, monkeypatch):
    def no_pass(*a, **k):
        raise AssertionError("a matrix pass was launched")
    monkeypatch.setattr(A, "axis_apply", no_pass)
    x = torch.rand(6, 12, 16, 20, device=DEV)
    blur = A.RandomBlur(std=(0.01, 0.1))
    for _ in range(20):
        assert torch.equal(blur(x), x)
    assert torch.equal(blur.apply(x, (0.124, 0.01, 0.1)), x)


def _signed(shape, seed):
    """per channel: zero-mean noise plus a strong plane wave, so that the maximum is a complex non-DC bin"""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.arange(n) for n in shape[1:]], indexing="ij")
    out = np.empty(shape)
    for c in range(shape[0]):
        f = (1 + c % 3, 2 + c % 2, 3)
        phase = 2 * np.pi * sum(fd * gd / n for fd, gd, n in zip(f, g, shape[1:])) + 0.7 + 0.1 * c
        v = rng.random(shape[1:]) - 0.5
        out[c] = v - v.mean() + 0.8 * np.cos(phase)
    return torch.from_numpy(out.astype(np.float32))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("signed", [False, True])
def test_spike_against_the_restatement(hip, shape, signed):
    x = _signed(shape, 3) if signed else torch.rand(shape, generator=torch.Generator().manual_seed(3))
    xd = x.to(DEV)
    vol = float(np.prod(shape[1:]))
    m_bound = [(sum(gamma(n) for n in shape[1:]) + 3 * U) * float(x[c].double().abs().sum()) for c in range(shape[0])]
    if signed:                                                        # the arg-max is well defined at f32 accuracy
        for c in range(shape[0]):
            top, second = K.top_two_real_parts(x[c].double().numpy())
            assert top - second > 2 * m_bound[c], (c, top, second, m_bound[c])
    m_dev = (A.spectrum_max_device(xd) if signed else A.channel_sum_min(xd)).cpu().numpy()
    sp = A.RandomSpike(intensity=(0.01, 0.1))
    for pos, intensity in (([0.0, 0.0, 0.0], 0.1), ([0.999, 0.995, 0.997], -0.07), ([0.31, 0.52, 0.77], 3.0)):
        pos = np.array([pos])
        got = sp.apply(xd, A.SpikeParams(intensity, pos)).cpu().double().numpy()      # path None: decided from the data
        forced = sp.apply(xd, A.SpikeParams(intensity, pos, "dft" if signed else "dc"))
        assert torch.equal(forced.cpu(), torch.from_numpy(got).float())
        worst = 0.0
        for c in range(shape[0]):
            x64 = x[c].double().numpy()
            want, maxima = K.spike(x64, pos, intensity, return_maxima=True)
            m = maxima[0]
            assert abs(m_dev[c, 0] - m.real) <= m_bound[c]
            if signed:
                assert abs(m_dev[c, 1] - abs(m.imag)) <= m_bound[c] and abs(m.imag) > 100 * m_bound[c]
            else:
                assert m.real == pytest.approx(x64.sum(), rel=1e-12)
            # |delta M| <= sqrt(2) (bound per component + the amplitude's rounding to f32)
            bound = (np.sqrt(2) * (m_bound[c] + U * abs(m)) * abs(intensity) + abs(m) * abs(intensity) * E_TRIG) / vol + _ulp(want)
            worst = max(worst, float((np.abs(got[c] - want) / bound).max()))
            assert float(np.abs(want - x64).max()) > 0.2 * abs(m) * abs(intensity) / vol
        print(f"spike {shape} signed={signed} I={intensity}: worst err / bound = {worst:.3f}")
        assert worst <= 1.0
    # the DFT path on non-negative data gives the DC bin too, within the three-pass bound
    if not signed:
        m3 = A.spectrum_max_device(xd).cpu().numpy()
        for c in range(shape[0]):
            assert abs(m3[c, 0] - m_dev[c, 0]) <= m_bound[c] and m3[c, 1] <= m_bound[c]
    assert sp.apply(xd, A.SpikeParams(0.0, pos)) is xd and sp.apply(xd, A.SpikeParams(0.5, np.zeros((0, 3)))) is xd
    from unet_bssfp_amd import _lib
    with pytest.raises(_lib.Mi355Error):
        sp.apply(xd, A.SpikeParams(0.5, np.zeros((2, 3))))


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
                x = t.apply(x, params)
        loc = np.array([list(p.origin) + [o + s for o, s in zip(p.origin, q.patch_size)]])
        out.append(extract_patches(x, loc, q.patch_size))
    return torch.cat(out)


def _check_batch(q, plan, batch, augmented_target=True):
    assert torch.equal(batch["bssfp"]["data"], _chained(q, plan, "bssfp", True))
    assert torch.equal(batch["dwi-tensor_orig"]["data"], _chained(q, plan, "dwi-tensor", False))
    if augmented_target:
        assert torch.equal(batch["dwi-tensor"]["data"], _chained(q, plan, "dwi-tensor", True))


GH, SP, BIAS, BLUR, NOISE, GAMMA = A.reference_training_transform()
_SETS = {
    "ghosting": [GH], "spike": [SP], "blur": [BLUR], "ghosting+spike": [GH, SP],
    "six": [GH, SP, BIAS, BLUR, NOISE, GAMMA], "blur_identity": [BIAS, BLUR, GAMMA], "local_then_blur": [NOISE, BLUR],
}


def _params(q, subject, t, before, rng, identity_blur=False):
    if t is GH:
        return (int(rng.integers(4, 11)), int(rng.integers(0, 3)), float(rng.uniform(0.5, 1)))
    if t is SP:
        return A.SpikeParams(float(rng.uniform(0.5, 2)), rng.random((1, 3)), q.spike_path(subject, before))
    if t is BLUR:
        return tuple(rng.uniform(0.01, 0.1, 3)) if identity_blur else (float(rng.uniform(0.5, 1.5)), 0.1, float(rng.uniform(0.5, 2)))
    if t is BIAS:
        return (rng.random(20) - 0.5).astype(np.float32)
    if t is NOISE:
        return (float(rng.uniform(-0.1, 0.1)), float(rng.uniform(0.01, 0.1)), int(rng.integers(0, 2 ** 62)))
    return float(np.exp(rng.uniform(-0.3, 0.3)))


@pytest.mark.parametrize("lo", [-0.3, 0.0])                            # signed subjects: DFT path; non-negative: DC path
@pytest.mark.parametrize("stages", list(_SETS))
def test_queue_batch_equals_the_chained_path(hip, stages, lo):
    target, patch = (20, 24, 32), (8, 12, 16)
    extents = [(23, 19, 32), (20, 24, 32), (17, 27, 37)]               # crop D + pad H; the target; pad D + crop H, W
    subs = _subjects(len(extents), extents, seed=len(stages), lo=lo)
    q = Q.PatchQueue(subs, "bssfp", sampler=Q.UniformSampler(patch), target_shape=target, transform=_SETS[stages])
    rng = np.random.default_rng(len(stages))
    hi = [t - p for t, p in zip(target, patch)]
    plan = []
    for i in range(len(extents)):
        st = []
        for t in _SETS[stages]:
            st.append((t, _params(q, i, t, st, rng, identity_blur=stages == "blur_identity")))
        load = Q.SubjectLoad(i, 0, 0, 0, tuple(st))
        origins = [(0, 0, 0), tuple(hi)] + [tuple(int(rng.integers(0, h + 1)) for h in hi) for _ in range(2)]
        plan += [Q.PlannedPatch(load, o) for o in origins]
    paths = {p.path for pl in plan for t, p in pl.load.stages if t is SP}
    if SP in _SETS[stages]:
        assert paths == ({"dft"} if lo < 0 or GH in _SETS[stages] else {"dc"})
    batch = q.gather(plan, augmented_target=True)
    if stages == "blur_identity":
        assert q._staged == {}                                        # nothing fired with an effect: no staging tensor
    else:
        assert len(q._staged) == len(extents) and all(set(e[1]) == {"bssfp", "dwi-tensor"} for e in q._staged.values())
        assert all(t.shape[1:] == target for e in q._staged.values() for t in e[1].values())
    _check_batch(q, plan, batch)
    q.gather(plan[:1])                                                # the other loads have no patch left
    assert len(q._staged) == (0 if stages == "blur_identity" else 1)


def _forced(p=1.0):
    tr = A.reference_training_transform()
    for t in tr:
        t.p = p
    tr[3].std_range = (0.5, 1.5)                                      # a blur that does blur
    return tr


def test_queue_straddles_fills_without_host_sync_and_releases_staging(hip):
    """batches that straddle fills equal the chained path, next_batch never synchronises, and the bytes held on the
    device after 40 fills with every stage forced equal those after 4 (staging is released with its load)"""
    target, patch = (20, 24, 32), (8, 12, 16)
    subs = _subjects(7, [(23, 19, 32), (20, 24, 32), (17, 27, 37)], seed=5)

    def queue(p):
        return Q.PatchQueue(subs, "bssfp", max_length=4, samples_per_volume=2, sampler=Q.UniformSampler(patch),
                            target_shape=target, transform=_forced(p), seed=21)
    q, twin = queue(0.5), queue(0.5)
    q.next_batch(2), twin.next_plan(2)                                # first use uploads the DFT matrices
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        batches = [(bs, q.next_batch(bs, augmented_target=True)) for bs in (3, 6, 5, 7)]   # fills of 4 patches
    finally:
        torch.cuda.set_sync_debug_mode("default")
    staged = 0
    for bs, batch in batches:
        plan = twin.next_plan(bs)
        assert len({p.load.fill for p in plan}) > 1
        staged += sum(bool(Q.PatchQueue.split_stages(p.load)[0]) for p in plan)
        _check_batch(q, plan, batch)
    assert staged > 4
    # device memory does not grow with the number of fills: a staged tensor lives no longer than its load's patches
    subs = _subjects(8, [(23, 19, 32), (20, 24, 32), (17, 27, 37)], seed=6)      # every fill: 2 loads = one batch of 4
    q = queue(1.0)

    def run(fills):
        while q.fill_count < fills:
            q.next_batch(4, augmented_target=True)
        while q._patches:
            q.next_batch(len(q._patches), augmented_target=True)
        gc.collect()                                                  # tensors that only unreachable host objects still hold
        torch.cuda.synchronize()
        # bytes the live tensors asked for.  memory_allocated() also counts the unsplit tail of a cached block that a
        # request was served from (the caching allocator splits a large block only if more than 1 MiB remains), so it
        # depends on the history of freed blocks, not only on what is held
        stats = torch.cuda.memory_stats()
        print(f"fills {q.fill_count}: requested {stats['requested_bytes.all.current']} allocated {torch.cuda.memory_allocated()}")
        return stats["requested_bytes.all.current"]
    after4 = run(4)
    assert len(q._staged) <= 2 and all(Q.PatchQueue.split_stages(l)[0] for l in q.last_fill)
    assert run(40) == after4


def test_queue_with_the_reference_training_transform_feeds_a_graphed_training_step(hip):
    import unet_bssfp_amd as M
    from unet_bssfp_amd.functional import DropoutState
    from unet_bssfp_amd.gan import GraphedTrainingStep, bSSFPToDWITensorModel, synthetic_batch

    torch.manual_seed(4)
    DropoutState.reset()
    gen, discr = M.Generator("bssfp", dropout=0.05), M.Discriminator("bssfp")
    model = bSSFPToDWITensorModel("bssfp", gen=gen.to(DEV), discr=discr.to(DEV)).train()
    subs = _subjects(5, [(40, 52, 36), (36, 44, 44)], seed=2, lo=0.0)

    def queue():
        tr = A.reference_training_transform()
        for t in tr:
            t.p = 0.5                                                 # the reference's stages, firing often enough to see
        return Q.PatchQueue(subs, "bssfp", max_length=4, samples_per_volume=2, sampler=Q.UniformSampler(32),
                            target_shape=(36, 48, 40), transform=tr, seed=17)
    q, twin = queue(), queue()
    gs = GraphedTrainingStep(model, synthetic_batch(2, 32, seed=1, device=DEV), warmup=2)
    static = gs.instances[0][0]
    x_ptr = static["bssfp"]["data"].data_ptr()
    staged = 0
    for _ in range(4):
        q.next_batch(2, out=static)
        staged += len(q._staged)
        want = twin.next_batch(2)
        assert static["bssfp"]["data"].data_ptr() == x_ptr
        assert torch.equal(static["bssfp"]["data"], want["bssfp"]["data"])
        assert torch.equal(static["dwi-tensor_orig"]["data"], want["dwi-tensor_orig"]["data"])
        gs(0)
        logs = torch.stack([v.reshape(()).float() for v in model.last_logs.values()])
        assert torch.isfinite(logs).all()
    assert staged > 0
