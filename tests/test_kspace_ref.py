"""Host mathematics of RandomGhosting / RandomSpike / RandomBlur (unet_bssfp_amd.augment) against the
literal f64 restatements of tests/kspace_ref.py, and the host plan of a patch queue that carries them.  No GPU needed.
TorchIO is absent: these tests pin the project's reading of TorchIO 0.19.6, parity with TorchIO itself is unpinned."""
import numpy as np
import pytest
import torch

import kspace_ref as K
from unet_bssfp_amd import augment as A
from unet_bssfp_amd import data as Q

EPS = np.finfo(np.float64).eps


def _along(m, x, axis):
    return np.moveaxis(np.tensordot(m, x, axes=([1], [axis])), 0, axis)


# ---- ghosting ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(12, 16, 20), (11, 13, 9), (96, 6, 10), (7, 96, 4), (5, 6, 96)])
def test_ghosting_matrix_equals_the_3d_restatement(shape):
    rng = np.random.default_rng(sum(shape))
    x = rng.random(shape)
    ntot = float(np.prod(shape))
    worst = 0.0
    for axis in range(3):
        n_axis = shape[axis]
        for n in range(4, 11):
            for intensity in (0.5, 0.73, 1.0):
                g = A.ghosting_matrix(n_axis, n, intensity)
                assert g.dtype == np.float64 and g.shape == (n_axis, n_axis)
                i = np.arange(n_axis)
                assert np.array_equal(g, g[:, 0][(i[:, None] - i[None, :]) % n_axis])    # circulant
                want = K.ghosting(x, n, axis, intensity)
                got = _along(g, x, axis)
                # f64 rounding of an N-term product: N eps sum|g| max|x| (a few ulps of the data range)
                bound = n_axis * EPS * np.abs(g[0]).sum() * np.abs(x).max()
                err = np.abs(got - want).max()
                worst = max(worst, err / bound)
                assert err <= bound, (axis, n, intensity, err, bound)
                assert np.abs(want - x).max() > 1e-3                   # the artifact is not the identity
    print(f"ghosting {shape}: worst err / bound = {worst:.3g}")


def test_ghosting_discards_a_large_imaginary_part_and_degenerates_to_the_identity():
    x = np.random.default_rng(1).random((12, 16, 20))
    y = K.ghosting(x, 5, 0, 0.8, return_complex=True)                # 5 does not divide 12
    assert np.abs(y.imag).max() > 0.05
    assert A.ghosting_matrix(16, 0, 0.7) is None and A.ghosting_matrix(16, 5, 0.0) is None
    assert np.array_equal(K.ghosting(x, 0, 1, 0.7), x)


# ---- blur -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sigma", [0.126, 0.6, 1.5])
@pytest.mark.parametrize("n", [5, 16, 96])
def test_blur_matrix_equals_scipy(sigma, n):
    from scipy.ndimage import gaussian_filter1d
    x = np.random.default_rng(n).random((n, 3))
    b = A.blur_matrix(n, sigma)
    assert b.shape == (n, n) and np.allclose(b.sum(1), 1.0, atol=4 * EPS * n, rtol=0)
    r = A.blur_radius(sigma)
    i, j = np.nonzero(b)
    assert (np.abs(i - j) <= r).all()                                 # banded: reflection folds into the border rows
    want = gaussian_filter1d(x, sigma, axis=0)
    assert np.abs(b @ x - want).max() <= 4 * (2 * r + 1) * EPS


def test_blur_reflection_wraps_more_than_once_on_a_short_axis():
    from scipy.ndimage import gaussian_filter1d
    x = np.random.default_rng(2).random(3)
    sigma = 2.0                                                        # radius 8 on an axis of 3: period 6 twice over
    assert A.blur_radius(sigma) == 8
    assert np.abs(A.blur_matrix(3, sigma) @ x - gaussian_filter1d(x, sigma)).max() <= 4 * 17 * EPS


def test_blur_with_the_reference_arguments_is_the_identity():
    """the recorded finding: scipy's radius is int(4 sigma + 0.5), 0 up to sigma = 0.124"""
    from scipy.ndimage import gaussian_filter
    x = np.random.default_rng(3).random((6, 7, 8)).astype(np.float32)
    for sigma in (0.01, 0.1, 0.124):
        assert A.blur_radius(sigma) == 0 and A.blur_matrix(8, sigma) is None     # the "skip" marker
        assert np.array_equal(gaussian_filter(x, sigma), x)
    assert A.blur_radius(0.126) == 1 and A.blur_matrix(8, 0.126) is not None
    x64 = x.astype(np.float64)                                        # the side taps are 2e-14: visible in f64 only
    assert not np.array_equal(gaussian_filter(x64, 0.126), x64)
    x3 = np.random.default_rng(4).random((6, 7, 8))
    got = x3
    for axis, s in enumerate((0.6, 0.1, 1.5)):                       # a skipped axis in the middle
        b = A.blur_matrix(x3.shape[axis], s)
        got = got if b is None else _along(b, got, axis)
    assert np.abs(got - K.blur(x3, (0.6, 0.1, 1.5))).max() <= 64 * EPS


# ---- spike ------------------------------------------------------------------------------------------------------------

def _signed_volume(shape, seed):
    """zero-mean noise plus a strong plane wave: the spectrum's maximum is a complex, non-DC bin"""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    phase = 2 * np.pi * (2 * g[0] / shape[0] + 1 * g[1] / shape[1] + 3 * g[2] / shape[2]) + 0.7
    x = rng.random(shape) - 0.5
    return x - x.mean() + 0.8 * np.cos(phase)


@pytest.mark.parametrize("k", [1, 3])
def test_spike_closed_form_on_non_negative_data(k):
    shape = (6, 7, 8)
    rng = np.random.default_rng(k)
    x = rng.random(shape)
    pos = rng.random((k, 3))
    pos[0] = 0.0 if k == 1 else [0.999, 0.99, 0.95]                   # exactly 0 / floors to N - 1 on every axis
    assert A.spike_frequencies([0.0, 0.0, 0.0], shape) == (-3, -3, -4)
    assert A.spike_frequencies([0.999, 0.99, 0.95], shape) == (5 - 3, 6 - 3, 7 - 4)
    m0 = A.spectrum_max(x)
    assert m0 == complex(x.sum(), 0.0)                                 # M == sum(x), no transform
    want, maxima = K.spike(x, pos, 0.7, return_maxima=True)
    assert abs(maxima[0] - x.sum()) <= 4 * EPS * x.size * x.sum()
    got, amps = A.spike_closed_form(x, pos, 0.7)
    assert len(amps) == k
    for a, m in zip(amps, maxima):
        assert abs(a - m * 0.7) <= 1e-12 * abs(m)
    assert np.abs(got - want).max() <= 64 * EPS * (np.abs(x).max() + sum(abs(a) for a in amps) / x.size)
    assert np.abs(want - x).max() > 1e-2


@pytest.mark.parametrize("k", [1, 3])
def test_spike_closed_form_on_signed_data(k):
    shape = (6, 7, 8)
    x = _signed_volume(shape, 10 + k)
    assert x.min() < 0
    m_np = K.spectrum_maximum(x)
    assert abs(m_np.imag) > 1.0                                        # a genuinely complex maximum
    m0 = A.spectrum_max(x)
    # the conjugate-pair rule equals numpy's max() up to the sign convention
    assert abs(m0.real - m_np.real) <= 1e-12 * abs(m_np) and abs(m0.imag - abs(m_np.imag)) <= 1e-12 * abs(m_np)
    assert m_np.imag > 0                                               # lexicographic: numpy picks Im > 0 of the pair
    pos = np.random.default_rng(k).random((k, 3))
    want = K.spike(x, pos, -0.4)
    got, amps = A.spike_closed_form(x, pos, -0.4)
    assert np.abs(got - want).max() <= 64 * EPS * (np.abs(x).max() + sum(abs(a) for a in amps) / x.size)
    # the same bin twice: the second spike sees the first one's amplitude in the current spectrum
    pos2 = np.array([[0.3, 0.4, 0.6], [0.3, 0.4, 0.6]])
    want, maxima = K.spike(x, pos2, 2.0, return_maxima=True)
    got, amps = A.spike_closed_form(x, pos2, 2.0)
    assert abs(maxima[1]) > 1.5 * abs(maxima[0])
    assert np.abs(got - want).max() <= 64 * EPS * (np.abs(x).max() + sum(abs(a) for a in amps) / x.size)


def test_several_spikes_need_a_positive_maximum():
    x = np.zeros((4, 4, 4))
    x[0, 0, 0] = -1.0                                                 # X(k) = -1 in every bin
    A.spike_closed_form(x, [[0.1, 0.2, 0.3]], 1.0)
    with pytest.raises(ValueError):
        A.spike_closed_form(x, [[0.1, 0.2, 0.3], [0.5, 0.5, 0.5]], 1.0)


def test_dft_matrix_passes_reproduce_fftn():
    x = np.random.default_rng(5).random((5, 6, 8)) - 0.5
    s = x.astype(np.complex128)
    for axis in (2, 1, 0):
        s = _along(A.dft_matrix(x.shape[axis]), s, axis)
    assert np.abs(s - np.fft.fftn(x)).max() <= 64 * EPS * np.abs(x).sum()
    f = A.dft_matrix(96)
    assert np.abs(f @ np.conj(f).T - 96 * np.eye(96)).max() <= 1e-11


# ---- host plan ----------------------------------------------------------------------------------------------------------

def _queue(n=4, lo=0.0, transform=None, **kw):
    g = torch.Generator().manual_seed(0)
    subs = [{"bssfp": {"data": torch.rand(24, 3, 3, 3, generator=g) + lo},
             "dwi-tensor": {"data": torch.rand(6, 3, 3, 3, generator=g) + lo}} for _ in range(n)]
    kw.setdefault("target_shape", (3, 3, 3))
    kw.setdefault("sampler", Q.UniformSampler(2))
    return Q.PatchQueue(subs, "bssfp", transform=transform, **kw)


def _with_p(p):
    tr = A.reference_training_transform()
    for t, pi in zip(tr, p if isinstance(p, (list, tuple)) else [p] * len(tr)):
        t.p = pi
    return tr


def test_reference_training_transform_lists_the_six_built_stages():
    tr = A.reference_training_transform()
    assert [type(t) for t in tr] == [A.RandomGhosting, A.RandomSpike, A.RandomBiasField, A.RandomBlur, A.RandomNoise, A.RandomGamma]
    assert all(t.p == 0.1 for t in tr)
    assert tr[1].intensity_range == (0.01, 0.1) and tr[1].num_spikes_range == (1, 1)
    assert tr[3].std_range == (0.01, 0.1) and tr[4].std_range == (0.01, 0.1)
    assert tr[0].num_ghosts_range == (4, 10) and tr[0].axes == (0, 1, 2) and tr[0].intensity_range == (0.5, 1.0)
    assert tr[0].restore == 0.02
    assert "RandomMotion" in A.reference_training_transform.__doc__
    assert [type(t) for t in A.reference_augmentation()] == [A.RandomBiasField, A.RandomNoise, A.RandomGamma]
    assert A.RandomSpike().intensity_range == (1.0, 3.0) and A.RandomSpike(intensity=2).intensity_range == (-2.0, 2.0)
    assert A.RandomSpike(num_spikes=3).num_spikes_range == (3, 3) and A.RandomBlur().std_range == (0.0, 2.0)


def test_six_stages_fire_at_rate_p_and_replay_from_the_recorded_seed():
    q = _queue(2, transform=_with_p(1.0), max_length=1, samples_per_volume=1)
    for pl in q.next_plan(20):
        assert [type(t) for t, _ in pl.load.stages] == [type(t) for t in q.transform]
    q = _queue(2, transform=_with_p(0.0), max_length=1, samples_per_volume=1)
    assert all(pl.load.stages == () for pl in q.next_plan(20))
    q = _queue(2, transform=A.reference_training_transform(), max_length=1, samples_per_volume=1, seed=3)
    loads = [pl.load for pl in q.next_plan(3000)]
    tol = 4.5 * np.sqrt(0.1 * 0.9 / 3000)
    for t in q.transform:
        rate = np.mean([any(s[0] is t for s in l.stages) for l in loads])
        assert abs(rate - 0.1) < tol, (type(t).__name__, rate)
    fired = 0
    for load in loads[:600]:
        torch.manual_seed(load.seed)                                  # the chain: _Random.__call__ for every transform
        want = [(t, t.sample()) for t in q.transform if torch.rand(1).item() < t.p]
        assert [t for t, _ in load.stages] == [t for t, _ in want]
        for (t, got), (_, exp) in zip(load.stages, want):
            if isinstance(t, A.RandomSpike):
                assert got.intensity == exp.intensity and np.array_equal(got.positions, exp.positions)
                assert exp.path is None and got.path in ("dc", "dft")
            elif isinstance(exp, np.ndarray):
                assert np.array_equal(got, exp)
            else:
                assert got == exp
        fired += len(want)
    assert fired > 100


def test_sample_consumes_draws_in_the_documented_order():
    gh = A.RandomGhosting(num_ghosts=(4, 10), axes=(2, 0), intensity=(0.5, 1))
    torch.manual_seed(7)
    got = gh.sample()
    torch.manual_seed(7)
    n = int(torch.randint(4, 11, (1,)).item())
    axis = (2, 0)[int(torch.randint(0, 2, (1,)).item())]
    assert got == (n, axis, torch.rand(1).item() * 0.5 + 0.5)
    assert 4 <= got[0] <= 10 and got[1] in (2, 0) and 0.5 <= got[2] <= 1.0
    sp = A.RandomSpike(num_spikes=(1, 3), intensity=(0.01, 0.1))
    torch.manual_seed(8)
    got = sp.sample()
    torch.manual_seed(8)
    k = int(torch.randint(1, 4, (1,)).item())
    intensity = torch.rand(1).item() * (0.1 - 0.01) + 0.01
    assert got.intensity == intensity and got.path is None
    assert np.array_equal(got.positions, torch.rand(k, 3).numpy().astype(np.float64)) and got.positions.shape == (k, 3)
    bl = A.RandomBlur(std=(0.5, 2))
    torch.manual_seed(9)
    got = bl.sample()
    torch.manual_seed(9)
    assert got == tuple(float(v) for v in torch.rand(3) * 1.5 + 0.5) and len(got) == 3
    for _ in range(200):                                              # the reference's range never leaves radius 0
        assert not A.RandomBlur.has_effect(A.RandomBlur(std=(0.01, 0.1)).sample())


def test_static_spike_path_rule():
    gh, sp, bias, blur, noise, gamma = A.reference_training_transform()
    q = _queue(3, transform=[gh, sp, bias, blur, noise, gamma])
    assert q.nonnegative == {0: True, 1: True, 2: True}
    s = lambda t: (t, None)
    assert q.spike_path(0, []) == "dc"
    assert q.spike_path(0, [s(bias), s(gamma), s(blur)]) == "dc"
    assert q.spike_path(0, [s(gh)]) == "dft" and q.spike_path(0, [s(bias), s(noise)]) == "dft"
    assert _queue(2, lo=-0.5, transform=[sp]).spike_path(0, []) == "dft"              # a negative raw minimum
    assert _queue(2, transform=[sp], target_shape=(3, 4, 3), padding_value=-1.0).spike_path(0, []) == "dft"
    assert _queue(2, transform=[sp], target_shape=(3, 4, 3), padding_value=0.0).spike_path(0, []) == "dc"
    # in the plan: the order of the transform list decides what runs before the spike
    for order, want in (([bias, gamma, blur, sp], "dc"), ([noise, sp], "dft"), ([gh, sp], "dft"), ([sp, gh, noise], "dc")):
        for t in order:
            t.p = 1.0
        q = _queue(2, transform=order)
        for pl in q.next_plan(6):
            path = [p.path for t, p in pl.load.stages if t is sp]
            assert path == [want], (order, path)
    assert _queue(2, transform=[bias]).nonnegative == {}              # no spike: the minima are never read


def test_split_stages_stages_up_to_the_last_non_local_stage_with_an_effect():
    gh, sp, bias, blur, noise, gamma = A.reference_training_transform()
    coef = np.zeros(20, np.float32)
    spike = A.SpikeParams(0.05, np.array([[0.1, 0.2, 0.3]]), "dc")
    stages = ((gh, (5, 1, 0.7)), (sp, spike), (bias, coef), (blur, (0.1, 0.05, 0.1)), (noise, (0.0, 0.05, 1)), (gamma, 1.1))
    staged, fused = Q.PatchQueue.split_stages(Q.SubjectLoad(0, 0, 0, 0, stages))
    assert [t for t, _ in staged] == [gh, sp] and [t for t, _ in fused] == [bias, noise, gamma]   # blur: identity, dropped
    stages = stages[:3] + ((blur, (0.1, 0.3, 0.1)),) + stages[4:]
    staged, fused = Q.PatchQueue.split_stages(Q.SubjectLoad(0, 0, 0, 0, stages))
    assert [t for t, _ in staged] == [gh, sp, bias, blur] and [t for t, _ in fused] == [noise, gamma]
    staged, fused = Q.PatchQueue.split_stages(Q.SubjectLoad(0, 0, 0, 0, ((bias, coef), (blur, (0.1, 0.1, 0.1)), (gamma, 1.1))))
    assert staged == () and [t for t, _ in fused] == [bias, gamma]                               # nothing is staged


def test_foreign_classes_still_raise_type_error():
    class RandomBlur(A._Random):
        pass
    with pytest.raises(TypeError):
        _queue(2, transform=[A.RandomNoise(), RandomBlur()])
    with pytest.raises(TypeError):
        _queue(2, transform=[A.RandomBlur(), A.RandomBlur()])
    _queue(2, transform=[A.RandomBlur(), A.RandomGhosting(), A.RandomSpike()])
    with pytest.raises(ValueError):
        A.RandomGhosting(axes=(3,))


def test_what_a_staged_stage_cannot_do_is_refused_at_construction():
    big = dict(target_shape=(3, 3, 130), sampler=Q.UniformSampler(2))
    with pytest.raises(ValueError, match="exceeds 128"):
        _queue(2, transform=[A.RandomGhosting()], **big)
    _queue(2, transform=[A.RandomGhosting(axes=(0, 1))], **big)                      # never works along W
    with pytest.raises(ValueError, match="exceeds 128"):
        _queue(2, transform=[A.RandomBlur()], **big)
    _queue(2, transform=[A.RandomBlur(std=(0.01, 0.1))], **big)                      # radius 0: no pass at all
    _queue(2, transform=[A.RandomBiasField(), A.RandomSpike()], **big)               # always the DC shortcut
    with pytest.raises(ValueError, match="exceeds 128"):
        _queue(2, transform=[A.RandomNoise(), A.RandomSpike()], **big)
    with pytest.raises(ValueError, match="exceeds 128"):
        _queue(2, lo=-0.5, transform=[A.RandomSpike()], **big)
    _queue(2, transform=A.reference_training_transform(), target_shape=(3, 128, 128))
    with pytest.raises(ValueError, match="more than one spike"):
        _queue(2, transform=[A.RandomSpike(num_spikes=(1, 3))])
    _queue(2, transform=[A.RandomSpike(num_spikes=(0, 1))])
    with pytest.raises(_lib_error()):
        A.RandomBlur(std=(1, 2))(torch.zeros(1, 4, 4, 4))             # GPU only, like the others


def _lib_error():
    from unet_bssfp_amd import _lib
    return _lib.Mi355Error


def test_kspace_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """every shipped instantiation of csrc/kspace.hip: 0 bytes of scratch, no spilled register, at most 64 KB of LDS"""
    import os
    import re
    import subprocess
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unet_bssfp_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "kspace.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-Wno-unused-function",
                    "-Wno-unused-variable", os.path.join(csrc, "kspace.hip"), "-o", str(out)], check=True, capture_output=True)
    isa = out.read_text()
    names = re.findall(r"\.name:\s+(\S*kernel\S*)", isa)
    assert sum("axis_apply_kernel" in n for n in names) == 7 and any("spike_add_kernel" in n for n in names)
    scratch = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", isa)]
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", isa)]
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", isa)]
    assert len(scratch) == len(names) and set(scratch) == {0} and set(spills) == {0}
    assert max(lds) <= 65536
