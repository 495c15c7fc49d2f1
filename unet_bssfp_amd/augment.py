"""GPU-side intensity augmentations -- SURVEY.md 8(f) rank 4 (augmentation part).

``RandomBiasField``, ``RandomNoise`` and ``RandomGamma`` with TorchIO's constructor arguments and sampling rules
(the three cheap, image-space members of the reference's training transform, src/data_module.py:130-139), applied
to device tensors of shape (C, D, H, W) so that the input pipeline can keep up with a GPU that trains > 60 volumes
per second.  Random parameters are drawn with torch's CPU generator like TorchIO does; the voxel noise comes from a
counter-based hash on the device.
TorchIO is absent: behaviour restated from its published algorithm (oracle/augment_ref.py, parity unpinned).

``RandomGhosting``, ``RandomSpike`` and ``RandomBlur`` need no FFT on the device: each reduces to a small
dense matrix applied along one axis of the volume (``axis_apply``, csrc/kspace.hip).  The reductions are this project's
reading of TorchIO 0.19.6 and are normative here; parity with TorchIO itself is **unpinned** like the rest.  The matrix
builders (``ghosting_matrix``, ``blur_matrix``, ``dft_matrix``, ``spike_frequencies``, ``spike_closed_form``) are plain
f64 host functions; a matrix is rounded to f32 once, when it is uploaded.  Blur takes the voxel spacing as 1 (the
project's subjects carry no affine).  Only RandomMotion (a rigid resampler) is not built.
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib

Range = Union[float, Tuple[float, float]]


def _range(v: Range, symmetric: bool) -> Tuple[float, float]:
    if isinstance(v, (int, float)):
        return (-float(v), float(v)) if symmetric else (0.0, float(v))
    lo, hi = v
    return float(lo), float(hi)


def _check(x: torch.Tensor):
    if not x.is_cuda:
        raise _lib.Mi355Error("augmentations run on the GPU only (no CPU fallback)")
    if x.dim() != 4:
        raise ValueError(f"expected (C, D, H, W), got {tuple(x.shape)}")
    return x.float().contiguous()


class _Random:
    def __init__(self, p: float = 1.0):
        self.p = float(p)

    def __call__(self, subject):
        """subject: a (C, D, H, W) tensor or ``{name: {'data': tensor}}`` -- like TorchIO, ONE set of random
        parameters per call, applied to every image of the subject."""
        if torch.rand(1).item() >= self.p:
            return subject
        params = self.sample()
        if isinstance(subject, torch.Tensor):
            return self.apply(subject, params)
        return {k: ({**v, "data": self.apply(v["data"], params)} if isinstance(v, dict) and "data" in v else v)
                for k, v in subject.items()}


class RandomBiasField(_Random):
    def __init__(self, coefficients: Range = 0.5, order: int = 3, p: float = 1.0):
        super().__init__(p)
        if not 0 <= order <= 4:
            raise ValueError("order must be in 0..4")
        self.coefficients_range, self.order = _range(coefficients, True), int(order)

    def sample(self):
        n = (self.order + 1) * (self.order + 2) * (self.order + 3) // 6
        lo, hi = self.coefficients_range
        return (torch.rand(n) * (hi - lo) + lo).numpy().astype(np.float32)

    def apply(self, x, coefficients):
        x = _check(x)
        out = torch.empty_like(x)
        coefficients = np.ascontiguousarray(coefficients, dtype=np.float32)
        _lib.check(_lib.load().mi355_aug_bias_field(x.data_ptr(), out.data_ptr(), *x.shape, coefficients.ctypes.data, self.order,
                                                    torch.cuda.current_stream().cuda_stream), "aug_bias_field")
        return out


class RandomGamma(_Random):
    def __init__(self, log_gamma: Range = (-0.3, 0.3), p: float = 1.0):
        super().__init__(p)
        self.log_gamma_range = _range(log_gamma, True)

    def sample(self):
        lo, hi = self.log_gamma_range
        return math.exp(torch.rand(1).item() * (hi - lo) + lo)

    def apply(self, x, gamma):
        x = _check(x)
        out = torch.empty_like(x)
        _lib.check(_lib.load().mi355_aug_gamma(x.data_ptr(), out.data_ptr(), x.numel(), float(gamma),
                                               torch.cuda.current_stream().cuda_stream), "aug_gamma")
        return out


class RandomNoise(_Random):
    def __init__(self, mean: Range = 0.0, std: Range = (0, 0.25), p: float = 1.0):
        super().__init__(p)
        self.mean_range, self.std_range = _range(mean, True), _range(std, False)

    def sample(self):
        (ml, mh), (sl, sh) = self.mean_range, self.std_range
        return (torch.rand(1).item() * (mh - ml) + ml, torch.rand(1).item() * (sh - sl) + sl,
                int(torch.randint(0, 2 ** 62, (1,)).item()))

    def apply(self, x, params):
        mean, std, seed = params
        x = _check(x)
        out = torch.empty_like(x)
        _lib.check(_lib.load().mi355_aug_noise(x.data_ptr(), out.data_ptr(), x.numel(), float(mean), float(std), int(seed),
                                               torch.cuda.current_stream().cuda_stream), "aug_noise")
        return out


# ---- k-space and blur stages: host mathematics (f64) ------------------------------------------------------------------

def _phase_matrix(n: int) -> np.ndarray:
    """2 pi (k j mod n) / n for k, j in 0..n-1, the product reduced exactly in integers"""
    k = np.arange(n, dtype=np.int64)
    return (2.0 * np.pi / n) * ((k[:, None] * k[None, :]) % n).astype(np.float64)


def dft_matrix(n_axis: int) -> np.ndarray:
    """the forward DFT along one axis as a complex128 (N, N) matrix: ``F[k][j] = exp(-2 pi i k j / N)`` (numpy's ``fft``
    convention, unshifted; the maximum RandomSpike needs does not depend on the order of the bins)"""
    ph = _phase_matrix(int(n_axis))
    return np.cos(ph) - 1j * np.sin(ph)


def ghosting_matrix(n_axis: int, num_ghosts: int, intensity: float) -> Optional[np.ndarray]:
    """RandomGhosting along one axis as a real f64 (N, N) circulant ``G[i][j] = g[(i - j) mod N]``.

    TorchIO: the planes ``s[::num_ghosts]`` of the shifted spectrum along the axis are multiplied by ``1 - intensity``,
    then the centre plane ``N // 2`` is restored.  The mask depends on the index along the axis only, so the other two
    transforms cancel, and the input is real, so ``real(x (*) h) = x (*) real(h)``: ``g = real(ifft(ifftshift(m)))``.
    ``None`` = the identity (``num_ghosts == 0`` or ``intensity == 0``): the stage returns its input."""
    n, k = int(n_axis), int(num_ghosts)
    if k == 0 or intensity == 0:
        return None
    m = np.ones(n, dtype=np.float64)
    m[::k] = 1.0 - float(intensity)
    m[n // 2] = 1.0
    mu = np.roll(m, -(n // 2))                      # ifftshift: bin N // 2 (DC of the shifted order) goes to 0
    g = np.cos(_phase_matrix(n)) @ mu / n           # real part of the inverse DFT
    i = np.arange(n)
    return g[(i[:, None] - i[None, :]) % n]


def blur_radius(sigma: float) -> int:
    """scipy.ndimage.gaussian_filter's kernel radius (truncate = 4): 0 for sigma <= 0.124"""
    return int(4.0 * float(sigma) + 0.5)


def blur_matrix(n_axis: int, sigma: float) -> Optional[np.ndarray]:
    """``scipy.ndimage.gaussian_filter1d(x, sigma)`` (mode 'reflect': d c b a | a b c d | d c b a) along one axis as a
    banded real f64 (N, N) matrix with the reflection folded into its border rows.  ``None`` = radius 0: the axis is
    skipped (the filter is the identity there, bit for bit)."""
    n, r = int(n_axis), blur_radius(sigma)
    if r == 0:
        return None
    t = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * t.astype(np.float64) ** 2)
    w /= w.sum()
    b = np.zeros((n, n), dtype=np.float64)
    p = (np.arange(n)[:, None] + t[None, :]) % (2 * n)     # reflection of period 2 N, as often as the radius needs
    np.add.at(b, (np.broadcast_to(np.arange(n)[:, None], p.shape), np.where(p < n, p, 2 * n - 1 - p)),
              np.broadcast_to(w[None, :], p.shape))
    return b


def spike_frequencies(position: Sequence[float], shape: Sequence[int]) -> Tuple[int, int, int]:
    """the bin a spike hits, as signed frequencies: ``idx = floor(position * shape)`` in the shifted spectrum,
    ``f = idx - N // 2``"""
    return tuple(int(math.floor(float(p) * int(n))) - int(n) // 2 for p, n in zip(position, shape))


def spectrum_max(x: np.ndarray) -> complex:
    """``M`` of RandomSpike for one real f64 channel: the complex maximum of its 3-D DFT, defined as
    ``max_k Re X(k) + i |Im X(k*)|`` at the arg-max (the spectrum of a real volume comes in conjugate pairs, so numpy's
    lexicographic maximum has Im >= 0; taking |Im| keeps rounding from picking the other member).  ``sum(x)`` when the
    channel has no negative voxel (Re X(k) <= sum |x| = X(0)), otherwise three dense passes of ``dft_matrix`` along
    W, H, D."""
    x = np.asarray(x, dtype=np.float64)
    if x.min() >= 0:
        return complex(x.sum(), 0.0)
    s = x.astype(np.complex128)
    for ax in (2, 1, 0):
        s = np.moveaxis(np.tensordot(dft_matrix(x.shape[ax]), s, axes=([1], [ax])), 0, ax)
    re = s.real.max()
    return complex(re, np.abs(s.imag[s.real == re]).max())


def spike_closed_form(x: np.ndarray, positions, intensity: float):
    """RandomSpike on one real channel without an inverse transform, f64.  Adding ``a`` to one bin adds a plane wave:
    ``y[n] = x[n] + real(a exp(+2 pi i sum_d f_d n_d / N_d)) / (N0 N1 N2)``, ``a = M * intensity``, ``M`` the complex
    maximum of the CURRENT spectrum: the lexicographic maximum of ``spectrum_max(x)`` and the current values of the bins
    already hit (one single-bin DFT each).  That holds while ``Re M0 > 0``; ``ValueError`` otherwise.
    -> (y, [a_1, ..., a_k])"""
    x = np.asarray(x, dtype=np.float64)
    grids = np.meshgrid(*[np.arange(n, dtype=np.int64) for n in x.shape], indexing="ij")
    m0 = spectrum_max(x)
    cur: Dict[Tuple[int, int, int], complex] = {}
    y, amps = x.copy(), []
    for pos in np.asarray(positions, dtype=np.float64).reshape(-1, 3):
        f = spike_frequencies(pos, x.shape)
        if cur and not m0.real > 0:
            raise ValueError("several spikes need a spectrum whose maximum has a positive real part")
        a = max([m0] + list(cur.values()), key=lambda v: (v.real, v.imag)) * float(intensity)
        phase = sum((2.0 * np.pi / n) * ((fd * g) % n) for fd, g, n in zip(f, grids, x.shape))
        cs, sn = np.cos(phase), np.sin(phase)
        if f not in cur:
            cur[f] = complex((x * cs).sum(), -(x * sn).sum())        # X(f), one weighted sum
        cur[f] += a
        amps.append(a)
        y += (a.real * cs - a.imag * sn) / x.size
    return y, amps


# ---- k-space and blur stages: device side ----------------------------------------------------------------------------

AXIS_MAX_N = 128   # MI355_AXIS_MAX_N: the largest extent along an axis that axis_apply takes (larger ones are not tiled)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _upload(a: np.ndarray, device) -> torch.Tensor:
    """f64 host matrix -> f32 device tensor (the one rounding), through pinned memory so that the copy never
    synchronises the host"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.pin_memory().to(device, non_blocking=True)


def axis_apply(x: torch.Tensor, matrix, axis: int) -> torch.Tensor:
    """``out[c][..i..] = sum_j matrix[i][j] x[c][..j..]`` along spatial axis 0 (D), 1 (H) or 2 (W) of a (C, D, H, W)
    device tensor; ``matrix``: an (N, N) host array or an f32 device tensor.  Extents above 128 raise."""
    x = _check(x)
    n = x.shape[1 + axis]
    m = matrix if isinstance(matrix, torch.Tensor) else _upload(matrix, x.device)
    if tuple(m.shape) != (n, n) or m.dtype != torch.float32 or m.device != x.device or not m.is_contiguous():
        raise ValueError(f"need a contiguous float32 ({n}, {n}) matrix on {x.device}, got {m.dtype} {tuple(m.shape)}")
    out = torch.empty_like(x)
    _lib.check(_lib.load().mi355_axis_apply(x.data_ptr(), m.data_ptr(), out.data_ptr(), *x.shape, int(axis), _stream()),
               "axis_apply")
    return out


# the DFT matrices of the extents seen so far, per device, uploaded once and kept for the life of the process (two f32
# N x N planes each, 128 KB at N = 128): a spike on the DFT path would otherwise rebuild and upload three of them per load
_DFT_ON_DEVICE: Dict[tuple, Tuple[torch.Tensor, torch.Tensor]] = {}


def _dft_planes(n: int, device):
    key = (int(n), str(device))
    if key not in _DFT_ON_DEVICE:
        f = dft_matrix(n)
        _DFT_ON_DEVICE[key] = (_upload(f.real, device), _upload(f.imag, device))
    return _DFT_ON_DEVICE[key]


def _workspace(x: torch.Tensor) -> torch.Tensor:
    nbytes = _lib.load().mi355_kspace_workspace_bytes(*x.shape)
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device)


def channel_sum_min(x: torch.Tensor) -> torch.Tensor:
    """(C, 2) f64 on the device: (sum, min) per channel, accumulated in f64"""
    x = _check(x)
    ws, out = _workspace(x), torch.empty(x.shape[0], 2, dtype=torch.float64, device=x.device)
    _lib.check(_lib.load().mi355_channel_sum_min(x.data_ptr(), x.shape[0], x[0].numel(), ws.data_ptr(), ws.numel() * 8,
                                                 out.data_ptr(), _stream()), "channel_sum_min")
    return out


def spectrum_max_device(x: torch.Tensor) -> torch.Tensor:
    """(C, 2) f64 on the device: ``spectrum_max`` per channel through three dense DFT passes along W, H, D in f32, the
    last of which reduces to (max Re, |Im| at it) instead of writing a volume"""
    x = _check(x)
    lib, shape = _lib.load(), tuple(x.shape)
    re, im = None, None
    for axis in (2, 1):
        mr, mi = _dft_planes(shape[1 + axis], x.device)
        outr, outi = torch.empty_like(x), torch.empty_like(x)
        _lib.check(lib.mi355_axis_apply_complex((x if re is None else re).data_ptr(), None if im is None else im.data_ptr(),
                                                mr.data_ptr(), mi.data_ptr(), outr.data_ptr(), outi.data_ptr(), *shape,
                                                axis, _stream()), "axis_apply_complex")
        re, im = outr, outi
    mr, mi = _dft_planes(shape[1], x.device)
    ws, out = _workspace(x), torch.empty(shape[0], 2, dtype=torch.float64, device=x.device)
    _lib.check(lib.mi355_axis_apply_complex_max(re.data_ptr(), im.data_ptr(), mr.data_ptr(), mi.data_ptr(), *shape,
                                                ws.data_ptr(), ws.numel() * 8, out.data_ptr(), _stream()),
               "axis_apply_complex_max")
    return out


class RandomGhosting(_Random):
    """``tio.RandomGhosting``: a real circular convolution along one axis (``ghosting_matrix``).  ``restore`` is accepted
    and stored; as in TorchIO 0.19 only the single centre plane is restored.  params = (num_ghosts, axis, intensity)."""

    def __init__(self, num_ghosts: Union[int, Tuple[int, int]] = (4, 10), axes: Union[int, Tuple[int, ...]] = (0, 1, 2),
                 intensity: Range = (0.5, 1), restore: float = 0.02, p: float = 1.0):
        super().__init__(p)
        self.num_ghosts_range = (int(num_ghosts),) * 2 if isinstance(num_ghosts, int) else tuple(int(v) for v in num_ghosts)
        self.axes = (int(axes),) if isinstance(axes, int) else tuple(int(a) for a in axes)
        if not self.axes or any(a not in (0, 1, 2) for a in self.axes):
            raise ValueError(f"axes must be among 0, 1, 2, got {axes}")
        if self.num_ghosts_range[0] < 0 or self.num_ghosts_range[0] > self.num_ghosts_range[1]:
            raise ValueError(f"bad num_ghosts range {num_ghosts}")
        self.intensity_range, self.restore = _range(intensity, False), float(restore)

    def sample(self):
        lo, hi = self.num_ghosts_range
        n = int(torch.randint(lo, hi + 1, (1,)).item())
        axis = self.axes[int(torch.randint(0, len(self.axes), (1,)).item())]
        il, ih = self.intensity_range
        return n, axis, torch.rand(1).item() * (ih - il) + il

    @staticmethod
    def has_effect(params) -> bool:
        return params[0] != 0 and params[2] != 0

    def apply(self, x, params):
        n, axis, intensity = params
        x = _check(x)
        g = ghosting_matrix(x.shape[1 + axis], n, intensity)
        return x if g is None else axis_apply(x, g, axis)


class SpikeParams(NamedTuple):
    """``path``: 'dc' (every channel is known to be non-negative: M = sum(x)), 'dft' (three DFT passes) or None: decide
    from the data, which synchronises once"""
    intensity: float
    positions: np.ndarray          # (k, 3) in [0, 1)
    path: Optional[str] = None


class RandomSpike(_Random):
    """``tio.RandomSpike``: each spike adds ``M * intensity`` to one bin of the spectrum, i.e. a plane wave to the volume
    (``spike_closed_form``); ``M`` comes from ``channel_sum_min`` (non-negative channels) or ``spectrum_max_device``.
    One spike per call is built on the device (the reference's ``num_spikes=1``); more raise."""

    def __init__(self, num_spikes: Union[int, Tuple[int, int]] = 1, intensity: Range = (1, 3), p: float = 1.0):
        super().__init__(p)
        self.num_spikes_range = (int(num_spikes),) * 2 if isinstance(num_spikes, int) else tuple(int(v) for v in num_spikes)
        if self.num_spikes_range[0] < 0 or self.num_spikes_range[0] > self.num_spikes_range[1]:
            raise ValueError(f"bad num_spikes range {num_spikes}")
        self.intensity_range = _range(intensity, True)

    def sample(self) -> SpikeParams:
        lo, hi = self.num_spikes_range
        k = int(torch.randint(lo, hi + 1, (1,)).item())
        il, ih = self.intensity_range
        intensity = torch.rand(1).item() * (ih - il) + il
        return SpikeParams(intensity, torch.rand(k, 3).numpy().astype(np.float64))

    @staticmethod
    def has_effect(params) -> bool:
        return len(params[1]) > 0 and params[0] != 0

    def apply(self, x, params):
        params = SpikeParams(*params)
        x = _check(x)
        if not self.has_effect(params):
            return x
        if len(params.positions) != 1:
            raise _lib.Mi355Error("RandomSpike with more than one spike per call is not built on the device")
        path, m = params.path, None
        if path != "dft":
            m = channel_sum_min(x)
            if path is None:
                path = "dc" if bool((m[:, 1] >= 0).all().item()) else "dft"
        if path == "dft":
            m = spectrum_max_device(x)
        elif path != "dc":
            raise ValueError(f"spike path must be 'dc', 'dft' or None, got {path!r}")
        f = spike_frequencies(params.positions[0], x.shape[1:])
        out = torch.empty_like(x)
        _lib.check(_lib.load().mi355_aug_spike_add(x.data_ptr(), out.data_ptr(), *x.shape, *f, m.data_ptr(),
                                                   int(path == "dc"), float(params.intensity), _stream()), "aug_spike_add")
        return out


class RandomBlur(_Random):
    """``tio.RandomBlur``: ``scipy.ndimage.gaussian_filter`` with one sigma per axis (voxel spacing 1), a banded matrix per
    axis (``blur_matrix``).  An axis whose radius is 0 is skipped, so with the reference's ``std=(0.01, 0.1)`` the stage
    returns its input and launches nothing.  params = (sigma_D, sigma_H, sigma_W)."""

    def __init__(self, std: Range = (0, 2), p: float = 1.0):
        super().__init__(p)
        self.std_range = _range(std, False)
        if self.std_range[0] < 0 or self.std_range[0] > self.std_range[1]:
            raise ValueError(f"bad std range {std}")

    def sample(self):
        lo, hi = self.std_range
        return tuple(float(v) for v in (torch.rand(3) * (hi - lo) + lo))

    @staticmethod
    def has_effect(params) -> bool:
        return any(blur_radius(s) > 0 for s in params)

    def apply(self, x, sigmas):
        x = _check(x)
        for axis, sigma in enumerate(sigmas):
            b = blur_matrix(x.shape[1 + axis], sigma)
            if b is not None:
                x = axis_apply(x, b, axis)
        return x


def crop_or_pad(x: torch.Tensor, target: Sequence[int], padding_value: float = 0.0) -> torch.Tensor:
    """``tio.CropOrPad(target, 0)`` (src/data_module.py:125-128): centred crop / constant pad of (C, D, H, W)."""
    out = x
    for ax, t in enumerate(target, start=1):
        n = out.shape[ax]
        if n > t:
            lo = (n - t) // 2
            out = out.narrow(ax, lo, t)
        elif n < t:
            lo = (t - n) // 2
            pad = [0, 0] * (out.dim() - 1 - ax) + [lo, t - n - lo]
            out = torch.nn.functional.pad(out, pad, value=padding_value)
    return out.contiguous()


def reference_augmentation() -> list:
    """the image-space members of src/data_module.py:131-139 that are built, with the reference's arguments"""
    return [RandomBiasField(p=0.1), RandomNoise(p=0.1, std=(0.01, 0.1)), RandomGamma(p=0.1)]


def reference_training_transform() -> list:
    """the reference's training transform, src/data_module.py:131-139, in its order and with its arguments -- the six
    members that are built.  The seventh, RandomMotion (first in the reference's list), is missing: it needs a rigid
    resampler."""
    return [RandomGhosting(p=0.1), RandomSpike(p=0.1, intensity=(0.01, 0.1)), RandomBiasField(p=0.1),
            RandomBlur(p=0.1, std=(0.01, 0.1)), RandomNoise(p=0.1, std=(0.01, 0.1)), RandomGamma(p=0.1)]
