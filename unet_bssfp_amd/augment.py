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
project's subjects carry no affine).

``RandomMotion``, the first stage of the reference's list, needs no FFT either: the band composite of
the K + 1 moved copies is ``sum_k C_k x_k`` with real circulants along the last axis, and one launch fuses the rigid
trilinear resampler (``rigid_resample`` on its own) with that sum (csrc/motion.hip).  ``reference_full_transform()``
lists all seven stages.
"""
from __future__ import annotations

import ctypes as C
import functools
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
    per_image = False       # one parameter set per call for every image of the subject (RandomMotion: one per image)

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


# ---- motion: host mathematics (f64) ------------------------------------------------------------------------------------

def _hat(v: np.ndarray) -> np.ndarray:
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def _se3_log(m: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """the principal logarithm of a rigid 4 x 4 matrix in closed form: (omega, v) with ``logm(M) = [[hat(omega), v], [0, 0]]``,
    ``v = V^-1 t``.  The unit axis k = omega / theta keeps every coefficient free of a division by theta^2; the identity and
    pure translations (theta = 0: not diagonalisable) take the first-order branch, which is exact to theta^2."""
    r, t = m[:3, :3], m[:3, 3]
    s = 0.5 * np.array([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]])     # sin(theta) k
    sin_t, cos_t = float(np.linalg.norm(s)), 0.5 * (float(np.trace(r)) - 1.0)
    if cos_t < -0.99:
        raise ValueError("a rotation within 8 degrees of a half turn has no stable principal logarithm")
    theta = math.atan2(sin_t, cos_t)
    if theta < 1e-8:
        return s, t - 0.5 * np.cross(s, t)
    k = _hat(s / sin_t)
    half = 0.5 * theta
    v_inv = np.eye(3) - half * k + (1.0 - half * math.cos(half) / math.sin(half)) * (k @ k)
    return theta * s / sin_t, v_inv @ t


def _se3_exp(omega: np.ndarray, v: np.ndarray) -> np.ndarray:
    """``expm([[hat(omega), v], [0, 0]])`` in closed form (Rodrigues; ``t = V v``)"""
    theta = float(np.linalg.norm(omega))
    out = np.eye(4)
    if theta < 1e-8:
        out[:3, :3] += _hat(omega)
        out[:3, 3] = v + 0.5 * np.cross(omega, v)
        return out
    k = _hat(omega / theta)
    kk = k @ k
    versine = 2.0 * math.sin(0.5 * theta) ** 2                      # 1 - cos(theta) without the cancellation
    out[:3, :3] += math.sin(theta) * k + versine * kk
    out[:3, 3] = (np.eye(3) + (versine / theta) * k + (1.0 - math.sin(theta) / theta) * kk) @ v
    return out


def euler_index_matrix(degrees: Sequence[float], translation: Sequence[float], shape: Sequence[int]) -> np.ndarray:
    """ITK's ``Euler3DTransform`` in index space (spacing 1, physical point = voxel index) as a 4 x 4 f64 matrix:
    ``p_in = R (p_out - c) + c + t``, ``R = Rz Rx Ry`` (ITK's default order), centre ``c = shape / 2``"""
    ax, ay, az = (math.radians(float(d)) for d in degrees)
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    r = rz @ rx @ ry
    c = 0.5 * np.asarray(shape, dtype=np.float64)
    m = np.eye(4)
    m[:3, :3] = r
    m[:3, 3] = c + np.asarray(translation, dtype=np.float64) - r @ c
    return m


def motion_matrices(degrees, translation, shape: Sequence[int]) -> np.ndarray:
    """RandomMotion's transforms as (K + 1, 4, 4) f64 index-space matrices (output voxel ``i`` reads the input at
    ``M i``): the identity and the K Euler draws (``degrees``, ``translation``: (K, 3)), demeaned as TorchIO does,
    ``mean = expm(mean_k logm(M_k))``, ``M_k <- inv(mean) M_k``.  The logarithm and exponential are the closed SE(3) forms."""
    degrees = np.asarray(degrees, dtype=np.float64).reshape(-1, 3)
    translation = np.asarray(translation, dtype=np.float64).reshape(-1, 3)
    if len(degrees) != len(translation):
        raise ValueError(f"{len(degrees)} rotations for {len(translation)} translations")
    ms = [np.eye(4)] + [euler_index_matrix(d, t, shape) for d, t in zip(degrees, translation)]
    logs = [_se3_log(m) for m in ms]
    mean = _se3_exp(np.mean([w for w, _ in logs], axis=0), np.mean([v for _, v in logs], axis=0))
    inv = np.eye(4)
    inv[:3, :3] = mean[:3, :3].T
    inv[:3, 3] = -mean[:3, :3].T @ mean[:3, 3]
    return np.stack([inv @ m for m in ms])


def motion_bands(times, n_axis: int) -> list:
    """which image owns which bins of the shifted spectrum along the last axis: ``[(image, first, last), ...]``, bins
    ``[first, last)``.  TorchIO: ``idx = (N * times).astype(int)`` with N appended; ``sort_spectra`` swaps image 0 (the
    identity before demeaning) with image ``j``, ``j`` the first index with ``times[j] > 0.5``, else K, so that it fills
    the centre of k-space; then the image at position k owns ``[idx[k - 1], idx[k])``.  Empty bands are dropped."""
    times = np.asarray(times)
    n, k = int(n_axis), len(times)
    order = list(range(k + 1))
    above = np.nonzero(times > 0.5)[0]
    j = int(above.min()) if len(above) else k
    order[0], order[j] = order[j], order[0]
    idx = (n * times).astype(int).tolist() + [n]
    bands, ini = [], 0
    for image, fin in zip(order, idx):
        if fin > ini:
            bands.append((image, ini, fin))
        ini = fin
    return bands


@functools.lru_cache(maxsize=8)
def _cos_phase(n: int) -> np.ndarray:
    """cos(_phase_matrix(n)), kept per extent: RandomMotion builds K + 1 band matrices per call from it"""
    c = np.cos(_phase_matrix(n))
    c.setflags(write=False)
    return c


def motion_band_matrix(n_axis: int, first: int, last: int) -> np.ndarray:
    """keeping the bins ``[first, last)`` of the shifted spectrum along one axis of a real volume and taking the real part
    of the inverse, as a real f64 (N, N) circulant ``C[i][j] = g[(i - j) mod N]``, ``g = real(ifft(ifftshift(b)))``"""
    n = int(n_axis)
    b = np.zeros(n, dtype=np.float64)
    b[int(first):int(last)] = 1.0
    g = _cos_phase(n) @ np.roll(b, -(n // 2)) / n
    i = np.arange(n)
    return g[(i[:, None] - i[None, :]) % n]


# ---- k-space and blur stages: device side ----------------------------------------------------------------------------

AXIS_MAX_N = _lib.H["AXIS_MAX_N"]   # the largest extent along an axis that axis_apply takes (larger ones are not tiled)


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


MOTION_MAX_IMAGES = _lib.H["MOTION_MAX_IMAGES"]   # K + 1 of one fused launch


def _rigid_rows(matrix) -> np.ndarray:
    """the first three rows of a 4 x 4 (or 3 x 4) index-space matrix as 12 f32 (the one rounding)"""
    m = np.asarray(matrix, dtype=np.float64)
    if m.shape not in ((4, 4), (3, 4)):
        raise ValueError(f"need a 4 x 4 or 3 x 4 matrix, got {m.shape}")
    return np.ascontiguousarray(m[:3], dtype=np.float32).reshape(12)


def _resampled_like(x: torch.Tensor) -> torch.Tensor:
    """the output of a resample (``rigid_resample``, ``affine_resample``): the launch writes every voxel of it"""
    return torch.empty_like(x)


def rigid_resample(x: torch.Tensor, matrix, fill: Optional[float] = None) -> torch.Tensor:
    """``sitk.Resample(image, image, transform, sitkLinear, fill)`` on a (C, D, H, W) device tensor with voxel spacing 1:
    output voxel ``i`` reads the input at the continuous index ``matrix @ (i, 1)``, trilinearly, inside
    ``-0.5 <= s < N - 0.5``; outside it gets ``fill``, or with ``fill=None`` the minimum of its channel, which is read
    on the device (no synchronisation)."""
    x = _check(x)
    m = _rigid_rows(matrix)
    cmin = channel_sum_min(x) if fill is None else None
    out = _resampled_like(x)
    _lib.check(_lib.load().mi355_rigid_resample(x.data_ptr(), out.data_ptr(), *x.shape, m.ctypes.data,
                                                None if cmin is None else cmin.data_ptr(),
                                                0.0 if fill is None else float(fill), _stream()), "rigid_resample")
    return out


class MotionParams(NamedTuple):
    """one image's RandomMotion draw: ``times`` (K,) f32 in (0, 1), ``degrees`` and ``translation`` (K, 3) f32"""
    times: np.ndarray
    degrees: np.ndarray
    translation: np.ndarray


class RandomMotion(_Random):
    """``tio.RandomMotion``: the spectra of K + 1 rigidly moved copies of the volume composited in bands along the last
    spatial axis, real part kept; on the device ``sum_k C_k resample(x, M_k)`` in one launch (``motion_matrices``,
    ``motion_bands``, ``motion_band_matrix``).  Spatial axes (0, 1, 2) of (C, D, H, W) are x, y, z; voxel
    spacing is 1 and a physical point is its voxel index (the project's subjects carry no affine).  The LPS sign flip of
    TorchIO's ``nib_to_sitk`` is not reproduced: with ranges symmetric about 0 it only relabels the draws.  Unlike the
    other stages, TorchIO draws a fresh parameter set per image of a subject, and so does ``__call__``.  Only linear
    interpolation is built.  At most 7 transforms per call; the extent along W is at most 128.  The demeaning takes the
    principal logarithm of every draw, which is unstable within 8 degrees of a half turn (``motion_matrices`` raises
    there).  A draw's three Euler angles compose to a rotation of at most their sum, so a ``degrees`` range that reaches
    beyond +-55 is refused at construction instead of failing in the load where such a draw appears."""

    per_image = True
    MAX_DEGREES = 55.0      # 3 x 55 = 165 < 171.9 = acos(-0.99), the limit of _se3_log

    def __init__(self, degrees: Range = 10, translation: Range = 10, num_transforms: int = 2,
                 image_interpolation: str = "linear", p: float = 1.0):
        super().__init__(p)
        if image_interpolation != "linear":
            raise NotImplementedError(f"image_interpolation={image_interpolation!r}: only 'linear' is built")
        if int(num_transforms) < 1:
            raise ValueError(f"num_transforms must be at least 1, got {num_transforms}")
        self.degrees_range, self.translation_range = _range(degrees, True), _range(translation, True)
        if max(abs(v) for v in self.degrees_range) > self.MAX_DEGREES:
            raise ValueError(f"degrees={degrees}: a range beyond +-{self.MAX_DEGREES:g} can compose to a rotation near a half "
                             "turn, where the demeaning of the transforms is not built")
        self.num_transforms, self.image_interpolation = int(num_transforms), image_interpolation

    def sample(self) -> MotionParams:
        """one image's parameters, drawn in TorchIO's order: degrees, translation, times"""
        k = self.num_transforms
        degrees = torch.FloatTensor(k, 3).uniform_(*self.degrees_range)
        translation = torch.FloatTensor(k, 3).uniform_(*self.translation_range)
        step = 1 / (k + 1)
        times = torch.arange(0, 1, step)[1:] + torch.FloatTensor(k).uniform_(-0.3 * step, 0.3 * step)
        return MotionParams(times.numpy(), degrees.numpy(), translation.numpy())

    @staticmethod
    def has_effect(params) -> bool:
        """false iff every rotation and translation is 0 (every copy is the input and the bands sum to the identity);
        for the per-image dict of a patch-queue load: whether any image's set has an effect"""
        if isinstance(params, dict):
            return any(RandomMotion.has_effect(p) for p in params.values())
        return bool(np.any(np.asarray(params[1]) != 0) or np.any(np.asarray(params[2]) != 0))

    def apply(self, x, params):
        params = MotionParams(*params)
        x = _check(x)
        if not self.has_effect(params):
            return x
        n = x.shape[3]
        if n > AXIS_MAX_N:
            raise _lib.Mi355Error(f"RandomMotion: extent {n} along axis 2 exceeds {AXIS_MAX_N} (larger extents are not tiled)")
        if len(params.times) + 1 > MOTION_MAX_IMAGES:
            raise _lib.Mi355Error(f"RandomMotion: {len(params.times)} transforms per call exceed {MOTION_MAX_IMAGES - 1}")
        cmin = channel_sum_min(x)                                      # enqueued first: it runs while the host builds matrices
        ms = motion_matrices(params.degrees, params.translation, x.shape[1:])
        bands = motion_bands(params.times, n)
        rows = np.concatenate([_rigid_rows(ms[image]) for image, _, _ in bands])
        cmat = np.zeros((len(bands), -(-n // 8) * 8, n))               # rows padded to a multiple of 8 with zeros
        for b, (_, first, last) in enumerate(bands):
            cmat[b, :n] = motion_band_matrix(n, first, last)
        cmat = _upload(cmat, x.device)
        out = torch.empty_like(x)
        _lib.check(_lib.load().mi355_aug_motion(x.data_ptr(), out.data_ptr(), *x.shape, len(bands), rows.ctypes.data,
                                                cmat.data_ptr(), cmin.data_ptr(), _stream()), "aug_motion")
        return out

    def apply_chained(self, x, params):
        """the same stage as K + 1 stand-alone resamples and K + 1 passes of ``axis_apply``, summed image by image: the
        comparator of the fused launch (tests, tools/bench_motion.py), not a fallback"""
        params = MotionParams(*params)
        x = _check(x)
        if not self.has_effect(params):
            return x
        ms = motion_matrices(params.degrees, params.translation, x.shape[1:])
        out = None
        for image, first, last in motion_bands(params.times, x.shape[3]):
            y = axis_apply(rigid_resample(x, ms[image]), motion_band_matrix(x.shape[3], first, last), 2)
            out = y if out is None else out + y
        return out

    def __call__(self, subject):
        """one decision per call whether the stage fires, then one parameter set per image, in the subject's order"""
        if torch.rand(1).item() >= self.p:
            return subject
        if isinstance(subject, torch.Tensor):
            return self.apply(subject, self.sample())
        return {k: ({**v, "data": self.apply(v["data"], self.sample())} if isinstance(v, dict) and "data" in v else v)
                for k, v in subject.items()}


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
    """the reference's training transform, src/data_module.py:131-139, in its order and with its arguments, without its
    first member: the six stages from RandomGhosting on.  With RandomMotion in front: ``reference_full_transform()``."""
    return [RandomGhosting(p=0.1), RandomSpike(p=0.1, intensity=(0.01, 0.1)), RandomBiasField(p=0.1),
            RandomBlur(p=0.1, std=(0.01, 0.1)), RandomNoise(p=0.1, std=(0.01, 0.1)), RandomGamma(p=0.1)]


def reference_full_transform() -> list:
    """all seven stages of the reference's training transform, src/data_module.py:131-139, in its order and with its
    arguments: ``RandomMotion(p=0.1)`` first, then ``reference_training_transform()``"""
    return [RandomMotion(p=0.1)] + reference_training_transform()


# ---- spatial stages: host mathematics (f64) ---------------------------------------------------------------------------
#
# RandomFlip and RandomAffine.  A spatial stage is an index-space matrix, as RandomMotion's copies are:
# output voxel ``i`` reads the input at ``M (i, 1)``.  Several stages compose into one matrix and the volume is resampled
# once, inside the patch gather (csrc/spatial.hip).  Axes (0, 1, 2) of (C, D, H, W) are x, y, z.  TorchIO is absent: its
# scale direction, its centre, its LPS sign flips and its random streams are not reproduced (**parity unpinned**).

TENSOR_COMPONENTS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))   # dxx, dxy, dxz, dyy, dyz, dzz (eval.ERROR_COLUMNS)


def flip_index_matrix(axes: Sequence[int], shape: Sequence[int]) -> np.ndarray:
    """mirroring along ``axes`` as a 4 x 4 f64 index-space matrix: ``s_a = (T_a - 1) - i_a`` on a flipped axis.  Exact in
    f32, and trilinear interpolation at an integer coordinate returns the voxel itself."""
    m = np.eye(4)
    for a in axes:
        if a not in (0, 1, 2):
            raise ValueError(f"axes must be among 0, 1, 2, got {a}")
        m[a, a] = -1.0
        m[a, 3] = float(int(shape[a]) - 1)
    return m


def affine_index_matrix(scales: Sequence[float], degrees: Sequence[float], translation: Sequence[float],
                        shape: Sequence[int]) -> np.ndarray:
    """``p_in = c + R diag(1 / s) (i - c) + t`` as a 4 x 4 f64 index-space matrix, ``R = Rz Rx Ry`` as in
    ``euler_index_matrix`` and ``c = (shape - 1) / 2``, the centre of the voxel grid; ``s > 1`` zooms in"""
    s = np.asarray(scales, dtype=np.float64).reshape(3)
    if not np.all(s > 0):
        raise ValueError(f"scales must be positive, got {tuple(s)}")
    a = euler_index_matrix(degrees, (0, 0, 0), (0, 0, 0))[:3, :3] @ np.diag(1.0 / s)
    c = 0.5 * (np.asarray(shape, dtype=np.float64).reshape(3) - 1.0)
    m = np.eye(4)
    m[:3, :3] = a
    m[:3, 3] = c + np.asarray(translation, dtype=np.float64).reshape(3) - a @ c
    return m


def compose_index_matrices(matrices) -> np.ndarray:
    """``M = M_1 M_2 ...`` in list order: resampling through ``M`` once is resampling through ``M_1``, then ``M_2``, ..."""
    m = np.eye(4)
    for k in matrices:
        m = m @ np.asarray(k, dtype=np.float64)
    return m


def check_tensor_rescale(rescale) -> Optional[np.ndarray]:
    """``None`` or a (6, 2) f64 array of per-component (min, max), the layout of the reference's rescale_args_dwi.txt"""
    if rescale is None:
        return None
    r = np.asarray(rescale, dtype=np.float64)
    if r.shape != (6, 2) or not np.all(np.isfinite(r)) or np.any(r[:, 0] == r[:, 1]):
        raise ValueError(f"a tensor rescale is a finite (6, 2) array of (min, max) with min != max, got shape {r.shape}")
    return r


def tensor_reorientation(matrix, rescale=None) -> Tuple[np.ndarray, np.ndarray]:
    """how a diffusion tensor turns with the volume, -> (T6 (6, 6), t6 (6,)) f64 with ``vec(D') = T6 vec(D) + t6`` on the
    components dxx, dxy, dxz, dyy, dyz, dzz.  ``F = inv(M[:3, :3])`` carries input points to output points; its
    finite-strain rotation ``R_t = U V^T`` (SVD of ``F``) turns the tensor, ``D' = R_t D R_t^T``; a reflection stays a
    reflection, a scale does not touch the tensor.  With ``rescale`` ((6, 2): min, max per component) the map acts on
    values normalised as ``n = (D - lo) / w``, ``w = |max - min|``: ``T6 <- W^-1 T6 W``, ``t6 = W^-1 (T6 lo - lo)``."""
    m = np.asarray(matrix, dtype=np.float64)
    if m.shape not in ((4, 4), (3, 4), (3, 3)):
        raise ValueError(f"need a 4 x 4, 3 x 4 or 3 x 3 matrix, got {m.shape}")
    u, _, vt = np.linalg.svd(np.linalg.inv(m[:3, :3]))
    r = u @ vt
    t6 = np.zeros((6, 6))
    for col, (a, b) in enumerate(TENSOR_COMPONENTS):
        e = np.zeros((3, 3))
        e[a, b] = e[b, a] = 1.0
        d = r @ e @ r.T
        t6[:, col] = [d[i, j] for i, j in TENSOR_COMPONENTS]
    rescale = check_tensor_rescale(rescale)
    if rescale is None:
        return t6, np.zeros(6)
    lo, w = rescale[:, 0], np.abs(rescale[:, 1] - rescale[:, 0])
    return t6 * w[None, :] / w[:, None], (t6 @ lo - lo) / w


NOT_A_TENSOR = "not a tensor"   # affine_resample(tensor_rescale=...): the image is no tensor image (None = one without rescale)


def affine_resample(x: torch.Tensor, matrix, fill: Optional[float] = None, tensor_rescale=NOT_A_TENSOR) -> torch.Tensor:
    """``rigid_resample`` through any invertible index-space matrix, as the patch queue does it: the spatial gather
    (``mi355_patch_queue_gather_spatial``) with one patch that is the whole volume, so the queue and this function share
    every bit.  ``fill=None``: an outside voxel gets the minimum of its channel, read on the device (no synchronisation).
    ``tensor_rescale`` = ``None`` or a (6, 2) array: ``x`` is a tensor image (6 channels) and every inside voxel is
    reoriented by ``tensor_reorientation(matrix, tensor_rescale)``; the fill is not."""
    x = _check(x)
    sp = _lib.QueueSpatial()
    sp.m[:] = _rigid_rows(matrix).tolist()
    tensor = tensor_rescale is not NOT_A_TENSOR
    if tensor:
        if x.shape[0] != 6:
            raise ValueError(f"a tensor image has 6 channels (dxx, dxy, dxz, dyy, dyz, dzz), got {x.shape[0]}")
        sp.t6[:] = _tensor_rows(matrix, tensor_rescale).tolist()
    cmin = channel_sum_min(x) if fill is None else None
    out = _resampled_like(x)
    rs = _lib.QueueResampling(None if cmin is None else cmin.data_ptr(), 0.0 if fill is None else float(fill), 1)
    src = _lib.QueueSource(x.data_ptr(), *x.shape[1:])
    one = lambda v: (C.c_int32 * 1)(v)
    _lib.check(_lib.load().mi355_patch_queue_gather_spatial(
        (_lib.QueueLoad * 1)(), (_lib.QueueSpatial * 1)(sp), 1, (_lib.QueueSource * 1)(src), (_lib.QueueResampling * 1)(rs),
        one(x.shape[0]), one(0), one(int(tensor)), (C.c_void_p * 1)(out.data_ptr()), 1, (C.c_int32 * 4)(0, 0, 0, 0), 1,
        *x.shape[1:], *x.shape[1:], 0.0, _stream()), "patch_queue_gather_spatial")
    return out


def _tensor_rows(matrix, rescale) -> np.ndarray:
    """``tensor_reorientation`` as 42 f32: the 6 x 6 matrix row-major, then the 6-vector (the one rounding)"""
    t6, t = tensor_reorientation(matrix, rescale)
    return np.concatenate([t6.reshape(36), t]).astype(np.float32)


class _Spatial(_Random):
    """a stage that moves voxels: ``matrix(params, shape)`` is its index-space matrix.  It applies to EVERY image of a
    subject with one parameter set, the target included, and a tensor image is reoriented with it."""

    fill: Optional[float] = 0.0        # what an outside voxel gets; None = the channel minimum

    def apply(self, x, params, tensor_rescale=NOT_A_TENSOR):
        x = _check(x)
        if not self.has_effect(params):
            return x
        return affine_resample(x, self.matrix(params, x.shape[1:]), self.fill, tensor_rescale)

    def __call__(self, subject, tensor_images: Optional[Dict] = None):
        """as ``_Random.__call__``: one decision and one parameter set per call for every image of the subject;
        ``tensor_images = {name: rescale or None}`` names the images that hold diffusion tensors"""
        if torch.rand(1).item() >= self.p:
            return subject
        params = self.sample()
        if isinstance(subject, torch.Tensor):
            return self.apply(subject, params)
        tensor_images = tensor_images or {}
        return {k: ({**v, "data": self.apply(v["data"], params, tensor_images.get(k, NOT_A_TENSOR))}
                    if isinstance(v, dict) and "data" in v else v) for k, v in subject.items()}


class RandomFlip(_Spatial):
    """``tio.RandomFlip``: each listed axis is mirrored with probability ``flip_probability``.  params = the tuple of axes
    that flip.  Axes are 0, 1, 2 of (C, D, H, W); TorchIO's anatomical axis labels are not built.  Parity unpinned."""

    def __init__(self, axes: Union[int, Tuple[int, ...]] = 0, flip_probability: float = 0.5, p: float = 1.0):
        super().__init__(p)
        self.axes = (axes,) if isinstance(axes, int) else tuple(axes)
        if not self.axes or any(not isinstance(a, int) or a not in (0, 1, 2) for a in self.axes) \
                or len(set(self.axes)) != len(self.axes):
            raise ValueError(f"axes must be distinct and among 0, 1, 2, got {axes}")
        if not 0.0 <= flip_probability <= 1.0:
            raise ValueError(f"flip_probability must be in [0, 1], got {flip_probability}")
        self.flip_probability = float(flip_probability)

    def sample(self) -> Tuple[int, ...]:
        """one ``torch.rand`` per listed axis"""
        return tuple(a for a in self.axes if torch.rand(1).item() < self.flip_probability)

    @staticmethod
    def has_effect(params) -> bool:
        return len(params) > 0

    @staticmethod
    def matrix(params, shape) -> np.ndarray:
        return flip_index_matrix(params, shape)


class AffineParams(NamedTuple):
    """one RandomAffine draw: (3,) f64 each"""
    scales: np.ndarray
    degrees: np.ndarray
    translation: np.ndarray


class RandomAffine(_Spatial):
    """``tio.RandomAffine``: a scale per axis from ``(1 - scales, 1 + scales)``, Euler angles in degrees and a translation
    in voxels, about the centre of the grid (``affine_index_matrix``).  Only ``center='image'``, linear interpolation and
    ``default_pad_value`` = ``'minimum'`` (the channel minimum) or a number are built.  Parity unpinned: TorchIO's scale
    direction, centre and random streams are not reproduced."""

    def __init__(self, scales: Range = 0.1, degrees: Range = 10, translation: Range = 0, isotropic: bool = False,
                 center: str = "image", default_pad_value: Union[str, float] = "minimum",
                 image_interpolation: str = "linear", p: float = 1.0):
        super().__init__(p)
        if image_interpolation != "linear":
            raise NotImplementedError(f"image_interpolation={image_interpolation!r}: only 'linear' is built")
        if center != "image":
            raise NotImplementedError(f"center={center!r}: only 'image' is built")
        if isinstance(default_pad_value, str):
            if default_pad_value != "minimum":
                raise NotImplementedError(f"default_pad_value={default_pad_value!r}: only 'minimum' or a number is built")
            self.fill = None
        elif isinstance(default_pad_value, (int, float)) and not isinstance(default_pad_value, bool) \
                and math.isfinite(default_pad_value):
            self.fill = float(default_pad_value)
        else:
            raise ValueError(f"default_pad_value must be 'minimum' or a finite number, got {default_pad_value!r}")
        if isinstance(scales, (int, float)):
            self.scales_range = (1.0 - float(scales), 1.0 + float(scales))
        else:
            self.scales_range = _range(scales, False)
        if not 0 < self.scales_range[0] <= self.scales_range[1]:
            raise ValueError(f"scales={scales}: need 0 < lowest <= highest scale")
        self.degrees_range, self.translation_range = _range(degrees, True), _range(translation, True)
        self.isotropic, self.center, self.default_pad_value = bool(isotropic), center, default_pad_value
        self.image_interpolation = image_interpolation

    def sample(self) -> AffineParams:
        """scales, then degrees, then translation, 3 values each; with ``isotropic`` the first scale serves all axes"""
        draw = lambda lo, hi: (torch.rand(3, dtype=torch.float64) * (hi - lo) + lo).numpy()
        scales = draw(*self.scales_range)
        if self.isotropic:
            scales = np.full(3, scales[0])
        return AffineParams(scales, draw(*self.degrees_range), draw(*self.translation_range))

    @staticmethod
    def has_effect(params) -> bool:
        s, d, t = (np.asarray(v, dtype=np.float64) for v in params)
        return bool(np.any(s != 1) or np.any(d != 0) or np.any(t != 0))

    @staticmethod
    def matrix(params, shape) -> np.ndarray:
        return affine_index_matrix(*params, shape)
