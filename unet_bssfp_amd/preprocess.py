"""Device preprocessing: scanner data -> the volumes the patch queue reads.

    python -m unet_bssfp_amd.preprocess manifest.json

The thesis builds every input and target from scanner data (doc/thesis/03-methods.tex:661-685):

* DWI: a per-voxel tensor fit (FSL ``DTIFIT``) -> the 6 upper-triangular elements, min-max normalised over the dataset with
  the diagonal and the off-diagonal elements as separate groups -- ``gradient_table`` + ``fit_tensor``;
* phase-cycled bSSFP: scanner phase [0, 4095] -> [-pi, pi], every cycle rotated by exp(-j angle(sum_xyz complex_i)), then
  magnitude and phase, each normalised to [0, 1] over the dataset and interleaved -- ``phase_correct`` + ``assemble_bssfp``
  (``repeat_cycle`` gives the one-bSSFP input).  Gibbs removal and resampling sit between the two calls in the thesis:
  resampling is ``regrid`` (below; the pipeline runs it on (re, im) with the ``regrid`` option), Gibbs removal is not part of
  this module, the caller runs it on (re, im) if wanted;
* T1w: masked, normalised to [0, 1], repeated to 6 channels -- ``assemble_t1w``.

Files of one subject need not share a grid: ``index_matrix`` turns two NIfTI affines and an optional
co-registration matrix into the voxel-to-voxel matrix, ``regrid`` resamples a volume through it on the device with nearest,
linear or cubic B-spline interpolation (``bspline_coefficients`` is the prefilter), and ``preprocess_subject(regrid=...)`` /
the manifest key ``"regrid"`` bring mask, T1w and bSSFP onto the DWI grid.  The B-spline path is pinned against
``scipy.ndimage`` (``mode='mirror'``); parity with SPM's or FSL's reslicing is not pinned.

``RangeAccumulator`` gathers the dataset ranges on the device (one host read at the end), ``preprocess_subject`` goes from files
to files, and the command line runs the two passes (ranges, then outputs) over a manifest.

Everything runs on the GPU; a CPU tensor raises (no fallback).  The wrappers allocate zero-filled results unless ``out=`` is
given: the package's uninitialised allocation sites are the ones tests/test_gpu_alloc_poison.py pins, and a caller that loops
over subjects passes its own buffers.  Every kernel writes every element of its outputs.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, nifti

MAX_MEAS = _lib.H["DTIFIT_MAX_MEAS"]
MAX_CYCLES = _lib.H["BSSFP_MAX_CYCLES"]
MAX_CHANNELS = _lib.H["PREP_MAX_CHANNELS"]
_METHODS = {"ols": _lib.H["DTIFIT_OLS"], "wls": _lib.H["DTIFIT_WLS"]}
_DT = {torch.float32: _lib.H["DT_F32"], torch.float64: _lib.H["DT_F64"]}
TENSOR_GROUPS = ((0, 3, 5), (1, 2, 4))        # diagonal (dxx, dyy, dzz) and off-diagonal (dxy, dxz, dyz) elements


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _require_cuda(what: str, **tensors):
    for name, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise _lib.Mi355Error(f"{what} runs on the GPU only (no CPU fallback): {name} is on {t.device}")


def _f32(what: str, **tensors):
    for name, t in tensors.items():
        if t.dtype != torch.float32:
            raise _lib.Mi355Error(f"{what}: {name} must be float32, got {t.dtype}")


def _mask_u8(mask: Optional[torch.Tensor], spatial, what: str) -> Optional[torch.Tensor]:
    if mask is None:
        return None
    if tuple(mask.shape) != tuple(spatial):
        raise ValueError(f"{what}: mask {tuple(mask.shape)} does not match the volume {tuple(spatial)}")
    return (mask if mask.dtype == torch.uint8 else (mask != 0).to(torch.uint8)).contiguous()


def _out(out: Optional[torch.Tensor], shape, dtype, device, what: str) -> torch.Tensor:
    if out is None:
        return torch.zeros(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device or not out.is_contiguous():
        raise ValueError(f"{what}: out must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}")
    return out


def _pair(r, what: str) -> Tuple[float, float]:
    lo, hi = (float(v) for v in r)
    if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo):
        raise ValueError(f"{what}: a range is a finite (min, max) with max > min, got ({lo}, {hi})")
    return lo, hi


def _ranges(r, c: int, what: str) -> np.ndarray:
    a = np.asarray(r, dtype=np.float64)
    if a.shape == (2,):
        a = np.tile(a, (c, 1))
    if a.shape != (c, 2) or not np.all(np.isfinite(a)) or np.any(a[:, 1] <= a[:, 0]):
        raise ValueError(f"{what}: ranges are finite (min, max) pairs with max > min, one or {c} of them, got shape {a.shape}")
    return np.ascontiguousarray(a)


# ----------------------------------------------------------------------------------------------------------------------
# tensor fit
# ----------------------------------------------------------------------------------------------------------------------
class GradientTable:
    """design (N, 7) and pinv (7, N), f64, on the host; ``on(device)`` uploads both once per device."""

    def __init__(self, bvals: np.ndarray, bvecs: np.ndarray, design: np.ndarray, pinv: np.ndarray):
        self.bvals, self.bvecs, self.design, self.pinv = bvals, bvecs, design, pinv
        self._device = {}

    @property
    def n(self) -> int:
        return self.design.shape[0]

    def on(self, device) -> Tuple[torch.Tensor, torch.Tensor]:
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = (torch.from_numpy(self.design).to(device), torch.from_numpy(self.pinv).to(device))
        return self._device[key]


def _table_array(x, rows: int, what: str) -> np.ndarray:
    a = np.loadtxt(x, dtype=np.float64, ndmin=2) if isinstance(x, (str, os.PathLike)) else np.asarray(x, dtype=np.float64)
    if rows == 1:
        a = np.atleast_1d(np.squeeze(a))
        if a.ndim != 1:
            raise ValueError(f"{what}: expected one row of b-values, got shape {a.shape}")
        return a
    if a.ndim != 2 or 3 not in a.shape:
        raise ValueError(f"{what}: expected three rows of b-vectors, got shape {a.shape}")
    return a if a.shape[0] == 3 else a.T       # FSL writes 3 x N; an N x 3 array is taken too


def gradient_table(bvals, bvecs) -> GradientTable:
    """The design matrix of ln S_i = ln S0 - b_i g_i^T D g_i and its pseudo-inverse.  ``bvals`` / ``bvecs``: arrays, or FSL
    text files (one row of N b-values; three rows of N b-vector components).  Row i of the design matrix is
    (-b gx^2, -2b gx gy, -2b gx gz, -b gy^2, -2b gy gz, -b gz^2, 1); the unknowns are (Dxx, Dxy, Dxz, Dyy, Dyz, Dzz, ln S0).
    Raises ValueError for N < 7, N > 512 or a rank below 7 (too few distinct directions, or no second b-value)."""
    b = _table_array(bvals, 1, "bvals")
    g = _table_array(bvecs, 3, "bvecs")
    n = b.shape[0]
    if g.shape[1] != n:
        raise ValueError(f"{n} b-values but {g.shape[1]} b-vectors")
    if n < 7 or n > MAX_MEAS:
        raise ValueError(f"{n} measurements: the fit takes 7 .. {MAX_MEAS}")
    if not (np.all(np.isfinite(b)) and np.all(np.isfinite(g))):
        raise ValueError("b-values and b-vectors must be finite")
    gx, gy, gz = g
    design = np.stack([-b * gx * gx, -2 * b * gx * gy, -2 * b * gx * gz, -b * gy * gy, -2 * b * gy * gz, -b * gz * gz,
                       np.ones(n)], axis=1)
    rank = np.linalg.matrix_rank(design)
    if rank < 7:
        raise ValueError(f"the design matrix has rank {rank} < 7: the tensor and S0 are not determined by these gradients")
    return GradientTable(b, g, np.ascontiguousarray(design), np.ascontiguousarray(np.linalg.pinv(design)))


def fit_tensor(dwi: torch.Tensor, table: GradientTable, method: str = "ols", mask: Optional[torch.Tensor] = None,
               norm=None, channels_first: bool = True, out_channels_first: bool = True, dtype: torch.dtype = torch.float32,
               return_s0: bool = False, out: Optional[torch.Tensor] = None, out_s0: Optional[torch.Tensor] = None):
    """Log-linear tensor fit of a float32 DWI series on the GPU.

    dwi: (N, ...) with ``channels_first`` (a [N][D][H][W] tensor) or (..., N) (the NIfTI (X, Y, Z, N) order); contiguous.
    method: "ols" (beta = pinv(A) y, DTIFIT's default) or "wls" (weights S_i^2; Cholesky on the normal equations; a voxel
    with fewer than 7 positive signals or a non-positive pivot takes the OLS solution).  y_i = ln S_i where S_i > 0, else 0.
    mask: (...) -- a voxel with mask == 0 gets 0 in every output.  norm: six (min, max) pairs (or one pair for all): the
    components are written as (D_c - min_c) / (max_c - min_c).  Returns the tensor, (6, ...) or (..., 6) by
    ``out_channels_first``, in ``dtype`` (float32 / float64); with ``return_s0`` also S0 = exp(beta_7), shape (...)."""
    _require_cuda("fit_tensor", dwi=dwi, mask=mask, out=out, out_s0=out_s0)
    _f32("fit_tensor", dwi=dwi)
    if method not in _METHODS:
        raise ValueError(f"method must be 'ols' or 'wls', got {method!r}")
    if dtype not in _DT:
        raise _lib.Mi355Error(f"fit_tensor: output dtype must be float32 or float64, got {dtype}")
    if dwi.dim() < 2:
        raise ValueError(f"fit_tensor: expected a series of volumes, got shape {tuple(dwi.shape)}")
    dwi = dwi.contiguous()
    n = dwi.shape[0] if channels_first else dwi.shape[-1]
    if n != table.n:
        raise ValueError(f"the series holds {n} measurements, the gradient table {table.n}")
    spatial = tuple(dwi.shape[1:]) if channels_first else tuple(dwi.shape[:-1])
    nvox = int(np.prod(spatial))
    ms, vs = (nvox, 1) if channels_first else (1, n)
    ocs, ovs = (nvox, 1) if out_channels_first else (1, 6)
    mask = _mask_u8(mask, spatial, "fit_tensor")
    tensor = _out(out, (6,) + spatial if out_channels_first else spatial + (6,), dtype, dwi.device, "fit_tensor")
    s0 = _out(out_s0, spatial, dtype, dwi.device, "fit_tensor") if (return_s0 or out_s0 is not None) else None
    norm_arr = None if norm is None else (C.c_double * 12)(*_ranges(norm, 6, "fit_tensor").reshape(-1))
    design, pinv = table.on(dwi.device)
    _lib.check(_lib.load().mi355_dtifit(
        dwi.data_ptr(), nvox, n, ms, vs, design.data_ptr(), pinv.data_ptr(), _METHODS[method],
        None if mask is None else mask.data_ptr(), tensor.data_ptr(), _DT[dtype], ocs, ovs,
        None if s0 is None else s0.data_ptr(), norm_arr, _stream(dwi)), "dtifit")
    return (tensor, s0) if s0 is not None else tensor


# ----------------------------------------------------------------------------------------------------------------------
# dataset ranges
# ----------------------------------------------------------------------------------------------------------------------
def bssfp_groups(channels: int) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """even channels (magnitudes) and odd channels (phases) of an assembled bSSFP tensor"""
    return tuple(range(0, channels, 2)), tuple(range(1, channels, 2))


def write_rescale_args(path: str, ranges) -> None:
    """``ranges`` ((C, 2) or one (min, max)) as the reference reads it: ``min_v, max_v = np.loadtxt(path)`` (src/eval.py:51-52),
    a row of minima over a row of maxima, written with repr precision."""
    a = np.asarray(ranges, dtype=np.float64)
    a = a.reshape(1, 2) if a.shape == (2,) else a
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"ranges must be (C, 2) or (2,), got shape {a.shape}")
    np.savetxt(path, a.T if a.shape[0] > 1 else a.reshape(2), fmt="%.17g")


def read_rescale_args(path: str) -> np.ndarray:
    """-> (C, 2) f64 (min, max) rows from a file of ``write_rescale_args`` (C = 1 for the reference's two scalars)"""
    a = np.loadtxt(path, dtype=np.float64)
    if a.shape == (2,):
        return a.reshape(1, 2)
    if a.ndim != 2 or a.shape[0] != 2:
        raise ValueError(f"{path}: expected a row of minima over a row of maxima, got shape {a.shape}")
    return np.ascontiguousarray(a.T)


class RangeAccumulator:
    """Masked per-channel minimum and maximum over a dataset, kept in device memory: ``update`` launches one kernel and reads
    nothing back, so a loop over subjects never waits for the host.  ``groups``: tuples of channels that share one range
    (``TENSOR_GROUPS``, ``bssfp_groups(24)``); a channel in no group keeps its own.  Min and max do not depend on the order
    of the work: the result is bit-identical however the kernel is scheduled."""

    def __init__(self, channels: int, groups: Optional[Sequence[Sequence[int]]] = None, device="cuda:0"):
        if channels < 1:
            raise ValueError("channels must be positive")
        self.channels = int(channels)
        self.groups = self._check_groups(groups, self.channels)
        if torch.device(device).type != "cuda":
            raise _lib.Mi355Error("RangeAccumulator runs on the GPU only (no CPU fallback)")
        self.buffer = torch.tensor([[float("inf"), float("-inf")]] * self.channels, dtype=torch.float32, device=device)

    @staticmethod
    def _check_groups(groups, channels):
        groups = tuple(tuple(int(c) for c in g) for g in (groups or ()))
        seen = [c for g in groups for c in g]
        if any(c < 0 or c >= channels for c in seen) or len(seen) != len(set(seen)) or any(not g for g in groups):
            raise ValueError(f"groups must be disjoint, non-empty sets of channels 0 .. {channels - 1}, got {groups}")
        return groups

    def update(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None) -> None:
        """x: (C, ...) float32 on the accumulator's device; mask: (...), voxels with mask != 0 count (None: all)"""
        _require_cuda("RangeAccumulator.update", x=x, mask=mask)
        _f32("RangeAccumulator.update", x=x)
        if x.dim() < 1 or x.shape[0] != self.channels:
            raise ValueError(f"expected {self.channels} channels first, got shape {tuple(x.shape)}")
        if x.device != self.buffer.device:
            raise ValueError(f"x is on {x.device}, the accumulator on {self.buffer.device}")
        x = x.contiguous()
        mask = _mask_u8(mask, tuple(x.shape[1:]), "RangeAccumulator.update")
        _lib.check(_lib.load().mi355_channel_minmax(
            x.data_ptr(), self.channels, x[0].numel(), None if mask is None else mask.data_ptr(), self.buffer.data_ptr(),
            _stream(x)), "channel_minmax")

    @staticmethod
    def merge(per_channel: np.ndarray, groups) -> np.ndarray:
        """(C, 2) per-channel (min, max) -> the same with every channel of a group carrying the group's range"""
        out = np.array(per_channel, dtype=np.float64)
        for g in groups:
            idx = list(g)
            out[idx, 0] = out[idx, 0].min()
            out[idx, 1] = out[idx, 1].max()
        return out

    def per_channel(self) -> np.ndarray:
        """(C, 2) f64, one host read; a channel that saw no voxel holds (+inf, -inf)"""
        return self.buffer.detach().cpu().numpy().astype(np.float64)

    def ranges(self) -> np.ndarray:
        """(C, 2) f64 (min, max) per channel after merging the groups: what ``fit_tensor(norm=)``, ``normalize_tensor`` and
        ``augment.check_tensor_rescale`` take"""
        return self.merge(self.per_channel(), self.groups)

    def group_ranges(self) -> list:
        """[(min, max)] per group, in group order: what ``assemble_bssfp`` / ``assemble_t1w`` and, for a single group,
        ``eval.calc_scalar_maps(min_v, max_v)`` take"""
        r = self.ranges()
        return [(float(r[g[0], 0]), float(r[g[0], 1])) for g in self.groups]

    def save(self, path: str) -> None:
        write_rescale_args(path, self.ranges())


# ----------------------------------------------------------------------------------------------------------------------
# bSSFP
# ----------------------------------------------------------------------------------------------------------------------
def _cycles(what: str, a: torch.Tensor, b: torch.Tensor):
    _f32(what, a=a, b=b)
    if a.dim() < 2 or a.shape != b.shape:
        raise ValueError(f"{what}: expected two (P, ...) tensors of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    if not 1 <= a.shape[0] <= MAX_CYCLES:
        raise ValueError(f"{what}: {a.shape[0]} phase cycles, the kernels take 1 .. {MAX_CYCLES}")
    return a.contiguous(), b.contiguous(), a.shape[0], a[0].numel()


def phase_sums(mag: torch.Tensor, phase_raw: torch.Tensor) -> torch.Tensor:
    """(P, 2) float64 device tensor: (Re, Im) of sum_xyz mag exp(j phi) per cycle, phi = phase_raw / 4095 * 2 pi - pi.
    Two-stage f64 sum in a fixed order: bit-identical from call to call."""
    _require_cuda("phase_sums", mag=mag, phase_raw=phase_raw)
    mag, phase_raw, p, nvox = _cycles("phase_sums", mag, phase_raw)
    lib = _lib.load()
    ws_bytes = lib.mi355_bssfp_workspace_bytes(p, nvox)
    ws = torch.zeros(max(ws_bytes, 8) // 8, dtype=torch.float64, device=mag.device)
    sums = torch.zeros((p, 2), dtype=torch.float64, device=mag.device)
    _lib.check(lib.mi355_bssfp_phase_sums(mag.data_ptr(), phase_raw.data_ptr(), p, nvox, ws.data_ptr(), ws.numel() * 8,
                                          sums.data_ptr(), _stream(mag)), "bssfp_phase_sums")
    return sums


def phase_correct(mag: torch.Tensor, phase_raw: torch.Tensor, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """The thesis's global phase correction.  mag, phase_raw: (P, D, H, W) float32, P <= 16, the phase in scanner units
    [0, 4095].  Every cycle is rotated by exp(-j theta_i), theta_i = angle(sum_xyz mag_i exp(j phi_i)); the angle stays on the
    device.  Returns (re, im) = (mag cos(phi - theta_i), mag sin(phi - theta_i)), float32, shaped like the inputs."""
    _require_cuda("phase_correct", mag=mag, phase_raw=phase_raw)
    sums = phase_sums(mag, phase_raw)
    mag, phase_raw, p, nvox = _cycles("phase_correct", mag, phase_raw)
    re = _out(None if out is None else out[0], mag.shape, torch.float32, mag.device, "phase_correct")
    im = _out(None if out is None else out[1], mag.shape, torch.float32, mag.device, "phase_correct")
    _lib.check(_lib.load().mi355_bssfp_phase_correct(mag.data_ptr(), phase_raw.data_ptr(), p, nvox, sums.data_ptr(),
                                                     re.data_ptr(), im.data_ptr(), _stream(mag)), "bssfp_phase_correct")
    return re, im


def assemble_bssfp(re: torch.Tensor, im: torch.Tensor, mask: Optional[torch.Tensor], mag_range, pha_range,
                   repeat_cycle: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(P, D, H, W) real and imaginary parts -> the network's (2P, D, H, W) input: channel 2i = (|z_i| - min) / (max - min)
    with ``mag_range``, channel 2i + 1 = (atan2(im_i, re_i) - min) / (max - min) with ``pha_range``; 0 where mask == 0.
    ``repeat_cycle=k`` fills every pair from cycle k (the one-bSSFP input).  Ranges (0, 1) give the raw values."""
    _require_cuda("assemble_bssfp", re=re, im=im, mask=mask, out=out)
    re, im, p, nvox = _cycles("assemble_bssfp", re, im)
    if repeat_cycle is not None and not 0 <= int(repeat_cycle) < p:
        raise ValueError(f"repeat_cycle {repeat_cycle} outside 0 .. {p - 1}")
    (mlo, mhi), (plo, phi) = _pair(mag_range, "assemble_bssfp"), _pair(pha_range, "assemble_bssfp")
    spatial = tuple(re.shape[1:])
    mask = _mask_u8(mask, spatial, "assemble_bssfp")
    res = _out(out, (2 * p,) + spatial, torch.float32, re.device, "assemble_bssfp")
    _lib.check(_lib.load().mi355_bssfp_assemble(
        re.data_ptr(), im.data_ptr(), p, nvox, None if mask is None else mask.data_ptr(), mlo, mhi, plo, phi,
        -1 if repeat_cycle is None else int(repeat_cycle), res.data_ptr(), _stream(re)), "bssfp_assemble")
    return res


# ----------------------------------------------------------------------------------------------------------------------
# T1w and ready-made tensors
# ----------------------------------------------------------------------------------------------------------------------
def _normalize(what: str, src: torch.Tensor, channel_map: Sequence[int], ranges: np.ndarray, mask, out) -> torch.Tensor:
    _require_cuda(what, src=src, mask=mask, out=out)
    _f32(what, src=src)
    src = src.contiguous()
    c_out, spatial = len(channel_map), tuple(src.shape[1:])
    if not 1 <= c_out <= MAX_CHANNELS:
        raise ValueError(f"{what}: {c_out} output channels, the kernel takes 1 .. {MAX_CHANNELS}")
    mask = _mask_u8(mask, spatial, what)
    res = _out(out, (c_out,) + spatial, torch.float32, src.device, what)
    _lib.check(_lib.load().mi355_normalize_channels(
        src.data_ptr(), src.shape[0], (C.c_int32 * c_out)(*channel_map), (C.c_double * (2 * c_out))(*ranges.reshape(-1)),
        c_out, src[0].numel(), None if mask is None else mask.data_ptr(), res.data_ptr(), _stream(src)), "normalize_channels")
    return res


def assemble_t1w(t1: torch.Tensor, mask: Optional[torch.Tensor], range, channels: int = 6,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(D, H, W) or (1, D, H, W) float32 -> (channels, D, H, W): masked, normalised to [0, 1] with ``range`` = (min, max),
    the one volume repeated ``channels`` times (the thesis's 6-channel T1w input)."""
    if t1.dim() == 3:
        t1 = t1[None]
    if t1.dim() != 4 or t1.shape[0] != 1:
        raise ValueError(f"assemble_t1w: expected (D, H, W) or (1, D, H, W), got {tuple(t1.shape)}")
    return _normalize("assemble_t1w", t1, [0] * int(channels), _ranges(_pair(range, "assemble_t1w"), int(channels), "assemble_t1w"),
                      mask, out)


def normalize_tensor(t: torch.Tensor, ranges, mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """(C, ...) float32 -> the same shape, channel c as (t_c - min_c) / (max_c - min_c), 0 where mask == 0: the normalisation
    of a tensor image that FSL produced.  ``ranges``: (C, 2), or one (min, max) for every channel."""
    if t.dim() < 2:
        raise ValueError(f"normalize_tensor: expected channels first, got shape {tuple(t.shape)}")
    return _normalize("normalize_tensor", t, list(range(t.shape[0])), _ranges(ranges, t.shape[0], "normalize_tensor"), mask, out)


# ----------------------------------------------------------------------------------------------------------------------
# regridding onto a common grid
# ----------------------------------------------------------------------------------------------------------------------
MAX_SPLINE_EXTENT = _lib.H["REGRID_MAX_N"]
_ORDERS = {"nearest": _lib.H["REGRID_NEAREST"], "linear": _lib.H["REGRID_LINEAR"], "bspline": _lib.H["REGRID_CUBIC"]}


def _affine(a, what: str) -> np.ndarray:
    a = np.asarray(a, dtype=np.float64)
    if a.shape != (4, 4) or not np.all(np.isfinite(a)):
        raise ValueError(f"{what}: expected a finite 4 x 4 matrix, got shape {a.shape}")
    s = np.linalg.svd(a[:3, :3], compute_uv=False)
    if not s[-1] > 1e-12 * s[0]:
        raise ValueError(f"{what}: the matrix is singular (singular values {s})")
    return a


def index_matrix(src_affine, dst_affine, xfm=None) -> np.ndarray:
    """The (3, 4) f64 matrix that carries a voxel index of the destination grid to the continuous voxel index of the source
    image: ``inv(src_affine) @ xfm @ dst_affine``.  The affines are NIfTI voxel-to-world matrices; ``xfm`` (default: identity)
    is a 4 x 4 world-to-world matrix from destination-grid world coordinates to source-image world coordinates, which is what
    a co-registration returns.  Tensor axes (D, H, W) are the NIfTI array axes (X, Y, Z).  A singular matrix raises."""
    src, dst = _affine(src_affine, "index_matrix: src_affine"), _affine(dst_affine, "index_matrix: dst_affine")
    x = np.eye(4) if xfm is None else _affine(xfm, "index_matrix: xfm")
    return np.ascontiguousarray((np.linalg.inv(src) @ x @ dst)[:3])


def _volume(what: str, x: torch.Tensor, dtype) -> torch.Tensor:
    if x.dim() != 4 or x.dtype != dtype or min(x.shape) < 1:
        raise ValueError(f"{what}: expected a non-empty (C, D, H, W) {dtype} tensor, got {x.dtype} {tuple(x.shape)}")
    return x.contiguous()


def bspline_coefficients(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(C, D, H, W) float32 samples -> float64 cubic B-spline coefficients of the same shape (the separable prefilter with
    mirror boundaries, ``scipy.ndimage.spline_filter(order=3, mode='mirror')``): what ``regrid(..., "bspline")`` reads.  A
    caller that regrids one volume several times computes them once.  Extents up to 512 per axis."""
    _require_cuda("bspline_coefficients", x=x, out=out)
    x = _volume("bspline_coefficients", x, torch.float32)
    coef = _out(out, x.shape, torch.float64, x.device, "bspline_coefficients")
    _lib.check(_lib.load().mi355_bspline_prefilter(x.data_ptr(), coef.data_ptr(), *x.shape, _stream(x)), "bspline_prefilter")
    return coef


def regrid(x: torch.Tensor, matrix, out_shape, interpolation: str = "linear", fill: float = 0.0,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Resample a (C, D, H, W) float32 device tensor onto a grid of ``out_shape`` = (D', H', W'): output voxel i reads the
    source at the continuous index ``matrix @ (i, 1)`` (``index_matrix``; (3, 4) or (4, 4), f64 on the device too).  Inside
    ``-0.5 <= s < N - 0.5`` the value is interpolated -- ``"nearest"``, ``"linear"`` (taps clamped into the volume) or
    ``"bspline"`` (cubic, mirror boundaries) -- outside it is ``fill``.  With ``"bspline"`` a float64 ``x`` is taken as the
    coefficients of ``bspline_coefficients``; a float32 ``x`` is prefiltered first.  Returns (C, D', H', W') float32."""
    if interpolation not in _ORDERS:
        raise ValueError(f"interpolation must be one of {sorted(_ORDERS)}, got {interpolation!r}")
    m = np.asarray(matrix, dtype=np.float64)
    if m.shape not in ((3, 4), (4, 4)) or not np.all(np.isfinite(m)):
        raise ValueError(f"regrid: matrix must be a finite (3, 4) or (4, 4) array, got shape {m.shape}")
    out_shape = tuple(int(n) for n in out_shape)
    if len(out_shape) != 3 or min(out_shape) < 1:
        raise ValueError(f"regrid: out_shape must be three positive extents, got {out_shape}")
    _require_cuda("regrid", x=x, out=out)
    if interpolation == "bspline" and x.dtype == torch.float64:
        src = _volume("regrid", x, torch.float64)
    else:
        src = _volume("regrid", x, torch.float32)
        if interpolation == "bspline":
            src = bspline_coefficients(src)
    res = _out(out, (src.shape[0],) + out_shape, torch.float32, src.device, "regrid")
    _lib.check(_lib.load().mi355_regrid(src.data_ptr(), res.data_ptr(), *src.shape, *out_shape,
                                        (C.c_double * 12)(*m[:3].reshape(-1)), _ORDERS[interpolation], float(fill),
                                        _stream(src)), "regrid")
    return res


def _regrid_options(regrid_opts) -> Optional[Tuple[str, float]]:
    if regrid_opts is None:
        return None
    unknown = set(regrid_opts) - {"interpolation", "fill"}
    if unknown:
        raise ValueError(f"regrid: unknown options {sorted(unknown)}; the keys are 'interpolation' and 'fill'")
    interpolation = regrid_opts.get("interpolation", "linear")
    if interpolation not in _ORDERS:
        raise ValueError(f"regrid: interpolation must be one of {sorted(_ORDERS)}, got {interpolation!r}")
    return interpolation, float(regrid_opts.get("fill", 0.0))


# ----------------------------------------------------------------------------------------------------------------------
# files to files
# ----------------------------------------------------------------------------------------------------------------------
OUTPUTS = {"dwi-tensor": "desc-normtensor_dwi", "pc-bssfp": "desc-normflatbet_pc-bssfp", "bssfp": "desc-normflatbet_bssfp",
           "t1w": "desc-normflatbet_t1w"}
RANGE_KEYS = ("dwi-tensor", "bssfp-mag", "bssfp-phase", "t1w")


def _load_subject(files: Dict[str, str], device, regrid_opts=None):
    """raw device tensors of one subject: dwi (X, Y, Z, N), mask (X, Y, Z) u8, mag / phase (P, X, Y, Z), t1 (X, Y, Z).
    ``regrid_opts`` = (interpolation, fill): mask and t1 arrive on the DWI grid, mag / phase stay on their own and
    ``bssfp_matrix`` says how to bring the corrected series over (``_corrected_bssfp``)."""
    if regrid_opts is not None:
        return _load_on_dwi_grid(files, device, *regrid_opts)

    def vol(key):
        return torch.from_numpy(np.ascontiguousarray(nifti.load(files[key])[0], dtype=np.float32)).to(device)
    sub = {"dwi": vol("dwi"), "mask": (vol("mask") != 0).to(torch.uint8)}
    if "bssfp_mag" in files:
        sub["mag"] = vol("bssfp_mag").movedim(-1, 0).contiguous()
        sub["phase"] = vol("bssfp_phase").movedim(-1, 0).contiguous()
    if "t1w" in files:
        sub["t1"] = vol("t1w")
    return sub


def _load_on_dwi_grid(files: Dict[str, str], device, interpolation: str, fill: float):
    """The DWI file's (shape, affine) is the common grid.  A file is regridded when its shape or its affine differs from the
    DWI's, or when ``files["xfm"][key]`` names a 4 x 4 text matrix (destination world -> source world; key ``bssfp_mag``
    stands for the series, whose phase file shares the magnitude's grid).  The mask always takes "nearest" and fill 0."""
    def vol(key):
        data, affine = nifti.load(files[key])
        return torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).to(device), affine
    dwi, grid_affine = vol("dwi")
    grid, xfms = tuple(dwi.shape[:3]), files.get("xfm", {})

    def matrix(key, t, affine):                                # None: the file already sits on the DWI grid
        if key not in xfms and tuple(t.shape[:3]) == grid and np.allclose(affine, grid_affine, rtol=0, atol=1e-5):
            return None
        return index_matrix(affine, grid_affine, np.loadtxt(xfms[key], dtype=np.float64, ndmin=2) if key in xfms else None)

    mask, affine = vol("mask")
    m = matrix("mask", mask, affine)
    mask = (mask != 0).to(torch.float32)
    sub = {"dwi": dwi, "mask": ((mask if m is None else regrid(mask[None], m, grid, "nearest", 0.0)[0]) != 0).to(torch.uint8)}
    if "bssfp_mag" in files:
        (mag, affine), (phase, phase_affine) = vol("bssfp_mag"), vol("bssfp_phase")
        if phase.shape != mag.shape or not np.allclose(phase_affine, affine, rtol=0, atol=1e-5):
            raise ValueError(f"bssfp_phase {tuple(phase.shape)} does not sit on the grid of bssfp_mag {tuple(mag.shape)}: "
                             "the shapes or the affines differ")
        sub["mag"], sub["phase"] = mag.movedim(-1, 0).contiguous(), phase.movedim(-1, 0).contiguous()
        sub["bssfp_matrix"] = matrix("bssfp_mag", mag, affine)
    if "t1w" in files:
        t1, affine = vol("t1w")
        m = matrix("t1w", t1, affine)
        sub["t1"] = t1 if m is None else regrid(t1[None], m, grid, interpolation, fill)[0]
    return sub


def _corrected_bssfp(sub, regrid_opts):
    """(re, im) of the phase-corrected series.  The correction runs on the series' NATIVE grid and the real and imaginary
    parts are regridded: a wrapped phase is never interpolated."""
    re, im = phase_correct(sub["mag"], sub["phase"])
    m = sub.get("bssfp_matrix")
    if m is not None:
        grid, (interpolation, fill) = tuple(sub["dwi"].shape[:3]), regrid_opts
        re, im = regrid(re, m, grid, interpolation, fill), regrid(im, m, grid, interpolation, fill)
    return re, im


def _table_of(files, table):
    return table if table is not None else gradient_table(files["bval"], files["bvec"])


def accumulate_subject(files: Dict[str, str], accumulators: Dict[str, RangeAccumulator], table: Optional[GradientTable] = None,
                       method: str = "ols", device="cuda:0", regrid: Optional[Dict[str, object]] = None) -> None:
    """First pass: folds one subject's raw tensor, bSSFP magnitude / phase and T1w values inside the mask into
    ``accumulators`` (made by ``make_accumulators``).  No host read.  ``regrid``: as in ``preprocess_subject``; the ranges are
    then those of the regridded values, the ones the second pass normalises."""
    opts = _regrid_options(regrid)
    sub = _load_subject(files, device, opts)
    tensor = fit_tensor(sub["dwi"], _table_of(files, table), method, sub["mask"], channels_first=False)
    accumulators["dwi-tensor"].update(tensor, sub["mask"])
    if "mag" in sub:
        re, im = _corrected_bssfp(sub, opts)
        accumulators["pc-bssfp"].update(assemble_bssfp(re, im, sub["mask"], (0.0, 1.0), (0.0, 1.0)), sub["mask"])
    if "t1" in sub:
        accumulators["t1w"].update(sub["t1"][None], sub["mask"])


def make_accumulators(cycles: int = 12, device="cuda:0", tensor_groups=TENSOR_GROUPS) -> Dict[str, RangeAccumulator]:
    """the accumulators of the first pass: the raw tensor (diagonal / off-diagonal groups), the raw assembled bSSFP channels
    (even = magnitude, odd = phase) and the T1w volume"""
    return {"dwi-tensor": RangeAccumulator(6, tensor_groups, device),
            "pc-bssfp": RangeAccumulator(2 * cycles, bssfp_groups(2 * cycles), device),
            "t1w": RangeAccumulator(1, ((0,),), device)}


def ranges_of(accumulators: Dict[str, RangeAccumulator]) -> Dict[str, object]:
    """the ``ranges`` argument of ``preprocess_subject`` (keys ``RANGE_KEYS``): a (6, 2) array for the tensor, one (min, max)
    for the others; a modality no subject had is left out.  The tensor and bSSFP ranges are widened outward by one float32
    ulp: the accumulated extrema are those of float32-ROUNDED values, while the output pass normalises the f64 values
    themselves, which may lie half an ulp outside -- widened, every written value stays inside [0, 1]."""
    def widen(r):
        r = np.asarray(r, dtype=np.float32)
        return np.stack([np.nextafter(r[..., 0], np.float32(-np.inf)), np.nextafter(r[..., 1], np.float32(np.inf))], -1).astype(np.float64)
    out = {"dwi-tensor": widen(accumulators["dwi-tensor"].ranges())}
    mag, pha = accumulators["pc-bssfp"].group_ranges()
    for k, r, wide in (("bssfp-mag", mag, True), ("bssfp-phase", pha, True), ("t1w", accumulators["t1w"].group_ranges()[0], False)):
        if np.all(np.isfinite(r)):                           # (+inf, -inf): no subject had this modality
            lo, hi = widen(r) if wide else r
            out[k] = (float(lo), float(hi))
    return out


def preprocess_subject(files: Dict[str, str], ranges: Dict[str, object], out_dir: str, table: Optional[GradientTable] = None,
                       method: str = "ols", device="cuda:0", one_bssfp_cycle: int = 0,
                       regrid: Optional[Dict[str, object]] = None) -> Dict[str, str]:
    """Second pass, files to files.  ``files``: ``dwi`` (X, Y, Z, N), ``bval`` / ``bvec`` (FSL text; or pass ``table``),
    ``mask`` (X, Y, Z), optionally ``bssfp_mag`` + ``bssfp_phase`` (X, Y, Z, P; phase in scanner units) and ``t1w`` (X, Y, Z),
    and the labels ``sub`` / ``ses`` of the file names.  ``ranges``: ``ranges_of(...)``.  Writes (X, Y, Z, C) float32 NIfTI
    files -- ``dwi-tensor`` (6 channels), ``pc-bssfp`` (2P), ``bssfp`` (cycle ``one_bssfp_cycle`` repeated, 2P) and ``t1w`` (6) --
    and returns ``{image name: path}``, an entry of the ``train`` / ``val`` lists that ``data.subjects_from_nifti`` reads.
    ``regrid`` = ``{"interpolation": "linear" | "bspline" | "nearest", "fill": 0.0}`` (default None: every file must already sit
    on the DWI grid): the DWI file's shape and affine are the common grid, and ``mask`` (always "nearest"), ``t1w`` and the
    bSSFP series are regridded onto it where their shape or affine differs or ``files["xfm"][key]`` names a 4 x 4 text matrix
    (DWI-grid world -> that file's world, as a co-registration returns it; key ``bssfp_mag`` for the series).  The series is
    phase-corrected on its own grid, then (re, im) are regridded.  The DWI series itself is never regridded."""
    opts = _regrid_options(regrid)
    sub = _load_subject(files, device, opts)
    os.makedirs(out_dir, exist_ok=True)
    stem = os.path.join(out_dir, f"sub-{files.get('sub', 'unknown')}_ses-{files.get('ses', 'unknown')}_")
    affine = nifti.load(files["dwi"])[1]
    entry = {}

    def write(name, t):
        entry[name] = stem + OUTPUTS[name] + ".nii.gz"
        nifti.save(np.ascontiguousarray(t.movedim(0, -1).cpu().numpy()), entry[name], affine)

    write("dwi-tensor", fit_tensor(sub["dwi"], _table_of(files, table), method, sub["mask"], norm=ranges["dwi-tensor"],
                                   channels_first=False))
    if "mag" in sub:
        re, im = _corrected_bssfp(sub, opts)
        write("pc-bssfp", assemble_bssfp(re, im, sub["mask"], ranges["bssfp-mag"], ranges["bssfp-phase"]))
        write("bssfp", assemble_bssfp(re, im, sub["mask"], ranges["bssfp-mag"], ranges["bssfp-phase"], repeat_cycle=one_bssfp_cycle))
    if "t1" in sub:
        write("t1w", assemble_t1w(sub["t1"], sub["mask"], ranges["t1w"]))
    return entry


def main(argv=None) -> int:
    """manifest.json: ``{"subjects": [files, ...], "out_dir": ..., "method": "ols", "device": "cuda:0", "val": [indices],
    "cycles": 12, "regrid": {"interpolation": "linear", "fill": 0.0}}`` (``files`` and ``regrid`` as in ``preprocess_subject``;
    only the first two keys are required).
    Pass 1 gathers the dataset ranges, pass 2 writes the volumes.  Leaves ``rescale_args_<key>.txt`` per range and
    ``train_manifest.json`` with the ``train`` / ``val`` / ``tensor_rescale`` keys of ``python -m unet_bssfp_amd.train``."""
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 1:
        print(__doc__)
        return 2
    with open(argv[0]) as f:
        manifest = json.load(f)
    device, method, out_dir = manifest.get("device", "cuda:0"), manifest.get("method", "ols"), manifest["out_dir"]
    regrid_opts = manifest.get("regrid")
    subjects = manifest["subjects"]
    os.makedirs(out_dir, exist_ok=True)
    cycles = manifest.get("cycles")                          # phase cycles per bSSFP series; default: the first series'
    if cycles is None:
        first = [s["bssfp_mag"] for s in subjects if "bssfp_mag" in s][:1]
        cycles = nifti.load(first[0])[0].shape[-1] if first else 12
    acc = make_accumulators(cycles, device)
    tables = [gradient_table(s["bval"], s["bvec"]) for s in subjects]
    for s, t in zip(subjects, tables):
        accumulate_subject(s, acc, t, method, device, regrid_opts)
    ranges = ranges_of(acc)
    for key in ranges:
        write_rescale_args(os.path.join(out_dir, f"rescale_args_{key}.txt"), ranges[key])
    entries = [preprocess_subject(s, ranges, out_dir, t, method, device, regrid=regrid_opts) for s, t in zip(subjects, tables)]
    val = set(manifest.get("val", ()))
    out = {"train": [e for i, e in enumerate(entries) if i not in val], "val": [e for i, e in enumerate(entries) if i in val],
           "tensor_rescale": ranges["dwi-tensor"].tolist()}
    with open(os.path.join(out_dir, "train_manifest.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(f"preprocessed {len(entries)} subjects into {out_dir}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
