"""CPU ORACLE -- TEST INFRASTRUCTURE ONLY.  DTI relative-error maps and per-tissue error table.

Vectorised numpy restatement of ``do_calc_diff_maps`` (reference src/eval.py:154-166), the post-processing
and weighted means of ``do_calc_error_avg`` (:240-257) and the probseg preparation of ``calc_error_table``
(:285-287), on arrays instead of NIfTI files:
  tensor columns : |p - t| / t of the tensors as passed
  md, fa, ad, rd : the same of ``oracle.dti_ref.scalar_maps`` of the de-normalised tensors
  angles         : r = (p - t) % 360, where(r < 180, r, 360 - r), of the principal direction with the
                   eigenvector flipped to z >= 0 (the kernel's convention; LAPACK's sign is arbitrary)
  then |diff|, 0 outside the mask, +inf -> 0 (NaN stays); weights probseg where mask > 0 and probseg > 1e-5;
  table[r, c] = sum(w_r * diff_c) / sum(w_r).
Pinned by tests/golden/dti_errors.npz (tools/gen_golden_dti_errors.py: the reference's own functions).
"""
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from oracle import dti_ref  # noqa: E402

COLUMNS = ("dxx", "dxy", "dxz", "dyy", "dyz", "dzz", "md", "fa", "ad", "rd", "azimuth", "inclination")


def _full(d):
    dxx, dxy, dxz, dyy, dyz, dzz = (d[..., i] for i in range(6))
    return np.stack([np.stack([dxx, dxy, dxz], -1), np.stack([dxy, dyy, dyz], -1), np.stack([dxz, dyz, dzz], -1)], -2)


def angles(d):
    """azimuth, inclination (degrees) of the principal eigenvector, sign fixed to z >= 0 (ties: y, then x >= 0)."""
    _, v = np.linalg.eigh(_full(d), "U")
    e = v[..., :, 2].copy()
    flip = (e[..., 2] < 0) | ((e[..., 2] == 0) & ((e[..., 1] < 0) | ((e[..., 1] == 0) & (e[..., 0] < 0))))
    e[flip] = -e[flip]
    with np.errstate(invalid="ignore", divide="ignore"):
        az = 180 / np.pi * np.arctan2(e[..., 1], e[..., 0])
        az = np.where(az > 180, az - 360, az)
        r = np.sqrt((e ** 2).sum(-1))
        inc = 180 / np.pi * np.arccos(e[..., 2] / r)
    return az, inc


def raw_diffs(pred, target, min_v=None, max_v=None):
    """(..., 6) x 2 -> (12, ...) diffs of do_calc_diff_maps, before the post-processing."""
    p, t = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    dp, dt = p, t
    if min_v is not None:
        dp, dt = dti_ref.invert_dwi_tensor_norm(p, min_v, max_v), dti_ref.invert_dwi_tensor_norm(t, min_v, max_v)
    mp, mt = dti_ref.scalar_maps(dp), dti_ref.scalar_maps(dt)
    ap, at = angles(dp), angles(dt)
    out = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(6):
            out.append(np.abs(p[..., i] - t[..., i]) / t[..., i])
        for k in ("md", "fa", "ad", "rd"):
            out.append(np.abs(mp[k] - mt[k]) / mt[k])
        for a, b in zip(ap, at):
            r = (a - b) % 360
            out.append(np.where(r < 180, r, 360 - r))
    return np.stack(out)


def post_process(diffs, mask):
    """|diff|, 0 where mask (as uint8) is not > 0, +inf -> 0; NaN stays."""
    m = np.asarray(mask).astype(np.uint8) > 0
    d = np.abs(diffs)
    d = np.where(m, d, 0)
    return np.where(d == np.inf, 0, d)


def weights(mask, probseg):
    """(..., R) probseg -> (..., R) f64 weights of calc_error_table."""
    m = (np.asarray(mask).astype(np.uint8) > 0)[..., None]
    ps = np.asarray(probseg, np.float64)
    ps = np.where(m, ps, 0)
    return np.where(ps > 1e-5, ps, 0)


def error_maps(pred, target, mask, min_v=None, max_v=None):
    return post_process(raw_diffs(pred, target, min_v, max_v), mask)


def error_table(pred, target, mask, probseg, min_v=None, max_v=None):
    """NIfTI-order inputs -> ((R, 12) table, (12, ...) post-processed diff maps), float64."""
    maps = error_maps(pred, target, mask, min_v, max_v)
    w = weights(mask, probseg)
    table = np.empty((w.shape[-1], len(COLUMNS)))
    with np.errstate(invalid="ignore", divide="ignore"):
        for r in range(w.shape[-1]):
            wr = w[..., r]
            for c in range(len(COLUMNS)):
                table[r, c] = (wr * maps[c]).sum() / wr.sum()
    return table, maps


def synthetic_case(shape, nroi=3, seed=0, normalised=False):
    """pred, target (..., 6) f32, mask (...) uint8 (a ball), probseg (..., R) f32 (rows sum to 1, some < 1e-5).
    Targets are SPD diffusion-like tensors, predictions perturb them by ~10 %; ``normalised`` maps both
    to [0, 1] per the min-max (min_v, max_v) returned as the last two values (else None, None)."""
    rng = np.random.default_rng(seed)
    t = dti_ref.synthetic_tensor_field(shape, seed=seed)
    p = t * (1 + 0.1 * rng.standard_normal(t.shape))
    min_v = max_v = None
    if normalised:
        min_v, max_v = -2e-3, 6e-3
        t, p = (t - min_v) / (max_v - min_v), (p - min_v) / (max_v - min_v)
    idx = np.stack(np.meshgrid(*[np.linspace(-1, 1, n) if n > 1 else np.zeros(1) for n in shape], indexing="ij"), -1)
    mask = ((idx ** 2).sum(-1) < 0.8).astype(np.uint8)
    ps = rng.random(shape + (nroi,)) ** 3
    ps /= ps.sum(-1, keepdims=True)
    return p.astype(np.float32), t.astype(np.float32), mask, ps.astype(np.float32), min_v, max_v
