"""f64 numpy restatement of the preprocessing kernels (csrc/dtifit.hip, csrc/prep.hip), and the synthetic
cases the tests share.  Written from the definitions in include/mi355_unet.h, not from the kernels: sums run in numpy's order,
the weighted fit is solved twice (Cholesky on the normal equations, and lstsq on sqrt(W) A) so that their difference gives
the scale of what the conditioning alone does to a solution."""
from __future__ import annotations

import functools

import numpy as np

GRIDS = ((1, 1, 1), (5, 7, 9), (17, 16, 33))
MEAS = (7, 13, 64, 512)
EPS64 = 2.0 ** -53


# ---------------------------------------------------------------------------------------------------------------- the model
def design_matrix(bvals, bvecs):
    b = np.asarray(bvals, np.float64)
    gx, gy, gz = np.asarray(bvecs, np.float64)
    return np.stack([-b * gx * gx, -2 * b * gx * gy, -2 * b * gx * gz, -b * gy * gy, -2 * b * gy * gz, -b * gz * gz,
                     np.ones_like(b)], axis=1)


def scheme(n, seed=0):
    """(bvals (n,), bvecs (3, n)): b = 0 rows first (several of them once n allows), then shells of 1000 and 2000 s/mm^2 on
    random unit directions"""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    n0 = 1 if n < 10 else max(2, n // 10)
    g = rng.standard_normal((3, n))
    g /= np.linalg.norm(g, axis=0)
    b = np.where(np.arange(n) % 2 == 0, 1000.0, 2000.0)
    b[:n0] = 0.0
    g[:, :n0] = 0.0
    return b, g


def tensor_field(nvox, seed=0):
    """random positive-definite tensors (nvox, 6) in (xx, xy, xz, yy, yz, zz) order, eigenvalues in [0.2, 2.0] 1e-3 mm^2/s, and
    S0 (nvox,) in [500, 1500]"""
    rng = np.random.default_rng(2000 + seed)
    q, _ = np.linalg.qr(rng.standard_normal((nvox, 3, 3)))
    lam = rng.uniform(0.2e-3, 2.0e-3, (nvox, 3))
    d = np.einsum("vij,vj,vkj->vik", q, lam, q)
    s0 = rng.uniform(500.0, 1500.0, nvox)
    return np.stack([d[:, 0, 0], d[:, 0, 1], d[:, 0, 2], d[:, 1, 1], d[:, 1, 2], d[:, 2, 2]], axis=1), s0


def signals(d6, s0, design):
    """noise-free S_i = S0 exp(-b g^T D g), f64 (nvox, n)"""
    beta = np.concatenate([d6, np.log(s0)[:, None]], axis=1)
    return np.exp(beta @ design.T)


def logsig(s):
    s = np.asarray(s, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > 0, np.log(np.where(s > 0, s, 1.0)), 0.0)


# ------------------------------------------------------------------------------------------------------------------ the fits
def fit_ols(s, pinv):
    """beta (nvox, 7) = pinv y"""
    return logsig(s) @ pinv.T


def ols_bound(s, pinv, n):
    """2 (N + 4) 2^-53 sum_i |P_ji| |y_i| per voxel and component: the rounding bound of an N-term dot product plus one ulp
    of log (4 spare terms), doubled because both sides carry it"""
    return 2.0 * (n + 4) * EPS64 * (np.abs(logsig(s)) @ np.abs(pinv).T)


def _tri(i, j):
    return i * 7 - i * (i - 1) // 2 + (j - i)


def fit_wls_cholesky(s, design, pinv):
    """weights w = S^2 (0 where S <= 0); the 28 + 7 sums accumulated measurement by measurement, Cholesky per voxel
    (vectorised over voxels); fewer than 7 positive signals or a pivot that is not > 0 -> the OLS solution.
    -> (beta (nvox, 7), fallback (nvox,) bool)"""
    s = np.asarray(s, np.float64)
    y = logsig(s)
    nvox, n = s.shape
    pos = s > 0
    w = np.where(pos, s * s, 0.0)
    m = np.zeros((28, nvox))
    r = np.zeros((7, nvox))
    for k in range(n):
        for i in range(7):
            wa = w[:, k] * design[k, i]
            r[i] += wa * y[:, k]
            for j in range(i, 7):
                m[_tri(i, j)] += wa * design[k, j]
    ok = pos.sum(1) >= 7
    u = np.zeros((28, nvox))
    inv = np.zeros((7, nvox))
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(7):
            for j in range(i, 7):
                t = m[_tri(i, j)].copy()
                for k in range(i):
                    t -= u[_tri(k, i)] * u[_tri(k, j)]
                if j == i:
                    ok &= t > 0
                    u[_tri(i, i)] = np.sqrt(t)
                    inv[i] = 1.0 / u[_tri(i, i)]
                else:
                    u[_tri(i, j)] = t * inv[i]
        z = np.zeros((7, nvox))
        for i in range(7):
            t = r[i].copy()
            for k in range(i):
                t -= u[_tri(k, i)] * z[k]
            z[i] = t * inv[i]
        beta = np.zeros((7, nvox))
        for i in range(6, -1, -1):
            t = z[i].copy()
            for k in range(i + 1, 7):
                t -= u[_tri(i, k)] * beta[k]
            beta[i] = t * inv[i]
    ols = fit_ols(s, pinv)
    return np.where(ok[:, None], beta.T, ols), ~ok


def fit_wls_lstsq(s, design, pinv, fallback):
    """the same problem through np.linalg.lstsq on sqrt(W) A, voxel by voxel; ``fallback`` voxels take the OLS solution"""
    s = np.asarray(s, np.float64)
    y = logsig(s)
    out = fit_ols(s, pinv)
    for v in np.flatnonzero(~fallback):
        sw = np.where(s[v] > 0, s[v], 0.0)
        out[v] = np.linalg.lstsq(sw[:, None] * design, sw * y[v], rcond=None)[0]
    return out


@functools.lru_cache(maxsize=None)
def fit_case(grid, n, bad=False):
    """One shared case per (grid, N): the scheme, an exact-model f32 series (nvox, n), and every reference solution of it.
    ``bad``: some signals are set <= 0 -- isolated ones in a third of the voxels, and all but 6 in a few voxels (which must
    take the WLS-to-OLS fallback).  Computed once; treat as read-only."""
    nvox = int(np.prod(grid))
    b, g = scheme(n)
    design = design_matrix(b, g)
    pinv = np.linalg.pinv(design)
    d6, s0 = tensor_field(nvox, seed=n)
    s32 = signals(d6, s0, design).astype(np.float32)
    if bad:
        rng = np.random.default_rng(3000 + n + nvox)
        hit = rng.random((nvox, n)) < 0.08
        hit[rng.random(nvox) > 0.34] = False
        few = np.flatnonzero(rng.random(nvox) < 0.1)
        if nvox == 1:
            few = np.array([0])
        hit[few] = True
        hit[few, :6] = False                                 # 6 positive signals left: fewer than the 7 unknowns
        s32 = np.where(hit, np.where(rng.random((nvox, n)) < 0.5, 0.0, -3.0), s32).astype(np.float32)
    s = s32.astype(np.float64)
    chol, fallback = fit_wls_cholesky(s, design, pinv)
    case = dict(grid=grid, n=n, nvox=nvox, bvals=b, bvecs=g, design=design, pinv=pinv, d6=d6, s0=s0, dwi=s32,
                ols=fit_ols(s, pinv), ols_bound=ols_bound(s, pinv, n), wls=chol, fallback=fallback,
                wls_lstsq=fit_wls_lstsq(s, design, pinv, fallback))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def wls_bound(case):
    """(7,) per component: 4 x the largest difference between the two reference solutions of the case.  The unknowns differ in
    scale by four orders of magnitude (D ~ 1e-3, ln S0 ~ 7), so the difference is taken relative to each component's largest
    magnitude in the case, the largest such figure over all voxels AND components is the case's one number, and it is scaled
    back per component.  (Per component alone it can be exactly 0 on a one-voxel grid, which would demand bit identity.)"""
    scale = np.abs(case["wls"]).max(0)
    return 4.0 * (np.abs(case["wls"] - case["wls_lstsq"]) / scale).max() * scale


def roundtrip_bound(case, method):
    """How far a fit of the f32-rounded exact-model series may lie from the generating (D, ln S0), per voxel and component.
    Rounding S to f32 moves y = ln S by at most 2^-24 (1 + 2^-24); the solution is linear in y, beta = Q y with Q = pinv(A)
    (OLS) or (sqrt(W) A)^+ sqrt(W) (WLS), and Q y is exact for exact-model y whatever the weights, so
    |beta - beta_true| <= 2^-24 sum_i |Q_ji| (+ the arithmetic: the OLS rounding bound, or for WLS the conditioning term
    8 cond(sqrt(W) A)^2 2^-53 max|beta| of a Cholesky solve of the normal equations).  Doubled for slack in the first-order step."""
    s = case["dwi"].astype(np.float64)
    if method == "ols":
        return 2.0 * (2.0 ** -24 * np.abs(case["pinv"]).sum(1)[None, :] + case["ols_bound"])
    sa = s[:, :, None] * case["design"][None]
    q = np.linalg.pinv(sa) * s[:, None, :]
    cond = np.linalg.cond(sa)
    beta_max = np.abs(case["wls"]).max(1)
    return 2.0 * (2.0 ** -24 * np.abs(q).sum(2) + (8.0 * cond ** 2 * EPS64 * beta_max)[:, None])


def normalize(v, lo, hi):
    return (np.asarray(v, np.float64) - lo) / (hi - lo)


# -------------------------------------------------------------------------------------------------------------------- ranges
def channel_minmax(x, mask=None, start=None):
    """(C, 2) f32 (min, max) over the voxels with mask != 0, folded into ``start`` (default (+inf, -inf))"""
    x = np.asarray(x, np.float32).reshape(x.shape[0], -1)
    out = np.tile(np.array([np.inf, -np.inf], np.float32), (x.shape[0], 1)) if start is None else np.array(start, np.float32)
    sel = np.ones(x.shape[1], bool) if mask is None else (np.asarray(mask).reshape(-1) != 0)
    if sel.any():
        out[:, 0] = np.minimum(out[:, 0], x[:, sel].min(1))
        out[:, 1] = np.maximum(out[:, 1], x[:, sel].max(1))
    return out


# --------------------------------------------------------------------------------------------------------------------- bSSFP
def phase(raw):
    return np.asarray(raw, np.float64) / 4095.0 * (2.0 * np.pi) - np.pi


def phase_sums(mag, raw):
    """-> (sums (P, 2) f64, sum of |term| (P,)) over the voxels of (P, ...) f32 arrays"""
    m = np.asarray(mag, np.float64).reshape(mag.shape[0], -1)
    ph = phase(raw).reshape(mag.shape[0], -1)
    return np.stack([(m * np.cos(ph)).sum(1), (m * np.sin(ph)).sum(1)], axis=1), np.abs(m).sum(1)


def phase_correct(mag, raw):
    """-> (re, im) f64, every cycle rotated by exp(-j angle(its complex sum))"""
    sums, _ = phase_sums(mag, raw)
    theta = np.arctan2(sums[:, 1], sums[:, 0]).reshape((-1,) + (1,) * (np.ndim(mag) - 1))
    m, ph = np.asarray(mag, np.float64), phase(raw) - theta
    return m * np.cos(ph), m * np.sin(ph)


def assemble(re, im, mask, mag_range, pha_range, repeat_cycle=None):
    """-> (out (2P, ...) f64, raw phase (P, ...) f64 of the cycles as used)"""
    re, im = np.asarray(re, np.float64), np.asarray(im, np.float64)
    if repeat_cycle is not None:
        re, im = np.repeat(re[repeat_cycle][None], re.shape[0], 0), np.repeat(im[repeat_cycle][None], im.shape[0], 0)
    pha = np.arctan2(im, re)
    out = np.empty((2 * re.shape[0],) + re.shape[1:])
    out[0::2] = normalize(np.sqrt(re * re + im * im), *mag_range)
    out[1::2] = normalize(pha, *pha_range)
    if mask is not None:
        out = np.where(np.asarray(mask)[None] != 0, out, 0.0)
    return out, pha


@functools.lru_cache(maxsize=None)
def bssfp_case(p, grid, seed=0):
    """magnitudes in [0, 1000), scanner phases as integers 0 .. 4095 (both exact in f32), and a mask; read-only"""
    rng = np.random.default_rng(4000 + 31 * p + int(np.prod(grid)) + seed)
    mag = rng.uniform(0.0, 1000.0, (p,) + grid).astype(np.float32)
    raw = rng.integers(0, 4096, (p,) + grid).astype(np.float32)
    mask = (rng.random(grid) < 0.7).astype(np.uint8)
    for a in (mag, raw, mask):
        a.setflags(write=False)
    return mag, raw, mask
