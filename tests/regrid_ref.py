"""f64 numpy restatement of unet_bssfp_amd/csrc/regrid_core.h and the cases the regridding tests share.

Output voxel i = (i_D, i_H, i_W) reads the source at s_a = m[4a] i_D + m[4a+1] i_H + m[4a+2] i_W + m[4a+3], three fused
multiply-adds per axis (exact here: rational arithmetic, rounded once per fma).  Inside iff -0.5 <= s_a < N_a - 0.5 on every
axis; outside voxels take ``fill``.  Order 0: tap floor(s + 0.5) clamped.  Order 1: taps floor(s), floor(s) + 1 clamped.
Order 3: taps floor(s) - 1 .. floor(s) + 2 mirrored about the centres of the edge voxels, read from the prefiltered
coefficients.  The sums run with axis D outermost, taps ascending, every product and sum rounded separately (the device may
contract a product and a sum into one fma: that is what the bounds of the GPU tests leave room for).

The prefilter runs along W, then H, then D, as the kernels do.  Nothing here reads the package."""
import functools
from fractions import Fraction

import numpy as np

EPS64 = 2.0 ** -53
POLE = np.sqrt(3.0) - 2.0
assert POLE == -0.2679491924311228                           # the literal of regrid_core.h
GAIN = 6.0
PREFILTER_GAIN = 27.0                                       # L-infinity gain of the three-axis prefilter: 3 per axis

# (source, output) extents
PAIRS = [((1, 5, 7), (3, 4, 5)),                            # an axis of extent 1
         ((2, 3, 9), (4, 4, 4)),                            # extent 2: the recursion's loops are empty
         ((5, 7, 9), (6, 5, 11)),
         ((17, 16, 33), (9, 20, 40)),                       # crosses an LDS row tile, odd W
         ((3, 4, 130), (3, 4, 70))]                         # W lines longer than two waves
MATRICES = ("rot", "down", "perm")
CASES = [(src, dst, name) for src, dst in PAIRS for name in MATRICES]
NEAREST_CASES = [(src, dst, "rot") for src, dst in PAIRS[:4]]          # no rounding tie within the tolerance
IDENTITY_SHAPES = [src for src, _ in PAIRS]
SHIFT_SHAPES = [src for src, _ in PAIRS[2:]]                # (1, -2, 3) leaves an extent-1 or extent-3 axis (almost) empty
EXACT_CASES = [(s, s, "identity") for s in IDENTITY_SHAPES] + [(s, s, "shift") for s in SHIFT_SHAPES]
SHIFT = (1, -2, 3)
FILLS = (0.0, -1.5)


def matrix(name, src, dst):
    """(3, 4) f64 index matrix: a linear part L centred by off = (src - 1) / 2 - L (dst - 1) / 2"""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    extra = np.zeros(3)
    if name == "identity":
        return np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    if name == "shift":
        return np.concatenate([np.eye(3), np.asarray(SHIFT, np.float64)[:, None]], 1)
    if name == "rot":
        c, s = np.cos(0.3), np.sin(0.3)
        lin = 0.8 * np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.diag([1.2, 0.9, 2.1])
        extra = np.array([0.21, -0.33, 0.4])
    elif name == "down":
        lin = np.diag(src / dst)
    elif name == "perm":
        lin = 0.37 * np.array([[0.0, 1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])      # a reoriented file
    else:
        raise ValueError(name)
    off = (src - 1) / 2 - lin @ ((dst - 1) / 2) + extra
    return np.ascontiguousarray(np.concatenate([lin, off[:, None]], 1))


@functools.lru_cache(maxsize=None)
def volume(c, shape):
    """(c, *shape) f32, read-only: smooth part + noise + offset, so that neighbours differ and the sign changes"""
    rng = np.random.default_rng(1000 * c + int(np.prod(shape)) + shape[2])
    g = np.meshgrid(*[np.linspace(-1, 1, n) if n > 1 else np.zeros(1) for n in shape], indexing="ij")
    x = np.stack([2.0 * np.sin(2.1 * g[0] + 1.3 * g[1] * (k + 1) - 0.7 * g[2]) + rng.standard_normal(shape) + 0.5 for k in range(c)])
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------------------------------------------------- prefilter
def powi(z, e):
    r, b = 1.0, z
    while e:
        if e & 1:
            r *= b
        b *= b
        e >>= 1
    return r


def prefilter_axis(x, axis):
    """the recursion of regrid_prefilter_line along one axis of an f64 array, every other index at once"""
    c = np.moveaxis(np.array(x, dtype=np.float64), axis, 0)
    n = c.shape[0]
    if n < 2:
        return np.moveaxis(c, 0, axis)
    z = POLE
    zn1 = powi(z, n - 1)
    zi = z
    c0 = GAIN * c[0] + zn1 * (GAIN * c[n - 1])
    for i in range(1, n - 1):
        c0 = c0 + zi * (GAIN * c[i] + zn1 * (GAIN * c[n - 1 - i]))
        zi *= z
    c0 = c0 / (1.0 - zn1 * zn1)
    prev = before = c0
    c[0] = c0
    for i in range(1, n):
        before = prev
        prev = GAIN * c[i] + z * prev
        c[i] = prev
    prev = (z * before + prev) * z / (z * z - 1.0)
    c[n - 1] = prev
    for i in range(n - 2, -1, -1):
        prev = z * (prev - c[i])
        c[i] = prev
    return np.moveaxis(c, 0, axis)


def prefilter(x):
    """(..., D, H, W) samples -> f64 cubic B-spline coefficients (mirror boundaries): along W, then H, then D"""
    c = np.asarray(x, dtype=np.float64)
    for axis in (-1, -2, -3):
        c = prefilter_axis(c, axis)
    return c


# ----------------------------------------------------------------------------------------------------------- coordinates
def _fma(a, b, c):
    """round(a b + c) with ONE rounding, elementwise: b a non-negative integer array"""
    fa = Fraction(a)
    return np.array([float(fa * int(bi) + Fraction(ci)) for bi, ci in zip(b.ravel(), c.ravel())]).reshape(c.shape)


def coordinates(m, out_shape):
    """(3, D', H', W') f64: fma(m2, i_W, fma(m1, i_H, fma(m0, i_D, m3))) per axis"""
    od, oh, ow = out_shape
    m = np.asarray(m, np.float64).reshape(-1)[:12].reshape(3, 4)
    out = np.zeros((3, od, oh, ow))
    for a in range(3):
        u = _fma(m[a, 0], np.arange(od), np.full(od, m[a, 3]))
        v = _fma(m[a, 1], np.broadcast_to(np.arange(oh), (od, oh)), np.broadcast_to(u[:, None], (od, oh)).copy())
        out[a] = _fma(m[a, 2], np.broadcast_to(np.arange(ow), (od, oh, ow)), np.broadcast_to(v[:, :, None], (od, oh, ow)).copy())
    return out


def inside(s, src_shape):
    n = np.asarray(src_shape, np.float64).reshape(3, 1, 1, 1)
    return np.all((s >= -0.5) & (s < n - 0.5), axis=0)


def near_boundary(s, src_shape):
    """voxels whose coordinate lies within 1e-9 (1 + N_a) of an inside boundary on some axis"""
    n = np.asarray(src_shape, np.float64).reshape(3, 1, 1, 1)
    tol = 1e-9 * (1 + n)
    return np.any((np.abs(s + 0.5) <= tol) | (np.abs(s - (n - 0.5)) <= tol), axis=0)


def near_tie(s, src_shape):
    """... or, for order 0, within that distance of a rounding tie (s + 0.5 an integer)"""
    n = np.asarray(src_shape, np.float64).reshape(3, 1, 1, 1)
    r = s + 0.5
    return np.any(np.abs(r - np.round(r)) <= 1e-9 * (1 + n), axis=0)


def clamp(i, n):
    return np.clip(i, 0, n - 1)


def mirror(i, n):
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def taps(s, n, order):
    """([T] index arrays, [T] weight arrays) of one axis"""
    if order == 0:
        return [clamp(np.floor(s + 0.5).astype(np.int64), n)], [np.ones_like(s)]
    f = np.floor(s)
    t, a = s - f, f.astype(np.int64)
    if order == 1:
        return [clamp(a, n), clamp(a + 1, n)], [1.0 - t, t]
    u, t2 = 1.0 - t, t * t
    t3 = t2 * t
    w = [u * u * u / 6.0, (3.0 * t3 - 6.0 * t2 + 4.0) / 6.0, (-3.0 * t3 + 3.0 * t2 + 3.0 * t + 1.0) / 6.0, t3 / 6.0]
    return [mirror(a - 1 + k, n) for k in range(4)], w


def regrid(src, m, out_shape, order, fill=0.0, s=None):
    """src: (C, D, H, W) samples (orders 0, 1) or coefficients (order 3) -> ((C, D', H', W') f64, inside mask, coordinates).
    Outside voxels hold ``fill``; the inside values are NOT rounded to f32."""
    src = np.asarray(src, dtype=np.float64)
    s = coordinates(m, out_shape) if s is None else s
    ins = inside(s, src.shape[1:])
    safe = np.where(ins[None], s, 0.0)
    (i0, w0), (i1, w1), (i2, w2) = (taps(safe[a], src.shape[1 + a], order) for a in range(3))
    out = np.zeros((src.shape[0],) + tuple(out_shape))
    for ch in range(src.shape[0]):
        acc0 = 0.0
        for a in range(len(i0)):
            acc1 = 0.0
            for b in range(len(i1)):
                acc2 = 0.0
                for c in range(len(i2)):
                    acc2 = acc2 + w2[c] * src[ch][i0[a], i1[b], i2[c]]
                acc1 = acc1 + w1[b] * acc2
            acc0 = acc0 + w0[a] * acc1
        out[ch] = np.where(ins, acc0, fill)
    return out, ins, s


# ----------------------------------------------------------------------------------------------------------- shared cases
@functools.lru_cache(maxsize=None)
def case(src, dst, name, c=3):
    """everything a test needs of one case, computed once and read-only: the volume, its coefficients, the matrix, the
    coordinates, the masks and the f64 reference per order (fill 0)"""
    x = volume(c, src)
    m = matrix(name, src, dst)
    s = coordinates(m, dst)
    coef = prefilter(x)
    out = {"x": x, "coef": coef, "m": m, "s": s, "inside": inside(s, src), "boundary": near_boundary(s, src),
           "tie": near_tie(s, src), "xmax": float(np.abs(x).max())}
    for order, source in ((0, x), (1, x), (3, coef)):
        out[order] = regrid(source, m, dst, order, 0.0, s)[0]
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def coefficient_bound(xmax, k=64.0):
    """k f64 ulps of 27 max|x|"""
    return k * EPS64 * PREFILTER_GAIN * xmax
