"""Literal f64 restatement of the spatial stages of the patch feed: the index-space matrices of a flip and
of an affine, the crop / pad that comes before them, the trilinear resample of the padded volume (``motion_ref``'s) and the
reorientation of a diffusion tensor, done voxel by voxel as ``R D R^T`` with 3 x 3 products and a rotation taken from the
polar decomposition through an eigen-decomposition -- never through a 6 x 6 map or an SVD, which is how the package does it.
Test infrastructure only.  TorchIO is absent, so parity with it stays unpinned.

Voxel spacing is 1 and a physical point is its voxel index; spatial axes (0, 1, 2) are x, y, z."""
import numpy as np

import motion_ref as R

COMPONENTS = ["xx", "xy", "xz", "yy", "yz", "zz"]
_INDEX = {"x": 0, "y": 1, "z": 2}


def flip(axes, shape):
    """output index i reads (T - 1) - i along every flipped axis"""
    m = np.eye(4)
    for a in axes:
        m[a, a], m[a, 3] = -1.0, shape[a] - 1.0
    return m


def affine(scales, degrees, translation, shape):
    """p_in = c + Rz Rx Ry diag(1 / s) (i - c) + t about the centre c = (shape - 1) / 2 of the voxel grid, assembled from
    homogeneous 4 x 4 factors"""
    ax, ay, az = np.radians(np.asarray(degrees, dtype=np.float64))
    rot = np.eye(4)
    rot[:3, :3] = (np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
                   @ np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
                   @ np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]]))
    zoom = np.diag(list(1.0 / np.asarray(scales, dtype=np.float64)) + [1.0])
    c = (np.asarray(shape, dtype=np.float64) - 1.0) / 2.0
    to_centre, back = np.eye(4), np.eye(4)
    to_centre[:3, 3] = -c
    back[:3, 3] = c + np.asarray(translation, dtype=np.float64)
    return back @ rot @ zoom @ to_centre


def chain(matrices):
    """resampling through M_1, then through M_2, ...: y_1(i) = x(M_1 i), y_2(i) = y_1(M_2 i) = x(M_1 M_2 i)"""
    out = np.eye(4)
    for m in matrices:
        out = out @ m
    return out


def crop_or_pad(x, target, value=0.0):
    """tio.CropOrPad(target, 0) on (C, D, H, W): centred, the odd voxel dropped or added at the far end"""
    x = np.asarray(x, dtype=np.float64)
    for ax, t in enumerate(target, start=1):
        n = x.shape[ax]
        if n > t:
            lo = (n - t) // 2
            x = np.take(x, np.arange(lo, lo + t), axis=ax)
        elif n < t:
            lo = (t - n) // 2
            width = [(0, 0)] * x.ndim
            width[ax] = (lo, t - n - lo)
            x = np.pad(x, width, constant_values=value)
    return x


def rotation_of(m):
    """the finite-strain rotation of F = inv(M[:3, :3]): R = F (F^T F)^(-1/2), the inverse root from the eigen-decomposition
    of the symmetric positive definite F^T F"""
    f = np.linalg.inv(np.asarray(m, dtype=np.float64)[:3, :3])
    lam, v = np.linalg.eigh(f.T @ f)
    return f @ (v @ np.diag(lam ** -0.5) @ v.T)


def tensor_of(n6):
    """(6, ...) components xx, xy, xz, yy, yz, zz -> (..., 3, 3) symmetric matrices"""
    d = np.zeros(n6.shape[1:] + (3, 3))
    for k, name in enumerate(COMPONENTS):
        a, b = _INDEX[name[0]], _INDEX[name[1]]
        d[..., a, b] = n6[k]
        d[..., b, a] = n6[k]
    return d


def components_of(d):
    return np.stack([d[..., _INDEX[name[0]], _INDEX[name[1]]] for name in COMPONENTS])


def denormalise(n6, rescale):
    """the inverse of the reference's rescale of the tensor components: D = n |max - min| + min"""
    r = np.asarray(rescale, dtype=np.float64)
    shape = (6,) + (1,) * (n6.ndim - 1)
    return n6 * np.abs(r[:, 1] - r[:, 0]).reshape(shape) + r[:, 0].reshape(shape)


def normalise(d6, rescale):
    r = np.asarray(rescale, dtype=np.float64)
    shape = (6,) + (1,) * (d6.ndim - 1)
    return (d6 - r[:, 0].reshape(shape)) / np.abs(r[:, 1] - r[:, 0]).reshape(shape)


def reorient(n6, rot, rescale=None):
    """R D R^T in every voxel of a (6, ...) array, on denormalised values when a rescale is given"""
    d6 = n6 if rescale is None else denormalise(n6, rescale)
    d = rot @ tensor_of(d6) @ rot.T
    out = components_of(d)
    return out if rescale is None else normalise(out, rescale)


def inside(m, shape):
    s = R.source_coordinates(m, shape)
    n = np.array(shape, dtype=np.float64)[:, None, None, None]
    return ((s >= -0.5) & (s < n - 0.5)).all(0)


def spatial(x, m, fill=None, tensor=False, rescale=None, rotation_from=None):
    """(C, D, H, W) already cropped / padded -> resampled through ``m`` (outside: ``fill``, None = the channel minimum);
    a tensor image is reoriented where the point is inside, by the rotation of ``rotation_from`` (default ``m``).
    -> (result, sampled): ``sampled`` is the volume before the reorientation"""
    x = np.asarray(x, dtype=np.float64)
    sampled = R.resample(x, m, fill)
    if not tensor:
        return sampled, sampled
    rot = rotation_of(m if rotation_from is None else rotation_from)
    return np.where(inside(m, x.shape[1:])[None], reorient(sampled, rot, rescale), sampled), sampled
