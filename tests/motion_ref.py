"""Literal f64 restatement of tio.RandomMotion as this project reads it: ITK Euler transforms in index
space, TorchIO's demeaning through ``scipy.linalg.logm / expm``, ``sitk.Resample`` with a linear interpolator and the
channel minimum as the default value, and the band composite through ``numpy.fft`` on the whole 3-D volume.  Test
infrastructure only: the package reaches the same result without any FFT and without scipy (unet_bssfp_amd.augment), and
these functions are what it is compared against.  TorchIO and SimpleITK are absent, so parity with them stays unpinned.

Voxel spacing is 1 and a physical point is its voxel index; spatial axes (0, 1, 2) are x, y, z."""
import numpy as np

from kspace_ref import ft, ift


def euler(degrees, translation, shape):
    """itk.Euler3DTransform, default order R = Rz Rx Ry, centre shape / 2: p_in = R (p_out - c) + c + t, as 4 x 4"""
    ax, ay, az = np.radians(np.asarray(degrees, dtype=np.float64))
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    r = rz @ rx @ ry
    c = np.asarray(shape, dtype=np.float64) / 2
    m = np.eye(4)
    m[:3, :3] = r
    m[:3, 3] = c + np.asarray(translation, dtype=np.float64) - r @ c
    return m


def matrices(degrees, translation, shape):
    """[identity] + the K draws, demeaned: mean = real(expm(mean_k logm(M_k))), M_k <- inv(mean) @ M_k"""
    from scipy.linalg import expm, logm
    ms = [np.eye(4)] + [euler(d, t, shape) for d, t in zip(np.reshape(degrees, (-1, 3)), np.reshape(translation, (-1, 3)))]
    logs = np.stack([logm(m) for m in ms])
    mean = np.real(expm(logs.mean(0)))
    inv = np.linalg.inv(mean)
    return np.stack([inv @ m for m in ms])


def source_coordinates(m, shape):
    """s = M i for every output voxel i: (3, D, H, W)"""
    m = np.asarray(m, dtype=np.float64)
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"))
    return np.tensordot(m[:3, :3], grid, axes=([1], [0])) + m[:3, 3][:, None, None, None]


def resample(x, m, fill=None):
    """sitk.Resample(image, image, transform, sitkLinear, fill) on (..., D, H, W): inside iff -0.5 <= s_a < N_a - 0.5 on
    every axis, then trilinear between floor(s) and floor(s) + 1, both clamped into [0, N_a - 1]; outside ``fill``
    (None: the minimum of that channel, i.e. of each leading index)"""
    x = np.asarray(x, dtype=np.float64)
    shape = x.shape[-3:]
    s = source_coordinates(m, shape)
    n = np.array(shape, dtype=np.float64)[:, None, None, None]
    inside = ((s >= -0.5) & (s < n - 0.5)).all(0)
    f = np.floor(s)
    t = s - f
    f = f.astype(np.int64)
    lo = [np.clip(f[a], 0, shape[a] - 1) for a in range(3)]
    hi = [np.clip(f[a] + 1, 0, shape[a] - 1) for a in range(3)]
    out = np.zeros_like(x)
    for b0, i0 in ((1 - t[0], lo[0]), (t[0], hi[0])):
        for b1, i1 in ((1 - t[1], lo[1]), (t[1], hi[1])):
            for b2, i2 in ((1 - t[2], lo[2]), (t[2], hi[2])):
                out += (b0 * b1 * b2) * x[..., i0, i1, i2]
    fillv = x.min(axis=(-3, -2, -1), keepdims=True) if fill is None else fill
    return np.where(inside, out, fillv)


def band_limits(times, last):
    """TorchIO's sort_spectra and index arithmetic: [(image, ini, fin), ...] in list order, the image at each position
    of the re-ordered list and the bins [ini, fin) of the shifted spectrum along the last axis that it fills"""
    times = np.asarray(times)
    order = list(range(len(times) + 1))
    index = int(np.where(times > 0.5)[0].min()) if np.any(times > 0.5) else len(order) - 1
    order[0], order[index] = order[index], order[0]
    indices = (last * times).astype(int).tolist() + [last]
    out, ini = [], 0
    for image, fin in zip(order, indices):
        out.append((image, ini, fin))
        ini = fin
    return out


def composite(images, times, return_complex=False):
    """TorchIO's add_artifact on one channel: spectra of the images, sort_spectra, bands along the LAST axis in fftshift
    order, inverse transform (the caller keeps the real part)"""
    spectra = [ft(np.asarray(im, dtype=np.float64)) for im in images]
    result = np.zeros_like(spectra[0])                                 # an empty band contributes nothing
    for image, ini, fin in band_limits(times, result.shape[2]):
        result[..., ini:fin] = spectra[image][..., ini:fin]
    y = ift(result)
    return y if return_complex else y.real


def band_response(n, ini, fin):
    """|real(ifft(ifftshift(b)))| for the band b = [ini, fin) of N bins, as the (N, N) matrix of its circular
    convolution: what the error of a copy is weighted with on its way through the composite"""
    b = np.zeros(n)
    b[ini:fin] = 1.0
    g = np.fft.ifft(np.fft.ifftshift(b)).real
    i = np.arange(n)
    return np.abs(g[(i[:, None] - i[None, :]) % n])


def motion(x, times, degrees, translation):
    """the whole stage on (C, D, H, W) or (D, H, W), f64"""
    x = np.asarray(x, dtype=np.float64)
    if not np.any(np.asarray(degrees)) and not np.any(np.asarray(translation)):
        return x.copy()
    ms = matrices(degrees, translation, x.shape[-3:])
    images = [resample(x, m) for m in ms]
    if x.ndim == 3:
        return composite(images, times)
    return np.stack([composite([im[c] for im in images], times) for c in range(x.shape[0])])
