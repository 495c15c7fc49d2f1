"""Literal f64 restatements of tio.RandomGhosting, tio.RandomSpike and tio.RandomBlur (TorchIO 0.19.6 as this project
reads it) on one real channel of shape (N0, N1, N2): ghosting and spike through ``numpy.fft`` on the whole
3-D volume, blur through ``scipy.ndimage.gaussian_filter``.  Test infrastructure only: the package reaches the same
results without any FFT (unet_bssfp_amd.augment), and these functions are what it is compared against.  TorchIO is
absent, so parity with TorchIO itself stays unpinned."""
import numpy as np


def ft(x):
    return np.fft.fftshift(np.fft.fftn(x))


def ift(s):
    return np.fft.ifftn(np.fft.ifftshift(s))


def ghosting(x, num_ghosts, axis, intensity, return_complex=False):
    """the planes s[::n] along ``axis`` times 1 - I, the centre plane restored, real part of the inverse"""
    x = np.asarray(x, dtype=np.float64)
    if num_ghosts == 0 or intensity == 0:
        return x.copy()
    s = ft(x)
    centre = [slice(None)] * 3
    centre[axis] = slice(x.shape[axis] // 2, x.shape[axis] // 2 + 1)
    kept = s[tuple(centre)].copy()
    planes = [slice(None)] * 3
    planes[axis] = slice(None, None, num_ghosts)
    s[tuple(planes)] *= 1.0 - intensity
    s[tuple(centre)] = kept
    y = ift(s)
    return y if return_complex else y.real


def spectrum_maximum(x):
    """numpy's complex maximum of the shifted spectrum (largest real part, ties by larger imaginary part)"""
    return ft(np.asarray(x, dtype=np.float64)).max()


def spike(x, positions, intensity, return_maxima=False):
    """for each position in order: s[floor(position * shape)] += max(s) * I on the CURRENT spectrum; real part of the
    inverse"""
    x = np.asarray(x, dtype=np.float64)
    s = ft(x)
    maxima = []
    for pos in np.asarray(positions, dtype=np.float64).reshape(-1, 3):
        idx = tuple(np.floor(pos * np.array(x.shape)).astype(int))
        maxima.append(s.max())
        s[idx] += maxima[-1] * intensity
    y = ift(s).real
    return (y, maxima) if return_maxima else y


def blur(x, sigmas):
    """scipy.ndimage.gaussian_filter with scipy's defaults (truncate 4, mode 'reflect'), spacing 1 voxel"""
    from scipy.ndimage import gaussian_filter
    return gaussian_filter(np.asarray(x, dtype=np.float64), sigmas)


def top_two_real_parts(x):
    """the two largest real parts of the spectrum, a conjugate pair counted once"""
    s = np.fft.fftn(np.asarray(x, dtype=np.float64))
    n = np.array(x.shape)
    idx = np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing="ij"), -1).reshape(-1, 3)
    conj = (-idx) % n
    flat = np.ravel_multi_index(idx.T, n)
    cflat = np.ravel_multi_index(conj.T, n)
    keep = flat <= cflat                                 # one member of every pair (self-conjugate bins once)
    re = np.sort(s.real.ravel()[keep])
    return re[-1], re[-2]
