"""Weight-pack descriptors as unet_bssfp_amd.functional.ConvSpec builds them, from plain numbers: shared by the host-side
and the GPU tests of the paired re-pack (mi355_weight_pack_multi writes a forward and a data-gradient packing of one tensor
from one read of it).  `src` / `dst` are addresses; W is the torch weight [rows][cols][k^3] in f32."""
from unet_bssfp_amd import _lib


def round_up(x, m):
    return (x + m - 1) // m * m


def _desc(src, dst, cout, cin, coutp, cinp, ks, s_co, s_ci, s_k, tbase, tstep, dtype, s2d_mode=0, s2d_cp=0, q_amax=None):
    d = _lib.WpackDesc(src=src, dst=dst, cout=cout, cin=cin, coutp=coutp, cinp=cinp, ks=ks, s_co=s_co, s_ci=s_ci, dtype=dtype,
                       s2d_mode=s2d_mode, s2d_cp=s2d_cp, q_amax=q_amax)
    d.s_k[:] = s_k
    d.tbase[:] = tbase
    d.tstep[:] = tstep
    return d


def dense_fwd(src, dst, rows, cols, dtype, cinp=None, c_off=0, c_n=None, q_amax=None):
    """Forward packing of a 3x3x3 weight W[rows = cout][cols = cin][27]; (c_off, c_n): a channel slice of it."""
    c_n = cols if c_n is None else c_n
    return _desc(src + 4 * 27 * c_off, dst, rows, c_n, round_up(rows, 32), cinp or round_up(c_n, 16), 3, cols * 27, 27, (9, 3, 1),
                 (0, 0, 0), (1, 1, 1), dtype, q_amax=q_amax)


def dense_dgrad(src, dst, rows, cols, dtype, cinp=None, c_off=0, c_n=None, q_amax=None):
    """Data-gradient packing of the same weight: roles swapped, taps flipped."""
    c_n = cols if c_n is None else c_n
    return _desc(src + 4 * 27 * c_off, dst, c_n, rows, round_up(c_n, 32), cinp or round_up(rows, 16), 3, 27, cols * 27, (9, 3, 1),
                 (2, 2, 2), (-1, -1, -1), dtype, q_amax=q_amax)


def s2d_fwd(src, dst, rows, cols, cp, dtype):
    """Forward packing of a k4 s2 weight W[rows = cout][cols = cin][64] for the space-to-depth formulation."""
    return _desc(src, dst, rows, cols, round_up(rows, 32), 8 * cp, 2, cols * 64, 64, (16, 4, 1), (0, 0, 0), (2, 2, 2), dtype,
                 s2d_mode=1, s2d_cp=cp)


def s2d_dgrad(src, dst, rows, cols, cp, dtype):
    return _desc(src, dst, cols, rows, 8 * cp, round_up(rows, 16), 2, 64, cols * 64, (16, 4, 1), (2, 2, 2), (-2, -2, -2), dtype,
                 s2d_mode=2, s2d_cp=cp)


def pointwise(src, dst, rows, cols, dtype):
    """Forward packing of a 1x1x1 weight W[rows][cols]: neither dense 3x3x3 nor space-to-depth, so it takes the gather."""
    return _desc(src, dst, rows, cols, round_up(rows, 32), round_up(cols, 16), 1, cols, 1, (1, 1, 1), (0, 0, 0), (1, 1, 1), dtype)


def packed_elems(d):
    return d.cinp * d.ks ** 3 * d.coutp


def pair_count(descs):
    arr = (_lib.WpackDesc * len(descs))(*descs)
    return _lib.load().mi355_weight_pack_multi_pairs(arr, len(descs))
