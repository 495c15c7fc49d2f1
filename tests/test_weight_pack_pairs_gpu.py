"""mi355_weight_pack_multi writes the forward and the data-gradient packing of one tensor from one read of it (dense 3x3x3 and
space-to-depth k4 pairs).  Reference: every descriptor alone through mi355_weight_pack, the element gather.  The list goes
into separate destinations pre-filled with NaN (e4m3: 0x7f, its NaN) and must equal the reference byte for byte, padding
included; the host query confirms that the pairs were formed, so a fall-back to the unpaired kernels cannot pass."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wpack_descs as W  # noqa: E402
from unet_bssfp_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_TORCH = {_lib.DT_F32: torch.float32, _lib.DT_BF16: torch.bfloat16, _lib.DT_FP8: torch.uint8}
_DTYPES = {"bf16": _lib.DT_BF16, "f32": _lib.DT_F32, "e4m3": _lib.DT_FP8}


def _weight(rows, cols, taps, seed, misalign=False):
    """f32 W[rows][cols][taps]; misalign: 4 bytes past a 16-byte boundary (the packers then load 4 bytes at a time)"""
    g = torch.Generator().manual_seed(seed)
    n = rows * cols * taps
    buf = torch.randn(n + 4, generator=g).to(DEV)
    w = buf[1:1 + n] if misalign else buf[:n]
    assert w.data_ptr() % 16 == (4 if misalign else 0)
    return w


def _poisoned(d):
    dt = _TORCH[d.dtype]
    return torch.full((W.packed_elems(d),), 0x7f if dt == torch.uint8 else float("nan"), dtype=dt, device=DEV)


def _check(hip, makers, want_pairs):
    """makers: functions dst -> descriptor.  Packs each alone (reference) and all through the list entry point."""
    stream = torch.cuda.current_stream().cuda_stream
    ref, got, descs = [], [], []
    for make in makers:
        ref.append(_poisoned(make(1)))
        d = make(ref[-1].data_ptr())
        _lib.check(hip.mi355_weight_pack(ctypes.byref(d), stream), "weight_pack")
        got.append(_poisoned(d))
        descs.append(make(got[-1].data_ptr()))
    assert W.pair_count(descs) == want_pairs
    arr = (_lib.WpackDesc * len(descs))(*descs)
    _lib.check(hip.mi355_weight_pack_multi(arr, len(descs), stream), "weight_pack_multi")
    torch.cuda.synchronize()
    for k, (r, g) in enumerate(zip(ref, got)):
        r8, g8 = r.view(torch.uint8), g.view(torch.uint8)
        assert torch.equal(r8, g8), (k, descs[k].cout, descs[k].cin, descs[k].s2d_mode, int((r8 != g8).sum()))


def _amax(w, factor):
    return (w.abs().max() * factor).reshape(1).contiguous()


@pytest.mark.parametrize("dtype", ["bf16", "f32", "e4m3"])
@pytest.mark.parametrize("rows,cols,cinp", [(32, 32, None),    # exact
                                            (48, 24, 32),      # ragged in both roles: forward grid 2 x 4 patches, data gradient 3 x 2
                                            (32, 18, None)])   # row stride not a multiple of 16 bytes: 4-byte loads
def test_dense_pair_matches_the_gather(hip, rows, cols, cinp, dtype):
    dt = _DTYPES[dtype]
    w = _weight(rows, cols, 27, 1)
    # e4m3: each packing scales by its own amax buffer (different values here, so a mixed-up pointer shows)
    qf, qg = (_amax(w, 1.0), _amax(w, 2.0)) if dtype == "e4m3" else (None, None)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    makers = [lambda dst: W.dense_fwd(w.data_ptr(), dst, rows, cols, dt, cinp=cinp, q_amax=ptr(qf)),
              lambda dst: W.dense_dgrad(w.data_ptr(), dst, rows, cols, dt, q_amax=ptr(qg))]
    _check(hip, makers, 1)
    _check(hip, makers[::-1], 1)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("rows,cols,cp", [(24, 16, 16), (64, 30, 32)])
def test_space_to_depth_pair_matches_the_gather(hip, rows, cols, cp, dtype):
    dt = _DTYPES[dtype]
    w = _weight(rows, cols, 64, 2)
    makers = [lambda dst: W.s2d_fwd(w.data_ptr(), dst, rows, cols, cp, dt),
              lambda dst: W.s2d_dgrad(w.data_ptr(), dst, rows, cols, cp, dt)]
    _check(hip, makers, 1)
    _check(hip, makers[::-1], 1)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_mixed_list_matches_the_gather(hip, dtype):
    """22 descriptors (two launch groups of 16): pairs whose members stand far apart, pairs of sources off the 16-byte grid,
    single packings of each family (the unpaired kernels), channel slices and a 1x1x1 packing (the gather)."""
    dt = _DTYPES[dtype]
    dense = [(32, 32, None, False), (48, 24, 32, False), (32, 18, None, False), (32, 96, None, False), (32, 32, None, True)]
    s2d = [(24, 16, 16, False), (64, 30, 32, False), (24, 16, 16, True)]
    fwd, dgrad, keep = [], [], []            # keep: the sources stay allocated while descriptors hold their addresses

    def src(*a):
        keep.append(_weight(*a))
        return keep[-1].data_ptr()
    for k, (rows, cols, cinp, mis) in enumerate(dense):
        p = src(rows, cols, 27, 10 + k, mis)
        fwd.append(lambda dst, a=(p, rows, cols), cinp=cinp: W.dense_fwd(a[0], dst, a[1], a[2], dt, cinp=cinp))
        dgrad.append(lambda dst, a=(p, rows, cols): W.dense_dgrad(a[0], dst, a[1], a[2], dt))
        if cols == 96:       # the skip part of a concat convolution: channels 32..95 of the same weight, both packings
            fwd.append(lambda dst, a=(p, rows, cols): W.dense_fwd(a[0], dst, a[1], a[2], dt, c_off=32, c_n=64))
            dgrad.append(lambda dst, a=(p, rows, cols): W.dense_dgrad(a[0], dst, a[1], a[2], dt, c_off=32, c_n=64))
    for k, (rows, cols, cp, mis) in enumerate(s2d):
        p = src(rows, cols, 64, 20 + k, mis)
        fwd.append(lambda dst, a=(p, rows, cols, cp): W.s2d_fwd(a[0], dst, a[1], a[2], a[3], dt))
        dgrad.append(lambda dst, a=(p, rows, cols, cp): W.s2d_dgrad(a[0], dst, a[1], a[2], a[3], dt))
    lone = src(40, 20, 27, 30), src(24, 16, 64, 31), src(64, 30, 64, 32), src(24, 24, 1, 33)
    singles = [lambda dst: W.dense_fwd(lone[0], dst, 40, 20, dt), lambda dst: W.s2d_fwd(lone[1], dst, 24, 16, 16, dt),
               lambda dst: W.s2d_dgrad(lone[2], dst, 64, 30, 32, dt), lambda dst: W.pointwise(lone[3], dst, 24, 24, dt)]
    makers = fwd + singles + dgrad[::-1]
    assert len(makers) == 22
    _check(hip, makers, len(dense) + len(s2d))
