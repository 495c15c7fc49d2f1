"""Descriptors for the host-side plan table (tests/test_conv_plans_host.py, tools/gen_golden_conv_plans.py).

Both convolution planners are pure host code: they read the integer fields of a descriptor and test a few pointers for
null, so they can be queried on a machine without a GPU with a dummy address in every pointer.  This module holds
  * the flattening of a descriptor into a row of integers (pointers become 0 / 1) and back,
  * the deterministic sweeps of forward and weight-gradient descriptors, and
  * the queries whose results the table pins.
The sweeps are code, so only their expected results live in tests/golden/conv_plans.npz; the descriptors captured from real
training steps live there as rows."""
import ctypes as C
import itertools

import numpy as np

from unet_bssfp_amd import _lib

DUMMY = 256                     # any non-null address: no planner dereferences a pointer
F32, BF16, FP8 = _lib.DT_F32, _lib.DT_BF16, _lib.DT_FP8
REJECTED = -1                   # every result column of a descriptor the planner refuses

FWD_RESULTS = ("plan_id", "seg_len", "tiles", "tiles_per_sample", "workspace_bytes")
WGRAD_RESULTS = ("kind", "workspace_bytes")


# ------------------------------------------------------------------------------------------------ descriptor <-> integer row
def columns(cls):
    """Column names of a flattened descriptor: one per scalar or pointer field, three per int[3] field."""
    out = []
    for name, typ in cls._fields_:
        out += [f"{name}[{i}]" for i in range(typ._length_)] if hasattr(typ, "_length_") else [name]
    return out


def flatten(d):
    """Every integer field of a descriptor; a pointer becomes 1 (non-null) or 0."""
    row = []
    for name, typ in type(d)._fields_:
        v = getattr(d, name)
        if typ is C.c_void_p:
            row.append(1 if v else 0)
        elif hasattr(typ, "_length_"):
            row += [int(e) for e in v]
        else:
            row.append(int(v))
    return row


def unflatten(cls, row):
    d, it = cls(), iter(int(v) for v in row)
    for name, typ in cls._fields_:
        if typ is C.c_void_p:
            setattr(d, name, DUMMY if next(it) else None)
        elif hasattr(typ, "_length_"):
            setattr(d, name, typ(*[next(it) for _ in range(typ._length_)]))
        else:
            setattr(d, name, next(it))
    return d


# ------------------------------------------------------------------------------------------------ the pinned queries
def query_fwd(lib, d):
    """(plan id, d-segment length, statistics rows, rows per sample, split-K workspace bytes), or REJECTED five times."""
    pid = lib.mi355_conv_plan_id(C.byref(d))
    if pid < 0:
        return (REJECTED,) * 5
    tiles, tps = C.c_int32(0), C.c_int32(0)
    rc = lib.mi355_conv_num_tiles(C.byref(d), C.byref(tiles), C.byref(tps))
    assert rc == 0, rc
    return (pid, lib.mi355_conv_plan_seg_len(C.byref(d)), tiles.value, tps.value, lib.mi355_conv_workspace_bytes(C.byref(d)))


def query_wgrad(lib, d):
    kind = lib.mi355_conv_wgrad_plan_kind(C.byref(d))
    return (REJECTED,) * 2 if kind < 0 else (kind, lib.mi355_conv_wgrad_workspace(C.byref(d)))


def table(lib, query, descs, width):
    return np.array([query(lib, d) for d in descs], dtype=np.int64).reshape(-1, width)


# ------------------------------------------------------------------------------------------------ forward sweep
def out_extent(e, ks, stride, pad):
    return (e + 2 * pad - ks) // stride + 1


def fwd_desc(n, ext, c0, c1, coutp, ks, stride, pad, dtype, *, cstore=None, ld_extra=0, os=1, ooff=(0, 0, 0), out_ext=None,
             cls_cout=0, stats=False, addend=False, y_f32=0, add_n=0, d2s=0, delta=False, add_bf16=0, grid=None):
    d = _lib.ConvDesc()
    d.x0, d.c0, d.ld0 = DUMMY, c0, c0 + ld_extra
    if c1:
        d.x1, d.c1, d.ld1 = DUMMY, c1, c1 + ld_extra
    d.n = n
    d.di, d.hi, d.wi = ext
    g = grid if grid is not None else tuple(out_extent(e, ks, stride, pad) for e in ext)
    d.do_, d.ho, d.wo = g
    d.ks, d.stride = ks, stride
    d.pad = (C.c_int32 * 3)(pad, pad, pad)
    d.wp, d.coutp = DUMMY, coutp
    cstore = coutp if cstore is None else cstore
    d.y, d.ldy, d.cstore = DUMMY, cstore + ld_extra, cstore
    d.dy, d.hy, d.wy = out_ext if out_ext is not None else tuple((e - 1) * os + 1 + max(ooff) if os > 1 else e for e in g)
    d.os = os
    d.ooff = (C.c_int32 * 3)(*ooff)
    d.stats_part = DUMMY if stats else None
    d.dtype = dtype
    if dtype == FP8:
        d.q_amax_x = d.q_amax_w = DUMMY
    d.cls_cout = cls_cout
    if addend:
        d.addend, d.ld_add = DUMMY, (coutp // 8 if d2s else coutp) + ld_extra
    d.y_f32, d.add_n, d.d2s, d.add_bf16 = y_f32, add_n, d2s, add_bf16
    d.delta = DUMMY if delta else None
    return d


def _cube(e):
    return (e, e, e)


# the 128^3, 64^3 and 160^3 level ladders, extents 2^k + 1 (space-to-depth operands and their gradients), thin and other
# non-cubic volumes
EXTENTS = [_cube(e) for e in (128, 64, 32, 16, 8, 4, 160, 80, 40, 20, 10, 129, 65, 33, 17, 9)] + \
          [(128, 64, 8), (8, 64, 128), (64, 128, 16), (96, 80, 48), (40, 24, 56), (20, 33, 65)]
BATCHES = (1, 2, 8)
CHANNELS = [(16, 0), (32, 0), (48, 0), (64, 0), (128, 0), (256, 0), (512, 0), (16, 16), (32, 32), (64, 64), (128, 128)]
COUTP = (32, 64, 96, 256)
GEOMETRY = [(1, 1, 0), (2, 1, 0), (2, 1, 1), (3, 1, 1), (3, 1, 0), (3, 2, 1), (4, 2, 1), (2, 2, 0)]     # (ks, stride, pad)
DTYPES = (F32, BF16, FP8)


def fwd_sweep():
    """The deterministic forward sweep, in a fixed order."""
    out = []
    for n, ext, (c0, c1), coutp, (ks, st, pad), dt in itertools.product(BATCHES, EXTENTS, CHANNELS, COUTP, GEOMETRY, DTYPES):
        out.append(fwd_desc(n, ext, c0, c1, coutp, ks, st, pad, dt))
    small = [_cube(e) for e in (64, 32, 16, 8, 33, 17)] + [(128, 64, 8), (40, 24, 56)]
    # rows wider than the channels, a stored width below coutp, fused statistics
    for n, ext, (c0, c1), coutp, (ks, st, pad) in itertools.product((1, 8), small, [(32, 0), (64, 64)], (32, 128), GEOMETRY):
        out.append(fwd_desc(n, ext, c0, c1, coutp, ks, st, pad, BF16, ld_extra=16, stats=True))
        out.append(fwd_desc(n, ext, c0, c1, coutp, ks, st, pad, BF16, cstore=coutp - 8))
        out.append(fwd_desc(n, ext, c0, c1, coutp, ks, st, pad, BF16, cstore=coutp - 12))
    # stride-2 parity classes: the output grid is every second voxel of y from an offset
    for n, ext, c0, coutp, ks, ooff in itertools.product((1, 8), small, (64, 256), (32, 128), (1, 2, 3),
                                                         [(0, 0, 0), (1, 0, 1), (1, 1, 1)]):
        pad = 1 if ks == 3 else 0
        g = tuple(out_extent(e, ks, 1, pad) for e in ext)
        out.append(fwd_desc(n, ext, c0, 0, coutp, ks, 1, pad, BF16, os=2, ooff=ooff, out_ext=tuple(2 * e for e in g)))
    # dense k2 with an addend / an f32 output (the PatchGAN's split first block), padding 0 and 1
    for n, ext, c0, coutp, pad, (addend, y_f32, add_n) in itertools.product(
            (1, 2, 8), [_cube(e) for e in (65, 33, 17, 64, 32)] + [(65, 33, 9)], (32, 64, 256, 48), (32, 64, 128), (0, 1),
            [(True, 0, 0), (True, 1, 0), (False, 1, 0), (True, 1, 1)]):
        out.append(fwd_desc(n, ext, c0, 0, coutp, 2, 1, pad, BF16, addend=addend, y_f32=y_f32, add_n=add_n))
    # depth-to-space (transposed k4 s2 p1 convolution as dense k2 over 8 output classes)
    for n, ext, c0, coutp, (addend, add_bf16, delta) in itertools.product(
            (1, 2, 8), [_cube(e) for e in (64, 32, 16, 8, 4, 80, 40, 20, 10)] + [(64, 32, 4), (20, 40, 80)], (32, 64, 256, 48),
            (256, 512, 128), [(False, 0, False), (True, 0, True), (True, 1, True)]):
        out.append(fwd_desc(n, ext, c0, 0, coutp, 2, 1, 0, BF16, grid=ext, out_ext=tuple(2 * e for e in ext), cstore=coutp // 8,
                            d2s=1, addend=addend, add_bf16=add_bf16, delta=delta, stats=True))
    # transposed convolution k2 s2 with its 8 classes folded into the GEMM columns
    for n, ext, c0, cls, dt, stats in itertools.product((1, 2, 8), [_cube(e) for e in (64, 32, 16, 8, 4, 80, 10)] + [(64, 32, 4)],
                                                        (32, 64, 128, 256, 512), (64, 128, 32), (BF16, F32), (False, True)):
        out.append(fwd_desc(n, ext, c0, 0, 8 * cls, 1, 1, 0, dt, os=2, out_ext=tuple(2 * e for e in ext), cstore=cls - 8,
                            cls_cout=cls, stats=stats))
    return out


# ------------------------------------------------------------------------------------------------ weight-gradient sweep
def wgrad_desc(n, ext, c0, c1, cg, ks, stride, pad, dtype, *, ld_extra=0, gs=1, goff=(0, 0, 0), g_ext=None, s2d_cp=0,
               g_cls_cout=0, xn=0, cin=None, cout=None):
    d = _lib.WgradDesc()
    d.x0, d.c0, d.ld0 = DUMMY, c0, c0 + ld_extra
    if c1:
        d.x1, d.c1, d.ld1 = DUMMY, c1, c1 + ld_extra
    d.n = n
    d.di, d.hi, d.wi = ext
    d.g, d.cg, d.ldg = DUMMY, cg, cg + ld_extra
    g = tuple(out_extent(e, ks, stride, pad) for e in ext)
    d.do_, d.ho, d.wo = g
    d.gd, d.gh, d.gw = g_ext if g_ext is not None else tuple(gs * e for e in g)
    d.gs = gs
    d.goff = (C.c_int32 * 3)(*goff)
    d.ks, d.stride = ks, stride
    d.pad = (C.c_int32 * 3)(pad, pad, pad)
    d.dw = DUMMY
    d.cin = (s2d_cp if s2d_cp else c0 + c1) if cin is None else cin
    d.cout = (g_cls_cout if g_cls_cout else cg) if cout is None else cout
    k3 = ks ** 3
    d.s_co, d.s_ci = d.cin * k3, k3
    d.s_k = (C.c_int64 * 3)(ks * ks, ks, 1)
    d.tbase = (C.c_int32 * 3)(0, 0, 0)
    d.tstep = (C.c_int32 * 3)(1, 1, 1)
    d.dtype = dtype
    d.s2d_cp, d.g_cls_cout, d.xn = s2d_cp, g_cls_cout, xn
    return d


W_EXTENTS = [_cube(e) for e in (128, 64, 32, 16, 8, 4, 160, 80, 40, 20, 10, 65, 33, 17, 9)] + \
            [(128, 64, 8), (8, 64, 128), (96, 80, 48), (20, 33, 65)]
W_CHANNELS = [(16, 0), (32, 0), (64, 0), (256, 0), (32, 32), (128, 128)]
W_CG = (16, 32, 64, 256)
W_GEOMETRY = [(1, 1, 0), (2, 1, 0), (3, 1, 1), (3, 2, 1), (4, 2, 1), (2, 1, 1)]


def wgrad_sweep():
    out = []
    for n, ext, (c0, c1), cg, (ks, st, pad), dt in itertools.product(BATCHES, W_EXTENTS, W_CHANNELS, W_CG, W_GEOMETRY, (F32, BF16)):
        out.append(wgrad_desc(n, ext, c0, c1, cg, ks, st, pad, dt))
    small = [_cube(e) for e in (64, 32, 8, 33)] + [(128, 64, 8)]
    for n, ext, (c0, c1), cg, (ks, st, pad) in itertools.product((1, 8), small, [(32, 0), (64, 64)], (32, 128), W_GEOMETRY):
        out.append(wgrad_desc(n, ext, c0, c1, cg, ks, st, pad, BF16, ld_extra=8))
        out.append(wgrad_desc(n, ext, c0, c1, cg, ks, st, pad, BF16, ld_extra=4))                 # rows off 16-byte alignment
        out.append(wgrad_desc(n, ext, c0, c1, cg, ks, st, pad, BF16, gs=2, goff=(1, 0, 1)))       # g on a strided grid
        if n == 8:
            out.append(wgrad_desc(n, ext, c0, c1, cg, ks, st, pad, BF16, xn=2))                   # one input under several gradients
    # the transposed-conv class form: g is the 2x tensor, its 8 classes are GEMM columns
    for n, ext, c0, cls, ld_extra in itertools.product(BATCHES, [_cube(e) for e in (64, 32, 16, 8, 4, 80, 10)] + [(64, 32, 4), (6, 10, 64)],
                                                       (32, 64, 256, 512), (32, 64, 128, 48), (0, 8)):
        out.append(wgrad_desc(n, ext, c0, 0, cls, 1, 1, 0, BF16, g_ext=tuple(2 * e for e in ext), g_cls_cout=cls, ld_extra=ld_extra))
    # space-to-depth operand (the PatchGAN's k4 s2 p1 layers as dense k2)
    for n, ext, cp, cg in itertools.product(BATCHES, [_cube(e) for e in (65, 33, 17, 9, 5)] + [(65, 33, 9)], (8, 16, 32), (32, 64, 256)):
        out.append(wgrad_desc(n, ext, 8 * cp, 0, cg, 2, 1, 0, BF16, s2d_cp=cp, cin=cp - 2))
    return out
