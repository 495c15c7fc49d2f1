"""The row kernels that only move or pick data -- csrc/layout_pack.hip, csrc/pool.hip, csrc/fp8_prep.hip -- against the
index-level references of tests/row_kernels_ref.py (tests/test_row_kernels_ref.py shows that each reference rejects a subtly
wrong result), at the edges where such kernels go wrong: the switch between the two pack forms, ragged last blocks and sample
boundaries inside a block, every window width, rows wider than the channels, NaN / inf / signed zeros, saturation and
rounding ties.  No tolerance: every comparison is `same_bits` (torch.equal on bit views, a NaN compared as a position).  Every
destination is pre-filled with a sentinel (NaN, 0xA5 for bytes) and is wider than what is written: what lies outside the written
range must come back unchanged."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_audit_ref as A  # noqa: E402
import row_kernels_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
DTYPES = [torch.float32, torch.bfloat16]
_DT = {torch.float32: 0, torch.bfloat16: 1}
FAR = 1.0e30          # pad of a SOURCE row beyond its channels: a kernel that read it would report it as the maximum


def _ops():
    from unet_bssfp_amd import ops
    return ops


def _call(rc, what):
    from unet_bssfp_amd import _lib
    _lib.check(rc, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _wide(t, ld, fill=NAN):
    """t (..., c) as the first c channels of rows of ld elements, on the device: (buffer, view)."""
    buf = torch.full((*t.shape[:-1], ld), fill, dtype=t.dtype)
    buf[..., :t.shape[-1]] = t
    buf = buf.to(DEV)
    return buf, buf[..., :t.shape[-1]]


# ------------------------------------------------------------------------------------------------------------- pack
def _pack(srcs, dst, coff, zero_to, cblk=0):
    ops = _ops()
    s = [t.to(DEV) for t in srcs]
    if len(s) == 2:
        ops.pack2(s[0], s[1], dst, coff, zero_to, s2d_cblk=cblk)
    elif cblk:
        ops.pack_ncdhw_s2d(s[0], dst, cblk, coff, zero_to)
    else:
        ops.pack_ncdhw(s[0], dst, coff, zero_to)


def _check_pack(dtype, n, dims, cs, coff, zero_to, ld, seed):
    g = torch.Generator().manual_seed(seed)
    srcs = [torch.randn(n, c, *dims, generator=g) for c in cs]
    before = torch.full((n, *dims, ld), NAN, dtype=dtype)
    dst = before.to(DEV)
    _pack(srcs, dst, coff, zero_to)
    val, mask = R.pack_ref(srcs, dtype, ld, coff, zero_to)
    assert R.same_bits(dst.cpu(), R.written(before, val, mask))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("dims", [(5, 7, 117), (16, 16, 16)], ids=["v4095", "v4096"])
def test_pack_on_both_sides_of_the_form_boundary(hip, dims, n, dtype):
    """pack_impl takes pack_tile_kernel from 4096 voxels on: the same window one voxel below it and at it."""
    _check_pack(dtype, n, dims, (27,), 0, 32, 40, seed=41)


# id, element types, source channels, coff, zero_to, ld
WINDOWS = [
    ("w4_f32", [torch.float32], (3,), 0, 4, 8),
    ("w8_bf16", [torch.bfloat16], (5,), 0, 8, 16),
    ("w32_two_sources", DTYPES, (24, 6), 0, 32, 40),
    ("w64_two_sources", DTYPES, (40, 20), 0, 64, 72),            # zeros at 60 .. 63; f32: the tile would not fit 64 KB of LDS
    ("w32_coff16_ld48", DTYPES, (30,), 16, 48, 48),
    ("w72", DTYPES, (70,), 0, 72, 80),                            # wider than the tile form takes: pack_kernel at any size
]
WINDOW_CASES = [pytest.param(w, dt, id=f"{w[0]}-{str(dt).split('.')[-1]}") for w in WINDOWS for dt in w[1]]


@pytest.mark.parametrize("n,dims", [(2, (3, 7, 197)), (1, (16, 16, 16))], ids=["ragged_n2", "v4096_n1"])
@pytest.mark.parametrize("window,dtype", WINDOW_CASES)
def test_pack_windows(hip, window, dtype, n, dims):
    """Every window width of the tile form (and one beyond it), one and two sources, a window that starts inside the row.
    3 x 7 x 197 = 4137 voxels, two samples: the last block of sample 0 ends mid-block, next to sample 1's rows."""
    _, _, cs, coff, zero_to, ld = window
    _check_pack(dtype, n, dims, cs, coff, zero_to, ld, seed=42)


def test_pack_f32_window_of_64_channels_at_4096_voxels(hip):
    """256 x (64 * 4 + 4) = 66 560 bytes of LDS is more than a launch gets without a raised limit: pack_impl keeps this one
    window on pack_kernel."""
    _check_pack(torch.float32, 2, (16, 16, 16), (61,), 0, 64, 72, seed=43)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["one_window", "two_windows", "two_sources"])
@pytest.mark.parametrize("n,dims", [(1, (16, 16, 16)), (2, (6, 10, 70)), (2, (4, 6, 8))], ids=["16x16x16", "6x10x70", "4x6x8"])
def test_pack_s2d_writes_every_slot_of_its_windows(hip, n, dims, mode, dtype):
    """Space-to-depth pack into a NaN-filled S: every slot of the written windows equals the definition, the zero blocks of the
    border cells included (the kernel owes them: S needs no prior zero-fill); the other channels are still NaN."""
    g = torch.Generator().manual_seed(44)
    cblk, ld = 32, 8 * 32 + 8
    x, y = torch.randn(n, 24, *dims, generator=g), torch.randn(n, 6, *dims, generator=g)
    steps = {"one_window": [([torch.cat([x, y], 1)], 0, 32)], "two_windows": [([x], 0, 24), ([y], 24, 32)],
             "two_sources": [([x, y], 0, 32)]}[mode]
    want = torch.full((n, dims[0] // 2 + 1, dims[1] // 2 + 1, dims[2] // 2 + 1, ld), NAN, dtype=dtype)
    dst = want.to(DEV)
    for srcs, coff, zero_to in steps:
        _pack(srcs, dst, coff, zero_to, cblk)
        val, mask = R.pack_ref(srcs, dtype, ld, coff, zero_to, cblk)
        want = R.written(want, val, mask)
        assert R.same_bits(dst.cpu(), want), (coff, zero_to)
    assert not bool(want[..., :8 * cblk].isnan().any()) and bool(want[..., 8 * cblk:].isnan().all())


# ------------------------------------------------------------------------------------------------------------- unpack / repack
def _unpack(hip, src, c, coff, dims, cblk=0):
    """mi355_unpack_ncdhw(_s2d) into a NaN-filled buffer with 64 floats to spare: (result, spare)."""
    n = src.shape[0]
    d, h, w = dims
    count = n * c * d * h * w
    out = torch.full((count + 64,), NAN, dtype=torch.float32, device=DEV)
    ld = src.stride(3)
    if cblk:
        _call(hip.mi355_unpack_ncdhw_s2d(src.data_ptr(), out.data_ptr(), n, c, d, h, w, cblk, ld, coff, _DT[src.dtype], _stream()), "unpack_s2d")
    else:
        _call(hip.mi355_unpack_ncdhw(src.data_ptr(), out.data_ptr(), n, c, d * h * w, ld, coff, _DT[src.dtype], _stream()), "unpack")
    out = out.cpu()
    return out[:count].view(n, c, d, h, w), out[count:]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("coff", [0, 24])
@pytest.mark.parametrize("c", [1, 5, 6])
def test_unpack_channel_slices_of_wider_rows(hip, c, coff, dtype):
    g = torch.Generator().manual_seed(45)
    n, dims, ld = 2, (3, 7, 13), 40                                      # 273 voxels: a ragged second block
    src = torch.randn(n, *dims, ld, generator=g).to(dtype)
    got, spare = _unpack(hip, src.to(DEV), c, coff, dims)
    assert R.same_bits(got, R.unpack_ref(src, c, coff)) and bool(spare.isnan().all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_unpack_s2d_channel_slice(hip, dtype):
    g = torch.Generator().manual_seed(46)
    n, dims, cblk, ld = 2, (4, 6, 8), 16, 8 * 16 + 8
    src = torch.randn(n, 3, 4, 5, ld, generator=g).to(dtype)
    got, spare = _unpack(hip, src.to(DEV), 5, 8, dims, cblk)
    assert R.same_bits(got, R.unpack_ref(src, 5, 8, (*dims, cblk))) and bool(spare.isnan().all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dims", [(4, 6, 8), (6, 10, 70)])
def test_s2d_repack_of_the_first_channels_of_a_wider_activation(hip, dims, dtype):
    """mi355_s2d_repack: the first 32 channels of a 48-wide activation; the whole result equals the definition, zero border
    blocks included, and nothing beyond the 8 blocks is written."""
    g = torch.Generator().manual_seed(47)
    n, c, lds_, ldd = 2, 32, 48, 8 * 32 + 8
    d, h, w = dims
    x = torch.randn(n, d, h, w, lds_, generator=g).to(dtype)
    dst = torch.full((n, d // 2 + 1, h // 2 + 1, w // 2 + 1, ldd), NAN, dtype=dtype, device=DEV)
    xd = x.to(DEV)
    _call(hip.mi355_s2d_repack(xd.data_ptr(), lds_, dst.data_ptr(), ldd, n, d, h, w, c, _DT[dtype], _stream()), "s2d_repack")
    got = dst.cpu()
    want = R.s2d_cells(x[..., :c].contiguous()).reshape(*got.shape[:4], 8 * c)
    assert R.same_bits(got[..., :8 * c].contiguous(), want) and bool(got[..., 8 * c:].isnan().all())
    assert torch.equal(_ops().s2d_repack(xd, c).cpu(), want)              # the wrapper's own dense result


# ------------------------------------------------------------------------------------------------------------- max-pool
@functools.lru_cache(maxsize=None)
def _pool_case(dims, c):
    """Input, gradients (bf16-exact, so one reference serves both element types) and references, computed once per shape."""
    n = 2
    x, _ = R.pool_case(n, dims, c, seed=50 + c)
    g = torch.Generator().manual_seed(51)
    od, oh, ow = (e // 2 for e in dims)
    dy = torch.randn(n, od, oh, ow, c, generator=g).to(torch.bfloat16).float()
    add = torch.randn(n, *dims, c, generator=g).to(torch.bfloat16).float()
    xt = x.permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    yt = F.max_pool3d(xt, 2)
    yt.backward(dy.permute(0, 4, 1, 2, 3))
    return x, dy, add, yt.detach().permute(0, 2, 3, 4, 1).contiguous(), xt.grad.permute(0, 2, 3, 4, 1).contiguous()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dims", [(4, 6, 16), (5, 7, 9), (2, 2, 2), (3, 2, 2)], ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("c", [16, 48])
def test_maxpool_on_slices_of_wider_buffers(hip, c, dims, dtype):
    """Forward (with and without the recorded window bytes) and both backward entry points, x, y, dy, dx and add each a slice of
    a buffer with its own row width: ties, +0 against -0, an all -inf window, +inf, one NaN at each window position, two and eight
    NaNs (R.pool_case).  Where a window holds at most one NaN the results are also F.max_pool3d's and its autograd's."""
    n = 2
    d, h, w = dims
    od, oh, ow = d // 2, h // 2, w // 2
    x, dy, add, y_t, dx_t = _pool_case(dims, c)
    ref = R.pool_ref(x.to(dtype), dy.to(dtype), add.to(dtype))
    dt = _DT[dtype]
    ldx, ldy, lddy, lddx, ldadd = c + 16, c + 32, c + 48, c + 64, c + 80
    xb, xv = _wide(x.to(dtype), ldx)
    dyb, dyv = _wide(dy.to(dtype), lddy)
    addb, addv = _wide(add.to(dtype), ldadd)
    yb = torch.full((n, od, oh, ow, ldy), NAN, dtype=dtype, device=DEV)
    dxb = torch.full((n, d, h, w, lddx), NAN, dtype=dtype, device=DEV)
    nout = n * od * oh * ow * c
    idx = torch.full((nout + 64,), 0xA5, dtype=torch.uint8, device=DEV)

    def inside(buf, want, what):
        got = buf.cpu()
        assert R.same_bits(got[..., :c].contiguous(), want), what
        assert bool(got[..., c:].isnan().all()), what + ": written beyond c"

    _call(hip.mi355_maxpool2_fwd(xb.data_ptr(), ldx, yb.data_ptr(), ldy, n, c, d, h, w, dt, _stream()), "fwd")
    inside(yb, ref.y, "y")
    yb.fill_(NAN)
    _call(hip.mi355_maxpool2_fwd_idx(xb.data_ptr(), ldx, yb.data_ptr(), ldy, idx.data_ptr(), n, c, d, h, w, dt, _stream()), "fwd_idx")
    inside(yb, ref.y, "y (idx)")
    got_idx = idx.cpu()
    assert torch.equal(got_idx[:nout].view(n, od, oh, ow, c), ref.where) and bool((got_idx[nout:] == 0xA5).all())
    _call(hip.mi355_maxpool2_bwd(xb.data_ptr(), ldx, yb.data_ptr(), ldy, dyb.data_ptr(), lddy, dxb.data_ptr(), lddx, n, c, d, h, w, dt,
                                 _stream()), "bwd")
    inside(dxb, ref.dx, "dx")
    dx_plain = dxb.cpu()[..., :c].float()
    dxb.fill_(NAN)
    _call(hip.mi355_maxpool2_bwd_add(xb.data_ptr(), ldx, yb.data_ptr(), ldy, dyb.data_ptr(), lddy, dxb.data_ptr(), lddx, addb.data_ptr(),
                                     ldadd, n, c, d, h, w, dt, _stream()), "bwd_add")
    inside(dxb, ref.dx_add, "dx + add")
    # the wrappers on the same views (dense results)
    ops = _ops()
    y_o, idx_o = ops.maxpool2_fwd(xv, want_idx=True)
    assert R.same_bits(y_o.cpu(), ref.y) and torch.equal(idx_o.cpu(), ref.where) and R.same_bits(ops.maxpool2_fwd(xv).cpu(), ref.y)
    assert R.same_bits(ops.maxpool2_bwd(xv, y_o, dyv).cpu(), ref.dx) and R.same_bits(ops.maxpool2_bwd(xv, y_o, dyv, addv).cpu(), ref.dx_add)
    # torch itself, where it follows the same rule (it routes to the LAST NaN of a window)
    ok = ref.nans <= 1
    nan = torch.full((), NAN)
    assert R.same_bits(torch.where(ok, yb.cpu()[..., :c].float(), nan), torch.where(ok, y_t, nan))
    okv = torch.ones(n, d, h, w, c, dtype=torch.bool)
    for kd, kh, kw in R.SCAN:
        okv[:, kd:2 * od:2, kh:2 * oh:2, kw:2 * ow:2] = ok
    assert R.same_bits(torch.where(okv, dx_plain, nan), torch.where(okv, dx_t, nan))


# ------------------------------------------------------------------------------------------------------------- amax
def _amax_f32(x_cpu):
    """ops.amax_f32 of x placed in front of FAR-filled memory; the result slot sits between two NaN sentinels."""
    n = x_cpu.numel()
    big = torch.full((n + 64,), FAR)
    big[:n] = x_cpu
    big = big.to(DEV)
    out = torch.full((3,), NAN, device=DEV)
    _ops().amax_f32(big[:n], out=out[1:2])
    out = out.cpu()
    assert bool(out[0].isnan()) and bool(out[2].isnan())
    return out[1]


@pytest.mark.parametrize("n", [1, 2, 3, 5, 1023, 4099])
def test_amax_f32_lengths_that_are_no_multiple_of_four(hip, n):
    g = torch.Generator().manual_seed(60)
    for pos in sorted({0, n - 1, n - n % 4 if n % 4 else n - 1}):      # first, last, first element of the scalar tail
        x = torch.rand(n, generator=g) * 2 - 1
        x[pos] = -7.5                                                     # a negative maximum
        assert torch.equal(R.bits(_amax_f32(x)), R.bits(torch.tensor(7.5))), pos
    assert torch.equal(R.bits(_amax_f32(torch.zeros(n))), R.bits(torch.tensor(0.0)))
    x = torch.rand(n, generator=g)
    x[n - 1] = float("-inf")
    assert float(_amax_f32(x)) == float("inf")
    if n > 1:
        x = torch.rand(n, generator=g)                                    # a NaN beside finite values is ignored
        x[n - 1] = NAN
        assert torch.equal(R.bits(_amax_f32(x)), R.bits(R.amax_ref(x)))
    assert float(_amax_f32(torch.full((n,), NAN))) == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_amax_act_of_a_channel_slice_with_the_maximum_in_the_last_row(hip, dtype):
    g = torch.Generator().manual_seed(61)
    rows, c, ld = 1031, 48, 64
    x = torch.randn(1, 1, 1, rows, c, generator=g).to(dtype)
    x[0, 0, 0, rows - 1, c - 1] = -9.5
    x[0, 0, 0, 7, 3] = NAN
    _, xv = _wide(x, ld, FAR)
    out = torch.full((3,), NAN, device=DEV)
    _ops().amax_act(xv, out=out[1:2])
    out = out.cpu()
    assert torch.equal(R.bits(out[1]), R.bits(torch.tensor(9.5))) and bool(out[0].isnan()) and bool(out[2].isnan())


# ------------------------------------------------------------------------------------------------------------- e4m3 cast
def _cast(hip, x, ld_src, amax, nxt, ld_dst, delayed=True):
    """mi355_cast_fp8(_delayed) of the rows x (rows, c) held in a FAR-padded buffer of ld_src columns into 0xA5-filled bytes."""
    rows, c = x.shape
    _, xv = _wide(x, ld_src, FAR)
    am = torch.tensor([amax], dtype=torch.float32, device=DEV)
    nx = None if nxt is None else torch.tensor([NAN, nxt, NAN], dtype=torch.float32, device=DEV)
    dst = torch.full((rows, ld_dst), 0xA5, dtype=torch.uint8, device=DEV)
    if delayed:
        _call(hip.mi355_cast_fp8_delayed(xv.data_ptr(), ld_src, c, rows, _DT[x.dtype], am.data_ptr(), None if nx is None else nx[1:2].data_ptr(),
                                         dst.data_ptr(), ld_dst, _stream()), "cast_fp8_delayed")
    else:
        _call(hip.mi355_cast_fp8(xv.data_ptr(), ld_src, c, rows, _DT[x.dtype], am.data_ptr(), dst.data_ptr(), ld_dst, _stream()), "cast_fp8")
    dst = dst.cpu()
    assert bool((dst[:, c:] == 0xA5).all()), "bytes beyond c written"
    if nx is not None:
        nx = nx.cpu()
        assert bool(nx[0].isnan()) and bool(nx[2].isnan())
        nx = nx[1]
    return dst[:, :c].contiguous(), nx


_EVERY_BF16 = {}


def _every_bf16(hip, amax):
    if amax not in _EVERY_BF16:
        x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).view(4096, 16)
        got, nxt = _cast(hip, x, 16, amax, 0.0, 32)
        plain, _ = _cast(hip, x, 16, amax, None, 32, delayed=False)
        _EVERY_BF16[amax] = (x, got, nxt, plain)
    return _EVERY_BF16[amax]


@pytest.mark.parametrize("amax", [224.0, 1.0, 3.0, 0.0])
@pytest.mark.parametrize("part", ["numbers", "nan"])
def test_cast_fp8_of_every_bf16_pattern(hip, part, amax):
    """All 65 536 bf16 patterns as a (1, 16, 16, 16, 16) activation, the amax slot set by hand (224: scale 1; 1: everything
    above 2 saturates on both signs; 3: a scale that is no power of two; 0: scale 1).  `numbers`: the finite values and +-inf
    (-> +-448); `nan`: the 254 NaN patterns, which must stay NaN bytes (either sign).  The gathered amax is not looked at here: half
    of these NaN patterns are signaling, which the amax chain does not drop the way it drops a quiet NaN (measured: 3.39e38, the
    largest finite bf16, instead of inf) -- arithmetic never produces one, and how amax treats NaN is not this file's subject."""
    x, got, _, plain = _every_bf16(hip, amax)
    ref = R.e4m3_ref(x.float(), amax)
    sel = x.float().isnan() if part == "nan" else ~x.float().isnan()
    assert int(sel.sum()) == (254 if part == "nan" else 65536 - 254)
    assert torch.equal(R.fold_nan(got)[sel], R.fold_nan(ref)[sel])
    assert torch.equal(R.fold_nan(plain)[sel], R.fold_nan(ref)[sel])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("prefill", [0.0, 1.0e6])
@pytest.mark.parametrize("amax", [224.0, 3.0])
def test_cast_fp8_rounding_probe_in_wide_rows(hip, amax, prefill, dtype):
    """Every e4m3 value, the midpoint between every pair of neighbours and the f32 neighbours of both (round-to-nearest-even, the
    subnormal range), then random values, as 1031 rows of 48 channels (three 16-channel groups) in rows of 64;
    amax_next is raised to the finite maximum and never lowered."""
    g = torch.Generator().manual_seed(62)
    rows, c = 1031, 48
    probe = R.e4m3_rounding_probe() * (amax / 224.0)
    x = torch.randn(rows * c, generator=g) * 100.0
    x[:probe.numel()] = probe
    x = x.view(rows, c).to(dtype)
    got, nxt = _cast(hip, x, 64, amax, prefill, 64)
    assert torch.equal(R.fold_nan(got), R.fold_nan(R.e4m3_ref(x.float(), amax)))
    assert torch.equal(R.bits(nxt), R.bits(torch.maximum(torch.tensor(prefill), R.amax_ref(x))))


@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_nan_policy_of_cast_and_amax(hip, dtype):
    """A (quiet) NaN element yields a NaN byte -- so it reaches the convolution's output -- while amax_act and the amax the cast
    gathers keep ignoring it: the scale stays that of the finite values."""
    g = torch.Generator().manual_seed(64)
    rows, c = 37, 32
    x = (torch.randn(rows, c, generator=g) * 3).to(dtype)
    x[0, 0] = x[17, 21] = NAN
    x[36, 31] = -NAN
    got, nxt = _cast(hip, x, 48, 5.0, 0.0, 48)
    ref = R.e4m3_ref(x.float(), 5.0)
    assert torch.equal((R.fold_nan(got) == 0x7F), x.isnan()) and torch.equal(R.fold_nan(got), R.fold_nan(ref))
    assert torch.equal(R.bits(nxt), R.bits(R.amax_ref(x)))
    _, xv = _wide(x.view(1, 1, 1, rows, c), 48, FAR)
    assert torch.equal(R.bits(_ops().amax_act(xv).cpu()[0]), R.bits(R.amax_ref(x)))


# ------------------------------------------------------------------------------------------------------------- scale roll
def _roll_table():
    i = torch.arange(320, dtype=torch.float32)
    use = 0.5 + i * 0.01
    nx = use * 1.5
    k = torch.arange(320) % 5
    use = torch.where(k == 0, torch.zeros(()), use)                      # no history: adopts the value, no count
    nx = torch.where(k == 1, torch.zeros(()), nx)                        # nothing gathered: keeps the one in use
    nx = torch.where(k == 2, 2.0 * use, nx)                              # exactly twice: nothing clamped
    nx = torch.where(k == 3, torch.nextafter(2.0 * use, torch.full((), float("inf"))), nx)      # one f32 step more: counted once
    return torch.stack([use, nx], 1).contiguous()


@pytest.mark.parametrize("n", [1, 256, 257, 300])
def test_fp8_scale_roll_rows_and_the_saturation_edge(hip, n):
    table = _roll_table()
    sat = torch.full((320,), 7, dtype=torch.int32)
    want_t, want_s = R.scale_roll_ref(table, n, sat)
    td, sd = table.to(DEV), sat.to(DEV)
    _ops().fp8_scale_roll(td, n, sd)
    assert torch.equal(R.bits(td.cpu()), R.bits(want_t)) and torch.equal(sd.cpu(), want_s)
    assert torch.equal(R.bits(td.cpu()[n:]), R.bits(table[n:])) and bool((sd.cpu()[n:] == 7).all())      # rows >= n: untouched
    assert int((want_s[:n] - 7).sum()) == len([i for i in range(n) if i % 5 == 3])
    td = table.to(DEV)
    _ops().fp8_scale_roll(td, n, None)                                    # no saturation record
    assert torch.equal(R.bits(td.cpu()), R.bits(want_t))


# ------------------------------------------------------------------------------------------------------------- e4m3 weights
def test_fp8_weight_pack_keeps_a_nan_weight(hip):
    """mi355_weight_pack, dtype fp8: amax ignores the NaN weight, the packed byte of that weight decodes to NaN, every other
    byte is the e4m3 cast of w * 224 / amax."""
    ops = _ops()
    g = torch.Generator().manual_seed(63)
    src = torch.randn(40, 24, 3, 3, 3, generator=g)
    src[7, 5, 1, 2, 0] = NAN
    srcd = src.to(DEV)
    amax = ops.amax_f32(srcd)
    a = float(amax.cpu()[0])
    assert a == float(R.amax_ref(src))
    wp, coutp, cinp = ops.weight_pack(srcd, 40, 24, 3, 24 * 27, 27, (9, 3, 1), (0, 0, 0), (1, 1, 1), ops.FP8, q_amax=amax)
    exp = A.pack_expect(src, 40, 24, coutp, cinp, 3, 24 * 27, 27, (9, 3, 1), (0, 0, 0), (1, 1, 1))
    got = A.decode_wp(wp.cpu().reshape(-1), A.FP8, cinp, 27, coutp)
    assert int(exp.isnan().sum()) == 1
    want = R.e4m3_ref(exp, a).view(torch.float8_e4m3fn).float()
    assert R.same_bits(got, want)
