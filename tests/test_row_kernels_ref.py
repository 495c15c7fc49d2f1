"""CPU tests of the row-kernel references (tests/row_kernels_ref.py) that tests/test_row_kernels_gpu.py compares the layout,
max-pool and fp8-preparation kernels with: each reference against an independent construction of the same operation (voxel
loops that follow the kernels' own cell arithmetic, F.max_pool3d and its autograd, a nearest-even search over the decoded
e4m3 table), and the sensitivity of the comparison -- the unperturbed result passes, one seeded corruption of it fails."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import row_kernels_ref as R  # noqa: E402

NAN = float("nan")


# ------------------------------------------------------------------------------------------------------------- layout
def _s2d_by_voxel(srcs, dtype, ld, coff, zero_to, cblk, before):
    """The space-to-depth pack voxel by voxel, with the cell arithmetic of elementwise_common.h (s2d_cell, s2d_zero_siblings)."""
    x = torch.cat(list(srcs), 1)
    n, c, D, H, W = x.shape
    out = before.clone()
    row = torch.zeros(zero_to - coff, dtype=dtype)
    for s in range(n):
        for d in range(D):
            for h in range(H):
                for w in range(W):
                    cell = (s, (d + 1) >> 1, (h + 1) >> 1, (w + 1) >> 1)
                    blk = ((d + 1) & 1) * 4 + ((h + 1) & 1) * 2 + ((w + 1) & 1)
                    border = (4 if d in (0, D - 1) else 0) | (2 if h in (0, H - 1) else 0) | (1 if w in (0, W - 1) else 0)
                    row.zero_()
                    row[:c] = x[s, :, d, h, w].to(dtype)
                    out[cell][blk * cblk + coff: blk * cblk + zero_to] = row
                    for sub in range(1, 8):
                        if sub & ~border == 0:
                            out[cell][(blk ^ sub) * cblk + coff: (blk ^ sub) * cblk + zero_to] = 0
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pack_ref_s2d_equals_the_voxel_loop_and_rejects_a_swapped_block(dtype):
    g = torch.Generator().manual_seed(1)
    n, dims, cblk, ld = 2, (4, 6, 8), 16, 136
    x0, x1 = torch.randn(n, 3, *dims, generator=g), torch.randn(n, 2, *dims, generator=g)
    before = torch.full((n, 3, 4, 5, ld), NAN, dtype=dtype)
    val, mask = R.pack_ref([x0, x1], dtype, ld, 8, 16, cblk)
    want = R.written(before, val, mask)
    got = _s2d_by_voxel([x0, x1], dtype, ld, 8, 16, cblk, before)
    assert R.same_bits(got, want)
    assert int(mask.sum()) == n * 3 * 4 * 5 * 8 * 8 and bool(want[..., :8].isnan().all()) and bool(want[..., 128:].isnan().all())
    assert float(want[:, 0, :, :, 8:16].abs().max()) == 0.0            # block 0 of the first plane of cells reads a[-1]: zeros
    bad = got.clone()                                                    # one interior cell with two of its blocks exchanged
    bad[1, 1, 2, 2, 3 * cblk + 8: 3 * cblk + 16] = got[1, 1, 2, 2, 5 * cblk + 8: 5 * cblk + 16]
    bad[1, 1, 2, 2, 5 * cblk + 8: 5 * cblk + 16] = got[1, 1, 2, 2, 3 * cblk + 8: 3 * cblk + 16]
    assert not R.same_bits(bad, want)
    stale = got.clone()                                                  # a border zero block left unwritten
    stale[0, 0, 1, 1, 8:16] = NAN
    assert not R.same_bits(stale, want)
    # unpack is the inverse on the real channels
    assert torch.equal(R.unpack_ref(want, 5, 8, (*dims, cblk)), torch.cat([x0, x1], 1).to(dtype).float())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pack_ref_plain_window_and_mask(dtype):
    g = torch.Generator().manual_seed(2)
    x, y = torch.randn(2, 24, 3, 4, 5, generator=g), torch.randn(2, 6, 3, 4, 5, generator=g)
    val, mask = R.pack_ref([x, y], dtype, 48, 8, 40)
    want = R.written(torch.full(val.shape, NAN, dtype=dtype), val, mask)
    ref = torch.cat([x, y, torch.zeros(2, 2, 3, 4, 5)], 1).to(dtype).permute(0, 2, 3, 4, 1)
    assert torch.equal(want[..., 8:40], ref) and bool(want[..., :8].isnan().all()) and bool(want[..., 40:].isnan().all())
    assert torch.equal(R.unpack_ref(want, 6, 32), y.to(dtype).float())
    neg0 = want.clone()
    neg0[0, 0, 0, 0, 39] = -0.0                                          # the zero padding is +0: bit views tell the two apart
    assert not R.same_bits(neg0, want)


# ------------------------------------------------------------------------------------------------------------- max-pool
@pytest.mark.parametrize("dims", [(4, 6, 16), (5, 7, 9), (2, 2, 2), (3, 2, 2)])
def test_pool_ref_equals_max_pool3d_and_its_autograd(dims):
    n, c = 2, 16
    x, special = R.pool_case(n, dims, c, seed=5)
    g = torch.Generator().manual_seed(6)
    od, oh, ow = (e // 2 for e in dims)
    dy = torch.randn(n, od, oh, ow, c, generator=g)
    r = R.pool_ref(x, dy)
    xt = x.permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    yt, flat = F.max_pool3d(xt, 2, return_indices=True)
    yt.backward(dy.permute(0, 4, 1, 2, 3))
    ok = r.nans <= 1                                                     # torch routes to the LAST NaN of a window
    y_t = yt.detach().permute(0, 2, 3, 4, 1)
    nan = torch.full((), NAN)
    assert R.same_bits(torch.where(ok, r.y, nan), torch.where(ok, y_t, nan))
    fd, fh, fw = flat // (dims[1] * dims[2]), (flat // dims[2]) % dims[1], flat % dims[2]
    where_t = ((fd & 1) * 4 + (fh & 1) * 2 + (fw & 1)).permute(0, 2, 3, 4, 1).to(torch.uint8)
    assert torch.equal(r.where[ok], where_t[ok])
    okv = torch.ones(x.shape, dtype=torch.bool)                          # voxels of windows with two or more NaNs are left out
    for kd, kh, kw in R.SCAN:
        okv[:, kd:2 * od:2, kh:2 * oh:2, kw:2 * ow:2] = ok
    dx_t = xt.grad.permute(0, 2, 3, 4, 1)
    assert R.same_bits(torch.where(okv, r.dx, nan), torch.where(okv, dx_t, nan))
    # the special slots one by one, from the rule itself
    w8 = R._windows(x).reshape(8, -1)
    y, where = r.y.reshape(-1), r.where.reshape(-1)
    for name, s in special.items():
        col = w8[:, s].tolist()
        isn = [v != v for v in col]
        if any(isn):
            assert y[s] != y[s] and int(where[s]) == isn.index(True), name
        else:
            assert float(y[s]) == max(col) and int(where[s]) == col.index(max(col)), name
    assert int(where[special["two_nans"]]) == 3 and int(where[special["eight_nans"]]) == 0 and int(where[special["all_neg_inf"]]) == 0
    assert int(where[special["zero_neg_first"]]) == 2 and int(where[special["zero_pos_first"]]) == 2
    assert torch.signbit(y[special["zero_neg_first"]]) and not torch.signbit(y[special["zero_pos_first"]])


def test_pool_comparison_rejects_a_tie_routed_to_the_second_maximum():
    n, dims, c = 2, (4, 6, 16), 16
    x, _ = R.pool_case(n, dims, c, seed=5)
    g = torch.Generator().manual_seed(7)
    dy = torch.randn(n, 2, 3, 8, c, generator=g)
    add = torch.randn(n, *dims, c, generator=g).to(torch.bfloat16)
    r = R.pool_ref(x.to(torch.bfloat16), dy.to(torch.bfloat16), add)
    assert R.same_bits(r.dx.clone(), r.dx)
    # one rounding of the f32 sum, not two
    exact = r.dx.float() + add.float()
    assert R.same_bits(r.dx_add, exact.to(torch.bfloat16)) and not torch.equal(exact, r.dx_add.float())
    w8 = R._windows(x)
    mx = torch.where(w8.isnan(), torch.full((), float("-inf")), w8).max(0).values
    tied = ((w8 == mx).sum(0) >= 2) & (r.nans == 0) & (dy.to(torch.bfloat16) != 0)
    s, od, oh, ow, ch = (int(v) for v in tied.nonzero()[0])
    hits = (w8[:, s, od, oh, ow, ch] == mx[s, od, oh, ow, ch]).nonzero().flatten().tolist()
    assert int(r.where[s, od, oh, ow, ch]) == hits[0]
    (d0, h0, w0), (d1, h1, w1) = R.SCAN[hits[0]], R.SCAN[hits[1]]
    bad = r.dx.clone()
    bad[s, 2 * od + d1, 2 * oh + h1, 2 * ow + w1, ch] = bad[s, 2 * od + d0, 2 * oh + h0, 2 * ow + w0, ch]
    bad[s, 2 * od + d0, 2 * oh + h0, 2 * ow + w0, ch] = 0.0
    assert not R.same_bits(bad, r.dx)
    bad_where = r.where.clone()
    bad_where[s, od, oh, ow, ch] = hits[1]
    assert not torch.equal(bad_where, r.where)


# ------------------------------------------------------------------------------------------------------------- fp8 preparation
def _e4m3_decode_table():
    """byte -> value from the format itself: 1 sign, 4 exponent (bias 7), 3 mantissa bits; 0x7f / 0xff are NaN, no infinities."""
    out = []
    for b in range(256):
        e, m = (b >> 3) & 15, b & 7
        v = NAN if (e == 15 and m == 7) else (m / 8 * 2.0 ** -6 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7))
        out.append(-v if b & 0x80 else v)
    return torch.tensor(out, dtype=torch.float64)


def _e4m3_nearest_even(x_f32, amax):
    """Saturating round-to-nearest-even onto the decoded table (f64 distances), NaN -> 0x7f, the sign of zero kept."""
    sc = torch.tensor(224.0, dtype=torch.float32) / torch.tensor(float(amax), dtype=torch.float32) if amax > 0 else torch.tensor(1.0)
    t = (x_f32 * sc).double()
    grid = _e4m3_decode_table()[:127]                                    # bytes 0 .. 0x7e: 0 .. 448 ascending
    a = t.abs().clamp(max=448.0)
    a = torch.where(t.isnan(), torch.zeros((), dtype=torch.float64), a)
    hi = torch.bucketize(a, grid).clamp(max=126)                         # first byte with grid >= a
    lo = (hi - 1).clamp(min=0)
    dlo, dhi = a - grid[lo], grid[hi] - a
    pick = torch.where(dlo < dhi, lo, torch.where(dhi < dlo, hi, torch.where(lo % 2 == 0, lo, hi)))
    byte = pick + torch.where(torch.signbit(t), 128, 0)
    return torch.where(t.isnan(), torch.full_like(byte, 0x7F), byte).to(torch.uint8)


@pytest.mark.parametrize("amax", [224.0, 1.0, 3.0, 0.0])
def test_e4m3_ref_over_every_bf16_pattern(amax):
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float()
    ref = R.e4m3_ref(x, amax)
    assert torch.equal(_e4m3_decode_table().float().nan_to_num(nan=-1.0), torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().nan_to_num(nan=-1.0))
    assert torch.equal(R.fold_nan(ref), _e4m3_nearest_even(x, amax))
    assert int(x.isnan().sum()) == 254 and bool(((ref[x.isnan()] & 0x7F) == 0x7F).all())      # the 254 NaN patterns stay NaN
    if amax == 224.0:
        assert len(set(R.fold_nan(ref).tolist())) == 255                 # every byte occurs (0xff folded onto 0x7f)
    if amax == 1.0:                                                       # everything above 2 saturates, on both signs
        assert bool((ref[x > 2.0] == 0x7E).all()) and bool((ref[x < -2.0] == 0xFE).all())


def test_e4m3_comparison_rejects_a_byte_rounded_away_from_even_and_a_lost_nan():
    x = R.e4m3_rounding_probe()
    ref = R.e4m3_ref(x, 224.0)
    assert torch.equal(R.fold_nan(ref), _e4m3_nearest_even(x, 224.0))
    v = torch.unique(R.e4m3_values())
    mids = (v[:-1] + v[1:]) / 2
    mref = R.e4m3_ref(mids, 224.0)
    assert bool(((mref & 1) == 0).all())                                 # a midpoint goes to the even byte ...
    nudged = R.e4m3_ref(torch.nextafter(mids, torch.full_like(mids, float("inf"))), 224.0).view(torch.float8_e4m3fn).float()
    assert torch.equal(nudged, v[1:])                                    # ... and one f32 step above it to the upper neighbour
    sub = mids[(mids > 0) & (mids < 2.0 ** -6)]
    assert sub.numel() == 8 and float(sub[0]) == 2.0 ** -10               # the subnormal range is in the probe
    i = int((x == float(mids[200])).nonzero()[0])
    bad = ref.clone()
    bad[i] = ref[i] + 1 if float(mids[200]) > 0 else ref[i] - 1           # the odd neighbour: equally near, not even
    assert abs(float(bad[i:i + 1].view(torch.float8_e4m3fn).float()) - float(x[i])) == abs(float(ref[i:i + 1].view(torch.float8_e4m3fn).float()) - float(x[i]))
    assert not torch.equal(R.fold_nan(bad), R.fold_nan(ref))
    xn = torch.tensor([1.0, NAN, -NAN, 3.0])
    rn = R.e4m3_ref(xn, 224.0)
    assert R.fold_nan(rn).tolist()[1:3] == [0x7F, 0x7F]
    lost = rn.clone()
    lost[1] = 0xFE                                                        # what fminf(fmaxf(NaN, -448), 448) stores: -448
    assert not torch.equal(R.fold_nan(lost), R.fold_nan(rn))
    flipped = rn.clone()
    flipped[1] = 0xFF                                                     # the other NaN encoding is the same answer
    assert torch.equal(R.fold_nan(flipped), R.fold_nan(rn))


def test_amax_and_scale_roll_refs():
    assert float(R.amax_ref(torch.tensor([1.0, NAN, -7.5, 2.0]))) == 7.5
    assert float(R.amax_ref(torch.tensor([1.0, float("-inf"), NAN]))) == float("inf")
    assert float(R.amax_ref(torch.zeros(5))) == 0.0
    above = float(torch.nextafter(torch.tensor(3.0), torch.tensor(9.0)))
    table = torch.tensor([[0.0, 3.0], [1.5, 0.0], [1.5, 3.0], [1.5, above], [2.0, 1.0], [4.0, 9.0]])
    sat = torch.full((6,), 7, dtype=torch.int32)
    t, s = R.scale_roll_ref(table, 5, sat)
    assert t.tolist() == [[3.0, 0.0], [1.5, 0.0], [3.0, 0.0], [above, 0.0], [1.0, 0.0], [4.0, 9.0]]
    assert s.tolist() == [7, 7, 7, 8, 7, 7]
    assert R.scale_roll_ref(table, 5)[1] is None and torch.equal(R.scale_roll_ref(table, 5)[0], t)
