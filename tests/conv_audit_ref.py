"""Descriptor-level reference of mi355_conv_fwd / mi355_conv_wgrad (include/mi355_unet.h), for the in-situ launch audit
(tests/test_conv_audit.py) and its CPU self-tests (tests/test_conv_audit_ref.py).

A descriptor is a ``types.SimpleNamespace`` with the field names of ``mi355_conv_desc`` / ``mi355_wgrad_desc``; every pointer
field holds a HOST tensor instead (flat, starting at the pointer, of the element type: float32, bfloat16 or uint8 for e4m3) or
None, and the fp8 scale pointers hold the float read at launch time.  Nothing here knows about tiles, plans or split-K: the
functions evaluate the formulas of the header on the exact operands.

Precision: the full-tensor references run in f32 on the decoded operands (a product of two bf16 or two e4m3 values is exact
in f32), the sampled ones in f64.  ``A = sum |x w|`` per output element comes with every forward reference: it bounds the
f32 accumulation error of any summation order (the bounds in ``fwd_errors``).
"""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

F32, BF16, FP8 = 0, 1, 3
_ELEM = {F32: torch.float32, BF16: torch.bfloat16, FP8: torch.uint8}


def elem_type(dtype):
    return _ELEM[dtype]


def fp8_mult(amax):
    """Decode multiplier of an e4m3 operand stored as e4m3(v * 224 / amax) (scale 1 when amax is 0: common.h fp8_scale_of)."""
    return float(amax) / 224.0 if amax is not None and float(amax) > 0.0 else 1.0


def decode(flat, dtype, amax=None):
    """Host element tensor -> f32 values (e4m3 bytes are viewed as float8_e4m3fn and scaled by amax / 224)."""
    if dtype == FP8:
        v = flat.view(torch.float8_e4m3fn).float()
        m = fp8_mult(amax)
        return v * m if m != 1.0 else v
    return flat.float()


def rows(flat, nrows, c, ld):
    """Rows of an NDHWC activation with row pitch ld: a [nrows, c] strided view of the flat buffer."""
    assert flat.numel() >= (nrows - 1) * ld + c, (flat.numel(), nrows, c, ld)
    return flat.as_strided((nrows, c), (ld, 1))


def act_extent(nrows, c, ld):
    """Elements a [nrows][ld] activation slice of c channels spans from its first element."""
    return (nrows - 1) * ld + c


# ------------------------------------------------------------------------------------------------------------- weights
def decode_wp(wp, dtype, cinp, taps, coutp, amax=None):
    """Packed weights [cinp/16][taps][coutp][16] (ci = chunk * 16 + e) -> the GEMM form w[tap][co][ci] (f32)."""
    w = decode(wp[: cinp * taps * coutp], dtype, amax).view(cinp // 16, taps, coutp, 16)
    return w.permute(1, 2, 0, 3).reshape(taps, coutp, cinp)


def pack_expect(src, cout, cin, coutp, cinp, ks, s_co, s_ci, s_k, tbase, tstep, s2d_mode=0, s2d_cp=0):
    """What mi355_weight_pack must produce, in the GEMM form w[tap][co][ci] (f32, before any fp8 scaling):
    src[co s_co + ci s_ci + sum_a (tbase_a + tstep_a t_a + bit_a(blk)) s_k_a], zero where co >= cout or ci >= cin."""
    src = src.reshape(-1)
    taps = ks ** 3
    t = torch.arange(taps)
    td, th, tw = t // (ks * ks), (t // ks) % ks, t % ks
    co = torch.arange(coutp).view(1, -1, 1)
    ci = torch.arange(cinp).view(1, 1, -1)
    blk = torch.zeros(1, 1, 1, dtype=torch.long)
    cor, cir = co, ci
    if s2d_mode == 1:
        blk, cir = ci // s2d_cp, ci % s2d_cp
    elif s2d_mode == 2:
        blk, cor = co // s2d_cp, co % s2d_cp
    ok = (cor < cout) & (cir < cin) & (blk < 8)
    k0 = (tbase[0] + tstep[0] * td).view(-1, 1, 1) + (blk >> 2)
    k1 = (tbase[1] + tstep[1] * th).view(-1, 1, 1) + ((blk >> 1) & 1)
    k2 = (tbase[2] + tstep[2] * tw).view(-1, 1, 1) + (blk & 1)
    idx = cor * s_co + cir * s_ci + k0 * s_k[0] + k1 * s_k[1] + k2 * s_k[2]
    idx = torch.where(ok, idx, torch.zeros_like(idx))
    return torch.where(ok, src[idx], torch.zeros((), dtype=src.dtype))


# ------------------------------------------------------------------------------------------------------------- forward
def _x(d):
    """The virtual concat [x0 | x1] of a descriptor, decoded: f32 [n, di, hi, wi, c0 + c1]."""
    nr = d.n * d.di * d.hi * d.wi
    amax = getattr(d, "q_amax_x", None) if d.dtype == FP8 else None
    parts = [decode(rows(d.x0, nr, d.c0, d.ld0), d.dtype, amax)]
    if d.x1 is not None and d.c1 > 0:
        parts.append(decode(rows(d.x1, nr, d.c1, d.ld1), d.dtype, amax))
    return torch.cat(parts, 1).view(d.n, d.di, d.hi, d.wi, -1)


def _w(d, cx):
    """GEMM weights w[tap][col][ci] of a forward descriptor (ci < cx)."""
    cinp = -(-cx // 16) * 16
    amax = getattr(d, "q_amax_w", None) if d.dtype == FP8 else None
    return decode_wp(d.wp, d.dtype, cinp, d.ks ** 3, d.coutp, amax)[:, :, :cx]


def _bias_vec(d, width):
    b = torch.zeros(width)
    if d.bias is not None:
        nb = d.nbias if d.nbias > 0 else d.coutp
        k = min(nb, width)
        b[:k] = d.bias[:k].float()
    return b


def _pad_ncdhw(x, lo, grid, stride, ks):
    """x [n, c, D, H, W] -> zero-padded so that input index i = p * stride + t - lo is (p * stride + t) of the result for every
    p < grid, t < ks; returns (padded, None)."""
    pads = []
    for a in (2, 1, 0):                                  # F.pad order: last dimension first
        e = x.shape[2 + a]
        need = (grid[a] - 1) * stride + ks
        hi = max(0, need - lo[a] - e)
        pads += [lo[a], hi]
    return F.pad(x, pads)


def _dense(xs, w, ks, stride, lo, grid, dt):
    """sum_{tap, ci} x[n, p stride + tap - lo, ci] w[tap][col][ci] for p < grid: [n, grid..., cols] (F.conv3d on dt).
    xs: [n, D, H, W, c] (dt), w: [taps][cols][c]."""
    x = xs.permute(0, 4, 1, 2, 3)
    xp = _pad_ncdhw(x, lo, grid, stride, ks)
    taps, cols, c = w.shape
    wt = w.permute(1, 2, 0).reshape(cols, c, ks, ks, ks).to(dt)
    z = F.conv3d(xp.to(dt), wt, None, stride)
    z = z[:, :, : grid[0], : grid[1], : grid[2]]
    return z.permute(0, 2, 3, 4, 1).contiguous()


def _class_bits(blk):
    return (blk >> 2) & 1, (blk >> 1) & 1, blk & 1


def _addend(d, width):
    """The addend in the output geometry: f32 [add_n or n, dy, hy, wy, width] (None when absent)."""
    if d.addend is None:
        return None
    na = d.add_n if d.add_n > 0 else d.n
    nr = na * d.dy * d.hy * d.wy
    a = rows(d.addend, nr, width, d.ld_add).float()
    return a.view(na, d.dy, d.hy, d.wy, width)


def _border_class(e):
    """0 first / 1 interior / 2 last voxel along an axis of extent e."""
    c = torch.ones(e, dtype=torch.long)
    c[0] = 0
    c[-1] = 2
    return c


def conv_fwd_ref(d, dt=torch.float32, with_abs=True):
    """Full reference of one mi355_conv_fwd descriptor in the OUTPUT tensor's geometry.
    Returns SimpleNamespace(acc, absum, bias, written, width):
      acc    [n, dy, hy, wy, width]  the accumulator (conv sum + addend + border delta, no bias) of every written voxel;
      absum  the same geometry: sum |x w| (+ |addend| + |delta|), the scale of the f32 summation error;
      bias   [width] the bias the epilogue adds (channel co < nbias);
      written [n, dy, hy, wy] bool: the voxels the launch writes (channels [0, cstore)).
    width = coutp (plain), cls_cout (ConvTranspose3d class folding) or coutp / 8 (depth-to-space)."""
    xs = _x(d)
    cx = xs.shape[-1]
    w = _w(d, cx)
    n, oshape = d.n, (d.dy, d.hy, d.wy)
    grid = (d.do_, d.ho, d.wo)
    if d.d2s:
        width = d.coutp // 8
    elif d.cls_cout:
        width = d.cls_cout
    else:
        width = d.coutp
    acc = torch.zeros(n, *oshape, width, dtype=dt)
    absum = torch.zeros(n, *oshape, width, dtype=dt) if with_abs else None
    written = torch.zeros(n, *oshape, dtype=torch.bool)
    if d.d2s:
        # class b = (bd, bh, bw): voxel 2 j + b = dense k2 convolution of the cells j - (1 - b) + e, e in {0, 1}
        for blk in range(8):
            b = _class_bits(blk)
            lo = tuple(1 - bb for bb in b)
            wb = w[:, blk * width:(blk + 1) * width, :]
            z = _dense(xs, wb, 2, 1, lo, grid, dt)
            sl = (slice(None), slice(b[0], None, 2), slice(b[1], None, 2), slice(b[2], None, 2))
            acc[sl] = z
            written[sl] = True
            if with_abs:
                absum[sl] = _dense(xs.abs(), wb.abs(), 2, 1, lo, grid, dt)
        if d.delta is not None:
            cls = (_border_class(d.dy).view(-1, 1, 1) * 9 + _border_class(d.hy).view(1, -1, 1) * 3 + _border_class(d.wy).view(1, 1, -1))
            dl = d.delta.float().view(27, -1)[:, :width].to(dt)
            corr = dl[cls]                                # [dy, hy, wy, width]; class 13 (interior) is never applied
            corr[cls == 13] = 0
            acc += corr
            if with_abs:
                absum += corr.abs()
    else:
        lo = tuple(d.pad)
        z = _dense(xs, w, d.ks, d.stride, lo, grid, dt)                            # [n, grid, coutp]
        za = _dense(xs.abs(), w.abs(), d.ks, d.stride, lo, grid, dt) if with_abs else None
        if d.cls_cout:
            for blk in range(8):
                b = _class_bits(blk)
                sl = (slice(None),) + tuple(slice(bb, bb + 2 * g - 1, 2) for bb, g in zip(b, grid))
                acc[sl] = z[..., blk * width:(blk + 1) * width]
                written[sl] = True
                if with_abs:
                    absum[sl] = za[..., blk * width:(blk + 1) * width]
        else:
            sl = (slice(None),) + tuple(slice(o, o + d.os * (g - 1) + 1, d.os) for o, g in zip(d.ooff, grid))
            acc[sl] = z
            written[sl] = True
            if with_abs:
                absum[sl] = za
    add = _addend(d, width)
    if add is not None:
        reps = n // add.shape[0]
        addn = add.repeat(reps, 1, 1, 1, 1) if reps > 1 else add      # grid sample i starts from addend sample i % add_n
        acc = torch.where(written[..., None], acc + addn.to(dt), acc)
        if with_abs:
            absum = torch.where(written[..., None], absum + addn.abs().to(dt), absum)
    return SimpleNamespace(acc=acc, absum=absum, bias=_bias_vec(d, width), written=written, width=width)


def conv_fwd_sampled(d, idx, dt=torch.float64):
    """The same accumulator (and A) at sampled written voxels, evaluated as one explicit f64 dot product each.
    idx: long [S, 4] of (n, od, oh, ow) in the OUTPUT tensor's coordinates (written voxels).  Returns (acc, absum) [S, width]."""
    xs = _x(d).to(dt)
    cx = xs.shape[-1]
    w = _w(d, cx).to(dt)
    width = d.coutp // 8 if d.d2s else (d.cls_cout if d.cls_cout else d.coutp)
    S = idx.shape[0]
    acc = torch.zeros(S, width, dtype=dt)
    absum = torch.zeros(S, width, dtype=dt)
    ks = 2 if d.d2s else d.ks
    taps = ks ** 3
    t = torch.arange(taps)
    tap3 = torch.stack([t // (ks * ks), (t // ks) % ks, t % ks], 1)            # [taps, 3]
    nn_, q = idx[:, 0], idx[:, 1:]
    ext = torch.tensor([d.di, d.hi, d.wi])
    if d.d2s or d.cls_cout:
        b = q % 2
        p = q // 2
        base = p + b - 1 if d.d2s else p                                       # d2s: first cell of class b's window
        cls = b[:, 0] * 4 + b[:, 1] * 2 + b[:, 2]
    else:
        p = (q - torch.tensor(d.ooff)) // d.os
        base = p * d.stride - torch.tensor(d.pad)
        cls = torch.zeros(S, dtype=torch.long)
    for blk in torch.unique(cls).tolist():
        sel = (cls == blk).nonzero().view(-1)
        wb = w[:, blk * width:(blk + 1) * width, :] if (d.d2s or d.cls_cout) else w
        wm = wb.permute(0, 2, 1).reshape(-1, width)                               # [taps * cx, width]
        for c0 in range(0, sel.numel(), 4096):
            s_ = sel[c0:c0 + 4096]
            pos = base[s_][:, None, :] + tap3[None]                               # [s, taps, 3]
            ok = ((pos >= 0) & (pos < ext)).all(-1)
            posc = torch.where(ok[..., None], pos, torch.zeros_like(pos))
            patch = xs[nn_[s_][:, None], posc[..., 0], posc[..., 1], posc[..., 2]] * ok[..., None].to(dt)   # [s, taps, cx]
            patch = patch.reshape(s_.numel(), -1)
            acc[s_] = patch @ wm
            absum[s_] = patch.abs() @ wm.abs()
    if d.d2s and d.delta is not None:
        dl = d.delta.to(dt).view(27, -1)[:, :width]
        def bc(v, e):
            return torch.where(v == 0, 0, torch.where(v == e - 1, 2, 1))
        cls = bc(q[:, 0], d.dy) * 9 + bc(q[:, 1], d.hy) * 3 + bc(q[:, 2], d.wy)
        corr = dl[cls] * (cls != 13).to(dt)[:, None]
        acc += corr
        absum += corr.abs()
    add = _addend(d, width)
    if add is not None:
        a = add[nn_ % add.shape[0], q[:, 0], q[:, 1], q[:, 2]].to(dt)
        acc += a
        absum += a.abs()
    return acc, absum


def sample_positions(written, nrand=4096, seed=0, planes=True):
    """Written voxels to evaluate in f64: the first and last written plane along each axis, one random interior plane along
    each axis (together they cross every tile and d-segment boundary) and `nrand` random voxels.  long [S, 4]."""
    g = torch.Generator().manual_seed(seed)
    shape = written.shape
    picks = []
    if planes:
        for a in range(3):
            dims = tuple(i for i in range(4) if i != 1 + a)
            vals = written.any(dim=dims[2]).any(dim=dims[1]).any(dim=dims[0]).nonzero().view(-1)
            if vals.numel() == 0:
                continue
            chosen = {int(vals[0]), int(vals[-1])}
            if vals.numel() > 2:
                chosen.add(int(vals[1 + torch.randint(vals.numel() - 2, (1,), generator=g)]))
            for v in sorted(chosen):
                p = written.select(1 + a, v).nonzero()                                # [k, 3]: the other three coordinates
                picks.append(torch.cat([p[:, : 1 + a], torch.full((p.shape[0], 1), v, dtype=p.dtype), p[:, 1 + a:]], 1))
    if nrand:
        flat = written.reshape(-1)
        # random written voxels: draw linear indices, keep the written ones (a launch writes at least 1/8 of its output
        # tensor's voxels: the transposed-convolution classes); the exhaustive list only when that falls short
        cand = torch.randint(flat.numel(), (16 * nrand,), generator=g)
        cand = cand[flat[cand]][:nrand]
        if cand.numel() < nrand:
            allw = flat.nonzero().view(-1)
            cand = allw[torch.randint(allw.numel(), (nrand,), generator=g)] if allw.numel() else cand
        idx = []
        for e in reversed(shape):
            idx.append(cand % e)
            cand = cand // e
        picks.append(torch.stack(idx[::-1], 1))
    if not picks:
        return torch.zeros((0, 4), dtype=torch.long)
    allp = torch.cat(picks)
    lin = ((allp[:, 0] * shape[1] + allp[:, 1]) * shape[2] + allp[:, 2]) * shape[3] + allp[:, 3]
    lin = torch.unique(lin)
    out = []
    for e in reversed(shape):
        out.append(lin % e)
        lin = lin // e
    return torch.stack(out[::-1], 1)


def bf16_half_spacing(y):
    """Half the bf16 spacing at |y| (the largest legitimate final-rounding error of a stored bf16 value), f32: 2^(E - 135) for
    a biased f32 exponent E, i.e. the exponent field minus 8 (the smallest f32 subnormal where that underflows, y = 0)."""
    bits = (y.float().view(torch.int32) & 0x7F800000) - (8 << 23)
    return torch.where(bits > 0, bits, torch.ones_like(bits)).view(torch.float32)


def fwd_bound(y, absum, out_dtype):
    """|y - exact| <= 1/2 spacing_bf16(y) + 2^-14 A (bf16 / e4m3 launches), 2^-14 A (f32 outputs)."""
    b = (2.0 ** -14) * absum.double()
    if out_dtype == torch.bfloat16:
        b = b + bf16_half_spacing(y).double()
    return b


def stats_ref(acc, written, nsamples, width):
    """Per-sample sums of the accumulator over the written voxels: f64 [n][2][width] of {sum, sum of squares} and the
    number of positions per sample."""
    a = acc.double() * written[..., None].to(torch.float64)
    s1 = a.reshape(nsamples, -1, width).sum(1)
    s2 = (a * a).reshape(nsamples, -1, width).sum(1)
    cnt = int(written[0].sum())
    return torch.stack([s1, s2], 1), cnt


def stats_errors(got, ref, cnt, nch):
    """got/ref [groups][2][width] (only channels < nch compared).  Bounds: sum within 2^-12 sqrt(P sum (z-b)^2), sum of squares
    within 2^-12 relative.  Returns the worst err/bound (<= 1 passes)."""
    g, r = got[:, :, :nch].double(), ref[:, :, :nch].double()
    b0 = (2.0 ** -12) * (cnt * r[:, 1]).sqrt()
    b1 = (2.0 ** -12) * r[:, 1].abs()
    e0 = (g[:, 0] - r[:, 0]).abs()
    e1 = (g[:, 1] - r[:, 1]).abs()
    return max(_ratio(e0, b0), _ratio(e1, b1))


def _ratio(err, bound):
    """max err / bound, with a zero bound demanding a zero error (inf otherwise); NaN anywhere -> inf."""
    err, bound = err.double(), bound.double()
    if bool(torch.isnan(err).any()):
        return math.inf
    r = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                    torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


def fwd_errors(y, y_out_dtype, ref, ref64=None, idx=None):
    """Worst err/bound of a stored output against the references (<= 1 passes).
    y: f32 [n, dy, hy, wy, cstore] (the stored values), ref: conv_fwd_ref, ref64: (acc, absum) of conv_fwd_sampled at idx.
    The full-tensor comparison runs in f32, plane blocks at a time: its own rounding (2^-24 relative) is far below the bound."""
    c = y.shape[-1]
    bias = ref.bias[:c].float()
    worst = 0.0
    step = max(1, (1 << 22) // max(1, y[0, 0].numel()))
    for n in range(y.shape[0]):
        for d0 in range(0, y.shape[1], step):
            sl = (n, slice(d0, d0 + step))
            m = ref.written[sl]
            if not bool(m.any()):
                continue
            yb, acc, ab = y[sl], ref.acc[sl][..., :c].float(), ref.absum[sl][..., :c].float()
            if not bool(m.all()):
                yb, acc, ab = yb[m], acc[m], ab[m]
            err = (yb - (acc + bias)).abs()
            bound = (2.0 ** -14) * ab
            if y_out_dtype == torch.bfloat16:
                bound = bound + bf16_half_spacing(yb)
            worst = max(worst, _ratio(err, 2.0 * bound))
    if ref64 is not None:
        acc64, abs64 = ref64
        ys = y[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]].double()
        r = acc64[:, :c] + ref.bias[:c].double()
        worst = max(worst, _ratio((ys - r).abs(), fwd_bound(ys, abs64[:, :c], y_out_dtype)))
    return worst


# ------------------------------------------------------------------------------------------------------------- weight grad
def _g_cols(d):
    """The gradient operand as GEMM columns at every grid position: f32 [n, do, ho, wo, cols]."""
    nr = d.n * d.gd * d.gh * d.gw
    g = decode(rows(d.g, nr, d.cg, d.ldg), d.dtype).view(d.n, d.gd, d.gh, d.gw, d.cg)
    grid = (d.do_, d.ho, d.wo)
    if d.g_cls_cout:
        parts = []
        for blk in range(8):
            b = _class_bits(blk)
            sl = (slice(None),) + tuple(slice(bb, bb + 2 * e - 1, 2) for bb, e in zip(b, grid))
            parts.append(g[sl][..., : d.g_cls_cout])
        return torch.cat(parts, -1)
    sl = (slice(None),) + tuple(slice(o, o + d.gs * (e - 1) + 1, d.gs) for o, e in zip(d.goff, grid))
    return g[sl]


def _wx(d):
    nr_x = (d.xn if d.xn > 0 else d.n) * d.di * d.hi * d.wi
    xn = d.xn if d.xn > 0 else d.n
    parts = [decode(rows(d.x0, nr_x, d.c0, d.ld0), d.dtype)]
    if d.x1 is not None and d.c1 > 0:
        parts.append(decode(rows(d.x1, nr_x, d.c1, d.ld1), d.dtype))
    x = torch.cat(parts, 1).view(xn, d.di, d.hi, d.wi, -1)
    if xn != d.n:
        x = x.repeat(d.n // xn, 1, 1, 1, 1)              # grid sample i reads x sample i % xn
    return x


def wgrad_gemm(d, taps=None, dt=torch.float32):
    """dw[tap][ci][col] = sum_{n, p} x[n % xn, p stride + tap - pad, ci] g[n, pos(p), col] for the listed taps (all: None).
    Returns {tap: [cx, cols] tensor of dt}."""
    x = _wx(d).to(dt)
    g = _g_cols(d).to(dt)
    ks = d.ks
    grid = (d.do_, d.ho, d.wo)
    xp = _pad_ncdhw(x.permute(0, 4, 1, 2, 3), tuple(d.pad), grid, d.stride, ks).permute(0, 2, 3, 4, 1)
    s = d.stride
    gm = g.reshape(-1, g.shape[-1])
    out = {}
    for t in (range(ks ** 3) if taps is None else taps):
        td, th, tw = t // (ks * ks), (t // ks) % ks, t % ks
        xt = xp[:, td: td + s * (grid[0] - 1) + 1: s, th: th + s * (grid[1] - 1) + 1: s, tw: tw + s * (grid[2] - 1) + 1: s]
        out[t] = xt.reshape(-1, xt.shape[-1]).t() @ gm
    return out


def wgrad_index(d, t, cx, cols):
    """Destination element (offset from dw) of GEMM entry (tap t, ci, col) and its validity mask: [cx, cols] each."""
    ks = d.ks
    td, th, tw = t // (ks * ks), (t // ks) % ks, t % ks
    ci = torch.arange(cx).view(-1, 1)
    co = torch.arange(cols).view(1, -1)
    blk = torch.zeros((1, 1), dtype=torch.long)
    if d.s2d_cp:
        blk, ci = ci // d.s2d_cp, ci % d.s2d_cp
    if d.g_cls_cout:
        blk, co = co // d.g_cls_cout, co % d.g_cls_cout
    ok = (co < d.cout) & (ci < d.cin) & (blk < 8)
    k0 = d.tbase[0] + d.tstep[0] * td + (blk >> 2)
    k1 = d.tbase[1] + d.tstep[1] * th + ((blk >> 1) & 1)
    k2 = d.tbase[2] + d.tstep[2] * tw + (blk & 1)
    idx = co * d.s_co + ci * d.s_ci + k0 * d.s_k[0] + k1 * d.s_k[1] + k2 * d.s_k[2]
    return torch.broadcast_to(idx, ok.shape), torch.broadcast_to(ok, idx.shape)


def wgrad_span(d, cx, cols):
    """Elements of dw from its first element up to the last one the descriptor addresses."""
    hi = 0
    for t in range(d.ks ** 3):
        idx, ok = wgrad_index(d, t, cx, cols)
        if bool(ok.any()):
            hi = max(hi, int(idx[ok].max()))
    return hi + 1


def wgrad_scatter(d, gemm, before):
    """The dw range after the launch: `before` (f32, wgrad_span elements) with every addressed element overwritten by (or,
    accumulate, added to) its GEMM sum; also returns the mask of addressed elements."""
    out = before.clone().double()
    addressed = torch.zeros(before.numel(), dtype=torch.bool)
    for t, m in gemm.items():
        idx, ok = wgrad_index(d, t, m.shape[0], m.shape[1])
        i, v = idx[ok], m[ok].double()
        out[i] = (out[i] + v) if d.accumulate else v
        addressed[i] = True
    return out, addressed


def wgrad_errors(d, after, before, gemm32, gemm64):
    """Worst err/bound of a weight-gradient launch (<= 1 passes).  Per tap: rel-L2 <= 2^-13 and max err <= 2^-10 max|ref| of
    the tap (+ one f32 rounding of the accumulation into `before`), against the f64 GEMM where it was evaluated, else the f32
    one; every element the descriptor does not address must be unchanged."""
    worst = 0.0
    cols = next(iter(gemm32.values())).shape[1]
    cx = next(iter(gemm32.values())).shape[0]
    addressed = torch.zeros(before.numel(), dtype=torch.bool)
    for t in gemm32:
        ref = gemm64.get(t, gemm32[t]).double()
        idx, ok = wgrad_index(d, t, cx, cols)
        i = idx[ok]
        addressed[i] = True
        r = ref[ok]
        got = after[i].double()
        base = before[i].double() if d.accumulate else torch.zeros_like(got)
        err = (got - (base + r)).abs()
        scale = float(r.abs().max()) if r.numel() else 0.0
        bound = (2.0 ** -10) * scale + (2.0 ** -23) * got.abs() * (1.0 if d.accumulate else 0.0)
        worst = max(worst, _ratio(err, bound))
        nr = float(r.norm())
        rel = float(err.norm()) / nr if nr > 0 else (0.0 if float(err.norm()) == 0 else math.inf)
        worst = max(worst, rel / 2.0 ** -13 if not d.accumulate else rel / (2.0 ** -13 + 2.0 ** -23 * float(got.norm()) / max(nr, 1e-300)))
    untouched = ~addressed
    if bool(untouched.any()):
        same = torch.equal(after[untouched].view(torch.int32), before[untouched].view(torch.int32))
        if not same:
            worst = math.inf
    return worst


def wgrad_check_taps(ks):
    """Taps evaluated in f64: all of a 1 / 2-tap-wide kernel, else the 8 corners and the centre (the taps that read padding)."""
    if ks <= 2:
        return list(range(ks ** 3))
    e = ks - 1
    corners = [(a * ks + b) * ks + c for a in (0, e) for b in (0, e) for c in (0, e)]
    c = ks // 2
    return sorted(set(corners + [(c * ks + c) * ks + c]))


# ------------------------------------------------------------------------------------------------------------- CPU-side builders
def pack_gemm(w, dtype=F32):
    """GEMM weights w[tap][coutp][cinp] (cinp % 16 == 0) -> the packed layout [cinp/16][tap][coutp][16], flat, as `dtype`
    host elements (the inverse of decode_wp; FP8: w must already be the e4m3 values, before scaling)."""
    taps, coutp, cinp = w.shape
    p = w.reshape(taps, coutp, cinp // 16, 16).permute(2, 0, 1, 3).reshape(-1)
    if dtype == FP8:
        return p.to(torch.float8_e4m3fn).view(torch.uint8)
    return p.to(_ELEM[dtype])


def act_flat(x, ld, dtype=F32):
    """[n, d, h, w, c] -> a flat host buffer with row pitch ld (the pad channels hold a marker value that must never be read)."""
    n, d, h, w, c = x.shape
    buf = torch.full((n * d * h * w, ld), 7.0e3, dtype=torch.float32)
    buf[:, :c] = x.reshape(-1, c)
    flat = buf.reshape(-1)[: act_extent(n * d * h * w, c, ld)]
    if dtype == FP8:
        return flat.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    return flat.to(_ELEM[dtype])


def conv_desc(x0, wp, coutp, ks, stride, pad, grid, out_shape, cstore, ldy, x1=None, ld0=None, ld1=None, bias=None, nbias=0,
              os=1, ooff=(0, 0, 0), dtype=F32, cls_cout=0, addend=None, ld_add=0, add_n=0, y_f32=0, d2s=0, delta=None,
              q_amax_x=None, q_amax_w=None):
    """A forward descriptor on host tensors (x0 / x1: [n, d, h, w, c] f32 values; wp: pack_gemm output)."""
    n, di, hi, wi, c0 = x0.shape
    ld0 = c0 if ld0 is None else ld0
    c1 = x1.shape[4] if x1 is not None else 0
    ld1 = (c1 if ld1 is None else ld1) if x1 is not None else 0
    return SimpleNamespace(
        x0=act_flat(x0, ld0, dtype), c0=c0, ld0=ld0, x1=act_flat(x1, ld1, dtype) if x1 is not None else None, c1=c1, ld1=ld1,
        n=n, di=di, hi=hi, wi=wi, do_=grid[0], ho=grid[1], wo=grid[2], ks=ks, stride=stride, pad=tuple(pad), wp=wp, coutp=coutp,
        bias=bias, nbias=nbias, ldy=ldy, cstore=cstore, dy=out_shape[0], hy=out_shape[1], wy=out_shape[2], os=os, ooff=tuple(ooff),
        dtype=dtype, cls_cout=cls_cout, q_amax_x=q_amax_x, q_amax_w=q_amax_w, addend=addend, ld_add=ld_add, y_f32=y_f32,
        add_n=add_n, d2s=d2s, delta=delta, add_bf16=0)


def wgrad_desc(x0, g, grid, ks, stride, pad, cout, cin, s_co, s_ci, s_k, tbase, tstep, x1=None, gs=1, goff=(0, 0, 0),
               accumulate=0, s2d_cp=0, g_cls_cout=0, n=None, dtype=F32):
    """A weight-gradient descriptor on host tensors (x0 / x1 / g: [n, d, h, w, c] f32 values)."""
    xn, di, hi, wi, c0 = x0.shape
    n = xn if n is None else n
    c1 = x1.shape[4] if x1 is not None else 0
    _, gd, gh, gw, cg = g.shape
    return SimpleNamespace(
        x0=act_flat(x0, c0, dtype), c0=c0, ld0=c0, x1=act_flat(x1, c1, dtype) if x1 is not None else None, c1=c1, ld1=c1,
        n=n, di=di, hi=hi, wi=wi, g=act_flat(g, cg, dtype), cg=cg, ldg=cg, do_=grid[0], ho=grid[1], wo=grid[2],
        gd=gd, gh=gh, gw=gw, gs=gs, goff=tuple(goff), ks=ks, stride=stride, pad=tuple(pad), cout=cout, cin=cin, s_co=s_co,
        s_ci=s_ci, s_k=tuple(s_k), tbase=tuple(tbase), tstep=tuple(tstep), accumulate=accumulate, dtype=dtype, s2d_cp=s2d_cp,
        g_cls_cout=g_cls_cout, xn=xn if xn != n else 0)


def s2d(a, cblk):
    """Space-to-depth tensor of a plain [n, D, H, W, c] tensor (even extents): [n, D/2+1, H/2+1, W/2+1, 8 cblk],
    S[n, j, blk cblk + c] = a[n, 2 j + b - 1, c] (zeros outside the volume)."""
    n, D, H, W, c = a.shape
    ap = F.pad(a, (0, cblk - c, 1, 2, 1, 2, 1, 2))
    out = torch.zeros(n, D // 2 + 1, H // 2 + 1, W // 2 + 1, 8 * cblk)
    for blk in range(8):
        bd, bh, bw = _class_bits(blk)
        out[..., blk * cblk:(blk + 1) * cblk] = ap[:, bd::2, bh::2, bw::2][:, : D // 2 + 1, : H // 2 + 1, : W // 2 + 1]
    return out
