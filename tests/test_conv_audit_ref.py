"""CPU tests of the descriptor-level convolution reference (tests/conv_audit_ref.py) that the in-situ audit of the training
step (tests/test_conv_audit.py) compares every launch with: every mode of mi355_conv_fwd / mi355_conv_wgrad against
F.conv3d, F.conv_transpose3d and torch.nn.grad.conv3d_weight, and the sensitivity of the audit's bounds -- each corruption a
subtly wrong kernel could make must fail them, the unperturbed result must pass."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_audit_ref as R  # noqa: E402


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bf(x):
    return x.to(torch.bfloat16).float()


def _gemm_k(wt, cinp=None, coutp=None):
    """torch Conv3d weight [cout][cin][k][k][k] -> GEMM w[tap][coutp][cinp]."""
    cout, cin, k = wt.shape[0], wt.shape[1], wt.shape[2]
    cinp = cinp or -(-cin // 16) * 16
    coutp = coutp or -(-cout // 32) * 32
    w = torch.zeros(k ** 3, coutp, cinp)
    w[:, :cout, :cin] = wt.permute(2, 3, 4, 0, 1).reshape(k ** 3, cout, cin)
    return w


def _ncdhw(x):
    return x.permute(0, 4, 1, 2, 3)


def _ndhwc(x):
    return x.permute(0, 2, 3, 4, 1)


def _agree(acc64, acc32, abs64):
    """The f64 samples and the f32 full reference differ by f32 summation noise only: far below 2^-14 A."""
    assert bool(((acc64 - acc32.double()).abs() <= 2.0 ** -18 * abs64 + 1e-30).all())


def _ref_y(ref, c):
    """Stored-value view of a reference: acc + bias at written voxels, zeros elsewhere."""
    return torch.where(ref.written[..., None], ref.acc[..., :c] + ref.bias[:c], torch.zeros(()))


# ------------------------------------------------------------------------------------------------------------- forward modes
@pytest.mark.parametrize("ks,stride,pad", [(3, 1, 1), (4, 2, 1), (1, 1, 0), (2, 1, 0)])
def test_fwd_plain_and_concat_vs_conv3d(ks, stride, pad):
    g = _gen(ks * 10 + stride)
    n, sp, c0, c1, cout = 2, (6, 8, 10), 16, 32, 40
    x0 = torch.randn(n, *sp, c0, generator=g)
    x1 = torch.randn(n, *sp, c1, generator=g)
    wt = torch.randn(cout, c0 + c1, ks, ks, ks, generator=g)
    bias = torch.randn(cout, generator=g)
    ref_t = F.conv3d(_ncdhw(torch.cat([x0, x1], -1)), wt, bias, stride, pad)
    grid = tuple(ref_t.shape[2:])
    coutp = 64
    d = R.conv_desc(x0, R.pack_gemm(_gemm_k(wt, coutp=coutp)), coutp, ks, stride, (pad,) * 3, grid, grid, 48, 64, x1=x1,
                    ld0=32, ld1=48, bias=bias, nbias=cout)
    r = R.conv_fwd_ref(d)
    assert bool(r.written.all())
    torch.testing.assert_close(_ref_y(r, cout), _ndhwc(ref_t), rtol=1e-5, atol=1e-4)
    assert float(r.acc[..., cout:].abs().max()) == 0.0                      # zero-weight pad columns, no bias there
    # f64 samples agree with the full f32 reference, and A >= |acc|
    idx = R.sample_positions(r.written, nrand=64)
    acc64, abs64 = R.conv_fwd_sampled(d, idx)
    full = r.acc[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]]
    _agree(acc64, full, abs64)
    assert bool((abs64 + 1e-9 >= acc64.abs()).all())


def test_fwd_output_grid_os_ooff_and_cstore():
    """The stride-2 data gradient's parity classes: z at output voxel 2 p + ooff; nothing else written."""
    g = _gen(3)
    x = torch.randn(1, 4, 5, 6, 16, generator=g)
    wt = torch.randn(32, 16, 2, 2, 2, generator=g)
    zt = F.conv3d(_ncdhw(x), wt, None, 1, 1)                             # grid (5, 6, 7)
    grid = tuple(zt.shape[2:])
    ooff = (1, 0, 1)
    out = tuple(2 * e + 1 for e in grid)
    d = R.conv_desc(x, R.pack_gemm(_gemm_k(wt)), 32, 2, 1, (1, 1, 1), grid, out, 32, 32, os=2, ooff=ooff)
    r = R.conv_fwd_ref(d)
    assert int(r.written.sum()) == grid[0] * grid[1] * grid[2]
    got = r.acc[:, 1::2, 0::2, 1::2][:, : grid[0], : grid[1], : grid[2]]
    torch.testing.assert_close(got, _ndhwc(zt), rtol=1e-5, atol=1e-4)


def test_fwd_transposed_class_folding_vs_conv_transpose3d():
    g = _gen(4)
    n, cin, cout, sp = 2, 32, 64, (3, 4, 5)
    x = torch.randn(n, *sp, cin, generator=g)
    wt = torch.randn(cin, cout, 2, 2, 2, generator=g)
    bias = torch.randn(cout, generator=g)
    yt = F.conv_transpose3d(_ncdhw(x), wt, bias, 2)
    w = torch.zeros(1, 8 * cout, cin)
    for blk in range(8):
        bd, bh, bw = (blk >> 2) & 1, (blk >> 1) & 1, blk & 1
        w[0, blk * cout:(blk + 1) * cout] = wt[:, :, bd, bh, bw].t()
    out = tuple(2 * e for e in sp)
    d = R.conv_desc(x, R.pack_gemm(w), 8 * cout, 1, 1, (0, 0, 0), sp, out, cout, cout, bias=bias, nbias=cout, os=2, cls_cout=cout)
    r = R.conv_fwd_ref(d)
    assert bool(r.written.all())
    torch.testing.assert_close(_ref_y(r, cout), _ndhwc(yt), rtol=1e-5, atol=1e-4)
    idx = R.sample_positions(r.written, nrand=64)
    acc64, abs64 = R.conv_fwd_sampled(d, idx)
    _agree(acc64, r.acc[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]], abs64)


def test_fwd_depth_to_space_vs_conv_transpose3d_k4s2p1_with_delta_and_addend():
    """d2s: ConvTranspose3d(k4, s2, p1) of the low-resolution tensor, + the addend (one addend sample under two grid samples),
    + bias, + the border class correction delta[9 cd + 3 ch + cw] (interior class 13 never applied)."""
    g = _gen(5)
    n, cl, co, sp = 2, 32, 32, (3, 4, 5)
    x = torch.randn(n, *sp, cl, generator=g)
    k4 = torch.randn(cl, co, 4, 4, 4, generator=g)
    bias = torch.randn(co, generator=g)
    delta = torch.randn(27, co, generator=g)
    out = tuple(2 * e for e in sp)
    add = torch.randn(1, *out, co, generator=g)
    # GEMM: class b, tap e (per axis) reads cell j + e + b - 1 with kernel index 3 - 2 e - b
    w = torch.zeros(8, 8 * co, cl)
    for blk in range(8):
        b = ((blk >> 2) & 1, (blk >> 1) & 1, blk & 1)
        for t in range(8):
            e = ((t >> 2) & 1, (t >> 1) & 1, t & 1)
            kk = tuple(3 - 2 * ee - bb for ee, bb in zip(e, b))
            w[t, blk * co:(blk + 1) * co] = k4[:, :, kk[0], kk[1], kk[2]].t()
    d = R.conv_desc(x, R.pack_gemm(w, R.BF16), 8 * co, 2, 1, (0, 0, 0), sp, out, co, co, bias=bias, nbias=co, dtype=R.BF16,
                    d2s=1, delta=delta.reshape(-1), addend=add.reshape(-1), ld_add=co, add_n=1)
    # (bf16 operands: the expectation uses the same rounded values)
    xq = _bf(x)
    wq = _bf(w)
    r = R.conv_fwd_ref(d)
    assert bool(r.written.all())
    k4q = torch.zeros_like(k4)
    for blk in range(8):
        b = ((blk >> 2) & 1, (blk >> 1) & 1, blk & 1)
        for t in range(8):
            e = ((t >> 2) & 1, (t >> 1) & 1, t & 1)
            kk = tuple(3 - 2 * ee - bb for ee, bb in zip(e, b))
            k4q[:, :, kk[0], kk[1], kk[2]] = wq[t, blk * co:(blk + 1) * co].t()
    exp = _ndhwc(F.conv_transpose3d(_ncdhw(xq), k4q, None, 2, 1)) + add
    cls = torch.zeros(out, dtype=torch.long)
    for a, e in enumerate(out):
        c = torch.ones(e, dtype=torch.long)
        c[0], c[-1] = 0, 2
        cls = cls + c.view([-1 if i == a else 1 for i in range(3)]) * (9, 3, 1)[a]
    corr = delta[cls] * (cls != 13)[..., None]
    exp = exp + corr
    torch.testing.assert_close(r.acc, exp, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(_ref_y(r, co), exp + bias, rtol=1e-5, atol=1e-4)
    idx = R.sample_positions(r.written, nrand=128)
    acc64, abs64 = R.conv_fwd_sampled(d, idx)
    _agree(acc64, r.acc[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]], abs64)


def test_fwd_addend_and_f32_output_of_the_split_first_block():
    """PatchGAN first block split into x- and y-part: z = conv(S(y)) + addend (x-part, f32), add_n = 1 under 2 samples."""
    g = _gen(6)
    n, sp, c, cout = 2, (4, 5, 6), 32, 32
    x = torch.randn(n, *sp, c, generator=g)
    wt = torch.randn(cout, c, 2, 2, 2, generator=g)
    grid = tuple(e - 1 for e in sp)
    add = torch.randn(1, *grid, cout, generator=g)
    bias = torch.randn(cout, generator=g)
    d = R.conv_desc(x, R.pack_gemm(_gemm_k(wt)), 32, 2, 1, (0, 0, 0), grid, grid, 32, 32, bias=bias, nbias=cout,
                    addend=add.reshape(-1), ld_add=32, add_n=1, y_f32=1)
    r = R.conv_fwd_ref(d)
    exp = _ndhwc(F.conv3d(_ncdhw(x), wt, None)) + add
    torch.testing.assert_close(r.acc, exp, rtol=1e-5, atol=1e-4)
    st, cnt = R.stats_ref(r.acc, r.written, n, 32)
    assert cnt == grid[0] * grid[1] * grid[2]
    torch.testing.assert_close(st[:, 0].float(), exp.sum((1, 2, 3)), rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(st[:, 1].float(), (exp * exp).sum((1, 2, 3)), rtol=1e-4, atol=1e-3)


def test_fwd_fp8_operands_vs_conv3d_on_the_decoded_values():
    g = _gen(7)
    x = torch.randn(1, 4, 6, 8, 32, generator=g)
    wt = torch.randn(32, 32, 3, 3, 3, generator=g) * 0.1
    ax, aw = float(x.abs().max()), float(wt.abs().max())
    x8 = (x * (224.0 / ax)).to(torch.float8_e4m3fn).float()
    w8 = (_gemm_k(wt) * (224.0 / aw)).to(torch.float8_e4m3fn).float()
    d = R.conv_desc(x8, R.pack_gemm(w8, R.FP8), 32, 3, 1, (1, 1, 1), (4, 6, 8), (4, 6, 8), 32, 32, dtype=R.FP8,
                    q_amax_x=ax, q_amax_w=aw)
    r = R.conv_fwd_ref(d)
    wdec = (w8 * (aw / 224.0))[:, :32, :32].reshape(3, 3, 3, 32, 32).permute(3, 4, 0, 1, 2)
    exp = _ndhwc(F.conv3d(_ncdhw(x8 * (ax / 224.0)), wdec, None, 1, 1))
    torch.testing.assert_close(r.acc, exp, rtol=1e-5, atol=1e-4)


# ------------------------------------------------------------------------------------------------------------- weight gradients
def _wgrad_all(d):
    gemm = R.wgrad_gemm(d)
    cx, cols = next(iter(gemm.values())).shape
    span = R.wgrad_span(d, cx, cols)
    return gemm, span


@pytest.mark.parametrize("ks,stride,pad", [(3, 1, 1), (4, 2, 1), (1, 1, 0)])
def test_wgrad_plain_concat_accumulate_vs_conv3d_weight(ks, stride, pad):
    g = _gen(11 + ks)
    n, sp, c0, c1, cout = 2, (6, 8, 10), 16, 16, 32
    x0 = torch.randn(n, *sp, c0, generator=g)
    x1 = torch.randn(n, *sp, c1, generator=g)
    cin = 28                                                  # real extent < the concat's 32 channels
    xt = _ncdhw(torch.cat([x0, x1], -1))[:, :cin]
    z = F.conv3d(xt, torch.zeros(cout, cin, ks, ks, ks), None, stride, pad)
    gz = torch.randn(z.shape, generator=g)
    exp = torch.nn.grad.conv3d_weight(xt, (cout, cin, ks, ks, ks), gz, stride, pad)
    d = R.wgrad_desc(x0, _ndhwc(gz), tuple(z.shape[2:]), ks, stride, (pad,) * 3, cout, cin, cin * ks ** 3, ks ** 3,
                     (ks * ks, ks, 1), (0, 0, 0), (1, 1, 1), x1=x1, accumulate=1)
    gemm, span = _wgrad_all(d)
    assert span == exp.numel()
    before = torch.randn(span, generator=g)
    after, addressed = R.wgrad_scatter(d, gemm, before)
    assert bool(addressed.all())
    torch.testing.assert_close(after.float(), before + exp.reshape(-1), rtol=1e-5, atol=1e-3)


def test_wgrad_space_to_depth_operand_vs_k4s2p1_weight_gradient_and_xn():
    """Dense k2 wgrad of S(a) scattered through s2d_cp / tstep 2 = the k4 s2 p1 weight gradient of a; xn = 1 under 2 grid samples."""
    g = _gen(12)
    a = torch.randn(1, 6, 8, 10, 8, generator=g)
    cin, cout, cp = 8, 32, 8
    z = F.conv3d(_ncdhw(a), torch.zeros(cout, cin, 4, 4, 4), None, 2, 1)
    gz = torch.randn((2,) + tuple(z.shape[1:]), generator=g)
    exp = torch.nn.grad.conv3d_weight(_ncdhw(a).repeat(2, 1, 1, 1, 1), (cout, cin, 4, 4, 4), gz, 2, 1)
    d = R.wgrad_desc(R.s2d(a, cp), _ndhwc(gz), tuple(z.shape[2:]), 2, 1, (0, 0, 0), cout, cin, cin * 64, 64, (16, 4, 1),
                     (0, 0, 0), (2, 2, 2), s2d_cp=cp, n=2)
    assert d.xn == 1
    gemm, span = _wgrad_all(d)
    after, addressed = R.wgrad_scatter(d, gemm, torch.zeros(span))
    assert bool(addressed.all())
    torch.testing.assert_close(after.float(), exp.reshape(-1), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("folded", [True, False])
def test_wgrad_transposed_conv_classes_vs_autograd(folded):
    """ConvTranspose3d(k2, s2) weight [cin][cout][2][2][2]: one launch with g_cls_cout, or eight with gs = 2, goff = tbase = class."""
    g = _gen(13)
    n, cin, cout, sp = 2, 16, 32, (3, 4, 5)
    x = torch.randn(n, *sp, cin, generator=g)
    wt = torch.zeros(cin, cout, 2, 2, 2, requires_grad=True)
    y = F.conv_transpose3d(_ncdhw(x), wt, None, 2)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    exp = wt.grad.reshape(-1)
    if folded:
        d = R.wgrad_desc(x, _ndhwc(gy), sp, 1, 1, (0, 0, 0), cout, cin, 8, cout * 8, (4, 2, 1), (0, 0, 0), (0, 0, 0),
                         g_cls_cout=cout)
        gemm, span = _wgrad_all(d)
        after, addressed = R.wgrad_scatter(d, gemm, torch.zeros(exp.numel()))
    else:
        after = torch.zeros(exp.numel()).double()
        addressed = torch.zeros(exp.numel(), dtype=torch.bool)
        for blk in range(8):
            cls = ((blk >> 2) & 1, (blk >> 1) & 1, blk & 1)
            d = R.wgrad_desc(x, _ndhwc(gy), sp, 1, 1, (0, 0, 0), cout, cin, 8, cout * 8, (4, 2, 1), cls, (0, 0, 0), gs=2, goff=cls)
            gemm, span = _wgrad_all(d)
            after, a1 = R.wgrad_scatter(d, gemm, after.float()[:span] if span <= exp.numel() else after.float())
            after = F.pad(after, (0, exp.numel() - after.numel()))
            addressed[: a1.numel()] |= a1
    assert bool(addressed.all())
    torch.testing.assert_close(after.float(), exp, rtol=1e-5, atol=1e-3)


def test_wgrad_unaddressed_elements_of_a_channel_slice():
    """The x-part launch of the split first block addresses only ci < cx of a [cout][cx + cy] weight: the y-part slice inside its
    span is untouched, and wgrad_errors flags any change there."""
    g = _gen(14)
    x = torch.randn(1, 4, 5, 6, 16, generator=g)
    gz = torch.randn(1, 3, 4, 5, 32, generator=g)
    cx, cy, cout = 16, 8, 32
    d = R.wgrad_desc(x, gz, (3, 4, 5), 2, 1, (0, 0, 0), cout, cx, (cx + cy) * 8, 8, (4, 2, 1), (0, 0, 0), (1, 1, 1))
    gemm, span = _wgrad_all(d)
    before = torch.randn(span, generator=g)
    after, addressed = R.wgrad_scatter(d, gemm, before)
    assert not bool(addressed.all())
    after = after.float()
    g64 = {t: m.double() for t, m in gemm.items()}
    assert R.wgrad_errors(d, after, before, gemm, g64) <= 1.0
    bad = after.clone()
    bad[(~addressed).nonzero()[0]] += 1.0
    assert R.wgrad_errors(d, bad, before, gemm, g64) > 1.0


def test_pack_expect_and_decoder_are_inverse():
    g = _gen(15)
    wt = torch.randn(40, 24, 3, 3, 3, generator=g)
    w = R.pack_expect(wt, 40, 24, 64, 32, 3, 24 * 27, 27, (9, 3, 1), (0, 0, 0), (1, 1, 1))
    torch.testing.assert_close(w, _gemm_k(wt, 32, 64))
    assert torch.equal(R.decode_wp(R.pack_gemm(w), R.F32, 32, 27, 64), w)
    # flipped / transposed (dgrad) packing: GEMM (co <- ci, ci <- co), taps reversed
    wf = R.pack_expect(wt, 24, 40, 32, 48, 3, 27, 24 * 27, (9, 3, 1), (2, 2, 2), (-1, -1, -1))
    torch.testing.assert_close(wf[:, :24, :40], _gemm_k(wt.flip(2, 3, 4).transpose(0, 1), 40, 24))


# ------------------------------------------------------------------------------------------------------------- sensitivity
def _sim_store(ref, c, dtype=torch.bfloat16):
    """What a correct kernel stores: bf16(acc + bias) at written voxels."""
    return _ref_y(ref, c).to(dtype).float()


def _fwd_case(name):
    g = _gen(21)
    if name == "wide":                                      # 32 -> 32 at 32 x 64 x 64 (the full-resolution layers' shape class)
        n, sp, cin, cout = 1, (16, 32, 64), 32, 32
    else:                                                   # 128 -> 64 at 16^3, two samples (a low level: split-K geometry)
        n, sp, cin, cout = 2, (8, 8, 16), 128, 64
    x = _bf(torch.randn(n, *sp, cin, generator=g))
    wt = _bf(torch.randn(cout, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5)
    bias = (torch.rand(cout, generator=g) - 0.5) * 0.5
    w = _gemm_k(wt)
    coutp = w.shape[1]
    d = R.conv_desc(x, R.pack_gemm(w, R.BF16), coutp, 3, 1, (1, 1, 1), sp, sp, cout, cout, bias=bias, nbias=cout, dtype=R.BF16)
    return d, x, w, bias


def _check(d, y, ref, ref64, idx):
    return R.fwd_errors(y, torch.bfloat16, ref, ref64, idx)


@pytest.mark.parametrize("shape", ["wide", "low"])
def test_audit_bounds_pass_a_correct_result_and_catch_each_corruption(shape):
    d, x, w, bias = _fwd_case(shape)
    ref = R.conv_fwd_ref(d)
    idx = R.sample_positions(ref.written, nrand=4096)
    ref64 = R.conv_fwd_sampled(d, idx)
    cout = d.cstore
    y = _sim_store(ref, cout)
    ok = _check(d, y, ref, ref64, idx)
    assert ok <= 1.0, ok

    def corrupted(**kw):
        import copy
        dd = copy.copy(d)
        xx, ww = kw.get("x", x), kw.get("w", w)
        dd.x0 = R.act_flat(xx, d.ld0, R.BF16)
        dd.wp = R.pack_gemm(ww, R.BF16)
        if "bias" in kw:
            dd.bias = kw["bias"]
        return _sim_store(R.conv_fwd_ref(dd, with_abs=False), cout)

    bad = {}
    w1 = w.clone()
    w1[13] = 0                                                # one tap dropped (the centre)
    bad["tap"] = corrupted(w=w1)
    w2 = w.clone()
    w2[:, :, 16:32] = 0                                       # one 16-channel input chunk dropped
    bad["chunk"] = corrupted(w=w2)
    x3 = x.clone()
    x3[:, x.shape[1] // 2] = 0                                # one input d-plane zeroed
    bad["plane"] = corrupted(x=x3)
    y4 = y.clone()
    e = y.shape[3] // 2                                       # output shifted by one voxel along w from a tile edge on
    y4[:, :, :, e:-1] = y[:, :, :, e + 1:]
    bad["shift"] = y4
    bad["bias_omitted"] = corrupted(bias=torch.zeros_like(bias))
    bad["bias_doubled"] = corrupted(bias=2 * bias)
    for k, yb in bad.items():
        r = _check(d, yb, ref, ref64, idx)
        assert r > 1.0, (k, r)


@pytest.mark.parametrize("shape", ["wide", "low"])
def test_audit_bounds_catch_a_missing_weight_gradient_plane(shape):
    d, x, w, bias = _fwd_case(shape)
    g = _gen(22)
    gz = _bf(torch.randn(x.shape[:4] + (d.cstore,), generator=g))
    cin = x.shape[-1]
    dw = R.wgrad_desc(x, gz, x.shape[1:4], 3, 1, (1, 1, 1), d.cstore, cin, cin * 27, 27, (9, 3, 1), (0, 0, 0), (1, 1, 1), dtype=R.BF16)
    gemm, span = _wgrad_all(dw)
    g64 = R.wgrad_gemm(dw, R.wgrad_check_taps(3), torch.float64)
    before = torch.full((span,), float("nan"))
    after, _ = R.wgrad_scatter(dw, gemm, before)
    assert R.wgrad_errors(dw, after.float(), before, gemm, g64) <= 1.0
    gz2 = gz.clone()
    gz2[:, gz.shape[1] // 3] = 0                              # one plane of positions missing
    dw2 = R.wgrad_desc(x, gz2, x.shape[1:4], 3, 1, (1, 1, 1), d.cstore, cin, cin * 27, 27, (9, 3, 1), (0, 0, 0), (1, 1, 1), dtype=R.BF16)
    bad, _ = R.wgrad_scatter(dw2, R.wgrad_gemm(dw2), before)
    assert R.wgrad_errors(dw, bad.float(), before, gemm, g64) > 1.0


def test_audit_bounds_catch_statistics_of_the_neighbouring_sample():
    d, x, w, bias = _fwd_case("low")
    ref = R.conv_fwd_ref(d)
    st, cnt = R.stats_ref(ref.acc, ref.written, d.n, ref.width)
    assert R.stats_errors(st.float(), st, cnt, d.cstore) <= 1.0
    assert R.stats_errors(st.flip(0).float(), st, cnt, d.cstore) > 1.0
    # tiles of sample 0 that land in sample 1: a partial shift of the sums
    moved = st.clone()
    moved[0] -= 0.1 * st[0]
    moved[1] += 0.1 * st[0]
    assert R.stats_errors(moved.float(), st, cnt, d.cstore) > 1.0
