"""Host side of the Perceptual term's backward (no GPU): the closed forms that csrc/medicalnet_bwd.hip implements and the weight
arrangements its kernels read, each against torch autograd in f64."""
import pytest
import torch
import torch.nn.functional as F

import medicalnet_grad_ref as GR
import medicalnet_ref as MR
from unet_bssfp_amd import medicalnet


def _q16(t):
    return t.to(torch.bfloat16).to(t.dtype)


@pytest.mark.parametrize("case", ["n1260", "mean3_std05"])
def test_normalise_backward_is_autograd_of_normalise(case):
    g = torch.Generator().manual_seed(3)
    if case == "n1260":
        v = torch.randn(2, 3, 5, 6, 7, generator=g, dtype=torch.float64)
    else:
        v = 3.0 + 0.5 * torch.randn(1, 2, 4, 9, 5, generator=g, dtype=torch.float64)
    up = torch.randn(v.shape, generator=g, dtype=torch.float64)
    a = v.clone().requires_grad_()
    want, = torch.autograd.grad((MR.normalise(a) * up).sum(), a)
    got = GR.normalise_backward(up, v)
    assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


def _gather_dgrad(packed, dy, in_shape, ks, stride, dil):
    """dx[i, ci] = sum_tap sum_co dy[(i + pad - tap dil) / stride, co] w[co, ci, tap], read from the [tap][cout / 16][cin][16] array
    that the kernel reads; a tap counts where the division is exact and the quotient is in range"""
    taps, q, ci, _ = packed.shape
    wt = packed.double().permute(0, 1, 3, 2).reshape(taps, q * 16, ci)           # [tap][co][ci]
    n, _, d, h, w = in_shape
    dx = torch.zeros(n, ci, d, h, w, dtype=torch.float64)
    pad = dil * (ks // 2)

    def axis(n_in, n_out, k):
        i = torch.arange(n_in)
        num = i + pad - k * dil
        ok = (num >= 0) & (num % stride == 0) & (torch.div(num, stride, rounding_mode="floor") < n_out)
        return i[ok], torch.div(num, stride, rounding_mode="floor")[ok]

    for tap in range(taps):
        kd, kh, kw = tap // (ks * ks), (tap // ks) % ks, tap % ks
        (id_, od), (ih, oh), (iw, ow) = axis(d, dy.shape[2], kd), axis(h, dy.shape[3], kh), axis(w, dy.shape[4], kw)
        if min(len(id_), len(ih), len(iw)) == 0:
            continue
        sub = dy[:, :, od][:, :, :, oh][:, :, :, :, ow]
        dx[:, :, id_[:, None, None], ih[None, :, None], iw[None, None, :]] += torch.einsum("nodhw,oc->ncdhw", sub, wt[tap])
    return dx


DGRAD = [(3, 1, 1), (3, 2, 1), (3, 1, 2), (3, 1, 4), (1, 1, 1), (1, 2, 1)]


@pytest.mark.parametrize("ks,stride,dil", DGRAD, ids=[f"k{k}_s{s}_d{d}" for k, s, d in DGRAD])
def test_pack_dgrad_weight_gives_the_data_gradient(ks, stride, dil):
    g = torch.Generator().manual_seed(10 * ks + 3 * stride + dil)
    cin, cout = 64, 128
    w32 = torch.randn(cout, cin, ks, ks, ks, generator=g) * (2.0 / (ks ** 3 * cin)) ** 0.5
    packed = medicalnet.pack_dgrad_weight(w32)
    assert packed.dtype == torch.bfloat16 and tuple(packed.shape) == (ks ** 3, cout // 16, cin, 16)
    # the same values as the forward's pack: element (tap, q, ci, e) of one is element (tap, ci / 16, 16 q + e, ci % 16) of the other
    fwd = medicalnet.pack_conv_weight(w32).float().permute(0, 2, 1, 3).reshape(ks ** 3, cout, cin)            # [tap][co][ci]
    assert torch.equal(packed.float().permute(0, 1, 3, 2).reshape(ks ** 3, cout, cin), fwd)
    x = torch.randn(2, cin, 5, 6, 9, generator=g, dtype=torch.float64, requires_grad=True)
    pad = dil * (ks // 2)
    y = F.conv3d(x, _q16(w32).double(), None, stride, pad, dil)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    want, = torch.autograd.grad((y * dy).sum(), x)
    got = _gather_dgrad(packed, dy, x.shape, ks, stride, dil)
    assert (got - want).abs().max().item() <= 1e-10
    if ks == 1 and stride == 2:
        assert got[:, :, 1::2].abs().max().item() == 0.0                  # input voxels that no tap reaches


def test_pack_stem_dgrad_weight_gives_the_stem_data_gradient():
    """the Toeplitz arrangement of mnet_stem_dgrad_kernel, evaluated the way the kernel does (cells of 2 x 2 x 2 input voxels
    against the 4 x 4 x 4 neighbourhood of dy), on 9 x 10 x 7: odd and even extents"""
    g = torch.Generator().manual_seed(21)
    w32 = torch.randn(64, 1, 7, 7, 7, generator=g) * (2.0 / 343) ** 0.5
    packed = medicalnet.pack_stem_dgrad_weight(w32)
    assert packed.dtype == torch.bfloat16 and tuple(packed.shape) == (64, 2, 8, 32)
    toep = packed.double().reshape(4, 4, 4, 2, 8, 32).permute(0, 1, 2, 4, 3, 5).reshape(4, 4, 4, 8, 64)     # [ad][ah][aw][cls][co]
    assert int((toep.abs().sum(-1) > 0).sum()) == 343
    x = torch.randn(2, 1, 9, 10, 7, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x, _q16(w32).double(), None, 2, 3)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    want, = torch.autograd.grad((y * dy).sum(), x)
    n, _, do, ho, wo = dy.shape
    dyp = F.pad(dy, (1, 2, 1, 2, 1, 2))
    cells = torch.zeros(n, 8, do, ho, wo, dtype=torch.float64)
    for ad in range(4):
        for ah in range(4):
            for aw in range(4):
                cells += torch.einsum("ncdhw,kc->nkdhw", dyp[:, :, ad:ad + do, ah:ah + ho, aw:aw + wo], toep[ad, ah, aw])
    got = torch.zeros(n, 1, 2 * do, 2 * ho, 2 * wo, dtype=torch.float64)
    for cls in range(8):
        got[:, 0, (cls >> 2) & 1::2, (cls >> 1) & 1::2, cls & 1::2] = cells[:, cls]
    got = got[:, :, :9, :10, :7]
    assert (got - want).abs().max().item() <= 1e-10


def test_tail_backward_formula_is_autograd_of_perceptual():
    """(B, CH) = (2, 24) on 2 x 3 x 2, features non-negative with zeros as after a ReLU.  One voxel of the prediction is all zero:
    the closed form gives 0 there and forms no NaN (autograd of sqrt at 0 does: inf * 0), everywhere else the two agree."""
    g = torch.Generator().manual_seed(5)
    fp = F.relu(torch.randn(2, 24, 2, 3, 2, generator=g, dtype=torch.float64))
    ft = F.relu(torch.randn(2, 24, 2, 3, 2, generator=g, dtype=torch.float64))
    fp[1, :, 0, 1, 1] = 0.0
    ft[0, :, 1, 2, 0] = 0.0                                               # a zero TARGET voxel is an ordinary point
    a = fp.clone().requires_grad_()
    want, = torch.autograd.grad(MR.perceptual(a, ft) * 2.5, a)
    got = GR.tail_backward(fp, ft, 2.5)
    assert bool(torch.isfinite(got).all())
    assert got[1, :, 0, 1, 1].abs().max().item() == 0.0
    keep = torch.ones(2, 1, 2, 3, 2, dtype=torch.bool)
    keep[1, :, 0, 1, 1] = False
    keep = keep.expand_as(got)
    assert bool(torch.isfinite(want[keep]).all())
    assert (got[keep] - want[keep]).abs().max().item() <= 1e-12 * want[keep].abs().max().item()
    # the device's algebraic form of the same expression: g_f = c_p p - c_t t
    eps, s = 1e-10, 2.0 * 2.5 / (2 * 12)
    n_p, n_t = fp.pow(2).sum(1, keepdim=True).sqrt(), ft.pow(2).sum(1, keepdim=True).sqrt()
    a_p, a_t = n_p + eps, n_t + eps
    safe = torch.where(n_p > 0, n_p, torch.ones_like(n_p))
    c_p = torch.where(n_p > 0, s * ((1 - n_p / a_p) + (fp * ft).sum(1, keepdim=True) / (a_t * safe)) / a_p ** 2, torch.zeros_like(n_p))
    c_t = torch.where(n_p > 0, s / (a_t * a_p), torch.zeros_like(n_p))
    assert ((c_p * fp - c_t * ft) - got).abs().max().item() <= 1e-12 * got.abs().max().item()


def test_grad_reference_modes_agree_on_a_small_case():
    """the three modes of the reference are one computation: f32 sits at rounding distance from f64, the emulation at bf16 distance"""
    net = MR.random_init(MR.RefResNet10(), seed=11)
    g = torch.Generator().manual_seed(9)
    y = torch.randn(1, 2, 17, 18, 19, generator=g)
    y_hat = y + 0.5 * torch.randn(y.shape, generator=g)
    out = {m: GR.perceptual_value_and_grad(net, y_hat, y, m, factor=1e3) for m in GR.MODES}

    def rel(a, b):
        return ((a.double() - b.double()).norm() / b.double().norm()).item()
    assert out["f64"][1].dtype == torch.float64 and out["emu"][1].dtype == torch.float32
    assert rel(out["f32"][1], out["f64"][1]) <= 1e-4
    assert 1e-4 < rel(out["emu"][1], out["f64"][1]) <= 0.2
    assert abs(out["f32"][0].item() - out["f64"][0].item()) <= 1e-4 * abs(out["f64"][0].item())
