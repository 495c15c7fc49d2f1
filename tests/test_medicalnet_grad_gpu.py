"""Backward of the MedicalNet Perceptual term on the GPU (csrc/medicalnet_bwd.hip) against tests/medicalnet_grad_ref.py.

The bounds are those of tests/medicalnet_checks.py, shared with tests/test_medicalnet_gpu.py: single_layer_check for one layer on
identical bf16-exact inputs; the WHOLE term is triangulated between the f64 reference and the bf16-emulating one.
Every device call under test runs on poisoned fresh memory (tests/alloc_poison.py).  The measured figures are printed
(pytest -s shows them) and quoted in DESIGN.md 8.13.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import medicalnet_grad_ref as GR
import medicalnet_ref as MR
import medicalnet_checks as C
from alloc_poison import KINDS, poisoned

pytestmark = pytest.mark.gpu
DEV = C.DEV
triangulate_f64 = functools.partial(C.triangulate, ref="f64")        # the exact reference of a gradient is f64


@pytest.fixture(scope="module")
def refnet():
    return C.make_refnet()


@pytest.fixture(scope="module")
def net(hip, refnet):
    return C.make_net(refnet)


# ------------------------------------------------------------------------------------------ data gradient, single layers
DGRAD = [
    # cin, cout, ks, stride, dilation, add + mask
    (64, 128, 3, 1, 1, False), (64, 128, 3, 2, 1, False), (64, 128, 3, 1, 2, False), (64, 128, 3, 1, 4, False),
    (256, 512, 3, 1, 4, True), (64, 128, 1, 1, 1, False), (64, 128, 1, 2, 1, False),
]


@pytest.mark.parametrize("cin,cout,ks,stride,dil,add_mask", DGRAD,
                         ids=[f"c{c[0]}_{c[1]}_k{c[2]}_s{c[3]}_d{c[4]}" + ("_add_mask" if c[5] else "") for c in DGRAD])
def test_dgrad_single_layer(hip, cin, cout, ks, stride, dil, add_mask):
    """N = 2, input 5 x 6 x 9 (odd, even, odd: both stride-2 border classes); the reference is f32 autograd of F.conv3d with the
    bf16-rounded weights, masked and summed in f32"""
    from unet_bssfp_amd import ops
    from unet_bssfp_amd.medicalnet import pack_dgrad_weight
    g = torch.Generator().manual_seed(1000 * ks + 100 * stride + dil + cin)
    x = torch.zeros(2, cin, 5, 6, 9, requires_grad=True)
    w = torch.randn(cout, cin, ks, ks, ks, generator=g) * (2.0 / (ks ** 3 * cin)) ** 0.5
    y = F.conv3d(x, C.q16(w), None, stride, dil * (ks // 2), dil)
    dy = C.q16(torch.randn(y.shape, generator=g))
    want, = torch.autograd.grad(y, x, dy)
    add = mask = None
    if add_mask:
        add, mask = C.q16(torch.randn(x.shape, generator=g)), C.q16(torch.randn(x.shape, generator=g))
        assert 0.4 < float((mask <= 0).float().mean()) < 0.6
        want = torch.where(mask > 0, want + add, torch.zeros_like(want))
    want = C.q16(want)
    wp = pack_dgrad_weight(w).to(DEV)
    dy_d = C.to_ndhwc(dy)
    add_d, mask_d = (None, None) if add is None else (C.to_ndhwc(add), C.to_ndhwc(mask))
    with poisoned("nan"):
        got = ops.medicalnet_dgrad(dy_d, wp, (2, 5, 6, 9, cin), ks, stride, dil, add=add_d, mask=mask_d)
        torch.cuda.synchronize()
    assert tuple(got.shape) == (2, 5, 6, 9, cin) and got.dtype == torch.bfloat16
    C.single_layer_check(f"dgrad {cin}->{cout} k{ks} s{stride} d{dil}" + (" +add +mask" if add_mask else ""), C.from_ndhwc(got), want)


@pytest.mark.parametrize("kind", KINDS)
def test_dgrad_writes_zeros_where_no_tap_reaches(hip, kind):
    """1 x 1 x 1 at stride 2: an input voxel with an odd coordinate is reached by no tap and must come back exactly 0 from
    poisoned memory; the extents 5 x 6 x 9 and 1 x 2 x 3 leave whole parity classes with one voxel or none"""
    from unet_bssfp_amd import ops
    from unet_bssfp_amd.medicalnet import pack_dgrad_weight
    g = torch.Generator().manual_seed(3)
    w = torch.randn(128, 64, 1, 1, 1, generator=g) * (2.0 / 64) ** 0.5
    wp = pack_dgrad_weight(w).to(DEV)
    for ext in ((5, 6, 9), (1, 2, 3)):
        out = tuple((n - 1) // 2 + 1 for n in ext)
        dy = C.q16(torch.randn(2, 128, *out, generator=g))
        dy_d = C.to_ndhwc(dy)
        with poisoned(kind):
            got = ops.medicalnet_dgrad(dy_d, wp, (2, *ext, 64), 1, 2, 1)
            torch.cuda.synchronize()
        got = C.from_ndhwc(got)
        reached = torch.zeros(ext, dtype=torch.bool)
        reached[::2, ::2, ::2] = True
        assert bool(torch.isfinite(got).all())
        assert got[:, :, ~reached].abs().max().item() == 0.0
        want = C.q16(torch.einsum("nodhw,oc->ncdhw", dy, C.q16(w).view(128, 64)))
        C.single_layer_check(f"dgrad k1 s2 {ext} ({kind})", got[:, :, ::2, ::2, ::2], want)


def test_dgrad_refuses_unsupported_shapes(hip):
    from unet_bssfp_amd import _lib, ops
    dy = torch.zeros(1, 4, 4, 4, 64, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(27 * 64 * 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.Mi355Error, match="dilation"):
        ops.medicalnet_dgrad(dy, w, (1, 4, 4, 4, 64), 3, 1, 3)
    dy3 = torch.zeros(1, 2, 2, 2, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.Mi355Error, match="stride"):
        ops.medicalnet_dgrad(dy3, w, (1, 4, 4, 4, 64), 3, 3, 1)
    w96 = torch.zeros(27 * 96 * 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.Mi355Error, match="cin and cout"):
        ops.medicalnet_dgrad(dy, w96, (1, 4, 4, 4, 96), 3, 1, 1)


def test_perceptual_loss_refusals(hip, net):
    from unet_bssfp_amd import losses
    x = torch.randn(1, 2, 16, 16, 16, device=DEV)
    with pytest.raises(NotImplementedError, match="backward"):
        losses.PerceptualLoss(net)(x.clone().requires_grad_(), x)
    with pytest.raises(NotImplementedError, match="target"):
        losses.PerceptualLoss(net, differentiable=True)(x.clone().requires_grad_(), x.clone().requires_grad_())
    terms = losses.reference_recon_terms(net)
    assert list(terms) == ["Perceptual"] and terms["Perceptual"].differentiable and terms["Perceptual"].factor == 1e3


# ------------------------------------------------------------------------------------------ pool backward and stem
def _stem_input(case):
    g = torch.Generator().manual_seed(31)
    x = 3.0 + 0.5 * torch.randn(3, 1, 17, 20, 23, generator=g)
    if case == "border_slab":
        x[..., :5] = 4.25
        x[:, :, -4:] = 1.5
    return x, g


def _positive_ties(x, pooled):
    """number of (window, channel) pairs of MaxPool3d(k3, s2, p1) whose maximum is positive and attained more than once"""
    od, oh, ow = pooled.shape[2:]
    xp = F.pad(x, (1, 1, 1, 1, 1, 1), value=float("-inf"))
    count = torch.zeros_like(pooled)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                count += xp[:, :, kd:kd + 2 * od - 1:2, kh:kh + 2 * oh - 1:2, kw:kw + 2 * ow - 1:2] == pooled
    return int(((count > 1) & (pooled > 0)).sum())


def test_pool_backward_takes_the_first_maximum_of_a_tie(hip):
    """values on a grid of 0.5, so that most windows hold their maximum more than once, on 7 x 6 x 9 (odd, even, odd): the
    gradient goes to the FIRST maximum in (d, h, w) order, as F.max_pool3d routes it on the CPU"""
    from unet_bssfp_amd import ops
    g = torch.Generator().manual_seed(17)
    x = torch.round(torch.randn(2, 64, 7, 6, 9, generator=g) * 2) / 2
    a = x.clone().requires_grad_()
    pooled = F.max_pool3d(a, 3, 2, 1)
    assert _positive_ties(x, pooled.detach()) > 0.3 * pooled.numel()
    dy = C.q16(torch.randn(pooled.shape, generator=g))
    want, = torch.autograd.grad(pooled, a, dy)
    want = C.q16(want * (x > 0))
    x_d, dy_d = C.to_ndhwc(x), C.to_ndhwc(dy)
    with poisoned("big"):
        got = ops.medicalnet_maxpool_bwd(x_d, dy_d)
        torch.cuda.synchronize()
    C.single_layer_check("pool backward, ties", C.from_ndhwc(got), want)


@pytest.mark.parametrize("case", ["offset", "border_slab"])
def test_pool_backward_with_the_stem_mask(hip, net, case):
    """N = 3 volumes of 17 x 20 x 23, the inputs of test_stem_and_pool; border_slab makes whole windows of equal positive values,
    so the arg-max has to be the FIRST maximum in (d, h, w) order as in F.max_pool3d on the CPU.  The stem output of the device
    is the input of both sides."""
    from unet_bssfp_amd import ops
    x, g = _stem_input(case)
    p = net.packed()
    xd = x.to(DEV)
    stem = ops.medicalnet_stem(xd.view(-1, *xd.shape[2:]), ops.medicalnet_moments(xd), p["stem.w"], p["stem.b"])
    s_cpu = C.from_ndhwc(stem)
    a = s_cpu.clone().requires_grad_()
    pooled = F.max_pool3d(a, 3, 2, 1)
    dy = C.q16(torch.randn(pooled.shape, generator=g))
    want, = torch.autograd.grad(pooled, a, dy)
    want = C.q16(want * (s_cpu > 0))
    C.log(f"pool backward ({case}): {_positive_ties(s_cpu, pooled.detach())} windows whose positive maximum occurs more than once")
    dy_d = C.to_ndhwc(dy)
    with poisoned("nan"):
        got = ops.medicalnet_maxpool_bwd(stem, dy_d)
        torch.cuda.synchronize()
    assert got.shape == stem.shape
    C.single_layer_check(f"pool backward x stem mask ({case})", C.from_ndhwc(got), want)


@pytest.mark.parametrize("case", ["offset", "border_slab"])
def test_stem_dgrad_and_normalisation_backward(hip, net, refnet, case):
    """the gradient with respect to the normalised input against f32 autograd of F.conv3d(x^, w_bf16, None, 2, 3); the device
    result is f32, so the single-layer bounds (which speak of bf16-representable tensors) are applied to both sides rounded to
    bf16, and rel-L2 <= 1e-3 to the f32 values as they are.  The two f64 sums against f64 sums of the device's own g."""
    from unet_bssfp_amd import ops
    x, g = _stem_input(case)
    p = net.packed()
    w, _ = MR.fold(refnet.conv1, refnet.bn1)
    xh = torch.zeros(3, 1, 17, 20, 23, requires_grad=True)
    y = F.conv3d(xh, C.q16(w), None, 2, 3)
    dy = C.q16(torch.randn(y.shape, generator=g)) * (torch.rand(y.shape, generator=g) > 0.5)     # as behind a ReLU mask
    want, = torch.autograd.grad(y, xh, dy)
    xd = x.to(DEV)
    vols = xd.view(-1, *xd.shape[2:])
    ms = ops.medicalnet_moments(xd)
    dy_d = C.to_ndhwc(dy)
    with poisoned("nan"):
        got, part = ops.medicalnet_stem_dgrad(dy_d, p["stem.dw"], vols, ms)
        dv = ops.medicalnet_norm_bwd(got, vols, ms, part)
        torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.shape == vols.shape
    got_c = got.cpu().view(want.shape)
    rel = C.rel(got_c, want)
    C.log(f"stem dgrad ({case}), f32 as it is: rel-L2 {rel:.2e}")
    assert rel <= 1e-3, rel
    C.single_layer_check(f"stem dgrad ({case}), both rounded to bf16", C.q16(got_c), C.q16(want))
    mean, std = ms.cpu().double()
    x_hat = (x.double() - mean) / std
    sums = part.cpu().sum(0)
    for name, s_got, s_want in (("sum g", sums[0], got_c.double().sum()), ("sum g x^", sums[1], (got_c.double() * x_hat).sum())):
        err = abs(s_got.item() - s_want.item()) / abs(s_want.item())
        C.log(f"stem dgrad ({case}): {name} {s_got.item():.9e}, f64 sum of the device's g {s_want.item():.9e}, relative {err:.1e}")
        assert err <= 1e-6, (name, err)
    # the last launch: closed form in f64 from the device's g.  f32 mean / std and f32 arithmetic on values of order |g|:
    # 1e-5 of the tensor's scale leaves two decimal digits of room over eps_f32 * (|mean| / std + a few operations)
    want_dv = GR.normalise_backward(got_c.double(), x.double())
    err = (dv.cpu().view(want_dv.shape).double() - want_dv).abs().max().item() / want_dv.abs().max().item()
    C.log(f"normalisation backward ({case}): max error {err:.1e} of the tensor's scale")
    assert err <= 1e-5, err


# ------------------------------------------------------------------------------------------ the whole term, triangulated
FACTOR = 1e3


def _hip_value_and_grad(net, y_hat, y, up=None, poison=None):
    from unet_bssfp_amd import losses
    term = losses.PerceptualLoss(net, differentiable=True, factor=FACTOR)
    a = y_hat.to(DEV).requires_grad_()
    b = y.to(DEV)

    def run():
        value = term(a, b)
        grad, = torch.autograd.grad(value, a, up)
        torch.cuda.synchronize()
        return value.detach(), grad
    if poison is None:
        return run()
    with poisoned(poison):
        return run()


@pytest.fixture(scope="module")
def grad_case(refnet):
    """(B, C) = (2, 2) at 33 x 40 x 47 (layer2 and later run at 5 x 5 x 6, the smallest extent where dilation-4 taps are live),
    prediction = target + noise, every channel at its own scale and offset; the three references, computed once"""
    g = torch.Generator().manual_seed(52)
    scale = torch.tensor([1.0, 2.5]).view(1, 2, 1, 1, 1)
    shift = torch.tensor([0.0, 1.0]).view(1, 2, 1, 1, 1)
    y = torch.randn(2, 2, 33, 40, 47, generator=g) * scale + shift
    y_hat = y + 0.5 * torch.randn(y.shape, generator=g) * scale
    ref = {m: GR.perceptual_value_and_grad(refnet, y_hat, y, m, FACTOR) for m in GR.MODES}
    return y_hat, y, ref


def test_perceptual_gradient_triangulated(hip, net, grad_case):
    from unet_bssfp_amd import losses
    y_hat, y, ref = grad_case
    value, grad = _hip_value_and_grad(net, y_hat, y, poison="nan")
    assert grad.shape == y_hat.shape and grad.dtype == torch.float32 and bool(torch.isfinite(grad).all())
    plain = losses.PerceptualLoss(net, factor=FACTOR)(y_hat.to(DEV), y.to(DEV))
    assert torch.equal(value, plain), (value.item(), plain.item())         # the non-differentiable path's value, bit for bit
    assert torch.equal(losses.PerceptualLoss(net)(y_hat.to(DEV), y.to(DEV)) * FACTOR, plain)
    C.log(f"Perceptual value x 1e3: hip {value.item():.6e}, f64 {ref['f64'][0].item():.6e}, emu {ref['emu'][0].item():.6e}")
    got = grad.cpu()
    C.log(f"rel(f32, f64) of the gradient {C.rel(ref['f32'][1], ref['f64'][1]):.3e}")
    triangulate_f64("dL/dy_hat, (B, C) = (2, 2) at 33 x 40 x 47", C.rel(got, ref["f64"][1]), C.rel(got, ref["emu"][1]),
                 C.rel(ref["emu"][1], ref["f64"][1]))
    # f32 reference: the f64 one in single precision, a third witness that the f64 bound is not met by luck
    assert C.rel(got, ref["f32"][1]) <= 1.25 * C.rel(ref["emu"][1], ref["f32"][1]) + 0.02
    for c in range(2):                                                    # every channel's gradient lands in its own channel
        own = C.rel(got[:, c], ref["f64"][1][:, c])
        swapped = C.rel(got[:, c], ref["f64"][1][:, 1 - c])
        C.log(f"channel {c}: rel to its own reference channel {own:.3e}, to the other {swapped:.3e}")
        assert own <= 1.25 * C.rel(ref["emu"][1][:, c], ref["f64"][1][:, c]) + 0.02 and swapped > 0.5, (c, own, swapped)
    # a second backward gives the same bits, also on memory poisoned with the other value
    again = _hip_value_and_grad(net, y_hat, y, poison="big")
    assert torch.equal(again[0], value) and torch.equal(again[1], grad)
    # an upstream gradient scales the result: (2 g) is exact in binary floating point
    twice = _hip_value_and_grad(net, y_hat, y, up=torch.tensor(2.0, device=DEV))
    assert torch.equal(twice[1], 2 * grad)


def test_perturbing_one_target_channel_moves_the_gradient_as_in_the_reference(hip, net, refnet):
    """(B, C) = (1, 2) at 17 x 18 x 19.  Only channel 1 of the TARGET is perturbed; the prediction's forward, and with it every
    ReLU mask of the backward, is unchanged, so the change of the gradient is the linear backward of the change at the tail.
    The channels are coupled where the reference couples them -- the unit normalisation over all 512 C feature channels of a
    voxel and the mean / std of the whole tensor -- so the other channel's gradient moves too, and it has to move as the
    reference's does: the change is triangulated as a whole and per channel, and does not fit the other channel's change."""
    g = torch.Generator().manual_seed(53)
    scale = torch.tensor([1.0, 2.5]).view(1, 2, 1, 1, 1)
    y = torch.randn(1, 2, 17, 18, 19, generator=g) * scale + torch.tensor([0.0, 1.0]).view(1, 2, 1, 1, 1)
    y_hat = y + 0.5 * torch.randn(y.shape, generator=g) * scale
    y2 = y.clone()
    y2[:, 1] += 1.5 * torch.randn(y[:, 1].shape, generator=g)
    delta = {}
    for m in ("f64", "emu"):
        delta[m] = (GR.perceptual_value_and_grad(refnet, y_hat, y2, m, FACTOR)[1]
                    - GR.perceptual_value_and_grad(refnet, y_hat, y, m, FACTOR)[1])
    delta["hip"] = (_hip_value_and_grad(net, y_hat, y2)[1] - _hip_value_and_grad(net, y_hat, y)[1]).cpu()
    triangulate_f64("change of dL/dy_hat", C.rel(delta["hip"], delta["f64"]), C.rel(delta["hip"], delta["emu"]),
                 C.rel(delta["emu"], delta["f64"]))
    for c in range(2):
        own = C.rel(delta["hip"][:, c], delta["f64"][:, c])
        swapped = C.rel(delta["hip"][:, c], delta["f64"][:, 1 - c])
        share = (delta["hip"][:, c].double().norm() / delta["hip"].double().norm()).item()
        C.log(f"change in channel {c}: share of the whole change {share:.3f}, rel to its own reference channel {own:.3e}, "
             f"to the other {swapped:.3e}")
        assert own <= 1.25 * C.rel(delta["emu"][:, c], delta["f64"][:, c]) + 0.02 and swapped > 0.5, (c, own, swapped)


# ------------------------------------------------------------------------------------------ hipGraph
def test_perceptual_forward_and_backward_replay_from_a_graph_bit_identically(hip, net):
    """as test_perceptual_forward_replays_from_a_graph_bit_identically, with the backward in the capture and a different upstream
    gradient per case, written into a device tensor: neither the inputs' statistics nor the gradient were baked in"""
    from unet_bssfp_amd import losses
    term = losses.PerceptualLoss(net, differentiable=True, factor=FACTOR)
    g = torch.Generator().manual_seed(61)
    cases = [(s0 + sc * torch.randn(1, 2, 17, 20, 23, generator=g), s0 + sc * torch.randn(1, 2, 17, 20, 23, generator=g))
             for s0, sc in ((0.0, 1.0), (3.0, 0.5), (-2.0, 4.0))]
    cases = [(a.to(DEV), b.to(DEV), torch.tensor(u, device=DEV)) for (a, b), u in zip(cases, (1.0, 0.37, -2.5))]

    def both(a, b, u):
        out = term(a, b)
        grad, = torch.autograd.grad(out, a, u)
        return out, grad
    eager = [tuple(t.clone() for t in both(a.clone().requires_grad_(), b, u)) for a, b, u in cases]
    sa, sb, su = cases[0][0].clone().requires_grad_(), cases[0][1].clone(), cases[0][2].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both(sa, sb, su)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, grad = both(sa, sb, su)
    for (a, b, u), (want_out, want_grad) in list(zip(cases, eager))[1:]:
        with torch.no_grad():
            sa.copy_(a), sb.copy_(b), su.copy_(u)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want_out), (out.item(), want_out.item())
        assert torch.equal(grad, want_grad)
    assert len({v[0].item() for v in eager}) == 3
    assert not torch.equal(eager[1][1], eager[2][1])


# ------------------------------------------------------------------------------------------ in the model's reconstruction slot
def test_generator_step_on_the_reference_objective(hip, net):
    """bSSFPToDWITensorModel with extra_recon_terms = reference_recon_terms(net): recon = (L1 + 1e3 Perceptual) / 2 * recon_factor"""
    import unet_bssfp_amd as M
    from unet_bssfp_amd import losses
    from unet_bssfp_amd.functional import DropoutState
    from unet_bssfp_amd.gan import bSSFPToDWITensorModel, synthetic_batch
    batch = synthetic_batch(2, 32, seed=77, device=DEV)

    def gen_phase(**kw):
        torch.manual_seed(0)                                              # both models start from the same weights
        DropoutState.reset()
        gen, discr = M.Generator("bssfp", dropout=0.0).to(DEV), M.Discriminator("bssfp").to(DEV)
        model = bSSFPToDWITensorModel("bssfp", gen=gen, discr=discr, **kw).train()
        logs = {}
        model._phase_gen(batch, logs)
        model._finish_grads("gen")
        torch.cuda.synchronize()
        return model, logs, {n: p.grad.detach().clone() for n, p in model.gen.named_parameters() if p.grad is not None}
    model, logs, grads = gen_phase(extra_recon_terms=losses.reference_recon_terms(net))
    _, plain_logs, plain_grads = gen_phase()
    assert "train_gen_loss_recon_Perceptual" in logs and "train_gen_loss_recon_Perceptual" not in plain_logs
    x, y = model.unpack_batch(batch)
    with torch.no_grad():
        want = losses.PerceptualLoss(net)(model._gen_for_discr(x), y) * 1e3
    perc = logs["train_gen_loss_recon_Perceptual"]
    assert torch.isfinite(perc) and perc.item() > 0 and torch.equal(perc, want), (perc.item(), want.item())
    v = {k: float(t) for k, t in logs.items()}
    recon = (v["train_gen_loss_recon_L1"] + v["train_gen_loss_recon_Perceptual"]) / 2 * model.recon_factor
    assert v["train_gen_loss_recon"] == pytest.approx(recon, rel=1e-6)
    assert v["train_gen_loss"] == pytest.approx(v["train_gen_loss_adversarial"] + recon, rel=1e-6)
    assert grads and set(grads) == set(plain_grads)
    # a convolution bias in front of a normalisation has no gradient under any objective: exactly zero in both steps
    idle = [n for n in grads if not grads[n].any() and not plain_grads[n].any()]
    C.log(f"generator step: {len(grads)} gradients, exactly zero under both objectives: {idle}")
    assert all(n.endswith(".bias") for n in idle) and len(idle) < len(grads) // 2, idle
    for name, gr in grads.items():
        assert bool(torch.isfinite(gr).all()), name
        assert name in idle or not torch.equal(gr, plain_grads[name]), name
