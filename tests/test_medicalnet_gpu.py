"""MedicalNet ResNet-10 extractor, Perceptual distance and FID on the GPU (csrc/medicalnet.hip) against tests/medicalnet_ref.py.

The bounds are those of tests/medicalnet_checks.py (single_layer_check for one layer on identical bf16-exact inputs, triangulate
for the whole network between the f32 and the bf16-emulating reference), shared with tests/test_medicalnet_grad_gpu.py.
The measured figures are printed (pytest -s shows them) and quoted in DESIGN.md 8.13.
"""
import pytest
import torch
import torch.nn.functional as F

import medicalnet_checks as C
import medicalnet_ref as MR

pytestmark = pytest.mark.gpu
DEV = C.DEV


@pytest.fixture(scope="module")
def refnet():
    return C.make_refnet()


@pytest.fixture(scope="module")
def net(hip, refnet):
    return C.make_net(refnet)


# ------------------------------------------------------------------------------------------ single layers, identical inputs
CONVS = [
    # cin, cout, stride, dilation, residual + ReLU
    (64, 128, 1, 1, False), (64, 128, 2, 1, False), (64, 128, 1, 2, False), (64, 128, 1, 4, False), (256, 512, 1, 4, True),
]


@pytest.mark.parametrize("cin,cout,stride,dil,res_relu", CONVS, ids=[f"c{c[0]}_{c[1]}_s{c[2]}_d{c[3]}" + ("_res" if c[4] else "")
                                                                     for c in CONVS])
def test_residual_conv_single_layer(hip, cin, cout, stride, dil, res_relu):
    """N = 2 on a 5 x 6 x 9 grid: the +-4 taps of dilation 4 fall in range and out of range on every axis"""
    from unet_bssfp_amd import ops
    from unet_bssfp_amd.medicalnet import pack_conv_weight
    g = torch.Generator().manual_seed(100 * stride + dil + cin)
    x = C.q16(torch.randn(2, cin, 5, 6, 9, generator=g))
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) * (2.0 / (27 * cin)) ** 0.5
    b = 0.3 * torch.randn(cout, generator=g)
    want = F.conv3d(x, C.q16(w), b, stride, dil, dil)
    res = C.q16(torch.randn(want.shape, generator=g)) if res_relu else None
    if res_relu:
        want = F.relu(want + res)
    want = C.q16(want)
    got = ops.medicalnet_conv(C.to_ndhwc(x), pack_conv_weight(w).to(DEV), b.to(DEV), cout, 3, stride, dil,
                              residual=None if res is None else C.to_ndhwc(res), relu=res_relu)
    assert tuple(got.shape) == (2, *want.shape[2:], cout)
    C.single_layer_check(f"conv {cin}->{cout} s{stride} d{dil}" + (" +res +relu" if res_relu else ""), C.from_ndhwc(got), want)


@pytest.mark.parametrize("stride", [1, 2])
def test_downsample_1x1x1_single_layer(hip, stride):
    from unet_bssfp_amd import ops
    from unet_bssfp_amd.medicalnet import pack_conv_weight
    g = torch.Generator().manual_seed(7 + stride)
    x = C.q16(torch.randn(2, 64, 5, 6, 9, generator=g))
    w = torch.randn(128, 64, 1, 1, 1, generator=g) * (2.0 / 64) ** 0.5
    b = 0.3 * torch.randn(128, generator=g)
    want = C.q16(F.conv3d(x, C.q16(w), b, stride))
    got = ops.medicalnet_conv(C.to_ndhwc(x), pack_conv_weight(w).to(DEV), b.to(DEV), 128, 1, stride, 1, relu=False)
    C.single_layer_check(f"downsample 64->128 s{stride}", C.from_ndhwc(got), want)


def test_conv_refuses_unsupported_shapes(hip):
    from unet_bssfp_amd import _lib, ops
    x = torch.zeros(1, 4, 4, 4, 64, dtype=torch.bfloat16, device=DEV)
    b = torch.zeros(64, device=DEV)
    w = torch.zeros(27 * 64 * 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.Mi355Error, match="dilation"):
        ops.medicalnet_conv(x, w, b, 64, 3, 1, 3)
    with pytest.raises(_lib.Mi355Error, match="stride"):
        ops.medicalnet_conv(x, w, b, 64, 3, 3, 1)
    x96 = torch.zeros(1, 4, 4, 4, 96, dtype=torch.bfloat16, device=DEV)
    w96 = torch.zeros(27 * 96 * 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.Mi355Error, match="cin and cout"):
        ops.medicalnet_conv(x96, w96, b, 64, 3, 1, 1)


def _stem_pool(net, x):
    from unet_bssfp_amd import ops
    p = net.packed()
    ms = ops.medicalnet_moments(x)
    y = ops.medicalnet_maxpool(ops.medicalnet_stem(x.view(-1, *x.shape[2:]), ms, p["stem.w"], p["stem.b"]))
    return ms, C.from_ndhwc(y)


@pytest.mark.parametrize("case", ["offset", "border_slab"])
def test_stem_and_pool(hip, net, refnet, case):
    """N = 3 volumes of 17 x 20 x 23 (odd and non-cubic: every border class of k7 s2 p3 and k3 s2 p1).  The input has mean ~3
    and std ~0.5, so a missing normalisation, one folded into the weights (padding would then enter as -mean / std instead of
    0) or a padding applied before it all fail.  border_slab: the input is constant on one border slab."""
    g = torch.Generator().manual_seed(31)
    x = 3.0 + 0.5 * torch.randn(3, 1, 17, 20, 23, generator=g)
    if case == "border_slab":
        x[..., :5] = 4.25
        x[:, :, -4:] = 1.5
    ms, got = _stem_pool(net, x.to(DEV))
    mean, std = x.double().mean().item(), x.double().std().item()
    assert abs(ms[0].item() - mean) <= 1e-6 * abs(mean) and abs(ms[1].item() - std) <= 1e-6 * std, (ms.tolist(), mean, std)
    with torch.no_grad():
        want = refnet.stem(MR.normalise(x), emulate=True)
    assert got.shape == want.shape == (3, 64, 5, 5, 6)
    C.single_layer_check(f"stem + pool ({case})", got, want)


# ------------------------------------------------------------------------------------------ whole network, triangulated
def test_whole_extractor(hip, net, refnet):
    """N = 4 volumes of 33 x 40 x 47: stem 17 x 20 x 24, pool 9 x 10 x 12, 5 x 5 x 6 from layer2 on"""
    g = torch.Generator().manual_seed(41)
    x = torch.randn(4, 1, 33, 40, 47, generator=g)
    got = net(x.to(DEV)).cpu()
    f32, emu = refnet(x), refnet(x, emulate=True)
    assert got.shape == f32.shape == (4, 512, 5, 5, 6) and got.dtype == torch.float32
    C.triangulate("whole extractor", C.rel(got, f32), C.rel(got, emu), C.rel(emu, f32))


@pytest.fixture(scope="module")
def pair_case(refnet):
    """(B, C) = (2, 3) at 33 x 40 x 47, prediction = target + noise, every channel at its own scale and offset; the reference
    features of both, f32 and emulated, computed once"""
    g = torch.Generator().manual_seed(51)
    scale = torch.tensor([1.0, 2.5, 0.4]).view(1, 3, 1, 1, 1)
    shift = torch.tensor([0.0, 1.0, -0.5]).view(1, 3, 1, 1, 1)
    y = torch.randn(2, 3, 33, 40, 47, generator=g) * scale + shift
    y_hat = y + 0.5 * torch.randn(y.shape, generator=g) * scale
    ref = {(name, emulate): MR.features(refnet, t, emulate) for name, t in (("y_hat", y_hat), ("y", y)) for emulate in (False, True)}
    return y_hat, y, ref


def _scalar_rel(a, b):
    return abs(a - b) / abs(b)


def test_perceptual_value_and_fid(hip, net, pair_case):
    from unet_bssfp_amd import losses, metrics
    from unet_bssfp_amd.medicalnet import medicalnet_distances
    y_hat, y, ref = pair_case
    a, b = y_hat.to(DEV), y.to(DEV)
    term, fid = losses.PerceptualLoss(net), metrics.FIDMedicalNet(net)
    value = term(a, b)
    assert value.dim() == 0 and value.dtype == torch.float32
    perc = {e: MR.perceptual(ref[("y_hat", e)], ref[("y", e)]).item() for e in (False, True)}
    C.triangulate("Perceptual value", _scalar_rel(value.item(), perc[False]), _scalar_rel(value.item(), perc[True]),
                 _scalar_rel(perc[True], perc[False]))
    # the FID features: per-channel feeding order (channel c of the input -> feature channels [512 c, 512 c + 512))
    _, fp, ft = medicalnet_distances(net, a, b)
    assert fp.shape == ft.shape == (2, 3 * 512)
    feat = {e: MR.fid_features(ref[("y_hat", e)]) for e in (False, True)}
    C.triangulate("FID features", C.rel(fp.cpu(), feat[False]), C.rel(fp.cpu(), feat[True]), C.rel(feat[True], feat[False]))
    for c in range(3):
        blk = slice(512 * c, 512 * c + 512)
        own = C.rel(fp.cpu()[:, blk], feat[False][:, blk])
        swapped = min(C.rel(fp.cpu()[:, blk], feat[False][:, slice(512 * o, 512 * o + 512)]) for o in range(3) if o != c)
        assert own < 0.05 < swapped, (c, own, swapped)
    got_fid = fid(a, b)
    assert got_fid.dim() == 0 and got_fid.dtype == torch.float32
    fids = {e: MR.fid_svd(MR.fid_features(ref[("y_hat", e)]), MR.fid_features(ref[("y", e)])) for e in (False, True)}
    C.triangulate("FID", _scalar_rel(got_fid.item(), fids[False]), _scalar_rel(got_fid.item(), fids[True]),
                 _scalar_rel(fids[True], fids[False]))
    # identical tensors
    assert term(a, a).item() == 0.0
    trace = ((ft.double() - ft.double().mean(0)) ** 2).sum().item()      # tr Sigma of the 2 items (divisor B - 1 = 1)
    assert trace > 0 and abs(fid(b, b).item()) <= 1e-6 * trace


def test_perceptual_loss_refuses_grad(hip, net):
    from unet_bssfp_amd import losses
    x = torch.randn(1, 2, 16, 16, 16, device=DEV)
    with pytest.raises(NotImplementedError, match="backward"):
        losses.PerceptualLoss(net)(x.clone().requires_grad_(), x)


def test_perceptual_forward_replays_from_a_graph_bit_identically(hip, net):
    """One stream; the replay on other inputs must equal the eager result bit for bit: no host value (mean, std, a shape-
    dependent sum) was baked in at capture.  FID is left out: its B x B f64 SVD goes through torch.linalg, whose backend may
    synchronise with the host."""
    from unet_bssfp_amd import losses
    term = losses.PerceptualLoss(net)
    g = torch.Generator().manual_seed(61)
    cases = [(s0 + sc * torch.randn(1, 2, 17, 20, 23, generator=g), s0 + sc * torch.randn(1, 2, 17, 20, 23, generator=g))
             for s0, sc in ((0.0, 1.0), (3.0, 0.5), (-2.0, 4.0))]
    cases = [(a.to(DEV), b.to(DEV)) for a, b in cases]
    eager = [term(a, b).clone() for a, b in cases]
    sa, sb = cases[0][0].clone(), cases[0][1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        term(sa, sb)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = term(sa, sb)
    for (a, b), want in list(zip(cases, eager))[1:]:
        sa.copy_(a), sb.copy_(b)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), (out.item(), want.item())
    assert len({v.item() for v in eager}) == 3


def test_model_logs_fid_and_perceptual_when_given_the_network(hip, net):
    from unet_bssfp_amd import losses
    from unet_bssfp_amd.gan import bSSFPToDWITensorModel, synthetic_batch
    batch = synthetic_batch(2, 32, seed=77, device=DEV)
    import unet_bssfp_amd as M
    torch.manual_seed(0)
    gen, discr = M.Generator("bssfp").to(DEV).eval(), M.Discriminator("bssfp").to(DEV).eval()      # shared: identical weights
    plain = bSSFPToDWITensorModel("bssfp", gen=gen, discr=discr).eval()
    model = bSSFPToDWITensorModel("bssfp", gen=gen, discr=discr, medicalnet=net).eval()
    plain.validation_step(batch)
    model.validation_step(batch)
    new = {"val_metric_FID", "val_metric_Perceptual"}
    assert set(model.last_logs) - set(plain.last_logs) == new and set(plain.last_logs) <= set(model.last_logs)
    assert {k for k in plain.last_logs if k.startswith("val_metric_")} == {"val_metric_PSNR", "val_metric_SSIM", "val_metric_L1"}
    for k in plain.last_logs:                                             # the objective and every other log are untouched
        assert torch.equal(plain.last_logs[k], model.last_logs[k]), k
    assert set(model.state_dict()) == set(plain.state_dict())
    x, y = model.unpack_batch(batch)
    with torch.no_grad():
        want = losses.PerceptualLoss(net)(model(x), y) * model.perceptual_factor
    got = model.last_logs["val_metric_Perceptual"]
    assert torch.isfinite(got) and got.item() > 0 and torch.equal(got, want)
    assert torch.isfinite(model.last_logs["val_metric_FID"])
