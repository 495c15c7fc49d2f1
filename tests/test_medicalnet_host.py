"""Host side of the MedicalNet ResNet-10 extractor (no GPU): weight extraction from a reference-style checkpoint, the
BatchNorm fold, and the B x B form of FID against the general sqrtm form."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import medicalnet_ref as MR
from oracle import unet_ref as R
from unet_bssfp_amd import checkpoint as ck, gan, medicalnet, metrics

PREFIX = "recon_criterion.perceptual.perceptual_function.model."      # arbitrary: only 'recon_criterion.' is fixed


def _cpu_model(seed=0):
    torch.manual_seed(seed)
    return gan.bSSFPToDWITensorModel("bssfp", batch_size=1, gen=R.RefGenerator("bssfp", dropout=0.0),
                                     discr=R.RefDiscriminator("bssfp"), optimizer_class=torch.optim.AdamW)


def test_medicalnet_state_dict_from_a_reference_style_checkpoint(tmp_path):
    ref = MR.random_init(MR.RefResNet10(), seed=5)
    model = _cpu_model()
    d = ck.checkpoint_dict(model)
    d["optimizer_states"] = []
    plain = dict(d)                                                       # the same checkpoint without the network
    plain["state_dict"] = dict(d["state_dict"])
    foreign = {PREFIX + k: v.clone() for k, v in ref.state_dict().items()}
    d["state_dict"].update(foreign)
    d["state_dict"]["recon_criterion.l1_weight"] = torch.ones(1)          # a key under recon_criterion that is not the network's
    torch.save(d, tmp_path / "ref.ckpt")

    for source in (tmp_path / "ref.ckpt", d, d["state_dict"]):
        sd = ck.medicalnet_state_dict(source)
        assert set(sd) == set(ref.state_dict()) and "conv1.weight" in sd and "layer2.0.downsample.1.running_var" in sd
    other = MR.RefResNet10()
    other.load_state_dict(sd, strict=True)
    ours = medicalnet.MedicalNetResNet10()
    ours.load_state_dict(sd, strict=True)
    for k, v in ref.state_dict().items():
        assert torch.equal(other.state_dict()[k], v) and torch.equal(ours.state_dict()[k], v), k
    assert not ours.training and not any(p.requires_grad for p in ours.parameters())
    assert not ours.train().training                                      # frozen: there is no training mode

    info = ck.load_checkpoint(_cpu_model(seed=3), tmp_path / "ref.ckpt")  # the model loader still lists, and does not load, them
    assert info["ignored_keys"] == sorted(list(foreign) + ["recon_criterion.l1_weight"])

    with pytest.raises(KeyError, match="MedicalNet"):
        ck.medicalnet_state_dict(plain)
    plain["state_dict"]["recon_criterion.perceptual.net.conv1.weight"] = torch.zeros(4, 1, 3, 3, 3)   # wrong shape: not the stem
    with pytest.raises(KeyError, match="MedicalNet"):
        ck.medicalnet_state_dict(plain)


def test_model_keeps_the_extractor_out_of_its_state(tmp_path):
    """the frozen network is shared, not owned: no new keys in state_dict / checkpoints, no new parameters to optimise"""
    net = medicalnet.MedicalNetResNet10()
    with_net = gan.bSSFPToDWITensorModel("bssfp", batch_size=1, gen=R.RefGenerator("bssfp", dropout=0.0),
                                         discr=R.RefDiscriminator("bssfp"), optimizer_class=torch.optim.AdamW, medicalnet=net)
    assert set(with_net.state_dict()) == set(_cpu_model().state_dict())
    assert metrics.reference_metric_fns()[-1][1] == "L1" and len(metrics.reference_metric_fns()) == 3
    fns = metrics.reference_metric_fns(medicalnet=net)
    assert [n for _, n in fns] == ["PSNR", "SSIM", "L1", "FID"] and fns[-1][0].net is net


@pytest.mark.parametrize("cin,cout,ks,stride,dil", [(1, 64, 7, 2, 1), (64, 128, 3, 2, 1), (16, 32, 3, 1, 4), (64, 128, 1, 2, 1)])
def test_bn_fold_matches_conv_then_eval_bn_in_f64(cin, cout, ks, stride, dil):
    g = torch.Generator().manual_seed(cin + cout)
    conv = torch.nn.Conv3d(cin, cout, ks, stride=stride, padding=dil * (ks // 2), dilation=dil, bias=False).double()
    bn = torch.nn.BatchNorm3d(cout, eps=medicalnet.EPS).double().eval()
    with torch.no_grad():
        bn.running_var.copy_(0.5 + 1.5 * torch.rand(cout, generator=g, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(cout, generator=g, dtype=torch.float64))
        bn.weight.copy_(0.5 + torch.rand(cout, generator=g, dtype=torch.float64))
        bn.bias.copy_(torch.randn(cout, generator=g, dtype=torch.float64))
    x = torch.randn(2, cin, 9, 10, 11, generator=g, dtype=torch.float64)
    with torch.no_grad():
        want = bn(conv(x))
        w, b = medicalnet.fold_bn(conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
        got = F.conv3d(x, w, b, stride, dil * (ks // 2), dil)
    assert w.dtype == torch.float64
    assert (got - want).norm() <= 1e-12 * want.norm()
    assert (got - want).abs().max() <= 1e-12 * want.abs().max()


def test_packed_weight_layouts():
    """element maps the kernels read (include/mi355_unet.h), checked with exactly representable integers"""
    w = torch.arange(128 * 64 * 27, dtype=torch.float32).reshape(128, 64, 3, 3, 3) % 251
    p = medicalnet.pack_conv_weight(w).float()
    assert p.shape == (27, 4, 128, 16)
    for tap, q, co, e in [(0, 0, 0, 0), (5, 1, 77, 3), (26, 3, 127, 15), (13, 2, 64, 8)]:
        kd, kh, kw = tap // 9, tap // 3 % 3, tap % 3
        assert p[tap, q, co, e] == w[co, 16 * q + e, kd, kh, kw]
    s = torch.arange(64 * 343, dtype=torch.float32).reshape(64, 1, 7, 7, 7) % 253 + 1
    ps = medicalnet.pack_stem_weight(s).float()
    assert ps.shape == (25, 64, 16)
    for step in range(25):
        for e in range(16):
            pair, kw = 2 * step + e // 8, e % 8
            want = s[9, 0, pair // 7, pair % 7, kw] if (pair < 49 and kw < 7) else 0.0
            assert ps[step, 9, e] == want
    assert (ps != 0).sum() == 64 * 343


def _feats(b, p, seed, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    mix = torch.randn(p, p, generator=g, dtype=torch.float64) / p ** 0.5
    return torch.randn(b, p, generator=g, dtype=torch.float64) @ mix + shift


def test_fid_bxb_form_equals_sqrtm_form_full_rank():
    x, y = _feats(40, 12, 1), _feats(40, 12, 2, shift=0.3)
    want = MR.fid_sqrtm(x, y)
    got = float(metrics.fid_from_features(x, y))
    assert abs(got - want) <= 1e-8 * abs(want), (got, want)
    assert abs(MR.fid_svd(x, y) - want) <= 1e-8 * abs(want)
    assert metrics.fid_from_features(x.float(), y.float()).dtype == torch.float64


def test_fid_of_a_set_with_itself_is_zero_in_the_rank_deficient_regime():
    x = _feats(8, 48, 3)                                                  # B < p: the reference's regime (8 items, 3072 features)
    tr = float(((x - x.mean(0)) ** 2).sum() / 7)
    assert abs(float(metrics.fid_from_features(x, x))) <= 1e-9 * tr
    assert abs(float(metrics.fid_from_features(x, x.clone() + 0.0))) <= 1e-9 * tr
    assert torch.isnan(metrics.fid_from_features(x[:1], x[:1]))           # one item: no covariance


def test_perceptual_loss_refuses_what_is_not_built():
    from unet_bssfp_amd import _lib, losses
    net = medicalnet.MedicalNetResNet10()
    with pytest.raises(NotImplementedError):
        losses.PerceptualLoss(net, spatial_dims=2)
    term = losses.PerceptualLoss(net)
    assert list(term.parameters()) == []                                  # the shared network is not the term's to train or save
    x = torch.zeros(1, 1, 8, 8, 8)
    with pytest.raises(NotImplementedError, match="backward"):
        term(x.clone().requires_grad_(), x)
    with pytest.raises(NotImplementedError, match="backward"):
        term(x, x.clone().requires_grad_())
    with pytest.raises(_lib.Mi355Error):                                  # no CPU fallback
        term(x, x)
