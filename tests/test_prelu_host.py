"""BasicUNet's ``act`` argument on the host: what constructs, what raises, the state-dict keys of a PReLU network against the
patched torch reference (tests/prelu_ref.py), and that reference's slope gradient against torch autograd."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import prelu_ref as PR  # noqa: E402
from oracle import unet_ref as R  # noqa: E402


def test_constructor_accepts_monai_act_choices():
    from unet_bssfp_amd import BasicUNet
    net = BasicUNet(act="PReLU")
    cfg = net.conv_0.conv_0.cfg
    assert cfg.act == "prelu" and net.conv_0.conv_0.adn.A.weight.item() == 0.25
    net = BasicUNet(act=("prelu", {"init": 0.1}))
    w = net.upcat_1.convs.conv_1.adn.A.weight
    assert isinstance(w, torch.nn.Parameter) and w.shape == (1,) and w.dtype == torch.float32
    assert abs(w.item() - 0.1) < 1e-7
    assert BasicUNet(act="relu").down_2.convs.conv_1.cfg.slope == 0.0
    assert BasicUNet(act="ReLU").down_2.convs.conv_1.cfg.act == "leakyrelu"
    assert BasicUNet(act=("LeakyReLU", {"negative_slope": 0.3})).conv_0.conv_1.cfg.slope == 0.3
    assert BasicUNet(act=("leakyrelu", {"inplace": True})).conv_0.conv_1.cfg.slope == 0.01        # torch's default
    assert BasicUNet().conv_0.conv_1.cfg.slope == 0.1                                           # MONAI BasicUNet's default
    for bad in (("prelu", {"num_parameters": 32}), "gelu"):
        with pytest.raises(NotImplementedError):
            BasicUNet(act=bad)
    with pytest.raises(NotImplementedError):
        BasicUNet(norm="batch")                                 # norm, upsample and bias stay as they are
    with pytest.raises(NotImplementedError):
        BasicUNet(act="PReLU", upsample="nontrainable")


@pytest.mark.parametrize("dims", [3, 2])
def test_prelu_state_dict_equals_the_patched_reference(dims):
    from unet_bssfp_amd import BasicUNet
    torch.manual_seed(3)
    net = BasicUNet(spatial_dims=dims, in_channels=3, out_channels=6, act=("PReLU", {"init": 0.2}))
    torch.manual_seed(3)
    ref = PR.ref_basic_unet(spatial_dims=dims, in_channels=3, out_channels=6, init=0.2)
    sd, sr = net.state_dict(), ref.state_dict()
    assert list(sd.keys()) == list(sr.keys())                   # key set AND order (optimiser-state indices depend on it)
    assert [n for n, _ in net.named_parameters()] == [n for n, _ in ref.named_parameters()]
    for k in sd:
        assert sd[k].shape == sr[k].shape and sd[k].dtype == sr[k].dtype, k
        assert torch.equal(sd[k], sr[k]), k                     # nn.PReLU draws no random numbers: same default initialisation
    names = [n for n, _ in net.conv_0.conv_0.named_parameters()]
    assert names == ["conv.weight", "conv.bias", "adn.N.weight", "adn.N.bias", "adn.A.weight"]
    assert len(PR.slopes(net)) == 18


@pytest.mark.parametrize("act", [None, "relu", ("LeakyReLU", {"negative_slope": 0.3})])
def test_leakyrelu_and_relu_keep_todays_keys(act):
    from unet_bssfp_amd import BasicUNet
    torch.manual_seed(3)
    net = BasicUNet(in_channels=3, out_channels=6, **({} if act is None else {"act": act}))
    torch.manual_seed(3)
    ref = R.RefBasicUNet(in_channels=3, out_channels=6)
    sd, sr = net.state_dict(), ref.state_dict()
    assert list(sd.keys()) == list(sr.keys())
    for k in sd:
        assert torch.equal(sd[k], sr[k]), k


def test_generator_passes_act_through():
    from unet_bssfp_amd import Generator
    from unet_bssfp_amd.checkpoint import HPARAM_KEYS
    torch.manual_seed(1)
    g = Generator("bssfp", 0.05, (32, 64, 128, 256, 512, 32), "PReLU")         # act is the last argument
    torch.manual_seed(1)
    ref = PR.ref_generator("bssfp")
    assert list(g.state_dict().keys()) == list(ref.state_dict().keys())
    assert not any(".A." in k for k in g.state_dict() if "unet" not in k)       # the modality heads keep LeakyReLU(0.2)
    torch.manual_seed(1)
    plain = Generator("bssfp")
    assert list(plain.state_dict().keys()) == list(R.RefGenerator("bssfp").state_dict().keys())
    assert "act" not in HPARAM_KEYS


def test_e4m3_mode_refuses_a_prelu_network():
    import unet_bssfp_amd as M
    with pytest.raises(NotImplementedError):
        M.set_compute_dtype(M.BasicUNet(act="PReLU"), "fp8")
    M.set_compute_dtype(M.BasicUNet(act="PReLU"), "bf16")
    M.set_compute_dtype(M.BasicUNet(), "fp8")


@pytest.mark.parametrize("alpha", [0.25, -0.4, 0.0, 1.0])
def test_reference_slope_gradient_equals_autograd_in_f64(alpha):
    """The closed form the kernels implement -- d alpha = sum over u <= 0 of da * u, u the dropped-out, normalised value --
    against torch autograd through F.prelu, with an explicit dropout mask, in f64; the activation and du likewise."""
    g = torch.Generator().manual_seed(5)
    n, c, sp, p = 2, 5, (3, 4, 5), 0.3
    z = torch.randn(n, c, *sp, generator=g, dtype=torch.float64, requires_grad=True)
    gamma = torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    beta = torch.rand(c, generator=g, dtype=torch.float64) - 0.5
    mask = (torch.rand(n, c, *sp, generator=g) >= p).double() / (1 - p)
    da = torch.rand(n, c, *sp, generator=g, dtype=torch.float64) - 0.3
    al = torch.tensor([alpha], dtype=torch.float64, requires_grad=True)
    u = F.instance_norm(z, None, None, gamma, beta, True, 0.0, R.NORM_EPS) * mask
    u.retain_grad()
    a = F.prelu(u, al)
    a.backward(da)
    a2, u2 = PR.adn_prelu(z.detach(), gamma, beta, alpha, mask)
    torch.testing.assert_close(a2, a.detach(), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(PR.dalpha_closed_form(u2, da).reshape(1), al.grad, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(torch.where(u2 > 0, da, alpha * da), u.grad, rtol=1e-13, atol=1e-13)
    assert float(((mask == 0) & (u2 != 0)).sum()) == 0          # dropped elements: u = 0, no contribution


def test_patched_reference_trains_its_slopes():
    torch.manual_seed(2)
    ref = PR.ref_basic_unet(spatial_dims=2, in_channels=1, out_channels=2, features=(4, 4, 8, 8, 16, 4)).train()
    x = torch.rand(1, 1, 32, 32)
    ref(x).abs().mean().backward()
    for n, p in PR.slopes(ref):
        assert p.grad is not None and p.grad.shape == (1,) and float(p.grad.abs()) > 0, n
