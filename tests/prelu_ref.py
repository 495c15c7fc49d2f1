"""Torch restatement of a PReLU U-Net for the tests: oracle/unet_ref.py's modules with every ``_RefConvolution.adn`` replaced by a
subclass that ends in ``F.prelu`` (MONAI 1.3 ADN, ordering "NDA", act "prelu": N, then D, then A = torch.nn.PReLU -- parity with
MONAI itself is unpinned, as for the rest of that oracle; ``torch.nn.PReLU`` is what these tests pin), and the closed form of
the slope gradient the kernels implement.  Test infrastructure only."""
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import unet_ref as R  # noqa: E402


class RefADNPReLU(R._RefADN):
    """InstanceNorm(affine) -> Dropout -> PReLU(one slope).  ``A`` is registered after ``N``: state-dict key ``adn.A.weight``.
    ``record = True``: the backward pass leaves ``s_abs`` = sum |da * u| over u <= 0, the scale of the slope gradient's terms."""

    def __init__(self, channels, dims, dropout, init=0.25):
        super().__init__(channels, dims, dropout)
        self.A = nn.PReLU(num_parameters=1, init=init)
        self.record = False
        self.s_abs = None

    def forward(self, z, drop_mask=None):
        u = F.instance_norm(z, None, None, self.N.weight, self.N.bias, True, 0.0, R.NORM_EPS)
        if drop_mask is not None:
            u = u * drop_mask
        elif self.training and self.p > 0.0:
            u = F.dropout(u, self.p, True)
        a = F.prelu(u, self.A.weight)
        if self.record and a.requires_grad:
            ud = u.detach()

            def hook(g):
                self.s_abs = float((g * ud)[ud <= 0].abs().sum())
            a.register_hook(hook)
        return a


def to_prelu(net: nn.Module, init=0.25) -> nn.Module:
    """Replace, in place, the ADN of every ``_RefConvolution`` under ``net``; the norm's parameters are kept.  Draws no random
    numbers, so a network built and patched after ``torch.manual_seed(s)`` holds the default initialisation of seed s."""
    for m in net.modules():
        if isinstance(m, R._RefConvolution):
            old = m.adn
            new = RefADNPReLU(old.N.num_features, 3 if isinstance(old.N, nn.InstanceNorm3d) else 2, old.p, init)
            new.N = old.N
            m.adn = new
    return net


def ref_basic_unet(*args, init=0.25, **kw) -> nn.Module:
    return to_prelu(R.RefBasicUNet(*args, **kw), init)


def ref_generator(modality, dropout=R.UNET_DROPOUT, init=0.25) -> nn.Module:
    return R.RefGenerator(modality, dropout=dropout, unet_cls=lambda **kw: ref_basic_unet(init=init, **kw))


def slopes(net: nn.Module):
    """[(name, parameter)] of every PReLU slope, in parameter order"""
    return [(n, p) for n, p in net.named_parameters() if n.endswith(".A.weight")]


def set_distinct_slopes(net: nn.Module):
    """18 distinct slopes, 0.02 ... 0.70 in steps of 0.04 (in parameter order)"""
    with torch.no_grad():
        for i, (_, p) in enumerate(slopes(net)):
            p.fill_(0.02 + 0.04 * i)


def network_reference(make_ref, x, y):
    """The patched oracle on one input, loss mean |y_hat - y|, in f32 and in f64 from the same f32 parameters (``make_ref()`` -> a
    fresh patched network; its slopes are set to distinct values here).  Slope gradients are heavily cancelling sums, so their
    error is measured in units of S_abs = sum |da * u| over u <= 0 (from a hook in the f64 run):
    e_cpu  = the largest |g32 - g64| / S_abs over the slopes -- what a correct f32 evaluation misses f64 by;
    margin = the smallest |g64| / S_abs -- a bound of 4 e_cpu S_abs tells a gradient from zero only when 4 e_cpu < margin.
    -> dict(ref, y, y_eval, grads {name: f32 gradient}, g64 / s_abs {slope name: float}, e_cpu, margin)"""
    ref = make_ref().train()
    set_distinct_slopes(ref)
    ref64 = make_ref().double().train()
    ref64.load_state_dict({k: v.double() for k, v in ref.state_dict().items()})
    for m in ref64.modules():
        if isinstance(m, RefADNPReLU):
            m.record = True
    y32 = ref(x)
    (y32 - y).abs().mean().backward()
    with torch.no_grad():
        y_eval = ref.eval()(x)
    ref.train()
    (ref64(x.double()) - y.double()).abs().mean().backward()
    mods = dict(ref64.named_modules())
    g32 = {n: p.grad.clone() for n, p in ref.named_parameters() if p.grad is not None}
    g64 = {n: float(p.grad) for n, p in slopes(ref64)}
    s_abs = {n: mods[n[:-len(".weight")].rsplit(".", 1)[0]].s_abs for n in g64}
    e_cpu = max(abs(float(g32[n]) - g64[n]) / s_abs[n] for n in g64)
    margin = min(abs(g64[n]) / s_abs[n] for n in g64)
    return dict(ref=ref, y=y32.detach(), y_eval=y_eval, grads=g32, g64=g64, s_abs=s_abs, e_cpu=e_cpu, margin=margin)


def adn_prelu(z, gamma, beta, alpha, mask=None, eps=R.NORM_EPS):
    """a = PReLU(u), u = mask * InstanceNorm(z) (mask: kept elements 1 / (1 - p), dropped 0; None: no dropout) -> (a, u)"""
    u = F.instance_norm(z, None, None, gamma, beta, True, 0.0, eps)
    if mask is not None:
        u = u * mask
    return torch.where(u > 0, u, alpha * u), u


def dalpha_closed_form(u, da):
    """d alpha = sum over u <= 0 of da * u (dropped elements have u = 0 and add nothing)"""
    return (da * u)[u <= 0].sum()
