"""CPU reference of the MedicalNet ResNet-10 extractor, the Perceptual distance and FID -- plain torch.nn.

The architecture is restated from MedicalNet's resnet.py as MONAI packages it (``medicalnet_resnet10_23datasets``); MONAI is
absent, so this file, not MONAI, is what the tests hold the kernels to (parity with MONAI unpinned).

``RefResNet10.forward(x, emulate=True)`` rounds through bf16 at exactly the points where csrc/medicalnet.hip stores bf16:
the stem input (after normalisation, which the caller applies), the BN-folded weights, and every activation that is written
to memory -- the stem output, each block's conv1 output, the downsample output and the block output.  conv2 + bias and the
residual sum stay in f32 until the block's ReLU, as in the kernel's epilogue.  Accumulation is f32 either way.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

EPS = 1e-5
BLOCKS = (("layer1", 64, 64, 1, 1), ("layer2", 64, 128, 2, 1), ("layer3", 128, 256, 1, 2), ("layer4", 256, 512, 1, 4))


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(t.dtype)


def fold(conv: nn.Conv3d, bn: nn.BatchNorm3d, dtype=torch.float32):
    """w' = w g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps)"""
    scale = bn.weight.detach().to(dtype) / torch.sqrt(bn.running_var.to(dtype) + bn.eps)
    return conv.weight.detach().to(dtype) * scale.view(-1, 1, 1, 1, 1), bn.bias.detach().to(dtype) - bn.running_mean.to(dtype) * scale


class RefBasicBlock(nn.Module):
    def __init__(self, cin, cout, stride, dilation):
        super().__init__()
        self.conv1 = nn.Conv3d(cin, cout, 3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.bn1 = nn.BatchNorm3d(cout, eps=EPS)
        self.conv2 = nn.Conv3d(cout, cout, 3, stride=1, padding=dilation, dilation=dilation, bias=False)
        self.bn2 = nn.BatchNorm3d(cout, eps=EPS)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv3d(cin, cout, 1, stride=stride, bias=False), nn.BatchNorm3d(cout, eps=EPS))

    def forward(self, x):
        out = F.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return F.relu(out + (x if self.downsample is None else self.downsample(x)))

    def forward_emulated(self, x):
        def conv(c, bn, t):
            w, b = fold(c, bn)
            return F.conv3d(t, bf16_round(w), b, c.stride, c.padding, c.dilation)
        out = bf16_round(F.relu(conv(self.conv1, self.bn1, x)))
        res = x if self.downsample is None else bf16_round(conv(self.downsample[0], self.downsample[1], x))
        return bf16_round(F.relu(conv(self.conv2, self.bn2, out) + res))


class RefResNet10(nn.Module):
    """(N, 1, D, H, W) -> (N, 512, d, h, w): layer4's output, no head.  Always eval."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv3d(1, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm3d(64, eps=EPS)
        for name, cin, cout, stride, dilation in BLOCKS:
            setattr(self, name, nn.Sequential(RefBasicBlock(cin, cout, stride, dilation)))
        self.eval()

    def stem(self, x, emulate=False):
        if emulate:
            w, b = fold(self.conv1, self.bn1)
            x = bf16_round(F.relu(F.conv3d(bf16_round(x), bf16_round(w), b, 2, 3)))
        else:
            x = F.relu(self.bn1(self.conv1(x)))
        return F.max_pool3d(x, 3, 2, 1)                               # padding counts as -inf

    @torch.no_grad()
    def forward(self, x, emulate=False):
        x = self.stem(x, emulate)
        for name, *_ in BLOCKS:
            blk = getattr(self, name)[0]
            x = blk.forward_emulated(x) if emulate else blk(x)
        return x


def random_init(net: nn.Module, seed: int) -> nn.Module:
    """He-scaled convolutions; BN running_var in [0.5, 2], running_mean / weight / bias nonzero, so a wrong fold shows"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Conv3d):
                fan_in = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * math.sqrt(2.0 / fan_in))
            elif isinstance(m, nn.BatchNorm3d):
                n = m.num_features
                m.running_var.copy_(0.5 + 1.5 * torch.rand(n, generator=g))
                m.running_mean.copy_(0.3 * torch.randn(n, generator=g) + 0.1)
                m.weight.copy_(0.75 + 0.5 * torch.rand(n, generator=g))
                m.bias.copy_(0.2 * torch.randn(n, generator=g) + 0.05)
    return net


def normalise(v: torch.Tensor) -> torch.Tensor:
    """over the WHOLE tensor, unbiased std"""
    return (v - v.mean()) / v.std()


@torch.no_grad()
def features(net: RefResNet10, x: torch.Tensor, emulate=False) -> torch.Tensor:
    """(B, C, D, H, W) -> (B, 512 C, d, h, w): whole-tensor normalisation, every channel fed as its own volume, outputs
    concatenated along channels in channel order"""
    x = normalise(x.float())
    return torch.cat([net(x[:, c:c + 1], emulate) for c in range(x.shape[1])], dim=1)


def perceptual(fp: torch.Tensor, ft: torch.Tensor) -> torch.Tensor:
    def unit(f):
        return f / (torch.sqrt((f * f).sum(1, keepdim=True)) + 1e-10)
    return ((unit(fp) - unit(ft)) ** 2).sum(1).mean()


def fid_features(f: torch.Tensor) -> torch.Tensor:
    return f.mean(dim=(2, 3, 4))


def fid_sqrtm(x: torch.Tensor, y: torch.Tensor) -> float:
    """the general form: |mu_x - mu_y|^2 + tr(Sx + Sy - 2 sqrtm(Sx Sy)), sample covariances, f64"""
    from scipy import linalg
    x, y = x.double().numpy(), y.double().numpy()
    mx, my = x.mean(0), y.mean(0)
    sx, sy = np.cov(x, rowvar=False), np.cov(y, rowvar=False)
    root = linalg.sqrtm(sx @ sy)
    if np.iscomplexobj(root):
        root = root.real
    return float(((mx - my) ** 2).sum() + np.trace(sx) + np.trace(sy) - 2 * np.trace(root))


def fid_svd(x: torch.Tensor, y: torch.Tensor) -> float:
    """the B x B form in f64 numpy, independent of the package's torch implementation"""
    x, y = x.double().numpy(), y.double().numpy()
    mx, my = x.mean(0), y.mean(0)
    a, b = (x - mx) / math.sqrt(len(x) - 1), (y - my) / math.sqrt(len(y) - 1)
    sv = np.linalg.svd(a @ b.T, compute_uv=False)
    return float(((mx - my) ** 2).sum() + (a * a).sum() + (b * b).sum() - 2 * sv.sum())
