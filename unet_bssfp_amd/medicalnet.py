"""MedicalNet ResNet-10 feature extractor on the device -- DESIGN.md 8.13.

The frozen network inside the reference's Perceptual term (src/model.py:123-138) and behind its FID metric (:158-163,
235-257): MONAI's ``medicalnet_resnet10_23datasets``.  MONAI is absent from this image, so the definition is restated from
MedicalNet's ``resnet.py`` and parity with MONAI is UNPINNED, as for ``metrics.SSIMMetric``.  The weights are not fetched:
a reference checkpoint carries them under ``recon_criterion.*`` and ``checkpoint.medicalnet_state_dict`` extracts them.

    net = MedicalNetResNet10()
    net.load_state_dict(checkpoint.medicalnet_state_dict("last.ckpt"))
    net = net.to("cuda")
    perceptual = losses.PerceptualLoss(net)(y_hat, y)          # the value: a validation / test quantity
    terms = losses.reference_recon_terms(net)                  # the term to train on: differentiable in the prediction

Parameter and buffer names are the reference's (``conv1.weight``, ``bn1.running_mean``, ``layer2.0.downsample.0.weight``,
...).  The network runs in eval mode only: every BatchNorm is folded into its convolution once, in f32, before the weights
are rounded to bf16 and packed for the kernels of csrc/medicalnet.hip; the packed copy is rebuilt after ``load_state_dict``
and after the module moves.  bf16 operands, f32 accumulation, bf16 NDHWC activations between layers.

The backward exists with respect to the PREDICTION only (csrc/medicalnet_bwd.hip, ``medicalnet_backward``): the network is
frozen and the target a constant, so there are no weight gradients.  ``functional.PerceptualFn`` carries it into autograd.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from . import _lib, ops

# (name, cin, cout, stride, dilation) of the four BasicBlocks; a block has a downsample iff stride != 1 or cin != cout
BLOCKS = (("layer1", 64, 64, 1, 1), ("layer2", 64, 128, 2, 1), ("layer3", 128, 256, 1, 2), ("layer4", 256, 512, 1, 4))
EPS = 1e-5
FEATURES = 512


def fold_bn(weight: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, mean: torch.Tensor, var: torch.Tensor,
            eps: float = EPS) -> Tuple[torch.Tensor, torch.Tensor]:
    """conv (no bias) -> eval BatchNorm as one convolution: w' = w g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps),
    in the dtype of the arguments"""
    scale = gamma / torch.sqrt(var + eps)
    return weight * scale.view(-1, 1, 1, 1, 1), beta - mean * scale


def pack_conv_weight(weight: torch.Tensor) -> torch.Tensor:
    """(cout, cin, k, k, k) f32 -> bf16 [k^3][cin / 16][cout][16], element (tap, q, co, e) = w[co][16 q + e][kd][kh][kw]"""
    co, ci, k = weight.shape[0], weight.shape[1], weight.shape[2]
    w = weight.permute(2, 3, 4, 1, 0).reshape(k ** 3, ci // 16, 16, co)
    return w.permute(0, 1, 3, 2).contiguous().to(torch.bfloat16)


def pack_dgrad_weight(weight: torch.Tensor) -> torch.Tensor:
    """(cout, cin, k, k, k) f32 -> bf16 [k^3][cout / 16][cin][16], element (tap, q, ci, e) = w[16 q + e][ci][kd][kh][kw]: the
    data-gradient kernel contracts over cout.  Same f32 values, rounded once, as ``pack_conv_weight``."""
    co, ci, k = weight.shape[0], weight.shape[1], weight.shape[2]
    w = weight.permute(2, 3, 4, 0, 1).reshape(k ** 3, co // 16, 16, ci)
    return w.permute(0, 1, 3, 2).contiguous().to(torch.bfloat16)


def pack_stem_dgrad_weight(weight: torch.Tensor) -> torch.Tensor:
    """(64, 1, 7, 7, 7) f32 -> bf16 [64][2][8][32], the Toeplitz arrangement of mnet_stem_dgrad_kernel: a cell j of 2 x 2 x 2
    input voxels i = 2 j + p reads dy at o = j - 1 + a (a = 0..3 per axis) through the tap k = p + 5 - 2 a.  Element
    (t, half, cls, e) = w[32 half + e][kd][kh][kw], t = (ad * 4 + ah) * 4 + aw, cls = 4 pd + 2 ph + pw; zero where a k is
    outside 0..6 (343 of the 512 (t, cls) pairs carry a weight)."""
    w = weight.reshape(64, 7, 7, 7)
    axis = [(a, p, p + 5 - 2 * a) for a in range(4) for p in range(2) if 0 <= p + 5 - 2 * a <= 6]
    z = weight.new_zeros((4, 4, 4, 64, 2, 2, 2))
    for ad, pd, kd in axis:
        for ah, ph, kh in axis:
            for aw, pw, kw in axis:
                z[ad, ah, aw, :, pd, ph, pw] = w[:, kd, kh, kw]
    return z.reshape(64, 2, 32, 8).permute(0, 1, 3, 2).contiguous().to(torch.bfloat16)


def pack_stem_weight(weight: torch.Tensor) -> torch.Tensor:
    """(64, 1, 7, 7, 7) f32 -> bf16 [25][64][16]: element (s, co, e) = w[co][kd][kh][kw], (kd, kh) = divmod(2 s + e // 8, 7),
    kw = e % 8; zero for kw == 7 and for the 50th (kd, kh) pair"""
    z = weight.new_zeros((64, 50, 8))
    z[:, :49, :7] = weight.reshape(64, 49, 7)
    return z.reshape(64, 25, 16).permute(1, 0, 2).contiguous().to(torch.bfloat16)


class _Downsample(nn.Sequential):
    def __init__(self, cin: int, cout: int, stride: int):
        super().__init__(nn.Conv3d(cin, cout, 1, stride=stride, bias=False), nn.BatchNorm3d(cout, eps=EPS))


class _BasicBlock(nn.Module):
    """holder of the reference's parameter names; the computation is in ``MedicalNetResNet10._extract``"""

    def __init__(self, cin: int, cout: int, stride: int, dilation: int):
        super().__init__()
        self.conv1 = nn.Conv3d(cin, cout, 3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.bn1 = nn.BatchNorm3d(cout, eps=EPS)
        self.conv2 = nn.Conv3d(cout, cout, 3, stride=1, padding=dilation, dilation=dilation, bias=False)
        self.bn2 = nn.BatchNorm3d(cout, eps=EPS)
        self.downsample = _Downsample(cin, cout, stride) if (stride != 1 or cin != cout) else None
        self.stride, self.dilation, self.cout = stride, dilation, cout


class MedicalNetResNet10(nn.Module):
    """``forward(x)``: (N, 1, D, H, W) on the GPU -> (N, 512, d, h, w) f32, the output of ``layer4`` (1/8 resolution; the
    network has no head).  Frozen, eval mode only.  ``features(x)`` is what the Perceptual term and FID feed on."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv3d(1, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm3d(64, eps=EPS)
        for name, cin, cout, stride, dilation in BLOCKS:
            setattr(self, name, nn.Sequential(_BasicBlock(cin, cout, stride, dilation)))
        self.requires_grad_(False)
        super().train(False)
        self._packed: Optional[Dict[str, torch.Tensor]] = None

    # ------------------------------------------------------------------ frozen, eval only
    def train(self, mode: bool = True):
        return super().train(False)            # the folded BatchNorm IS eval mode; there is no training path

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        self.requires_grad_(False)
        self._packed = None
        return out

    def _apply(self, fn, recurse=True):
        self._packed = None
        return super()._apply(fn, recurse)

    # ------------------------------------------------------------------ folded, packed weights
    @staticmethod
    def _folded(conv: nn.Conv3d, bn: nn.BatchNorm3d) -> Tuple[torch.Tensor, torch.Tensor]:
        return fold_bn(conv.weight.detach().float(), bn.weight.detach().float(), bn.bias.detach().float(),
                       bn.running_mean.float(), bn.running_var.float(), bn.eps)

    def packed(self) -> Dict[str, torch.Tensor]:
        """built once; rebuilt after ``load_state_dict`` / ``.to()``"""
        if self._packed is None:
            p: Dict[str, torch.Tensor] = {}
            w, b = self._folded(self.conv1, self.bn1)
            p["stem.w"], p["stem.b"] = pack_stem_weight(w), b.contiguous()
            p["stem.dw"] = pack_stem_dgrad_weight(w)
            for name, *_ in BLOCKS:
                blk = getattr(self, name)[0]
                pairs = [("conv1", blk.conv1, blk.bn1), ("conv2", blk.conv2, blk.bn2)]
                if blk.downsample is not None:
                    pairs.append(("down", blk.downsample[0], blk.downsample[1]))
                for tag, conv, bn in pairs:
                    w, b = self._folded(conv, bn)
                    p[f"{name}.{tag}.w"], p[f"{name}.{tag}.b"] = pack_conv_weight(w), b.contiguous()
                    p[f"{name}.{tag}.dw"] = pack_dgrad_weight(w)
            p["identity"] = torch.tensor([0.0, 1.0], dtype=torch.float32, device=self.conv1.weight.device)
            self._packed = p
        return self._packed

    # ------------------------------------------------------------------ the network
    def _extract(self, vols: torch.Tensor, mean_std: torch.Tensor, keep: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
        """f32 (S, D, H, W) volumes, normalised by ``mean_std`` while they are staged -> bf16 (S, d, h, w, 512).  ``keep``: a dict
        that receives what ``medicalnet_backward`` reads -- tensors the forward writes anyway, kept instead of dropped."""
        if not vols.is_cuda or not self.conv1.weight.is_cuda:
            raise _lib.Mi355Error("MedicalNetResNet10 runs on the GPU only (no CPU fallback)")
        p = self.packed()
        stem = ops.medicalnet_stem(vols, mean_std, p["stem.w"], p["stem.b"])
        a = ops.medicalnet_maxpool(stem)
        if keep is not None:
            keep.update(mean_std=mean_std, stem=stem, pool=a)
        for name, _cin, cout, stride, dilation in BLOCKS:
            t = ops.medicalnet_conv(a, p[f"{name}.conv1.w"], p[f"{name}.conv1.b"], cout, 3, stride, dilation)
            if f"{name}.down.w" in p:
                a = ops.medicalnet_conv(a, p[f"{name}.down.w"], p[f"{name}.down.b"], cout, 1, stride, 1, relu=False)
            a = ops.medicalnet_conv(t, p[f"{name}.conv2.w"], p[f"{name}.conv2.b"], cout, 3, 1, dilation, residual=a)
            if keep is not None:
                keep[f"{name}.t"], keep[f"{name}.out"] = t, a
        return a

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 5 or x.shape[1] != 1:
            raise ValueError(f"expected (N, 1, D, H, W), got {tuple(x.shape)}")
        vols = x.detach().float().contiguous().view(x.shape[0], *x.shape[2:])
        return self._extract(vols, self.packed()["identity"]).permute(0, 4, 1, 2, 3).float()

    @torch.no_grad()
    def features(self, x: torch.Tensor, keep: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
        """(B, C, D, H, W) -> bf16 (B * C, d, h, w, 512): the tensor is normalised as a whole, (v - v.mean()) / v.std() with
        the unbiased std (mean and std stay on the device), and every channel is fed as its own one-channel volume; sample
        b * C + c holds channels [512 c, 512 c + 512) of the reference's concatenated features of item b."""
        if x.dim() != 5:
            raise ValueError(f"expected (B, C, D, H, W), got {tuple(x.shape)}")
        x = x.detach().float().contiguous()
        return self._extract(x.view(-1, *x.shape[2:]), ops.medicalnet_moments(x), keep)


def medicalnet_distances(net: MedicalNetResNet10, y_hat: torch.Tensor, y: torch.Tensor):
    """-> (perceptual value f32[1], FID features of y_hat, of y: f32 (B, 512 C)) from one run of the extractor per tensor and
    one tail pass.  No host read."""
    if y_hat.shape != y.shape:
        raise ValueError(f"input and target should have same shapes, got {tuple(y_hat.shape)} and {tuple(y.shape)}.")
    b, c = y_hat.shape[0], y_hat.shape[1]
    value, _item_sum, mp, mt = ops.medicalnet_tail(net.features(y_hat), net.features(y), b, c)
    return value, mp, mt


@torch.no_grad()
def medicalnet_backward(net: MedicalNetResNet10, x: torch.Tensor, kept: Dict[str, torch.Tensor], g_feat: torch.Tensor) -> torch.Tensor:
    """g_feat: bf16 gradient of layer4's output, already times its ReLU mask (ops.medicalnet_tail_bwd); x: the contiguous f32
    (B, C, D, H, W) prediction of the forward; kept: what ``features(x, keep=...)`` left -> d / dx, f32 like x.  Per block, with
    g the masked gradient of its output: g_t = dgrad_conv2(g) [t > 0]; r = dgrad_down(g) or g; g_in = (dgrad_conv1(g_t) + r),
    masked by the previous block's output (layer1's input is the pool output: no mask).  No host read."""
    p = net.packed()
    g = g_feat
    inputs = (kept["pool"],) + tuple(kept[f"{name}.out"] for name, *_ in BLOCKS[:-1])
    for k in range(len(BLOCKS) - 1, -1, -1):
        name, _cin, _cout, stride, dilation = BLOCKS[k]
        a_in = inputs[k]
        g_t = ops.medicalnet_dgrad(g, p[f"{name}.conv2.dw"], kept[f"{name}.t"].shape, 3, 1, dilation, mask=kept[f"{name}.t"])
        r = ops.medicalnet_dgrad(g, p[f"{name}.down.dw"], a_in.shape, 1, stride, 1) if f"{name}.down.dw" in p else g
        g = ops.medicalnet_dgrad(g_t, p[f"{name}.conv1.dw"], a_in.shape, 3, stride, dilation, add=r, mask=a_in if k > 0 else None)
    g_stem = ops.medicalnet_maxpool_bwd(kept["stem"], g)
    vols = x.view(-1, *x.shape[2:])
    g_hat, part = ops.medicalnet_stem_dgrad(g_stem, p["stem.dw"], vols, kept["mean_std"])
    return ops.medicalnet_norm_bwd(g_hat, vols, kept["mean_std"], part).view(x.shape)
