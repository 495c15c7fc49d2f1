"""CPU reference of the gradient of the MedicalNet Perceptual term with respect to the prediction -- plain torch autograd.

Three modes of the same computation:
  f64 : the network of tests/medicalnet_ref.py in double precision (conv -> eval BatchNorm modules);
  f32 : the same in single precision;
  emu : ``stem(emulate=True)`` and ``forward_emulated``, which round through bf16 where csrc/medicalnet.hip stores bf16.  Autograd
        through ``.to(bfloat16).to(float32)`` rounds the GRADIENT to bf16 at exactly those points, which is the emulation of the
        bf16 gradient storage of csrc/medicalnet_bwd.hip.
``RefResNet10.forward`` and ``medicalnet_ref.features`` are ``no_grad``, so the feature function here calls ``net.stem`` and the
blocks directly.
"""
import copy

import torch

from medicalnet_ref import BLOCKS, RefResNet10, bf16_round, fold, normalise, perceptual  # noqa: F401  (re-exported for the tests)

MODES = ("f64", "f32", "emu")


def extractor(net: RefResNet10, x: torch.Tensor, emulate: bool) -> torch.Tensor:
    """(N, 1, D, H, W) -> (N, 512, d, h, w) with autograd"""
    x = net.stem(x, emulate)
    for name, *_ in BLOCKS:
        blk = getattr(net, name)[0]
        x = blk.forward_emulated(x) if emulate else blk(x)
    return x


def features(net: RefResNet10, x: torch.Tensor, emulate: bool) -> torch.Tensor:
    """(B, C, D, H, W) -> (B, 512 C, d, h, w): whole-tensor normalisation, every channel its own volume, with autograd"""
    x = normalise(x)
    return torch.cat([extractor(net, x[:, c:c + 1], emulate) for c in range(x.shape[1])], dim=1)


def perceptual_value_and_grad(net: RefResNet10, y_hat: torch.Tensor, y: torch.Tensor, mode: str, factor: float = 1.0):
    """-> (factor * Perceptual(y_hat, y), its gradient with respect to y_hat) in the precision of ``mode``"""
    assert mode in MODES
    dtype = torch.float64 if mode == "f64" else torch.float32
    m = copy.deepcopy(net).to(dtype)
    emulate = mode == "emu"
    a = y_hat.detach().to(dtype).requires_grad_()
    with torch.no_grad():
        ft = features(m, y.detach().to(dtype), emulate)
    value = perceptual(features(m, a, emulate), ft) * factor
    grad, = torch.autograd.grad(value, a)
    return value.detach(), grad


def normalise_backward(g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """closed form of the gradient through ``normalise``: with x^ = (v - mean) / std over the whole tensor (unbiased std) and
    N = v.numel(), dv = (g - sum g / N - x^ sum(g x^) / (N - 1)) / std"""
    n = v.numel()
    std = v.std()
    xh = (v - v.mean()) / std
    return (g - g.sum() / n - xh * (g * xh).sum() / (n - 1)) / std


def tail_backward(fp: torch.Tensor, ft: torch.Tensor, g_out: float = 1.0) -> torch.Tensor:
    """closed form of d perceptual(fp, ft) / d fp * g_out for (B, CH, d, h, w) features, as mnet_tail_bwd_kernel states it:
    n = sqrt(sum_ch f^2), u = f / (n + 1e-10), g_u = 2 (u_p - u_t) g_out / (B vox), g_f = g_u / (n + eps) - f (f . g_u) /
    (n (n + eps)^2); zeros where n == 0"""
    eps = 1e-10
    b, vox = fp.shape[0], fp[0, 0].numel()
    n_p = torch.sqrt((fp * fp).sum(1, keepdim=True))
    n_t = torch.sqrt((ft * ft).sum(1, keepdim=True))
    g_u = 2.0 * (fp / (n_p + eps) - ft / (n_t + eps)) * g_out / (b * vox)
    dot = (fp * g_u).sum(1, keepdim=True)
    safe = torch.where(n_p > 0, n_p, torch.ones_like(n_p))
    g_f = g_u / (n_p + eps) - fp * dot / (safe * (n_p + eps) ** 2)
    return torch.where(n_p > 0, g_f, torch.zeros_like(g_f))
