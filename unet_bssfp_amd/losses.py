"""Loss terms on the GPU beyond L1 -- the reconstruction slot of ``gan.bSSFPToDWITensorModel``.

The reference's objective sums L1, 1 - SSIM and the MedicalNet Perceptual term (thesis, 03-methods; src/model.py:209
averages the terms of the slot).  ``SSIMLoss`` has the constructor signature of ``monai.losses.SSIMLoss``; MONAI is
absent from this image, so parity with it is UNPINNED, as for ``metrics.SSIMMetric``: the formulas are the ones restated
in oracle/metrics_ref.py, and the tests check value and gradient against that oracle in f64.

``PerceptualLoss`` is the MedicalNet Perceptual term on the frozen ResNet-10 of ``medicalnet.py`` (weights:
``checkpoint.medicalnet_state_dict``; parity with MONAI's ``PerceptualLoss(network_type="medicalnet_resnet10_23datasets")``
unpinned for the same reason).  By default it is the VALUE only, a validation / test quantity that refuses tensors that
require grad.  ``differentiable=True`` adds the gradient with respect to the prediction (csrc/medicalnet_bwd.hip), and
``reference_recon_terms(net)`` is the slot content that makes the reference's objective (src/model.py:201-213):

    model = bSSFPToDWITensorModel("bssfp", extra_recon_terms=reference_recon_terms(net))   # (L1 + 1e3 Perceptual) / 2 * recon_factor
    model = bSSFPToDWITensorModel("bssfp", extra_recon_terms={"SSIM": SSIMLoss(3)})   # recon = (L1 + SSIM) / 2 * recon_factor
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib
from .functional import PerceptualFn, SSIM3dFn
from .medicalnet import MedicalNetResNet10, medicalnet_distances


class SSIMLoss(nn.Module):
    """``1 - SSIM(input, target)`` per batch item, reduced by ``mean`` / ``sum`` / ``none`` (``none``: (B, 1)).

    Differentiable in ``input`` only (csrc/ssim_loss.hip); a ``target`` that requires grad is refused.  Any float dtype and
    any strides: the tensors are made f32 and contiguous by ordinary torch ops, so autograd carries views and dtypes."""

    def __init__(self, spatial_dims: int, data_range: float = 1.0, kernel_type: str = "gaussian", win_size: int = 11,
                 kernel_sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03, reduction: str = "mean"):
        super().__init__()
        if spatial_dims != 3:
            raise NotImplementedError("only the reference's 3-D configuration is built")
        if kernel_type != "gaussian":
            raise NotImplementedError("only the Gaussian window (MONAI's default) is built")
        if not 1 <= win_size <= 15:
            raise ValueError("win_size must be in 1..15")
        if reduction not in ("mean", "sum", "none"):
            raise ValueError(f'Unsupported reduction: {reduction}, available options are ["mean", "sum", "none"].')
        self.spatial_dims, self.data_range, self.kernel_type, self.win_size = spatial_dims, data_range, kernel_type, win_size
        self.kernel_sigma, self.k1, self.k2, self.reduction = kernel_sigma, k1, k2, reduction
        dist = torch.arange(start=(1 - win_size) / 2, end=(1 + win_size) / 2, step=1)
        g = torch.exp(-torch.pow(dist / kernel_sigma, 2) / 2)
        self._window = (g / g.sum()).float().contiguous()             # host side: travels by value

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if not (input.is_cuda and target.is_cuda):
            raise _lib.Mi355Error("SSIMLoss runs on the GPU only (no CPU fallback)")
        if input.shape != target.shape:
            raise ValueError(f"input and target should have same shapes, got {tuple(input.shape)} and {tuple(target.shape)}.")
        if input.dim() != 5:
            raise ValueError(f"input should have 5 dimensions (batch, channel, D, H, W), got {input.dim()}.")
        if min(input.shape[2:]) < self.win_size:
            raise ValueError(f"spatial size {tuple(input.shape[2:])} is smaller than the {self.win_size}-wide window")
        if target.requires_grad:
            raise NotImplementedError("only the gradient with respect to `input` is built; detach `target`")
        c1, c2 = (self.k1 * self.data_range) ** 2, (self.k2 * self.data_range) ** 2
        ssim = SSIM3dFn.apply(input.float().contiguous(), target.detach().float().contiguous(), self._window, c1, c2)
        loss = 1 - ssim
        if self.reduction == "mean":
            return loss.mean()
        if self.reduction == "sum":
            return loss.sum()
        return loss


class PerceptualLoss(nn.Module):
    """The reference's Perceptual distance (MONAI ``MedicalNetPerceptualSimilarity``, ``channel_wise=False``) times ``factor``.

    Prediction and target are each normalised over the whole tensor, every channel runs through the ResNet-10 as its own
    volume, the C outputs are concatenated to (B, 512 C, d, h, w), and with f^ = f / (sqrt(sum_ch f^2) + 1e-10) the value is
    the mean over batch and positions of sum_ch (f^_input - f^_target)^2.  The whole computation stays on the device (no host
    read), so it records into a hipGraph.

    ``differentiable=False`` (the default): the value only; an ``input`` or ``target`` that requires grad raises
    ``NotImplementedError``.  ``differentiable=True``: the same value, bit for bit, with the gradient with respect to
    ``input`` (``functional.PerceptualFn``); a ``target`` that requires grad is refused, as by ``SSIMLoss``."""

    def __init__(self, net: MedicalNetResNet10, spatial_dims: int = 3, differentiable: bool = False, factor: float = 1.0):
        super().__init__()
        if spatial_dims != 3:
            raise NotImplementedError("only the reference's 3-D configuration is built")
        self._net = (net,)                                            # not a submodule: the frozen network is shared, not owned
        self.differentiable, self.factor = bool(differentiable), float(factor)

    @property
    def net(self) -> MedicalNetResNet10:
        return self._net[0]

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if not self.differentiable and (input.requires_grad or target.requires_grad):
            raise NotImplementedError("PerceptualLoss: this instance computes the value only, without the backward pass through "
                                      "the MedicalNet ResNet-10 -- detach both tensors, or pass differentiable=True to train on "
                                      "the term")
        if target.requires_grad:
            raise NotImplementedError("only the gradient with respect to `input` is built; detach `target`")
        if not (input.is_cuda and target.is_cuda):
            raise _lib.Mi355Error("PerceptualLoss runs on the GPU only (no CPU fallback)")
        if input.dim() != 5:
            raise ValueError(f"input should have 5 dimensions (batch, channel, D, H, W), got {input.dim()}.")
        if self.differentiable:
            if input.shape != target.shape:
                raise ValueError(f"input and target should have same shapes, got {tuple(input.shape)} and {tuple(target.shape)}.")
            value = PerceptualFn.apply(input.float().contiguous(), target.detach().float().contiguous(), self.net)
        else:
            value = medicalnet_distances(self.net, input, target)[0].reshape(())
        return value if self.factor == 1.0 else value * self.factor


def reference_recon_terms(net: MedicalNetResNet10, perceptual_factor: float = 1e3):
    """``extra_recon_terms`` of the reference's objective: with it ``recon = (L1 + perceptual_factor * Perceptual) / 2 *
    recon_factor`` (src/model.py:201-213; the default ``recon_divisor`` then counts the two terms)."""
    return {"Perceptual": PerceptualLoss(net, differentiable=True, factor=perceptual_factor)}
