"""Torch restatement of the ResNet input heads for the tests: ``RefResidualUnit`` is monai.networks.blocks.ResidualUnit(spatial_dims=3,
in_channels, out_channels, strides=1, kernel_size=3, subunits, adn_ordering="NDA", act="RELU", norm, bias=True,
last_conv_only=False) built from torch.nn.Conv3d / BatchNorm3d / InstanceNorm3d / ReLU under MONAI's module names, and
``ref_generator`` puts four of them in front of oracle/unet_ref.py's ``RefBasicUNet``.  MONAI is not installed, so parity with
MONAI itself is unpinned, as for the rest of that oracle; this restatement is what the tests pin.  ``R._qa`` / ``R._qw`` sit where
the HIP bf16 mode stores bf16 (each convolution's output, each norm + act output, the block's sum, packed weights), so
``R.storage_emulation`` works on it.  Test infrastructure only."""
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import unet_ref as R  # noqa: E402

HEAD_CHANNELS = {"dwi-tensor": 6, "pc-bssfp": 24, "bssfp": 24, "t1w": 6}      # doc/thesis/img/architecture.png: one block per modality
HEAD_OUT = 24


class _RefResADN(nn.Module):
    """MONAI ADN, ordering "NDA" without dropout: N (BatchNorm3d | InstanceNorm3d(affine)) then A (ReLU)"""

    def __init__(self, channels, norm):
        super().__init__()
        if norm == "batch":
            self.N = nn.BatchNorm3d(channels, eps=R.NORM_EPS, momentum=R.BN_MOMENTUM)
        else:
            self.N = nn.InstanceNorm3d(channels, eps=R.NORM_EPS, affine=True)
        self.A = nn.ReLU()


class _RefResSubunit(nn.Module):
    def __init__(self, cin, cout, norm):
        super().__init__()
        self.conv = nn.Conv3d(cin, cout, kernel_size=3, stride=1, padding=1, bias=True)
        self.adn = _RefResADN(cout, norm)
        self.last_u = None                      # the ReLU's input of the latest forward (detached): the tests' mask precondition

    def forward(self, x):
        c = self.conv
        u = self.adn.N(R._qa(c._conv_forward(x, R._qw(c.weight), c.bias)))
        self.last_u = u.detach()
        return R._qa(self.adn.A(u))


class RefResidualUnit(nn.Module):
    """state_dict: conv.unit{i}.conv.{weight,bias}, conv.unit{i}.adn.N.{weight,bias[,running_mean,running_var,num_batches_tracked]},
    residual.{weight,bias} when in_channels != out_channels (else an Identity without keys); output conv(x) + residual(x), no
    activation after the sum.  Modules are created in MONAI's order: the subunits, then the residual convolution."""

    def __init__(self, in_channels, out_channels, subunits=3, norm="batch"):
        super().__init__()
        assert norm in ("batch", "instance")
        self.conv = nn.Sequential()
        cin = in_channels
        for i in range(max(1, subunits)):
            self.conv.add_module(f"unit{i:d}", _RefResSubunit(cin, out_channels, norm))
            cin = out_channels
        self.residual = nn.Conv3d(in_channels, out_channels, kernel_size=1) if in_channels != out_channels else nn.Identity()

    def relu_inputs(self):
        return [u.last_u for u in self.conv]

    def forward(self, x):
        r = self.residual
        res = R._qa(F.conv3d(x, R._qw(r.weight), r.bias)) if isinstance(r, nn.Conv3d) else x
        return R._qa(self.conv(x) + res)


class RefResnetGenerator(nn.Module):
    """Generator(modality, head="resnet"): four separate ResidualUnit(3, cin, 24, subunits=3, act="RELU", norm="BATCH") heads and
    the shared BasicUNet(24 -> 6), created in the order of ``blocks``"""

    def __init__(self, input_modality, dropout=R.UNET_DROPOUT, unet_cls=R.RefBasicUNet):
        super().__init__()
        self.input_modality = input_modality
        heads = {m: RefResidualUnit(cin, HEAD_OUT, subunits=3, norm="batch") for m, cin in HEAD_CHANNELS.items()}
        unet = unet_cls(spatial_dims=3, in_channels=HEAD_OUT, out_channels=6, features=R.UNET_FEATURES, dropout=dropout)
        self.blocks = nn.ModuleDict({**heads, "unet": unet})

    def forward(self, x):
        return self.blocks["unet"](self.blocks[self.input_modality](R._qa(x)))


def ref_generator(modality, head="resnet", dropout=R.UNET_DROPOUT, unet_cls=R.RefBasicUNet) -> nn.Module:
    """The oracle's generator with the chosen heads.  ``prelu_ref.to_prelu(ref_generator(...))`` makes the U-Net's activations PReLU
    (it patches ``_RefConvolution`` blocks only: the heads keep their ReLU)."""
    if head == "conv":
        return R.RefGenerator(modality, dropout=dropout, unet_cls=unet_cls)
    assert head == "resnet", head
    return RefResnetGenerator(modality, dropout=dropout, unet_cls=unet_cls)


def mask_margin(ref32: RefResidualUnit, x: torch.Tensor):
    """ReLU is discontinuous: an element-wise gradient check is meaningful only where no correct f32 evaluation can flip a mask.
    Runs ``ref32`` (train mode; its BatchNorm buffers are restored) in f32 and a f64 copy of it on x and returns
    (min |u_f64|, max |u_f32 - u_f64|) over the inputs of all ReLUs; the tests assert min > 8 max."""
    import copy
    state = copy.deepcopy(ref32.state_dict())
    ref64 = copy.deepcopy(ref32).double()
    with torch.no_grad():
        ref32(x)
        ref64(x.double())
    ref32.load_state_dict(state)
    u32, u64 = ref32.relu_inputs(), ref64.relu_inputs()
    return (min(float(u.abs().min()) for u in u64), max(float((a.double() - b).abs().max()) for a, b in zip(u32, u64)))
