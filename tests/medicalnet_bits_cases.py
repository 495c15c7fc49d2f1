"""The cases of the MedicalNet bit pin: tools/gen_golden_medicalnet_bits.py records them, tests/test_medicalnet_bits_gpu.py
replays them.  Every kernel of csrc/medicalnet.hip and csrc/medicalnet_bwd.hip runs at the smallest shape where its edges are
live (partial tiles, partial workgroups, both stride-2 border classes, empty parity classes, the scalar tail of a vector loop),
and every output tensor is reduced to the SHA-256 of its bytes plus its f64 sum and absolute maximum, which say roughly where to
look when a hash moves.

Inputs come from INTEGER arithmetic on the element index -- a multiplicative hash, 16 bits of it mapped to [-1, 1) by exact
operations, then one IEEE multiply-add and, for activations, one rounding to bf16 -- so they are the same on any machine and any
torch build; no RNG.  Every device call runs on poisoned fresh memory (tests/alloc_poison.py).
"""
import hashlib
import math
from collections import OrderedDict

import torch

from alloc_poison import poisoned

DEV = "cuda:0"
# cin, cout, ks, stride, dilation, residual + ReLU (conv) / add + mask (dgrad): the single-layer lists of
# tests/test_medicalnet_gpu.py (CONVS and both 1x1x1 strides) and tests/test_medicalnet_grad_gpu.py (DGRAD)
LAYERS = [(64, 128, 3, 1, 1, False), (64, 128, 3, 2, 1, False), (64, 128, 3, 1, 2, False), (64, 128, 3, 1, 4, False),
          (256, 512, 3, 1, 4, True), (64, 128, 1, 1, 1, False), (64, 128, 1, 2, 1, False)]
EXTENT = (5, 6, 9)          # N = 2: 540 rows = 3 workgroups, the last partial; odd, even, odd: both stride-2 border classes
STEM_VOLUME = (9, 10, 37)   # -> 5 x 5 x 19: partial tiles in d and h, two w tiles, the second partial


def values(shape, salt, scale=1.0, shift=0.0):
    """f32 tensor (CPU) of ``shape``: element i is shift + scale * u_i, u_i in [-1, 1) from 16 bits of a two-round multiplicative hash"""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.int64)
    h = ((i + 1 + 7919 * salt) * 2654435761) % (1 << 32)
    h = ((h ^ (h >> 15)) * 1540483477) % (1 << 32)                    # a second round: the first alone is a sawtooth in i
    h = (h ^ (h >> 13)) >> 8 & 0xFFFF
    return ((h.to(torch.float32) - 32768.0) / 32768.0 * scale + shift).reshape(shape)


def act(shape, salt, scale=1.0, shift=0.0):
    """a bf16 activation on the device"""
    return values(shape, salt, scale, shift).to(torch.bfloat16).to(DEV)


def conv_weight(cout, cin, ks, salt):
    """(cout, cin, ks, ks, ks) f32, variance 2 / fan_in"""
    return values((cout, cin, ks, ks, ks), salt, math.sqrt(6.0 / (ks ** 3 * cin)))


def out_extent(n, stride):
    return (n - 1) // stride + 1


def integer_state_dict(net):
    """a state dict for MedicalNetResNet10 with the statistics of medicalnet_ref.random_init, from ``values`` instead of an RNG"""
    sd = OrderedDict()
    for k, (name, t) in enumerate(net.state_dict().items()):
        if name.endswith("num_batches_tracked"):
            sd[name] = t.clone()
        elif t.dim() == 5:
            sd[name] = conv_weight(t.shape[0], t.shape[1], t.shape[2], 1000 + k)
        elif name.endswith("running_var"):
            sd[name] = values(t.shape, 1000 + k, 0.75, 1.25)
        elif name.endswith("running_mean"):
            sd[name] = values(t.shape, 1000 + k, 0.3, 0.1)
        elif name.endswith("weight"):
            sd[name] = values(t.shape, 1000 + k, 0.25, 1.0)
        else:
            sd[name] = values(t.shape, 1000 + k, 0.2, 0.05)
    return sd


def digest(t):
    """(sha256 of the bytes, f64 sum, absolute maximum) of a tensor"""
    c = t.detach().cpu().contiguous()
    raw = c.view(-1).view(torch.uint8).numpy().tobytes()
    d = c.double()
    return hashlib.sha256(raw).hexdigest(), float(d.sum()), float(d.abs().max())


class Cases:
    """``run(name)`` -> OrderedDict output name -> tensor.  kind: the poison of every device call.  What several cases share
    (the stem's inputs and output) is computed once per instance."""

    def __init__(self, kind="nan"):
        self.kind = kind
        self._shared = {}

    def call(self, fn, *a, **k):
        with poisoned(self.kind):
            out = fn(*a, **k)
            torch.cuda.synchronize()
        return out

    def shared(self, key, make):
        if key not in self._shared:
            self._shared[key] = make()
        return self._shared[key]

    # ---------------------------------------------------------------------------------------- forward
    def moments(self):
        """n = 8195 = 4 * 2048 + 3: the float4 body and the scalar tail from an aligned pointer, the scalar path from one
        offset by one float"""
        from unet_bssfp_amd import ops
        buf = values((8196,), 1, 0.5, 3.0).to(DEV)
        assert buf.data_ptr() % 16 == 0
        return OrderedDict(aligned=self.call(ops.medicalnet_moments, buf[:8195]), offset=self.call(ops.medicalnet_moments, buf[1:]))

    def _stem_inputs(self):
        from unet_bssfp_amd import ops
        from unet_bssfp_amd.medicalnet import pack_stem_dgrad_weight, pack_stem_weight

        def make():
            vols = values((2, *STEM_VOLUME), 2, 0.5, 3.0).to(DEV)
            w = conv_weight(64, 1, 7, 3)
            return dict(vols=vols, ms=self.call(ops.medicalnet_moments, vols), w=pack_stem_weight(w).to(DEV),
                        dw=pack_stem_dgrad_weight(w).to(DEV), b=values((64,), 4, 0.3).to(DEV))
        return self.shared("stem_inputs", make)

    def _stem_out(self):
        from unet_bssfp_amd import ops
        s = self._stem_inputs()
        return self.shared("stem_out", lambda: self.call(ops.medicalnet_stem, s["vols"], s["ms"], s["w"], s["b"]))

    def stem(self):
        y = self._stem_out()
        assert tuple(y.shape) == (2, 5, 5, 19, 64)
        return OrderedDict(mean_std=self._stem_inputs()["ms"], y=y)

    def maxpool(self):
        from unet_bssfp_amd import ops
        y = self.call(ops.medicalnet_maxpool, self._stem_out())
        assert tuple(y.shape) == (2, 3, 3, 10, 64)
        return OrderedDict(y=y)

    def conv(self):
        from unet_bssfp_amd import ops
        from unet_bssfp_amd.medicalnet import pack_conv_weight
        out = OrderedDict()
        for k, (cin, cout, ks, stride, dil, res_relu) in enumerate(LAYERS):
            x = act((2, *EXTENT, cin), 10 + k)
            wp = pack_conv_weight(conv_weight(cout, cin, ks, 20 + k)).to(DEV)
            b = values((cout,), 30 + k, 0.3).to(DEV)
            res = act((2, *(out_extent(n, stride) for n in EXTENT), cout), 40 + k) if res_relu else None
            out[f"c{cin}_{cout}_k{ks}_s{stride}_d{dil}" + ("_res" if res_relu else "")] = self.call(
                ops.medicalnet_conv, x, wp, b, cout, ks, stride, dil, residual=res, relu=res_relu)
        return out

    def tail(self):
        """items = 2, c = 2, features 3 x 3 x 2: 18 voxels = two chunks of 16, the second partial; features >= 0 as behind a ReLU"""
        from unet_bssfp_amd import ops
        fp, ft = (act((4, 3, 3, 2, 512), s).clamp_(min=0) for s in (50, 51))
        value, item_sum, mp, mt = self.call(ops.medicalnet_tail, fp, ft, 2, 2)
        g_out = torch.tensor([370.0], device=DEV)
        return OrderedDict(value=value, item_sum=item_sum, mean_pred=mp, mean_target=mt,
                           bwd_g_feat=self.call(ops.medicalnet_tail_bwd, fp, ft, g_out, 2, 2))

    # ---------------------------------------------------------------------------------------- backward
    def dgrad(self):
        """the DGRAD list at 5 x 6 x 9, and the 1 x 1 x 1 stride-2 layer at 1 x 2 x 3, which leaves parity classes empty"""
        from unet_bssfp_amd import ops
        from unet_bssfp_amd.medicalnet import pack_dgrad_weight
        out = OrderedDict()
        for k, (cin, cout, ks, stride, dil, add_mask) in enumerate(LAYERS + [(64, 128, 1, 2, 1, False)]):
            ext = EXTENT if k < len(LAYERS) else (1, 2, 3)
            dy = act((2, *(out_extent(n, stride) for n in ext), cout), 60 + k)
            wp = pack_dgrad_weight(conv_weight(cout, cin, ks, 70 + k)).to(DEV)
            add, mask = (act((2, *ext, cin), 80 + k), act((2, *ext, cin), 90 + k)) if add_mask else (None, None)
            out[f"c{cin}_{cout}_k{ks}_s{stride}_d{dil}_{'x'.join(map(str, ext))}" + ("_add_mask" if add_mask else "")] = self.call(
                ops.medicalnet_dgrad, dy, wp, (2, *ext, cin), ks, stride, dil, add=add, mask=mask)
        return out

    def maxpool_bwd(self):
        """on the stem output, with an exact tie planted: three voxels of window (1, 1, 1) -- the first of them also the only
        large voxel of window (0, 0, 0) -- hold the same value 8 in every channel, above everything the stem produced"""
        from unet_bssfp_amd import ops
        x = self._stem_out().clone()
        assert float(x.float().max()) < 8.0
        for d, h, w in ((1, 1, 1), (2, 2, 2), (1, 3, 2)):
            x[:, d, h, w, :] = 8.0
        dy = act((2, 3, 3, 10, 64), 100)
        return OrderedDict(dx=self.call(ops.medicalnet_maxpool_bwd, x, dy))

    def stem_dgrad(self):
        """stem data gradient and normalisation backward on the stem case's volumes; dy is zero in about half of its elements,
        as behind a ReLU mask"""
        from unet_bssfp_amd import ops
        s = self._stem_inputs()
        dy = act((2, 5, 5, 19, 64), 110).clamp_(min=0)
        g, part = self.call(ops.medicalnet_stem_dgrad, dy, s["dw"], s["vols"], s["ms"])
        return OrderedDict(g=g, part=part, dv=self.call(ops.medicalnet_norm_bwd, g, s["vols"], s["ms"], part))

    # ---------------------------------------------------------------------------------------- the whole term
    def whole(self):
        """PerceptualFn value and gradient at (B, C) = (2, 2), 16^3, factor 1e3; the packed weights are outputs too, so a
        moved hash of the term can be told from moved weights"""
        from unet_bssfp_amd import losses
        from unet_bssfp_amd.medicalnet import MedicalNetResNet10
        net = MedicalNetResNet10()
        net.load_state_dict(integer_state_dict(net), strict=True)
        net = net.to(DEV)
        y = values((2, 2, 16, 16, 16), 120, 1.0, 0.25).to(DEV)
        y_hat = (y + values(y.shape, 121, 0.5).to(DEV)).requires_grad_()
        term = losses.PerceptualLoss(net, differentiable=True, factor=1e3)

        def both():
            value = term(y_hat, y)
            grad, = torch.autograd.grad(value, y_hat)
            return value.detach(), grad
        value, grad = self.call(both)
        out = OrderedDict(value=value, grad=grad)
        for name, t in net.packed().items():
            out["packed." + name] = t
        return out


CASES = ("moments", "stem", "maxpool", "conv", "tail", "dgrad", "maxpool_bwd", "stem_dgrad", "whole")


def run(name, cases):
    """[(full output name, (sha256, sum, absmax))] of case ``name``"""
    return [(f"{name}/{k}", digest(t)) for k, t in getattr(cases, name)().items()]
