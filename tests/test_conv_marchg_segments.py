"""conv_marchg_kernel on every d-segment length it has a code path for (GPU).

The kernel runs only the live kd blocks of an input plane, and which blocks are live depends on the plane's place in the
workgroup's d-segment [d0, d1): segments of one plane (masks 001, 010, 100), of two (001, 011, 110, 100) and of three or more
(lead-in, 111 planes -- (L - 2) % 3 of them in front of the loop of triples --, lead-out) are separate instruction sequences,
each with its own counted waits.  A miscounted wait gives wrong sums, so every sequence is compared here, bf16, against torch's
f32 conv3d on the bf16-rounded operands: forward output, fused statistics and (through ConvFn's backward) the data gradient,
with the tolerances of the k3_mg_* cases of test_gpu_ops.py (whose helpers are used).

Every case asserts the kernel (plan id 32141 = ROWS 4, 32121 = ROWS 2) and the planner's segment length, so a planner
change that moves a shape off its path fails here instead of silently testing another one.  Shapes: the real 32^3 layers for
L = 1 and the real 64^3 layer for L = 4; the others are the smallest found by scanning the planner on
the host (N <= 2, D <= 32, 24 x 40 rows: partial 16 x 32 / 8 x 32 footprints in h and w) for L = 2, 3, 4, 5, a ragged last
segment, two sources and ROWS = 2.  No ROWS = 2 plan with L >= 3 exists for D <= 32 in that scan.  L = 3, 4, 5 are the three
remainders (L - 2) % 3 = 1, 2, 0; L = 5 alone runs the loop of triples at these sizes.  The data gradient of a case is a
launch of its own (channels swapped): the 64 -> 128 case's gradient is the 128 -> 64 layer on ROWS = 2 at L = 1.
"""
import ctypes as C
import os
import sys
import zlib

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_ops import DEV, _conv_layer, _ops, close, close_f32_sum, from_act, q, to_act  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [
    # name, N, Cin(s), Cout, spatial, plan id, segment length, planes of the last segment
    ("L1_64to128", 1, (64,), 128, (32, 32, 32), 32141, 1, 1),          # down_2 / upcat_3 at 32^3
    ("L1_128to128", 1, (128,), 128, (32, 32, 32), 32141, 1, 1),
    ("L2_n2_cout192", 2, (64,), 192, (16, 32, 32), 32141, 2, 2),
    ("L2_ragged_2src_partial", 2, (32, 32), 192, (7, 24, 40), 32141, 2, 1),
    ("L3_partial", 1, (64,), 192, (24, 24, 40), 32141, 3, 3),
    ("L3_ragged_2src_partial", 1, (32, 32), 192, (22, 24, 40), 32141, 3, 1),
    ("L4_64to64", 1, (64,), 64, (64, 64, 64), 32141, 4, 4),            # the 64^3 level
    ("L4_ragged_2src_partial", 2, (32, 32), 128, (25, 24, 40), 32141, 4, 1),
    ("L5_ragged_partial", 2, (64,), 192, (22, 24, 40), 32141, 5, 2),
    ("rows2_L2_ragged", 1, (64,), 64, (11, 64, 64), 32121, 2, 1),
    ("rows2_L1_128to64", 1, (128,), 64, (32, 32, 32), 32121, 1, 1),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_marchg_segment_paths(hip, case):
    from unet_bssfp_amd import functional as Fn
    name, n, cins, cout, sp, want_plan, want_len, want_last = case
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 1000)
    layer = _conv_layer(cins, cout, 3, 1, 1, 1)
    with torch.no_grad():
        layer.weight.copy_(q(layer.weight, dtype))
    xs = [q(torch.rand(n, c, *sp, generator=g) - 0.3, dtype) for c in cins]
    w_cpu = layer.weight.detach().clone()
    b_cpu = layer.bias.detach().clone()
    xcat = torch.cat(xs, 1).requires_grad_(True)
    z_ref = F.conv3d(xcat, w_cpu, b_cpu, 1, 1)
    gz = q(torch.rand(z_ref.shape, generator=g) - 0.5, dtype)
    (dx_ref,) = torch.autograd.grad(z_ref, xcat, gz)

    layer = layer.to(DEV)
    acts = [to_act(x, dtype).requires_grad_(True) for x in xs]
    plans = []
    _ops().CONV_PROBE = lambda pid, d, real: plans.append((pid, hip.mi355_conv_plan_seg_len(C.byref(d))))
    try:
        z, part = Fn.ConvFn.apply(acts[0], acts[1] if len(acts) > 1 else None, layer.weight, layer.bias, layer.spec, True)
    finally:
        _ops().CONV_PROBE = None
    assert plans and plans[0] == (want_plan, want_len), (plans, want_plan, want_len)
    assert (sp[0] - 1) % want_len + 1 == want_last
    close(from_act(z, cout), z_ref.detach(), dtype, "z")
    cp = z.shape[4]
    if cp > cout:
        assert float(z[..., cout:].abs().max()) == 0.0
    # fused statistics of (z - bias), as in test_gpu_ops.test_conv_fwd_bwd
    s = part.sum(0).cpu()
    zc = z_ref.detach() - b_cpu.view(1, -1, 1, 1, 1)
    n_pos = zc.numel() / cout
    e0 = (s[0, :cout] - zc.sum((0, 2, 3, 4))).abs()
    assert bool((e0 <= 2e-3 * (n_pos * (zc * zc).sum((0, 2, 3, 4))).sqrt() + 1e-6).all()), e0.max()
    close_f32_sum(s[1, :cout], (zc * zc).sum((0, 2, 3, 4)), "sum (z-b)^2")
    # data gradient (ConvFn's backward; the weight gradient is another kernel's)
    z.backward(to_act(gz, dtype))
    off = 0
    for a, c in zip(acts, cins):
        close(from_act(a.grad, c), dx_ref[:, off:off + c], dtype, "dx")
        off += c
