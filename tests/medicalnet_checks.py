"""What tests/test_medicalnet_gpu.py and tests/test_medicalnet_grad_gpu.py share: the bounds of a single layer and of the whole
network, the layout helpers and the seeded network both are held to.  A plain module (no conftest, no plugin).

A SINGLE layer on identical bf16-exact inputs may differ from the bf16-emulating reference only by the rounding of single
elements (f32 summation order): rel-L2 <= 1e-3, no element further off than one bf16 spacing at the tensor's largest magnitude,
at most 10 % of the elements different (the tolerances of tests/test_gpu_bf16.py, for the reasons given there).  The WHOLE
network is triangulated between the exact reference (f32 for the forward, f64 for the gradient) and the bf16-emulating one:
rel(hip, ref) <= 1.25 rel(emu, ref) + 0.02 and rel(hip, emu) <= rel(emu, ref) + 0.02.
"""
import torch

import medicalnet_ref as MR

DEV = "cuda:0"


def log(line):
    print(line)


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).norm() / b.norm()).item()


def q16(t):
    return t.to(torch.bfloat16).float()


def single_layer_check(tag, got, ref):
    """got / ref: bf16-representable f32 tensors of one layer on identical inputs"""
    diff = (got - ref).abs()
    frac = float((diff > 0).float().mean())
    worst = float(diff.max() / (ref.abs().max() * 2.0 ** -7))
    r = rel(got, ref)
    log(f"{tag}: rel-L2 {r:.2e}, max diff {worst:.2f} bf16 spacings at the tensor's scale, differing elements {frac:.2e}")
    assert r <= 1e-3, r
    assert worst <= 1.0, worst
    assert frac <= 0.10, frac


def triangulate(tag, d_hip_ref, d_hip_emu, d_emu_ref, ref="f32"):
    """ref: the name of the exact reference in the printed line"""
    log(f"{tag}: rel(hip, {ref}) {d_hip_ref:.3e}, rel(hip, emu) {d_hip_emu:.3e}, rel(emu, {ref}) {d_emu_ref:.3e}")
    assert d_hip_ref <= 1.25 * d_emu_ref + 0.02, (d_hip_ref, d_emu_ref)
    assert d_hip_emu <= d_emu_ref + 0.02, (d_hip_emu, d_emu_ref)


def to_ndhwc(x):
    return x.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)


def from_ndhwc(a):
    return a.float().permute(0, 4, 1, 2, 3).cpu()


def make_refnet():
    """the fixture ``refnet`` of both files (each wraps it with module scope)"""
    return MR.random_init(MR.RefResNet10(), seed=11)


def make_net(refnet):
    """the fixture ``net``: the device network with the weights of ``refnet``"""
    from unet_bssfp_amd.medicalnet import MedicalNetResNet10
    m = MedicalNetResNet10()
    m.load_state_dict(refnet.state_dict(), strict=True)
    return m.to(DEV)
