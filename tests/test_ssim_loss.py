"""losses.SSIMLoss (csrc/ssim_loss.hip): 1 - SSIM as a differentiable term of the reconstruction slot.

Value and gradient against the f64 oracle (oracle/metrics_ref.py::ssim3d under autograd, on the CPU).  The gradient bound is
not a fixed number: kernel and f32 oracle are both f32 roundings of the same f64 gradient, the kernel sums 3 x 11 taps
separably where the oracle sums 1331 directly, so the kernel's spread max|g - g64| / max|g64| has to stay within 4 x the
spread of the f32 oracle measured in the same test."""
import functools

import pytest
import torch

from oracle import metrics_ref as MR

# shape, (win, sigma), input kind, |loss - loss_f64| bound (tests/test_metrics.py: 2e-5; 2e-3 where the variance terms are
# rounding noise against c2 = 9e-4)
CASES = {
    "one_window": ((1, 2, 11, 11, 11), (11, 1.5), "s0.2", 2e-5),        # every voxel gets exactly one tap: grad = g x g x g * P
    "all_clipped": ((2, 3, 13, 14, 19), (11, 1.5), "s0.2", 2e-5),       # valid extents 3, 4, 9 < window: every tap range clipped at both ends
    "background": ((1, 6, 24, 20, 37), (11, 1.5), "s0.05_bg", 2e-5),    # full 11 taps along D and W, clipped along H, odd W, zero background
    "win7": ((2, 1, 12, 17, 9), (7, 1.0), "s0.2", 2e-5),                # runtime-length window, W below 11
    "near_const": ((1, 2, 16, 16, 16), (11, 1.5), "near_const", 2e-3),  # variance terms at rounding level
    "patch32": ((1, 6, 32, 32, 32), (11, 1.5), "s0.2", 2e-5),           # the patch shape of the model test
}


def _inputs(shape, kind):
    g = torch.Generator().manual_seed(sum(shape))
    if kind == "near_const":
        y = 0.5 + 1e-3 * torch.randn(shape, generator=g)
        p = 0.3 + 1e-3 * torch.randn(shape, generator=g)
        return p, y
    y = torch.rand(shape, generator=g)
    s = 0.05 if kind == "s0.05_bg" else 0.2
    p = (y + s * torch.randn(shape, generator=g)).clamp(0, 1)
    if kind == "s0.05_bg":
        third = shape[-1] // 3
        p[..., :third] = 0
        y[..., :third] = 0
    return p, y


def _oracle_grad(p, y, win, sigma, dtype, compose):
    x = p.to(dtype).clone().requires_grad_(True)
    loss = compose(1 - MR.ssim3d(x, y.to(dtype), win_size=win, kernel_sigma=sigma))
    loss.backward()
    return loss.detach(), x.grad


def _spread(g, g64):
    return ((g.double() - g64).abs().max() / g64.abs().max()).item()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(p, y, f64 loss, f64 gradient, spread of the f32 oracle's gradient) of the mean-reduced loss; computed once, not modified"""
    shape, (win, sigma), kind, _ = CASES[name]
    p, y = _inputs(shape, kind)
    loss64, g64 = _oracle_grad(p, y, win, sigma, torch.float64, torch.mean)
    _, g32 = _oracle_grad(p, y, win, sigma, torch.float32, torch.mean)
    return p, y, loss64, g64, _spread(g32, g64)


def _device_grad(loss_fn, p, y, scale=None):
    x = p.cuda().requires_grad_(True)
    loss = loss_fn(x, y.cuda())
    (loss if scale is None else scale * loss).backward()
    return loss.detach(), x.grad


# ------------------------------------------------------------------ CPU: the ABI and the argument checks
def test_entry_points_and_host_validation():
    from unet_bssfp_amd import _lib
    lib = _lib.load()
    for name in ("mi355_ssim3d_loss_workspace_bytes", "mi355_ssim3d_loss_fwd", "mi355_ssim3d_loss_bwd"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    ws = lib.mi355_ssim3d_loss_workspace_bytes
    assert ws(2, 6, 32, 32, 32, 11) > 0
    assert ws(1, 1, 10, 32, 32, 11) == -1                       # d < win
    assert ws(1, 1, 32, 32, 32, 16) == -1                       # win > 15
    assert ws(0, 1, 32, 32, 32, 11) == -1 and ws(-1, 1, 32, 32, 32, 11) == -1
    rc = lib.mi355_ssim3d_loss_fwd(None, None, 1, 1, 11, 11, 11, 11, None, 1e-4, 9e-4, None, 0, None, None, None)
    assert rc < 0 and b"ssim3d_loss_fwd" in lib.mi355_last_error() and b"null" in lib.mi355_last_error()
    rc = lib.mi355_ssim3d_loss_bwd(None, None, None, None, 1, 1, 11, 11, 11, 11, None, None, 0, None, None)
    assert rc < 0 and b"ssim3d_loss_bwd" in lib.mi355_last_error() and b"null" in lib.mi355_last_error()
    rc = lib.mi355_ssim3d_loss_bwd(None, None, None, None, 1, 1, 11, 11, 8, 11, None, None, 0, None, None)
    assert rc < 0 and b"bad shape" in lib.mi355_last_error()


def test_constructor_and_cpu_tensor_errors():
    from unet_bssfp_amd import _lib
    from unet_bssfp_amd.losses import SSIMLoss
    with pytest.raises(NotImplementedError):
        SSIMLoss(2)
    with pytest.raises(NotImplementedError):
        SSIMLoss(3, kernel_type="uniform")
    with pytest.raises(ValueError):
        SSIMLoss(3, reduction="median")
    with pytest.raises(ValueError):
        SSIMLoss(3, win_size=17)
    loss = SSIMLoss(3, data_range=2.0, win_size=7, kernel_sigma=1.0, k1=0.02, k2=0.05, reduction="sum")
    assert (loss.data_range, loss.win_size, loss.kernel_sigma, loss.k1, loss.k2, loss.reduction) == (2.0, 7, 1.0, 0.02, 0.05, "sum")
    assert torch.allclose(loss._window, MR.gaussian_1d(7, 1.0))
    y = torch.rand(1, 1, 12, 12, 12)
    with pytest.raises(_lib.Mi355Error):
        SSIMLoss(3)(y, y)


# ------------------------------------------------------------------ GPU: value and gradient against the f64 oracle
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_loss_and_gradient_match_f64_oracle(name):
    from unet_bssfp_amd.losses import SSIMLoss
    _, (win, sigma), _, loss_tol = CASES[name]
    p, y, loss64, g64, spread32 = _reference(name)
    loss, g = _device_grad(SSIMLoss(3, win_size=win, kernel_sigma=sigma), p, y)
    g = g.cpu()
    spread = _spread(g, g64)
    print(f"{name}: |loss - loss64| = {abs(loss.item() - loss64.item()):.3e}  gradient spread: kernel {spread:.3e}, f32 oracle {spread32:.3e}")
    assert loss.shape == () and g.shape == p.shape and g.dtype == torch.float32
    assert abs(loss.item() - loss64.item()) <= loss_tol
    assert spread <= 4 * spread32


@pytest.mark.gpu
def test_gpu_gradient_scale_reductions_and_determinism():
    from unet_bssfp_amd.losses import SSIMLoss
    p, y, loss64, g64, spread32 = _reference("all_clipped")
    loss, g = _device_grad(SSIMLoss(3), p, y)
    # the incoming gradient is applied on the device
    loss_s, g_s = _device_grad(SSIMLoss(3), p, y, scale=3.5)
    assert torch.equal(loss_s, loss) and torch.allclose(g_s, 3.5 * g, rtol=1e-6, atol=0)
    # two calls: bit-identical
    loss_2, g_2 = _device_grad(SSIMLoss(3), p, y)
    assert torch.equal(loss_2, loss) and torch.equal(g_2, g)
    # sum: B per-item values within 2e-5 each; the gradient is B x the mean's (the spread measure is scale-free)
    b = p.shape[0]
    sum64, gsum64 = _oracle_grad(p, y, 11, 1.5, torch.float64, torch.sum)
    loss_sum, g_sum = _device_grad(SSIMLoss(3, reduction="sum"), p, y)
    assert abs(loss_sum.item() - sum64.item()) <= b * 2e-5
    assert _spread(g_sum.cpu(), gsum64) <= 4 * spread32
    # none: (B, 1), and a different weight per item reaches the right item
    wts = torch.tensor([[1.0], [-2.0]])
    compose = lambda t: (t * wts.to(t.dtype)).sum()
    none64 = 1 - MR.ssim3d(p.double(), y.double())
    _, gw64 = _oracle_grad(p, y, 11, 1.5, torch.float64, compose)
    _, gw32 = _oracle_grad(p, y, 11, 1.5, torch.float32, compose)
    x = p.cuda().requires_grad_(True)
    loss_none = SSIMLoss(3, reduction="none")(x, y.cuda())
    assert loss_none.shape == (b, 1) and torch.allclose(loss_none.cpu().double(), none64, atol=2e-5, rtol=0)
    (loss_none * wts.cuda()).sum().backward()
    assert _spread(x.grad.cpu(), gw64) <= 4 * _spread(gw32, gw64)


@pytest.mark.gpu
def test_gpu_known_answers_and_metric_consistency():
    from unet_bssfp_amd.losses import SSIMLoss
    from unet_bssfp_amd.metrics import SSIMMetric
    p, y, *_ = _reference("patch32")
    pd, yd = p.cuda(), y.cuda()
    assert abs(SSIMLoss(3)(pd, yd).item() - (1 - SSIMMetric(3)(pd, yd).mean().item())) <= 2e-5
    assert abs(SSIMLoss(3)(yd, yd).item()) <= 1e-6
    a, b = torch.full((1, 1, 12, 12, 12), 0.3, device="cuda"), torch.full((1, 1, 12, 12, 12), 0.5, device="cuda")
    want = 1 - (2 * 0.3 * 0.5 + 1e-4) / (0.09 + 0.25 + 1e-4)
    assert abs(SSIMLoss(3)(a, b).item() - want) <= 2e-3


@pytest.mark.gpu
def test_gpu_views_dtypes_and_errors():
    from unet_bssfp_amd.losses import SSIMLoss
    fn = SSIMLoss(3)
    g = torch.Generator().manual_seed(5)
    yd = torch.rand((1, 3, 12, 13, 14), generator=g).cuda()
    big = torch.rand((1, 5, 12, 13, 14), generator=g).cuda().requires_grad_(True)
    fn(big[:, :3], yd).backward()                                        # a non-contiguous view of a larger leaf
    _, want = _device_grad(fn, big.detach()[:, :3].contiguous().cpu(), yd.cpu())
    assert big.grad.shape == big.shape and torch.equal(big.grad[:, :3], want) and not big.grad[:, 3:].any()
    half = big.detach()[:, :3].bfloat16().requires_grad_(True)            # bf16 in, bf16 gradient: the f32 one rounded once
    fn(half, yd).backward()
    _, want = _device_grad(fn, half.detach().float().cpu(), yd.cpu())
    assert half.grad.dtype == torch.bfloat16 and torch.equal(half.grad, want.bfloat16())
    with pytest.raises(NotImplementedError):
        fn(big[:, :3], yd.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        fn(big, yd)                                                      # shape mismatch
    with pytest.raises(ValueError):
        fn(yd[0], yd[0])                                                 # not 5-D
    with pytest.raises(ValueError):
        fn(yd[..., :8], yd[..., :8])                                     # smaller than the window


# ------------------------------------------------------------------ GPU: in the model's reconstruction slot
def _model(dropout):
    import unet_bssfp_amd as M
    from unet_bssfp_amd.functional import DropoutState
    from unet_bssfp_amd.gan import bSSFPToDWITensorModel
    from unet_bssfp_amd.losses import SSIMLoss
    torch.manual_seed(4)
    DropoutState.reset()
    gen, discr = M.Generator("bssfp", dropout=dropout), M.Discriminator("bssfp")
    return bSSFPToDWITensorModel("bssfp", gen=gen.cuda(), discr=discr.cuda(), extra_recon_terms={"SSIM": SSIMLoss(3)}).train()


@pytest.mark.gpu
def test_gpu_training_step_logs_the_term():
    from unet_bssfp_amd.gan import synthetic_batch
    model = _model(0.0)
    model.training_step(synthetic_batch(2, 32, seed=9, device="cuda"), 0)
    logs = {k: float(v) for k, v in model.last_logs.items()}
    assert 0.0 < logs["train_gen_loss_recon_SSIM"] < 2.0
    want = (logs["train_gen_loss_recon_L1"] + logs["train_gen_loss_recon_SSIM"]) / 2 * 100
    assert logs["train_gen_loss_recon"] == pytest.approx(want, rel=1e-6)
    assert logs["train_gen_loss"] == pytest.approx(logs["train_gen_loss_adversarial"] + want, rel=1e-6)


@pytest.mark.gpu
def test_gpu_hipgraph_replayed_step_with_the_term_equals_eager_step():
    """as test_hipgraph_replayed_step_equals_eager_step: the term records into the graph (no host sync, no host read of a
    device value) and is deterministic"""
    from unet_bssfp_amd.gan import GraphedTrainingStep, synthetic_batch
    batch = synthetic_batch(2, 32, seed=9, device="cuda")
    eager = _model(0.05)
    for i in range(4):
        eager.training_step(batch, i)
    graphed = _model(0.05)
    gs = GraphedTrainingStep(graphed, batch, warmup=2)
    gs()
    gs()
    torch.cuda.synchronize()
    for (n, p), (_, q) in zip(eager.named_parameters(), graphed.named_parameters()):
        assert torch.equal(p, q), n
    for k in ("train_gen_loss", "train_gen_loss_recon_SSIM"):
        assert float(eager.last_logs[k]) == float(graphed.last_logs[k])
