"""PReLU with a trained slope on the device (BasicUNet(act="PReLU")): the fused norm + dropout + PReLU kernels against torch, the
network against the patched oracle of tests/prelu_ref.py, and everything downstream that has to pick ``adn.A.weight`` up through
``parameters()`` -- graph replay, FusedAdamW, checkpoints, training states.

Tolerances are those of tests/test_gpu_ops.py and tests/test_gpu_modules.py.  The slope gradient is ONE f32 sum over a whole
activation: at op level the incoming gradient is drawn from U[0, 1), so every term da * u (u <= 0) has one sign, nothing cancels,
and the f32-sum rule of test_gpu_ops.py holds relative to the result itself: |err| <= 2e-3 |ref|.  At network level the sums cancel
heavily and the bound is built from the f32 CPU oracle's own distance to the f64 oracle (prelu_ref.network_reference).

Measured on an MI355X (seed 41 / 31): see DESIGN.md section 8.15.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import prelu_ref as PR  # noqa: E402
from oracle import unet_ref as R  # noqa: E402
from test_gpu_ops import DEV, close, close_f32_sum, from_act, q, to_act  # noqa: E402

pytestmark = pytest.mark.gpu

SEED_3D, SEED_2D = 41, 31          # inputs on which the reference itself meets the preconditions of the slope check (asserted below)


# ---- 1: op level ---------------------------------------------------------------------------------------------------------------

def _reseed():
    """the same dropout mask in every forward that follows: the mask is a function of (counter, per-call salt, element)"""
    from unet_bssfp_amd.functional import DropoutState
    torch.manual_seed(77)
    DropoutState.reset()


def _run_op(z, gamma, beta, alpha, ga, dtype, p, small, prefill=None):
    """NormActFn forward + backward (+ a second backward into pre-filled gradient storage) -> a, dz, dgamma, dbeta, dalpha, ..."""
    from unet_bssfp_amd import functional as Fn
    c = z.shape[1]
    _reseed()
    cfg = Fn.NormCfg("instance", c, p=p, act="prelu")
    zd = to_act(z, dtype).requires_grad_(True)
    gd, bd = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
    ad = torch.tensor([alpha], device=DEV, requires_grad=True)
    a = Fn.NormActFn.apply(zd, None, gd, bd, None, ad, None, None, None, cfg, True, Fn.NormOpts(small=small))
    gact = to_act(ga, dtype)
    a.backward(gact, retain_graph=prefill is not None)
    out = dict(a=from_act(a.detach(), c), dz=from_act(zd.grad, c), dgamma=gd.grad.cpu().clone(), dbeta=bd.grad.cpu().clone(),
               dalpha=ad.grad.cpu().clone())
    if prefill is not None:
        # accumulate: the parameters' gradients live in a bucket (gradsink.GradBuckets) that already holds a first contribution
        from unet_bssfp_amd.gradsink import GradBuckets
        for t in (gd, bd, ad):
            t.grad = None
        sink = GradBuckets([[gd, bd, ad]], uses_per_phase=2)
        sink.begin_phase()
        for t in (gd, bd, ad):
            t.grad.fill_(prefill)
            sink.written(t)                                   # one contribution is in: the next one accumulates
        a.backward(gact)
        assert sink.complete()
        out.update(acc_dgamma=gd.grad.cpu().clone(), acc_dbeta=bd.grad.cpu().clone(), acc_dalpha=ad.grad.cpu().clone())
        sink.detach()
    return out


OP_CASES = [  # n, c, spatial, p: what the shape is there for
    (1, 32, (16, 16, 16), 0.0),    # streaming, two reduce blocks per group
    (2, 24, (5, 7, 9), 0.1),       # ragged rows, channels padded to 32, two groups, dropout
    (2, 128, (4, 6, 8), 0.0),      # small
    (1, 128, (16, 16, 16), 0.0),   # small, 8 row slots
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n,c,sp,p", OP_CASES)
def test_normact_prelu_fwd_bwd(hip, dtype, n, c, sp, p):
    from unet_bssfp_amd import ops
    g = torch.Generator().manual_seed(13)
    z = q(torch.randn(n, c, *sp, generator=g) * 1.5 + 0.7, dtype)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.rand(c, generator=g) - 0.5
    ga = q(torch.rand(n, c, *sp, generator=g), dtype)                  # U[0, 1): the slope gradient's terms share one sign
    cp = ops.round_up(c, 16)
    paths = [True, False] if ops.norm_is_small(n, *sp, cp) else [False]
    if c == 32:
        assert ops._lib.load().mi355_channel_stats_blocks(sp[0] * sp[1] * sp[2]) >= 2
    mask = None
    if p > 0.0:
        # the mask, recovered from a run with a slope that maps nothing but dropped elements to 0 (as
        # test_dropout_statistics_and_backward_mask recovers it); every run below draws the same one (_reseed)
        probe = _run_op(z, gamma, beta, 0.25, ga, dtype, p, False)
        mask = (probe["a"] != 0).float() / (1 - p)
        assert abs(float((mask == 0).float().mean()) - p) < 0.02
    for alpha in (0.25, -0.4, 0.0, 1.0):
        z_cpu = z.clone().requires_grad_(True)
        g_cpu, b_cpu = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        al = torch.tensor([alpha], requires_grad=True)
        u = F.instance_norm(z_cpu, None, None, g_cpu, b_cpu, True, 0.0, 1e-5)
        if mask is not None:
            u = u * mask
        a_ref = F.prelu(u, al)
        a_ref.backward(ga)
        got = {small: _run_op(z, gamma, beta, alpha, ga, dtype, p, small, prefill=0.5) for small in paths}
        for small, r in got.items():
            tag = f"alpha {alpha} {'small' if small else 'streaming'}"
            close(r["a"], a_ref.detach(), dtype, f"a, {tag}")
            if dtype == torch.float32:
                torch.testing.assert_close(r["dz"], z_cpu.grad, rtol=1e-3, atol=1e-5, msg=lambda m: f"dz, {tag}: {m}")
            else:
                close(r["dz"], z_cpu.grad, dtype, f"dz, {tag}")
            close_f32_sum(r["dgamma"], g_cpu.grad, f"dgamma, {tag}")
            close_f32_sum(r["dbeta"], b_cpu.grad, f"dbeta, {tag}")
            ref_a = float(al.grad)
            err = abs(float(r["dalpha"]) - ref_a)
            print(f"{tag} {dtype}: dalpha {float(r['dalpha']):.6e} ref {ref_a:.6e} rel err {err / abs(ref_a):.2e}")
            assert r["dalpha"].shape == (1,) and ref_a < 0
            assert err <= 2e-3 * abs(ref_a), (tag, float(r["dalpha"]), ref_a)
            # the second backward added to what the storage held
            close_f32_sum(r["acc_dgamma"], g_cpu.grad + 0.5, f"accumulated dgamma, {tag}")
            close_f32_sum(r["acc_dbeta"], b_cpu.grad + 0.5, f"accumulated dbeta, {tag}")
            assert abs(float(r["acc_dalpha"]) - (ref_a + 0.5)) <= 2e-3 * abs(ref_a), (tag, float(r["acc_dalpha"]), ref_a + 0.5)
        if len(got) == 2:                                              # eligible for both paths: they agree within the same bounds
            sm, big = got[True], got[False]
            close(sm["a"], big["a"], dtype, "a: small vs streaming")
            close_f32_sum(sm["dgamma"], big["dgamma"], "dgamma: small vs streaming")
            assert abs(float(sm["dalpha"]) - float(big["dalpha"])) <= 2e-3 * abs(float(big["dalpha"]))


def test_slope_gradient_is_bit_identical_from_run_to_run(hip):
    g = torch.Generator().manual_seed(3)
    for n, c, sp, small in ((1, 32, (16, 16, 32), False), (2, 128, (4, 6, 8), True)):
        z = torch.randn(n, c, *sp, generator=g)
        ga = torch.rand(n, c, *sp, generator=g) - 0.5
        runs = [_run_op(z, torch.ones(c), torch.zeros(c), 0.3, ga, torch.float32, 0.1, small)["dalpha"] for _ in range(3)]
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_prelu_kernels_read_no_unwritten_memory(hip, dtype):
    """The slope-gradient scratch (partials, per-channel totals) comes from torch.empty like every other buffer: forward, backward
    and an accumulating backward give the same bits with every fresh allocation poisoned (tests/alloc_poison.py)."""
    from alloc_poison import run_scenario

    def scenario():
        g = torch.Generator().manual_seed(21)
        out = {}
        for tag, (n, c, sp, small) in {"streaming": (2, 24, (5, 7, 9), False), "small": (2, 128, (4, 6, 8), True)}.items():
            z = q(torch.randn(n, c, *sp, generator=g), dtype)
            ga = q(torch.rand(n, c, *sp, generator=g) - 0.5, dtype)
            r = _run_op(z, torch.rand(c, generator=g) + 0.5, torch.rand(c, generator=g) - 0.5, 0.3, ga, dtype, 0.1, small, prefill=0.5)
            out.update({f"{tag}/{k}": v for k, v in r.items()})
        return out
    run_scenario(scenario, sync=torch.cuda.synchronize)


# ---- 2: fused forms ------------------------------------------------------------------------------------------------------------

def test_fused_forms_leave_prelu_gradients_as_they_leave_leakyrelu_gradients(hip):
    """PoolSide / LazyPool (a level's norm launch pools, its backward forms the pool's gradient) and FusedFinal / LazyDx (the last
    norm launch evaluates the final 1x1x1 convolution, its backward forms that convolution's data gradient), on and off: wherever
    the LeakyReLU network's parameter gradients do not change by a bit, the PReLU network's must not either -- the slope of a block
    goes with that block's norm weight, whose gradient leaves the same launches."""
    import unet_bssfp_amd as M
    from unet_bssfp_amd import functional as Fn
    from unet_bssfp_amd.functional import DropoutState
    x = torch.rand(1, 3, 32, 32, 32, generator=torch.Generator().manual_seed(8)).to(DEV)

    def grads(act, pool_side, lazy_pool, lazy_dx):
        torch.manual_seed(6)
        DropoutState.reset()
        net = M.BasicUNet(3, 3, 6, dropout=0.05, **({"act": act} if act else {}))
        net = M.set_compute_dtype(net.to(DEV).train(), torch.bfloat16)
        old = Fn.PoolSide.enabled, Fn.LazyPool.enabled, M.BasicUNet.lazy_final_dx
        Fn.PoolSide.enabled, Fn.LazyPool.enabled, M.BasicUNet.lazy_final_dx = pool_side, lazy_pool, lazy_dx
        try:
            net(x).abs().mean().backward()
        finally:
            Fn.PoolSide.enabled, Fn.LazyPool.enabled, M.BasicUNet.lazy_final_dx = old
        torch.cuda.synchronize()
        return {n: p.grad.clone() for n, p in net.named_parameters()}

    settings = {"all on": (True, True, True), "PoolSide off": (False, True, True), "LazyPool off": (True, False, True),
                "lazy_final_dx off": (True, True, False)}
    leaky = {k: grads(None, *v) for k, v in settings.items()}
    prelu = {k: grads("PReLU", *v) for k, v in settings.items()}
    assert len([n for n in prelu["all on"] if n.endswith(".A.weight")]) == 18
    for k in list(settings)[1:]:
        same = {n for n in leaky[k] if torch.equal(leaky[k][n], leaky["all on"][n])}
        assert len(same) >= 40, (k, len(same))                         # (the check below is not vacuous)
        for n, gp in prelu[k].items():
            partner = n.replace(".A.weight", ".N.weight")
            if partner in same:
                assert torch.equal(gp, prelu["all on"][n]), (k, n)
    for n, gp in prelu["all on"].items():
        assert torch.isfinite(gp).all() and (not n.endswith(".A.weight") or float(gp.abs()) > 0), n


# ---- 3, 8: the network against the patched oracle, f32 ---------------------------------------------------------------------------

def _check_network(net, r, x, y):
    """forward (.train() and .eval()), non-slope gradients and slope gradients of ``net`` (on the device, holding the reference's
    parameters) against prelu_ref.network_reference's result ``r``; -> E_hip, the largest slope error in units of S_abs"""
    print(f"reference alone: E_cpu {r['e_cpu']:.3e}, min |g64| / S_abs {r['margin']:.3e}")
    assert r["e_cpu"] <= 1e-4, "precondition on the reference: pick another seed"
    assert 4 * r["e_cpu"] < r["margin"], "precondition on the reference: pick another seed"
    y_hip = net.train()(x.to(DEV))
    (y_hip - y.to(DEV)).abs().mean().backward()
    for mode, ref_y in (("train", r["y"]), ("eval", r["y_eval"])):
        with torch.no_grad():
            got = (y_hip.detach() if mode == "train" else net.eval()(x.to(DEV))).cpu()
        assert (got - ref_y).abs().mean().item() <= 1e-4, mode
        torch.testing.assert_close(got, ref_y, rtol=2e-3, atol=2e-4, msg=lambda m: f"{mode}: {m}")
    e_hip = 0.0
    for name, p in net.named_parameters():
        gh = p.grad.cpu()
        if name.endswith(".A.weight"):
            err = abs(float(gh) - r["g64"][name]) / r["s_abs"][name]
            e_hip = max(e_hip, err)
            print(f"{name}: hip {float(gh):.6e} f64 {r['g64'][name]:.6e} S_abs {r['s_abs'][name]:.3e} err / S_abs {err:.2e}")
            continue
        gr = r["grads"][name]
        assert gh.shape == gr.shape, name
        if name.endswith(".conv.bias"):                               # zero by construction in front of a normalisation
            assert float(gh.abs().max()) <= 1e-5, name
            continue
        err = (gh - gr).norm()
        assert err <= 5e-3 * gr.norm() + 1e-7, (name, float(err), float(gr.norm()))
    print(f"E_hip {e_hip:.3e} against the bound 4 E_cpu = {4 * r['e_cpu']:.3e}")
    for name in r["g64"]:
        err = abs(float(dict(net.named_parameters())[name].grad) - r["g64"][name])
        assert err <= 4 * r["e_cpu"] * r["s_abs"][name], (name, err / r["s_abs"][name], 4 * r["e_cpu"])
    return e_hip


def test_prelu_network_matches_the_patched_oracle(hip):
    """32 x 48 x 64: streaming kernels at 32 and 64 channels, the small ones below; 18 distinct slopes."""
    from unet_bssfp_amd import BasicUNet
    feats = (32, 64, 128, 256, 512, 32)

    def make():
        torch.manual_seed(SEED_3D)
        return PR.ref_basic_unet(3, 24, 6, feats, dropout=0.0)
    g = torch.Generator().manual_seed(SEED_3D)
    x, y = torch.rand(1, 24, 32, 48, 64, generator=g), torch.rand(1, 6, 32, 48, 64, generator=g)
    r = PR.network_reference(make, x, y)
    net = BasicUNet(3, 24, 6, feats, act="PReLU", dropout=0)
    net.load_state_dict(r["ref"].state_dict())
    assert len({float(p) for _, p in PR.slopes(net)}) == 18
    _check_network(net.to(DEV), r, x, y)


def test_prelu_network_spatial_dims_2_matches_the_patched_oracle(hip):
    from unet_bssfp_amd import BasicUNet

    def make():
        torch.manual_seed(SEED_2D)
        return PR.ref_basic_unet(spatial_dims=2, in_channels=1, out_channels=6, dropout=0.0)
    g = torch.Generator().manual_seed(SEED_2D)
    x, y = torch.rand(2, 1, 64, 64, generator=g), torch.rand(2, 6, 64, 64, generator=g)
    r = PR.network_reference(make, x, y)
    net = BasicUNet(spatial_dims=2, in_channels=1, out_channels=6, act="PReLU", dropout=0.0)
    net.load_state_dict(r["ref"].state_dict())
    _check_network(net.to(DEV), r, x, y)


# ---- 4: graph replay -------------------------------------------------------------------------------------------------------------

def test_hipgraph_replay_follows_the_trained_slopes(hip):
    """As test_hipgraph_replayed_step_equals_eager_step, with a PReLU generator: 2 warm-up steps + 2 replays equal 4 eager steps
    bit for bit.  A slope baked into the capture (read on the host, or passed by value) fails: every slope moves in every step."""
    import unet_bssfp_amd as M
    from unet_bssfp_amd.functional import DropoutState
    from unet_bssfp_amd.gan import GraphedTrainingStep, bSSFPToDWITensorModel, synthetic_batch

    def build():
        torch.manual_seed(4)
        DropoutState.reset()
        gen, discr = M.Generator("bssfp", dropout=0.05, act="PReLU"), M.Discriminator("bssfp")
        return bSSFPToDWITensorModel("bssfp", gen=gen.to(DEV), discr=discr.to(DEV)).train()

    batch = synthetic_batch(2, 32, seed=9, device=DEV)
    eager = build()
    first = {n: p.detach().clone() for n, p in PR.slopes(eager)}
    assert len(first) == 18
    for i in range(4):
        if i == 3:
            third = {n: p.detach().clone() for n, p in PR.slopes(eager)}
        eager.training_step(batch, i)
    graphed = build()
    gs = GraphedTrainingStep(graphed, batch, warmup=2)
    gs()
    gs()
    torch.cuda.synchronize()
    for (n, p), (_, p2) in zip(eager.named_parameters(), graphed.named_parameters()):
        assert torch.equal(p, p2), n
    for n, p in PR.slopes(graphed):
        assert not torch.equal(p, third[n]) and not torch.equal(p, first[n]), n
    for k in ("train_gen_loss", "train_discr_loss"):
        assert float(eager.last_logs[k]) == float(graphed.last_logs[k])


# ---- 5: AdamW --------------------------------------------------------------------------------------------------------------------

def test_fused_adamw_steps_one_element_parameters(hip):
    """FusedAdamW against torch.optim.AdamW (weight decay applies to a slope as to any parameter) on given gradients, over a list
    in which (1,)-shaped parameters sit between the others."""
    from unet_bssfp_amd.optim import FusedAdamW
    torch.manual_seed(0)
    shapes = [(32, 24, 3, 3, 3), (32,), (1,), (32,), (7,), (1,), (1,)]
    ps = [torch.randn(s) for s in shapes]
    a = [p.clone().to(DEV).requires_grad_(True) for p in ps]
    b = [p.clone().requires_grad_(True) for p in ps]
    oa, ob = FusedAdamW(a, lr=1e-3), torch.optim.AdamW(b, lr=1e-3)
    for step in range(3):
        for pa, pb in zip(a, b):
            g = torch.randn(pb.shape)
            pa.grad, pb.grad = g.to(DEV), g.clone()
        oa.step()
        ob.step()
    for pa, pb in zip(a, b):
        torch.testing.assert_close(pa.detach().cpu(), pb.detach(), rtol=1e-5, atol=1e-6)


# ---- 6, 7: checkpoints and training states ---------------------------------------------------------------------------------------

def _prelu_model(modality="bssfp", seed=4, **kw):
    import unet_bssfp_amd as M
    from unet_bssfp_amd.functional import DropoutState
    from unet_bssfp_amd.gan import bSSFPToDWITensorModel
    torch.manual_seed(seed)
    DropoutState.reset()
    gen, discr = M.Generator(modality, act="PReLU"), M.Discriminator(modality)
    return bSSFPToDWITensorModel(modality, gen=gen.to(DEV), discr=discr.to(DEV), **kw).train()


def test_checkpoint_round_trip_of_a_prelu_model(hip, tmp_path):
    import unet_bssfp_amd as M
    from unet_bssfp_amd import checkpoint as ck
    from unet_bssfp_amd.gan import synthetic_batch
    a = _prelu_model(batch_size=2)
    a.training_step(synthetic_batch(2, 32, seed=9, device=DEV), 0)              # the slopes have left their initial value
    ck.save_checkpoint(a, tmp_path / "p.ckpt", epoch=1, global_step=1)
    assert "gen.blocks.unet.down_1.convs.conv_0.adn.A.weight" in torch.load(tmp_path / "p.ckpt", weights_only=True)["state_dict"]
    torch.manual_seed(11)
    b, info = ck.load_from_checkpoint(tmp_path / "p.ckpt", device="cuda", gen=M.Generator("bssfp", act="PReLU"))
    assert info["ignored_keys"] == [] and list(a.state_dict()) == list(b.state_dict())
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    assert all(float(p) != 0.25 for _, p in PR.slopes(b.gen))
    with pytest.raises(RuntimeError, match="does not match the model"):         # a LeakyReLU model has no place for the slopes
        ck.load_from_checkpoint(tmp_path / "p.ckpt", device="cuda")


def test_training_states_freeze_and_release_the_slopes(hip):
    from unet_bssfp_amd.gan import synthetic_batch
    from unet_bssfp_amd.stages import TrainingState
    model = _prelu_model("dwi-tensor", batch_size=2)
    model.change_training_state(TrainingState.TRANSFER, "bssfp")
    batch = synthetic_batch(2, 32, seed=100, modality="bssfp", device=DEV)
    before = {n: p.detach().clone() for n, p in PR.slopes(model.gen.blocks["unet"])}
    head = model.gen.blocks["bssfp"].conv.weight.detach().clone()
    model.training_step(batch, 0)
    torch.cuda.synchronize()
    for n, p in PR.slopes(model.gen.blocks["unet"]):
        assert p.grad is None and not p.requires_grad and torch.equal(p, before[n]), n
    assert not torch.equal(model.gen.blocks["bssfp"].conv.weight, head)          # the step did train what TRANSFER trains
    model.change_training_state(TrainingState.FINE_TUNE, "bssfp")
    model.training_step(batch, 1)
    torch.cuda.synchronize()
    for n, p in PR.slopes(model.gen.blocks["unet"]):
        assert p.requires_grad and p.grad is not None and not torch.equal(p, before[n]), n
