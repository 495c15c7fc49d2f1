"""The ResNet input heads on the device: the fused tail launch (mi355_restail_fwd through Fn.ResTailFn) against torch,
``nn.ResidualUnit`` against the torch restatement of tests/resunit_ref.py in f32 and bf16 mode, ``Generator(head="resnet")`` and a
training step against the oracle, TRANSFER on such a generator, and what has to pick the heads up through ``parameters()`` -- graph
replay, checkpoints, whole-volume prediction.

Tolerances are those of tests/test_gpu_ops.py (``close``, ``close_f32_sum``), of ``test_downsample_conv_golden`` (module, f32 mode),
of tests/test_gpu_bf16.py (``_compare``: module, bf16 mode) and of ``smoke()`` (network).  ReLU is discontinuous and a flipped mask
is no rounding error, so every element-wise gradient check runs on inputs for which the CPU reference itself, in f32 and in f64,
keeps every ReLU input away from zero: min |u_f64| > 8 max |u_f32 - u_f64| (asserted; the seeds below were chosen on the CPU so
that it holds).  CPU references are computed once per case and shared.
"""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import prelu_ref as PR  # noqa: E402
import resunit_ref as RR  # noqa: E402
from oracle import unet_ref as R  # noqa: E402
from test_gpu_bf16 import _compare  # noqa: E402
from test_gpu_modules import _check_grad_digests, _digest  # noqa: E402
from test_gpu_ops import DEV, close, close_f32_sum, from_act, q, to_act  # noqa: E402

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-5


# ---- 1: the tail op --------------------------------------------------------------------------------------------------------------

TAIL_CASES = {  # name: (n, cx, c, spatial, kind, seed per dtype): what the shape is there for
    "proj_ragged": (2, 6, 24, (5, 7, 9), "batch", {F32: 6, BF16: 3}),       # ragged rows, both paddings, two samples in one BatchNorm group
    "identity": (1, 24, 24, (16, 16, 16), "batch", {F32: 4, BF16: 2}),      # identity residual
    "proj_blocks": (1, 6, 24, (16, 32, 33), "batch", {F32: 1, BF16: 3}),    # several workgroups, ragged last block
    "identity_instance": (2, 24, 24, (5, 7, 9), "instance", {F32: 5, BF16: 3}),   # two statistic groups
}
_TAIL_REF = {}


def _tail_inputs(name, dtype):
    """inputs rounded through ``dtype`` and the CPU reference with its gradients, made once per (case, dtype)"""
    if (name, dtype) in _TAIL_REF:
        return _TAIL_REF[(name, dtype)]
    n, cx, c, sp, kind, seeds = TAIL_CASES[name]
    g = torch.Generator().manual_seed(seeds[dtype])
    z = q(torch.randn(n, c, *sp, generator=g) * 1.5 + 0.7, dtype)
    x = q(torch.rand(n, cx, *sp, generator=g), dtype)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.rand(c, generator=g) - 0.5
    dy = q(torch.rand(n, c, *sp, generator=g) - 0.3, dtype)
    w = b = None
    if cx != c:
        w, b = (torch.rand(c, cx, 1, 1, 1, generator=g) - 0.5) * 0.8, torch.rand(c, generator=g) - 0.5

    def reference(f64):
        cast = (lambda t: t.double()) if f64 else (lambda t: t.clone())
        leaves = {k: cast(v).requires_grad_(True) for k, v in dict(z=z, x=x, gamma=gamma, beta=beta).items()}
        if w is not None:
            leaves.update(w=cast(q(w, dtype) if dtype == BF16 else w).requires_grad_(True), b=cast(b).requires_grad_(True))
        if kind == "batch":
            u = F.batch_norm(leaves["z"], None, None, leaves["gamma"], leaves["beta"], True, 0.0, EPS)
        else:
            u = F.instance_norm(leaves["z"], None, None, leaves["gamma"], leaves["beta"], True, 0.0, EPS)
        res = F.conv3d(leaves["x"], leaves["w"], leaves["b"]) if w is not None else leaves["x"]
        y = F.relu(u) + res
        y.backward(cast(dy))
        return y.detach(), u.detach(), {k: v.grad for k, v in leaves.items()}

    y, u32, grads = reference(False)
    _, u64, _ = reference(True)
    margin, noise = float(u64.abs().min()), float((u32.double() - u64).abs().max())
    out = dict(z=z, x=x, gamma=gamma, beta=beta, dy=dy, w=w, b=b, y=y, grads=grads, margin=margin, noise=noise)
    _TAIL_REF[(name, dtype)] = out
    return out


def _run_tail(name, dtype, prefill=None):
    """ResTailFn forward + backward (+ a second backward into pre-filled gradient storage) on the device"""
    import unet_bssfp_amd as M
    from unet_bssfp_amd import functional as Fn
    n, cx, c, sp, kind, _ = TAIL_CASES[name]
    t = _tail_inputs(name, dtype)
    cfg = Fn.NormCfg(kind, c, eps=EPS, slope=0.0)
    zd, xd = to_act(t["z"], dtype).requires_grad_(True), to_act(t["x"], dtype).requires_grad_(True)
    gd, bd = t["gamma"].to(DEV).requires_grad_(True), t["beta"].to(DEV).requires_grad_(True)
    params, wd, wb, spec = [gd, bd], None, None, None
    if t["w"] is not None:
        conv = M.Conv3d(cx, c, 1).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(t["w"]), conv.bias.copy_(t["b"])
        wd, wb, spec = conv.weight, conv.bias, conv.spec
        params += [wd, wb]
    y = Fn.ResTailFn.apply(zd, None, xd, gd, bd, None, wd, wb, None, None, None, spec, cfg, True)
    gact = to_act(t["dy"], dtype)
    y.backward(gact, retain_graph=prefill is not None)
    out = dict(y_act=y.detach().clone(), y=from_act(y.detach(), c), dz=from_act(zd.grad, c), dx=from_act(xd.grad, cx),
               dgamma=gd.grad.cpu().clone(), dbeta=bd.grad.cpu().clone())
    if wd is not None:
        out.update(dw=wd.grad.cpu().clone(), db=wb.grad.cpu().clone())
    if prefill is not None:
        # accumulate: the parameters' gradients live in a bucket (gradsink.GradBuckets) that already holds a first contribution
        from unet_bssfp_amd.gradsink import GradBuckets
        for p in params:
            p.grad = None
        sink = GradBuckets([params], uses_per_phase=2)
        sink.begin_phase()
        for p in params:
            p.grad.fill_(prefill)
            sink.written(p)                                   # one contribution is in: the next one accumulates
        y.backward(gact)
        assert sink.complete()
        out.update(acc_dgamma=gd.grad.cpu().clone(), acc_dbeta=bd.grad.cpu().clone())
        if wd is not None:
            out.update(acc_dw=wd.grad.cpu().clone(), acc_db=wb.grad.cpu().clone())
        sink.detach()
    return out


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("name", list(TAIL_CASES))
def test_restail_fwd_bwd(hip, name, dtype):
    n, cx, c, sp, kind, _ = TAIL_CASES[name]
    t = _tail_inputs(name, dtype)
    print(f"{name} {dtype}: min |u_f64| {t['margin']:.3e}, max |u_f32 - u_f64| {t['noise']:.3e}")
    assert t["margin"] > 8 * t["noise"], "the reference itself cannot tell this input's ReLU mask: choose another seed"
    runs = [_run_tail(name, dtype, prefill=0.5) for _ in range(3)]
    r, g = runs[0], t["grads"]
    tag = f"{name} {dtype}"
    close(r["y"], t["y"], dtype, f"y, {tag}")
    assert r["y_act"].shape[4] == 32 and float(r["y_act"][..., c:].abs().max()) == 0.0     # pad channels: exact zeros
    close(r["dz"], g["z"], dtype, f"dz, {tag}")
    close(r["dx"], g["x"], dtype, f"dx, {tag}")
    close_f32_sum(r["dgamma"], g["gamma"], f"dgamma, {tag}")
    close_f32_sum(r["dbeta"], g["beta"], f"dbeta, {tag}")
    close_f32_sum(r["acc_dgamma"], g["gamma"] + 0.5, f"accumulated dgamma, {tag}")
    close_f32_sum(r["acc_dbeta"], g["beta"] + 0.5, f"accumulated dbeta, {tag}")
    if cx != c:
        close_f32_sum(r["dw"], g["w"], f"dW, {tag}")
        close_f32_sum(r["db"], g["b"], f"db, {tag}")
        close_f32_sum(r["acc_dw"], g["w"] + 0.5, f"accumulated dW, {tag}")
        close_f32_sum(r["acc_db"], g["b"] + 0.5, f"accumulated db, {tag}")
    for other in runs[1:]:
        for k, v in r.items():
            assert torch.equal(v, other[k]), f"{k} differs between two runs, {tag}"


def test_restail_refuses_what_it_does_not_implement(hip):
    import ctypes as C
    from unet_bssfp_amd import _lib, ops
    z, x = to_act(torch.rand(1, 24, 4, 4, 4), F32), to_act(torch.rand(1, 24, 4, 4, 4), F32)
    mean, rstd = torch.zeros(1, 32, device=DEV), torch.ones(1, 32, device=DEV)
    y = torch.zeros_like(z)
    d = _lib.ResTailDesc()
    d.z, d.ldz, d.x, d.ldx, d.cx, d.y, d.ldy = z.data_ptr(), 32, x.data_ptr(), 32, 24, y.data_ptr(), 32
    d.c, d.n_real, d.rows_per_group, d.groups = 32, 24, 64, 1
    d.mean, d.rstd, d.dtype, d.layout = mean.data_ptr(), rstd.data_ptr(), _lib.DT_F32, 1
    assert hip.mi355_restail_fwd(C.byref(d), None) == -2 and b"NDHWC" in hip.mi355_last_error()       # MI355_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        ops.restail_fwd(z, x, 2, mean, rstd, None, None, 24, 24)            # statistics of one group for two
    with pytest.raises(ValueError):
        ops.restail_fwd(z, to_act(torch.rand(1, 6, 4, 4, 4), F32), 1, mean, rstd, None, None, 24, 24)     # identity of a 16-channel x
    assert not ops.restail_supported(80, 6, True) and not ops.restail_supported(32, 48, True) and ops.restail_supported(32, 48, False)
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0                                      # nothing was launched


# ---- 2 / 3: the module -----------------------------------------------------------------------------------------------------------

MODULE_CASES = {"proj": (6, (6, 8, 10), 3), "identity": (24, (5, 7, 9), 12)}      # name: (cin, spatial, seed)
_MODULE_REF = {}


def _module_inputs(name):
    cin, sp, seed = MODULE_CASES[name]
    torch.manual_seed(seed)
    ref = RR.RefResidualUnit(cin, 24, subunits=3, norm="batch").train()
    g = torch.Generator().manual_seed(100 + seed)
    with torch.no_grad():
        for unit in ref.conv:
            unit.adn.N.weight.copy_(torch.rand(24, generator=g) + 0.5)
            unit.adn.N.bias.copy_(torch.rand(24, generator=g) - 0.5)
    # (bf16-representable, so that the f32 reference, the emulation and both modes of the device path read the same input: the
    #  block alone has no rounding at its entry, the pack kernel in front of the device path has)
    x = q(torch.rand(2, cin, *sp, generator=g), BF16)
    w = torch.rand(2, 24, *sp, generator=g)
    return ref, x, w


def _module_reference(name):
    """the f32 reference, the reference under bf16 storage emulation, and the mask margin; made once per case"""
    if name in _MODULE_REF:
        return _MODULE_REF[name]
    ref, x, w = _module_inputs(name)
    start = copy.deepcopy(ref.state_dict())
    margin, noise = RR.mask_margin(ref, x)
    out = dict(start=start, x=x, w=w, margin=margin, noise=noise)
    for tag, emulate in (("f32", False), ("emu", True)):
        m = copy.deepcopy(ref).train()
        xr = x.clone().requires_grad_(True)
        with R.storage_emulation(BF16 if emulate else None):
            y = m(xr)
            (y * w).sum().backward()
        res = dict(y=y.detach(), dx=xr.grad, grads={k: p.grad.detach().clone() for k, p in m.named_parameters()},
                   state={k: v.clone() for k, v in m.state_dict().items()})
        with torch.no_grad(), R.storage_emulation(BF16 if emulate else None):
            res["y_eval"] = m.eval()(x)
        out[tag] = res
    _MODULE_REF[name] = out
    return out


def _run_module(name, dtype, fuse_tail=True):
    import unet_bssfp_amd as M
    cin, sp, _ = MODULE_CASES[name]
    t = _module_reference(name)
    m = M.ResidualUnit(3, cin, 24, subunits=3, act="RELU", norm="BATCH")
    m.load_state_dict(t["start"])
    m = M.set_compute_dtype(m.to(DEV).train(), dtype)
    m.fuse_tail = fuse_tail
    xd = t["x"].to(DEV).requires_grad_(True)
    y = m(xd)
    (y * t["w"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    out = dict(module=m, y=y.detach().cpu(), dx=xd.grad.cpu(), grads={k: p.grad.detach().float().cpu() for k, p in m.named_parameters()},
               state={k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    m.eval()
    with torch.no_grad():
        out["y_eval"] = m(t["x"].to(DEV)).cpu()
    return out


@pytest.mark.parametrize("name", list(MODULE_CASES))
def test_residual_unit_f32_against_the_torch_restatement(hip, name):
    t = _module_reference(name)
    ref = t["f32"]
    print(f"{name}: min |u_f64| {t['margin']:.3e}, max |u_f32 - u_f64| {t['noise']:.3e}")
    assert t["margin"] > 8 * t["noise"], "the reference itself cannot tell this input's ReLU masks: choose another seed"
    gold = {f"g/{k}": np.array([float(v.double().sum()), float(v.double().abs().sum())]) for k, v in ref["grads"].items()}
    runs = {fuse: _run_module(name, F32, fuse) for fuse in (True, False)}
    for fuse, r in runs.items():
        tag = f"{name} fuse_tail={fuse}"
        np.testing.assert_allclose(r["y"].numpy(), ref["y"].numpy(), rtol=2e-4, atol=2e-5, err_msg=tag)
        np.testing.assert_allclose(r["dx"].numpy(), ref["dx"].numpy(), rtol=1e-3, atol=2e-5, err_msg=tag)
        # (the conv biases in front of BatchNorm: analytically zero gradient, exact zeros here, rounding noise in the reference)
        _check_grad_digests(gold, "g", r["module"], skip_fn=lambda k: k.endswith(".conv.bias"))
        for k, v in r["grads"].items():
            if k.endswith(".conv.bias"):
                assert float(v.abs().max()) == 0.0, k
        for i in range(3):
            for stat in ("running_mean", "running_var"):
                k = f"conv.unit{i}.adn.N.{stat}"
                np.testing.assert_allclose(r["state"][k].numpy(), ref["state"][k].numpy(), rtol=1e-4, atol=1e-6, err_msg=f"{tag} {k}")
            assert int(r["state"][f"conv.unit{i}.adn.N.num_batches_tracked"]) == 1
        np.testing.assert_allclose(r["y_eval"].numpy(), ref["y_eval"].numpy(), rtol=2e-4, atol=2e-5, err_msg=f"{tag} eval")
    np.testing.assert_allclose(runs[True]["y"].numpy(), runs[False]["y"].numpy(), rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(runs[True]["dx"].numpy(), runs[False]["dx"].numpy(), rtol=1e-3, atol=2e-5)


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("name", list(MODULE_CASES))
def test_residual_unit_bf16_triangulated(hip, name, fuse):
    """tests/test_gpu_bf16.py's triangulation, on the output, the input gradient and every parameter gradient: HIP-bf16 is no
    further from the f32 reference than bf16 storage alone puts the reference, and no further from the emulation than that"""
    t = _module_reference(name)
    r = _run_module(name, BF16, fuse)

    def entries(res):
        return {"y": res["y"], "y_eval": res["y_eval"], "dx": res["dx"], **res["grads"]}
    _compare(f"resunit {name} fuse_tail={fuse}", entries(r), entries(t["emu"]), entries(t["f32"]))


# ---- 4: the network ---------------------------------------------------------------------------------------------------------------

def _no_dropout(gen):
    """``bSSFPToDWITensorModel(gen_head=...)`` builds the generator with the reference's dropout 0.05; the oracle cannot draw the same
    masks, so the parity runs switch it off (NormCfg.p is read at every forward)"""
    for m in gen.modules():
        if hasattr(m, "cfg") and hasattr(m.cfg, "p"):
            m.cfg.p = 0.0
    return gen


@pytest.mark.parametrize("modality", ["dwi-tensor", "bssfp"])
def test_resnet_generator_and_training_step_against_the_oracle(hip, modality):
    import unet_bssfp_amd as M
    from unet_bssfp_amd.gan import bSSFPToDWITensorModel, synthetic_batch
    cin = RR.HEAD_CHANNELS[modality]
    x, y = R.synthetic_batch(2, 32, seed=1234, cin=cin)
    batch = synthetic_batch(2, 32, seed=1234, modality=modality, device=DEV)
    assert torch.equal(batch[modality]["data"].cpu(), x) and torch.equal(batch["dwi-tensor_orig"]["data"].cpu(), y)

    # PReLU U-Net behind the ResNet heads: forward only
    torch.manual_seed(1)
    gen_p = M.Generator(modality, head="resnet", dropout=0.0, act="prelu")
    ref_p = PR.to_prelu(RR.ref_generator(modality, head="resnet", dropout=0.0)).train()
    ref_p.load_state_dict(gen_p.state_dict())
    with torch.no_grad():
        err = (gen_p.to(DEV).train()(batch[modality]["data"]).cpu() - ref_p(x)).abs().mean().item()
    print(f"{modality}: PReLU generator per-voxel L1 vs oracle {err:.3e}")
    assert err <= 1e-4, err

    torch.manual_seed(0)
    model = bSSFPToDWITensorModel(modality, gen_head="resnet")
    gen, discr = _no_dropout(model.gen), model.discr
    assert isinstance(gen.blocks[modality], M.ResidualUnit)
    rgen = RR.ref_generator(modality, head="resnet", dropout=0.0).train()
    rdiscr = R.RefDiscriminator(modality).train()
    rgen.load_state_dict(gen.state_dict()), rdiscr.load_state_dict(discr.state_dict())
    model = model.to(DEV).train()
    with torch.no_grad():                                     # forward parity: smoke()'s gate
        err = (model.gen(batch[modality]["data"]).cpu() - rgen(x)).abs().mean().item()
    print(f"{modality}: generator per-voxel L1 vs oracle {err:.3e}")
    assert err <= 1e-4, err
    for unit in rgen.blocks[modality].conv:                   # (the two forwards above moved the running statistics on both sides alike)
        assert int(unit.adn.N.num_batches_tracked) == 1
    model.training_step(batch, 0)
    torch.cuda.synchronize()
    g_opt, d_opt = R.make_optimizers(rgen, rdiscr)
    ref = R.gan_training_step(rgen, rdiscr, g_opt, d_opt, x, y)
    for k in ("gen_loss_adversarial", "gen_loss_recon_L1", "gen_loss", "discr_loss"):
        a, b = float(model.last_logs["train_" + k]), float(ref[k])
        print(f"{modality}: {k} {a:.6f} oracle {b:.6f}")
        assert abs(a - b) <= 2e-3 * max(1.0, abs(b)), (k, a, b)


# ---- 5: TRANSFER trains the selected head and nothing else ------------------------------------------------------------------------

def _staged_model(modality, seed=4):
    import unet_bssfp_amd as M
    from unet_bssfp_amd.functional import DropoutState
    from unet_bssfp_amd.gan import bSSFPToDWITensorModel
    from unet_bssfp_amd.stages import TrainingState
    torch.manual_seed(seed)
    DropoutState.reset()
    model = bSSFPToDWITensorModel(modality, gen_head="resnet", batch_size=2).to(DEV).train()
    M.set_compute_dtype(model, BF16)
    DropoutState.base(torch.device(DEV))
    return model.change_training_state(TrainingState.TRANSFER, modality)


@pytest.mark.parametrize("modality,launches", [("dwi-tensor", 4), ("bssfp", 3)])
def test_transfer_on_resnet_heads(hip, modality, launches):
    """Fails without the feature: there is no ``gen_head``."""
    from test_stages_gpu import _packed
    from unet_bssfp_amd import ops
    from unet_bssfp_amd.gan import GraphedTrainingStep, synthetic_batch
    batches = [synthetic_batch(2, 32, seed=100 + i, modality=modality, device=DEV) for i in range(2)]
    model = _staged_model(modality)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.training_step(batches[0], 0)
    torch.cuda.synchronize()
    packed = {k: t.clone() for k, t in _packed(model.gen.blocks["unet"]).items()}       # (every packing exists after the first step)
    # launch accounting of the second step's generator phase: the head's three convolutions (+ the projection), nothing of the U-Net
    seen, logs = [], {}
    try:
        ops.WGRAD_PROBE = lambda kind, d: seen.append((d.ks, d.cout, d.cin)) and None
        model._phase_gen(batches[1], logs)
        model._finish_grads("gen")
    finally:
        ops.WGRAD_PROBE = None
    model._phase_gen_update_discr(batches[1], logs)
    model._finish_grads("discr")
    model._phase_discr_update()                                # (these five calls are training_step)
    model.last_logs = logs
    torch.cuda.synchronize()
    cin = RR.HEAD_CHANNELS[modality]
    assert sorted(seen) == sorted([(3, 24, cin), (3, 24, 24), (3, 24, 24)] + ([(1, 24, cin)] if launches == 4 else [])), seen
    after = {k: v.detach().clone() for k, v in model.state_dict().items()}
    head = f"gen.blocks.{modality}."
    others = tuple(f"gen.blocks.{m}." for m in RR.HEAD_CHANNELS if m != modality)
    assert sum(k.startswith("gen.blocks.unet.") for k in after) > 50
    for k in after:
        if k.startswith("gen.blocks.unet.") or k.startswith(others):
            assert torch.equal(after[k], before[k]), k
        elif k.startswith(head) and not k.endswith(".conv.bias"):     # (a conv bias in front of BatchNorm has a zero gradient: only
            assert not torch.equal(after[k], before[k]), k            #  AdamW's weight decay moves it, and that is not asked here)
    now = _packed(model.gen.blocks["unet"])
    assert len(packed) >= 20 and set(now) == set(packed) and all(torch.equal(now[k], t) for k, t in packed.items())
    eager_logs = {k: v.detach().clone() for k, v in model.last_logs.items()}

    # the same two steps through a captured graph, from the same start
    graphed = _staged_model(modality)
    gs = GraphedTrainingStep(graphed, copy.deepcopy(batches[0]), warmup=2, preserve_state=True)
    for b in batches:
        gs.load(b)
        gs()
    torch.cuda.synchronize()
    replayed = graphed.state_dict()
    assert list(replayed) == list(after)
    for k in after:
        assert torch.equal(replayed[k], after[k]), k
    for k, v in eager_logs.items():
        if k in graphed.last_logs:
            assert torch.equal(graphed.last_logs[k], v), k


# ---- 6: plumbing -------------------------------------------------------------------------------------------------------------------

def test_hipgraph_replay_equals_eager_on_resnet_heads(hip):
    from unet_bssfp_amd.functional import DropoutState
    from unet_bssfp_amd.gan import GraphedTrainingStep, bSSFPToDWITensorModel, synthetic_batch

    def build():
        torch.manual_seed(4)
        DropoutState.reset()
        return bSSFPToDWITensorModel("bssfp", gen_head="resnet").to(DEV).train()

    batch = synthetic_batch(2, 32, seed=9, device=DEV)
    eager = build()
    for i in range(4):
        eager.training_step(batch, i)
    graphed = build()
    gs = GraphedTrainingStep(graphed, batch, warmup=2)         # 2 eager warm-up steps, then capture (records, does not run)
    gs()                                                       # replay = step 3
    gs()                                                       # replay = step 4
    torch.cuda.synchronize()
    for (k, p), (_, r) in zip(eager.state_dict().items(), graphed.state_dict().items()):
        assert torch.equal(p, r), k
    for k in ("train_gen_loss", "train_discr_loss"):
        assert float(eager.last_logs[k]) == float(graphed.last_logs[k])
    assert int(graphed.gen.blocks["bssfp"].conv.unit2.adn.N.num_batches_tracked) > 0


def test_checkpoint_round_trip_and_whole_volume_prediction(hip, tmp_path):
    import unet_bssfp_amd as M
    from unet_bssfp_amd import checkpoint as ck
    from unet_bssfp_amd.gan import bSSFPToDWITensorModel, synthetic_batch
    from unet_bssfp_amd.inference import predict_volume
    torch.manual_seed(0)
    a = bSSFPToDWITensorModel("t1w", batch_size=2, gen_head="resnet", gen_act="prelu").to(DEV).train()
    b1, b2 = (synthetic_batch(2, 32, seed=s, modality="t1w", device=DEV) for s in (3, 4))
    a.training_step(b1, 0)
    ck.save_checkpoint(a, tmp_path / "g.ckpt", epoch=1, global_step=1)
    a.training_step(b2, 1)                                     # dropout 0.05 is on: the mask counter resumes too
    b, info = ck.load_from_checkpoint(tmp_path / "g.ckpt", device=DEV)
    assert info["global_step"] == 1 and b.gen_head == "resnet" and isinstance(b.gen.blocks["t1w"], M.ResidualUnit)
    b.train().training_step(b2, 1)
    torch.cuda.synchronize()
    assert set(a.last_logs) == set(b.last_logs)
    for k, v in a.last_logs.items():
        assert torch.equal(v, b.last_logs[k]), k
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka

    vol = torch.rand(6, 32, 64, 64, generator=torch.Generator().manual_seed(5)).to(DEV)
    stats = {k: v.clone() for k, v in b.gen.blocks["t1w"].state_dict().items()}
    out = predict_volume(b.gen, vol, patch_size=32, batch_size=4)
    assert tuple(out.shape) == (6, 32, 64, 64) and bool(torch.isfinite(out).all()) and b.gen.training
    b.gen.eval()
    with torch.no_grad():                                      # eval mode: running statistics, so a patch does not depend on its batch
        patch = b.gen(vol[None, :, :, 32:, :32])
    torch.testing.assert_close(out[:, :, 32:, :32], patch[0], rtol=2e-4, atol=2e-5)
    for k, v in b.gen.blocks["t1w"].state_dict().items():      # prediction did not touch the running statistics
        assert torch.equal(v, stats[k]), k


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_resnet_head_kernels_read_no_unwritten_memory(hip, dtype):
    """tail op and module, forward, backward and an accumulating backward: the same bits with every fresh allocation poisoned
    (tests/alloc_poison.py)"""
    from alloc_poison import run_scenario

    def scenario():
        out = {}
        for name in ("proj_ragged", "identity_instance"):
            out.update({f"{name}/{k}": v for k, v in _run_tail(name, dtype, prefill=0.5).items()})
        for name in MODULE_CASES:
            for fuse in (True, False):
                r = _run_module(name, dtype, fuse)
                out.update({f"{name}/{fuse}/y": r["y"], f"{name}/{fuse}/dx": r["dx"], f"{name}/{fuse}/y_eval": r["y_eval"]})
                out.update({f"{name}/{fuse}/grad/{k}": v for k, v in r["grads"].items()})
                out.update({f"{name}/{fuse}/state/{k}": v for k, v in r["state"].items()})
        return out

    for name in ("proj_ragged", "identity_instance"):
        _tail_inputs(name, dtype)                              # (CPU references: made before anything is poisoned)
    for name in MODULE_CASES:
        _module_reference(name)
    run_scenario(scenario, sync=torch.cuda.synchronize)
