"""Staged training on the device (unet_bssfp_amd.stages): TRANSFER runs the U-Net's data-gradient chain WITHOUT its weight
gradients -- ``UpCatConvFn``, ``FusedFinal`` / ``LazyDx``, ``SkipPoolFn`` / ``LazyPool``, ``DeferredReduce``, ``ColSumSide`` with
``needs_input_grad`` false for the parameters -- a path that had only ever run for the PatchGAN (frozen in the generator phase).

Runs that several tests look at are made once.  ``DropoutState`` is process-wide: every run is finished and snapshotted before
the next model is built.  The state machine is not in the reference's ``src/`` (parity unpinned); the CPU side of the parity test
is the independent loop of tests/stages_cases.py on oracle modules.
"""
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import unet_ref as R  # noqa: E402
from stages_cases import LOG_NAMES, StagedLoop  # noqa: E402
from unet_bssfp_amd.stages import TrainingState  # noqa: E402

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
_CACHE = {}


def _model(state, modality="bssfp", built="dwi-tensor", seed=4, dtype=torch.bfloat16, dropout=0.05, batch_size=4, lr=None, **kw):
    """a model built for ``built`` (the pretraining modality) and moved into ``state`` for ``modality``; seeded like every other"""
    import unet_bssfp_amd as M
    from unet_bssfp_amd.functional import DropoutState
    from unet_bssfp_amd.gan import bSSFPToDWITensorModel
    torch.manual_seed(seed)
    DropoutState.reset()
    gen, discr = M.Generator(built, dropout=dropout), M.Discriminator(built)
    model = bSSFPToDWITensorModel(built, gen=gen.to(DEV), discr=discr.to(DEV), batch_size=batch_size, **kw).train()
    M.set_compute_dtype(model, dtype)
    DropoutState.base(torch.device(DEV))
    if state is not None or modality != built:
        model.change_training_state(state, modality, lr=lr)
    return model


def _batches(n, s, count, modality="bssfp"):
    from unet_bssfp_amd.gan import synthetic_batch
    return [synthetic_batch(n, s, seed=100 + i, modality=modality, device=DEV) for i in range(count)]


def _packed(net):
    """every packed-weight buffer of ``net`` that exists now: (module, cache key) -> tensor"""
    from unet_bssfp_amd.functional import UpCatTables
    out = {}
    for name, m in net.named_modules():
        spec = getattr(m, "spec", None)
        if spec is not None and hasattr(spec, "cache"):
            for key, e in spec.cache._store.items():
                out[(name, key)] = e[1][0]
        tables = getattr(m, "upcat_tables", None)
        if isinstance(tables, UpCatTables) and tables.bufs is not None:
            for i, t in enumerate(list(tables.bufs) + [tables.wpk[0]]):
                if isinstance(t, torch.Tensor):
                    out[(name, "upcat", i)] = t
    return out


def _snapshot(model):
    from unet_bssfp_amd.functional import DropoutState
    torch.cuda.synchronize()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    moments, steps, owners = [], [], set()
    for o in model.optimizers():
        if hasattr(o, "sync_step_counts"):
            o.sync_step_counts()
        for p in o.param_groups[0]["params"]:
            st = o.state.get(p)
            if st:
                moments += [st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
                steps.append(int(st["step"]))
        owners |= {id(p) for p in o.state}
    return {"state": state, "moments": moments, "steps": steps, "owners": owners,
            "dropout": int(DropoutState.base(torch.device(DEV)).item())}


def _transfer_run(name):
    """three TRANSFER steps at 32^3, N = 4, bf16, dropout on, from the same start: 'eager' through ``training_step``, 'graph'
    through ``GraphedTrainingStep(preserve_state=True)``, 'segments' through the same with the multi-rank structure (five graph
    segments, two-stage backward passes) on one rank; made once each"""
    if name in _CACHE:
        return _CACHE[name]
    from unet_bssfp_amd.gan import GraphedTrainingStep
    model = _model(TrainingState.TRANSFER)
    batches = _batches(4, 32, 3)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    logs, gs = [], None
    if name in ("graph", "segments"):
        gs = GraphedTrainingStep(model, copy.deepcopy(batches[0]), warmup=2, preserve_state=True, force_segments=name == "segments")
        torch.cuda.synchronize()
        for k, v in model.state_dict().items():
            assert torch.equal(v, before[k]), f"preserve_state: {k} changed by the capture"
        packed = {k: t.clone() for k, t in _packed(model.gen.blocks["unet"]).items()}
    for i, b in enumerate(batches):
        if gs is not None:
            gs.load(b)
            gs()
        else:
            model.training_step(b, i)
        torch.cuda.synchronize()
        logs.append({k: v.detach().clone() for k, v in model.last_logs.items()})
        if gs is None and i == 0:       # eager: every packing (forward and data gradient) exists after the first step
            packed = {k: t.clone() for k, t in _packed(model.gen.blocks["unet"]).items()}
    out = {"model": model, "before": before, "logs": logs, "snap": _snapshot(model), "packed": packed, "graphed": gs}
    _CACHE[name] = out
    return out


# ---- 1: frozen means frozen ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["eager", "graph"])
def test_transfer_keeps_the_unet_frozen(hip, name):
    """Fails without the feature: after one step the U-Net was trainable again (``_toggle(self.gen, True)``), and with gradient
    sinks ``FusedAdamW`` stepped it with stale gradients and weight decay."""
    run = _transfer_run(name)
    model, before, after = run["model"], run["before"], run["snap"]["state"]
    unet = [k for k in after if k.startswith("gen.blocks.unet.")]
    assert len(unet) > 50
    for k in unet:
        assert torch.equal(after[k], before[k]), k
    now = _packed(model.gen.blocks["unet"])
    assert len(run["packed"]) >= 20 and set(now) == set(run["packed"])
    for k, t in run["packed"].items():
        assert torch.equal(now[k], t), k
    for k in ("gen.blocks.bssfp.conv.weight", "gen.blocks.bssfp.bn.weight", "gen.blocks.bssfp.bn.bias", "gen.blocks.bssfp.bn.running_mean",
              "discr.d1.bssfp.conv.weight", "discr.d2.conv.weight", "discr.d3.bn.weight", "discr.d5.conv.weight", "discr.final.weight"):
        assert not torch.equal(after[k], before[k]), k
    for k in after:                                                             # the heads that are not selected stay unused
        if k.startswith(("gen.blocks.dwi-tensor.", "discr.d1.dwi-tensor.")):
            assert torch.equal(after[k], before[k]), k
    frozen = list(model.gen.blocks["unet"].parameters())
    assert not ({id(p) for p in frozen} & run["snap"]["owners"])                # no optimiser state for a frozen parameter
    assert all(p.grad is None and not p.requires_grad and not hasattr(p, "_mi355_sink") for p in frozen)
    assert all(p.requires_grad for p in model.discr.parameters()) and all(p.requires_grad for p in model.gen.blocks["bssfp"].parameters())
    trainable = sum(p.numel() for p in model.gen.blocks["bssfp"].parameters())
    assert sum(f.numel() for f in model.sinks_gen.flat if f is not None) == trainable   # the buckets hold the trainable set only
    assert run["snap"]["steps"] and set(run["snap"]["steps"]) == {3}
    assert all(math.isfinite(float(v)) for step in run["logs"] for v in step.values())


# ---- 2: graph equals eager, bit for bit ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["graph", "segments"])
def test_transfer_graph_replays_equal_eager_steps_bit_for_bit(hip, name):
    a, b = _transfer_run(name), _transfer_run("eager")
    if name == "segments":          # the generator's late stage is the frozen U-Net alone: its bucket keeps its index and holds nothing
        assert len(a["graphed"].graphs) == 5 and a["model"].sinks_gen.params[0] == [] and a["model"].sinks_gen.flat[0] is None
        assert len(a["model"].sinks_gen.params[1]) == 4 and len(a["model"].sinks_discr.params) == 2
    assert list(a["snap"]["state"]) == list(b["snap"]["state"])
    for k in a["snap"]["state"]:
        assert torch.equal(a["snap"]["state"][k], b["snap"]["state"][k]), k     # parameters, BatchNorm statistics and counters
    assert len(a["snap"]["moments"]) == len(b["snap"]["moments"]) > 0
    for i, (x, y) in enumerate(zip(a["snap"]["moments"], b["snap"]["moments"])):
        assert torch.equal(x, y), f"optimiser moment {i}"
    assert a["snap"]["steps"] == b["snap"]["steps"] and a["snap"]["dropout"] == b["snap"]["dropout"]
    for step, (la, lb) in enumerate(zip(a["logs"], b["logs"])):
        assert set(la) == set(lb)
        for k in la:
            assert torch.equal(la[k], lb[k]), (step, k)


# ---- 3: a stale graph raises -----------------------------------------------------------------------------------------------------

def test_replay_after_a_state_change_raises(hip):
    """Fails without the feature (there is no state to change)."""
    run = _transfer_run("graph")
    gs, model = run["graphed"], run["model"]
    assert not gs.stale()
    try:
        model.change_training_state(TrainingState.FINE_TUNE)
        assert gs.stale()
        with pytest.raises(RuntimeError, match="training state changed"):
            gs()
        assert all(p.requires_grad for p in model.parameters())
    finally:
        model.change_training_state(TrainingState.TRANSFER)         # (the run is shared: leave its model as the other tests expect it)
    assert gs.stale()                                               # the same state again is still another version: new optimisers


# ---- 4: parity of the path that never ran ----------------------------------------------------------------------------------------

def _oracle_copies(model, modality):
    rgen, rdiscr = R.RefGenerator(modality, dropout=0.0).train(), R.RefDiscriminator(modality).train()
    rgen.load_state_dict({k: v.cpu() for k, v in model.gen.state_dict().items()})
    rdiscr.load_state_dict({k: v.cpu() for k, v in model.discr.state_dict().items()})
    return rgen, rdiscr


def test_transfer_step_matches_the_independent_cpu_loop_f32(hip, golden_dir):
    """f32 mode, N = 2, 64^3 (the last PatchGAN BatchNorm then sees 16 values per channel), dropout 0, ``torch.optim.AdamW`` on both
    sides.  Step 0 rtol 1e-3; step 1 by the rule of test_gan_step_matches_oracle_n2_s64_with_torch_adamw: |hip - f64| <=
    3 * max(largest |cpu_f32 - f64| among the losses, the committed ensemble spread of that loss).  After step 0 the head's
    gradient digests within ``_check_grad_digests``' bound (rtol 2e-3, atol 2e-5); the head's conv.bias is excluded, as
    ``noisy_bias`` does (a BatchNorm follows: its gradient is analytically zero)."""
    from tests.test_gpu_modules import _check_grad_digests, noisy_bias
    from unet_bssfp_amd.gan import synthetic_batch
    model = _model(TrainingState.TRANSFER, seed=3, dtype=torch.float32, dropout=0.0, batch_size=2, optimizer_class=torch.optim.AdamW)
    rgen, rdiscr = _oracle_copies(model, "bssfp")
    dgen, ddiscr = copy.deepcopy(rgen).double(), copy.deepcopy(rdiscr).double()
    loop = StagedLoop(rgen, rdiscr, frozen=[rgen.blocks["unet"]], watch=rgen.blocks["bssfp"])
    loop64 = StagedLoop(dgen, ddiscr, frozen=[dgen.blocks["unet"]])
    batch = synthetic_batch(2, 64, seed=77, device=DEV)
    x, y = R.synthetic_batch(2, 64, seed=77)
    spread = np.load(os.path.join(golden_dir, "gan_step_f32_spread.npz"))
    unet_before = [p.detach().clone() for p in model.gen.blocks["unet"].parameters()]
    for step in range(2):
        model.training_step(batch, step)
        ref, r64 = loop.step(x, y), loop64.step(x.double(), y.double())
        cpu_dev = max(abs(float(ref[k]) - float(r64[k])) / abs(float(r64[k])) for k in LOG_NAMES)
        for k in LOG_NAMES:
            got = float(model.last_logs["train_" + k])
            dev = abs(got - float(r64[k])) / abs(float(r64[k]))
            print(f"step {step} {k}: hip {got:.7f} cpu f32 {float(ref[k]):.7f} f64 {float(r64[k]):.7f}  |hip - f64| {dev:.2e} "
                  f"cpu {cpu_dev:.2e} spread {float(spread[f'step{step}/{k}']):.2e}")
            if step == 0:
                np.testing.assert_allclose(got, float(ref[k]), rtol=1e-3, err_msg=f"{step}/{k}")
            assert dev <= 3 * max(cpu_dev, float(spread[f"step{step}/{k}"])) + 1e-7, (step, k, dev, cpu_dev)
        if step == 0:
            # (gradient sinks: the head's .grad still holds the generator phase's values; the discriminator phase wrote none)
            gold = {f"head/{n}": np.array([g.double().sum().item(), g.double().abs().sum().item()]) for n, g in loop.head_grads.items()}
            assert set(gold) == {"head/conv.weight", "head/conv.bias", "head/bn.weight", "head/bn.bias"}
            for n, p in model.gen.blocks["bssfp"].named_parameters():
                print(f"head {n}: hip {p.grad.double().sum().item():.6e} / {p.grad.double().abs().sum().item():.6e}  cpu {gold['head/' + n]}")
            _check_grad_digests(gold, "head", model.gen.blocks["bssfp"], skip_fn=noisy_bias)
    assert all(torch.equal(p, b) for p, b in zip(model.gen.blocks["unet"].parameters(), unet_before))
    assert all(p.grad is None for p in model.gen.blocks["unet"].parameters())


def test_transfer_step0_bf16_against_the_f32_mode(hip):
    """32^3, N = 4, dropout 0: the bf16 step-0 losses against the f32-mode HIP step from the same start, with the bound of
    tests/test_gpu_bf16.py for step-0 losses (5e-3; 2e-2 for the discriminator loss, which follows the first AdamW update)."""
    batch = _batches(4, 32, 1)[0]
    logs = {}
    for mode, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        model = _model(TrainingState.TRANSFER, seed=11, dtype=dtype, dropout=0.0)
        model.training_step(batch, 0)
        torch.cuda.synchronize()
        logs[mode] = {k: float(v) for k, v in model.last_logs.items()}
        del model
    for k, ref in logs["f32"].items():
        got = logs["bf16"][k]
        print(f"transfer 32^3 step0 {k:28s} bf16 {got:.6f} f32-mode {ref:.6f}")
        assert np.isfinite(got)
        assert abs(got - ref) <= (5e-3 if "discr" not in k else 2e-2) * abs(ref), (k, got, ref)


# ---- 5: launch accounting ----------------------------------------------------------------------------------------------------------

def _wgrad_launches(state):
    """the weight-gradient descriptors of one step at 32^3, N = 2, bf16, per phase (pointers as null / non-null)"""
    import conv_plan_cases as P
    from unet_bssfp_amd import ops
    model = _model(state, built="bssfp", dropout=0.0, batch_size=2, lr=1e-3 if state is not None else None)
    batch = _batches(2, 32, 1)[0]
    model.training_step(batch, 0)                       # (a first step: caches, sinks, optimiser state)
    phases = {"gen": [], "discr": []}
    logs = {}
    try:
        ops.WGRAD_PROBE = lambda kind, d: phases["gen"].append(tuple(P.flatten(d))) and None
        model._phase_gen(batch, logs)
        model._finish_grads("gen")
        ops.WGRAD_PROBE = lambda kind, d: phases["discr"].append(tuple(P.flatten(d))) and None
        model._phase_gen_update_discr(batch, logs)
        model._finish_grads("discr")
        model._phase_discr_update()
        torch.cuda.synchronize()
    finally:
        ops.WGRAD_PROBE = None
    cols = P.columns(type(_lib_wgrad_desc()))
    return phases, cols


def _lib_wgrad_desc():
    from unet_bssfp_amd import _lib
    return _lib.WgradDesc()


def test_weight_gradient_launches_follow_the_state(hip):
    plain, cols = _wgrad_launches(None)
    transfer, _ = _wgrad_launches(TrainingState.TRANSFER)
    tuned, _ = _wgrad_launches(TrainingState.FINE_TUNE)
    ks, cout, cin = cols.index("ks"), cols.index("cout"), cols.index("cin")
    assert len(plain["gen"]) > 20                                               # the U-Net's 20-odd convolutions and the head
    # TRANSFER, generator phase: the head's 1x1x1 convolution (24 -> 24) and nothing else
    assert [(d[ks], d[cout], d[cin]) for d in transfer["gen"]] == [(1, 24, 24)]
    assert transfer["gen"][0] in plain["gen"]
    assert transfer["discr"] == plain["discr"] and len(plain["discr"]) >= 6
    assert tuned["gen"] == plain["gen"] and tuned["discr"] == plain["discr"]


# ---- 6: FINE_TUNE at the model's rate is the plain step ----------------------------------------------------------------------------

def test_fine_tune_at_the_models_rate_equals_the_plain_step(hip):
    batches = _batches(4, 32, 2)
    snaps = []
    for state in (None, TrainingState.FINE_TUNE):
        model = _model(state, built="bssfp", lr=1e-3 if state is not None else None)
        if state is not None:
            assert model.optimizers()[0].param_groups[0]["lr"] == model.lr == 1e-3
        for i, b in enumerate(batches):
            model.training_step(b, i)
        snaps.append(_snapshot(model))
        del model
    plain, tuned = snaps
    for k in plain["state"]:
        assert torch.equal(plain["state"][k], tuned["state"][k]), k
    assert len(plain["moments"]) == len(tuned["moments"]) > 0
    assert all(torch.equal(a, b) for a, b in zip(plain["moments"], tuned["moments"]))
    assert plain["steps"] == tuned["steps"] and plain["dropout"] == tuned["dropout"]


# ---- 7: modalities -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("modality,unused", [("bssfp", "dwi-tensor"), ("t1w", "bssfp")])
def test_transfer_to_another_modality_runs_and_leaves_the_other_heads_alone(hip, modality, unused):
    model = _model(TrainingState.TRANSFER, modality=modality, seed=8)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.training_step(_batches(4, 32, 1, modality=modality)[0], 0)
    torch.cuda.synchronize()
    after = model.state_dict()
    assert all(math.isfinite(float(v)) for v in model.last_logs.values())
    for k in after:
        if k.startswith((f"gen.blocks.{unused}.", f"discr.d1.{unused}.", "gen.blocks.unet.")):
            assert torch.equal(after[k], before[k]), k
    assert not torch.equal(after[f"gen.blocks.{modality}.conv.weight"], before[f"gen.blocks.{modality}.conv.weight"])
    assert not torch.equal(after[f"discr.d1.{modality}.conv.weight"], before[f"discr.d1.{modality}.conv.weight"])
    for net, table in ((model.gen, model.gen.blocks), (model.discr, model.discr.d1)):
        assert all(p.grad is None for p in table[unused].parameters())
    for o in model.optimizers():
        assert not any(o.state.get(p) for table in (model.gen.blocks, model.discr.d1) for p in table[unused].parameters())
    if modality == "t1w":                               # 'dwi-tensor' and 't1w' share one head object: it is the one that trained
        assert model.gen.blocks["t1w"] is model.gen.blocks["dwi-tensor"]


# ---- 8: the three stages through the fit loop --------------------------------------------------------------------------------------

def test_train_staged_on_the_device(hip, tmp_path):
    """32^3 patches, two subjects, one epoch per stage, graph on"""
    from unet_bssfp_amd import data as Q
    from unet_bssfp_amd.functional import DropoutState
    from unet_bssfp_amd.train import train_staged
    g = torch.Generator().manual_seed(2)
    subjects = []
    for s in ((40, 52, 36), (36, 44, 44)):
        subjects.append({"bssfp": {"data": (torch.rand((24,) + s, generator=g) - 0.3).to(DEV)},
                         "dwi-tensor": {"data": (torch.rand((6,) + s, generator=g) - 0.3).to(DEV)}})

    def queues(state, modality):
        kw = dict(max_length=4, samples_per_volume=2, sampler=Q.UniformSampler(32), target_shape=(36, 48, 40), transform=[])
        return Q.PatchQueue(subjects, modality, seed=17, **kw), Q.PatchQueue(subjects[:1], modality, seed=18, **kw)

    torch.manual_seed(6)
    DropoutState.reset()
    paths = train_staged(queues, "bssfp", str(tmp_path), max_epochs=1, device=DEV, graph=True, batch_size=4)
    assert len(paths) == 3 and all(os.path.exists(p) for p in paths)
    names = [os.path.basename(p) for p in paths]
    assert names[0].startswith("TrainingState.PRETRAIN-dwi-tensor-epoch=00-") and names[1].startswith("TrainingState.TRANSFER-bssfp-epoch=00-")
    assert names[2].startswith("TrainingState.FINE_TUNE-bssfp-epoch=00-")
    ckpts = [torch.load(p, weights_only=True) for p in paths]
    for c, state in zip(ckpts, TrainingState):
        assert c["hyper_parameters"]["training_state"] == str(state)
        history = c["mi355"]["history"]
        assert len(history) == 1 and history[0]["nonfinite"] == {}
        assert all(math.isfinite(v) for k, v in history[0].items() if isinstance(v, float))
        assert "train_gen_loss" in history[0] and "val_loss" in history[0]
    unet = [{k: v for k, v in c["state_dict"].items() if k.startswith("gen.blocks.unet.")} for c in ckpts]
    assert len(unet[0]) > 50
    for k in unet[0]:
        assert torch.equal(unet[0][k], unet[1][k]), k                          # TRANSFER started from PRETRAIN's best and kept it
    assert any(not torch.equal(unet[1][k], unet[2][k]) for k in unet[1])
    head = "gen.blocks.bssfp.conv.weight"
    assert not torch.equal(ckpts[0]["state_dict"][head], ckpts[1]["state_dict"][head])
