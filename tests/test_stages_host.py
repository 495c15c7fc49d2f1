"""Staged training on the host (unet_bssfp_amd.stages, gan.change_training_state, train.train_staged): oracle modules on CPU at
32^3, N = 2, ``torch.optim.AdamW``.  The state machine is not in the reference's ``src/`` (parity unpinned): these tests pin the
contract of ``stages.py``.  Runs that several tests look at are made once (a CPU oracle step takes seconds); the tests that are
about files and plumbing use the tiny networks of tests/stages_cases.py."""
import copy
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import unet_ref as R  # noqa: E402
from stages_cases import LOG_NAMES, StagedLoop, TinyDiscriminator, TinyGenerator, TinyQueue  # noqa: E402
from unet_bssfp_amd import checkpoint  # noqa: E402
from unet_bssfp_amd.gan import bSSFPToDWITensorModel, synthetic_batch  # noqa: E402
from unet_bssfp_amd.stages import TrainingState  # noqa: E402
from unet_bssfp_amd.trainer import ModelCheckpoint, Trainer  # noqa: E402

_CACHE = {}


def _oracle_model(modality="dwi-tensor", seed=0, **kw):
    torch.manual_seed(seed)
    gen, discr = R.RefGenerator(modality, dropout=0.0).train(), R.RefDiscriminator(modality).train()
    return bSSFPToDWITensorModel(modality, gen=gen, discr=discr, optimizer_class=torch.optim.AdamW, **kw).train()


def _transfer_run():
    """pretrain-shaped model -> TRANSFER on 'bssfp' -> two steps, against the independent loop on copies; made once"""
    if "transfer" not in _CACHE:
        model = _oracle_model()
        model.change_training_state(TrainingState.TRANSFER, "bssfp")
        rgen, rdiscr = copy.deepcopy(model.gen), copy.deepcopy(model.discr)
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        loop = StagedLoop(rgen, rdiscr, frozen=[rgen.blocks["unet"]], lr=model.lr)
        batch = synthetic_batch(2, 32, seed=5)
        x, y = batch["bssfp"]["data"], batch["dwi-tensor_orig"]["data"]
        logs, ref_logs, flags = [], [], []
        for step in range(2):
            model.training_step(batch, step)
            logs.append({k: float(model.last_logs["train_" + k]) for k in LOG_NAMES})
            flags.append([p.requires_grad for p in model.gen.blocks["unet"].parameters()])
            ref_logs.append({k: float(v) for k, v in loop.step(x, y).items()})
        _CACHE["transfer"] = (model, before, logs, ref_logs, loop, flags)
    return _CACHE["transfer"]


def test_training_state_names():
    assert str(TrainingState.TRANSFER) == "TrainingState.TRANSFER"                  # the prefix of the reference's file names
    assert [s.name for s in TrainingState] == ["PRETRAIN", "TRANSFER", "FINE_TUNE"]
    model = bSSFPToDWITensorModel("bssfp", gen=TinyGenerator("bssfp"), discr=TinyDiscriminator("bssfp"))
    assert model.training_state is None and model.stage_version == 0
    model.change_training_state("TrainingState.FINE_TUNE")
    assert model.training_state is TrainingState.FINE_TUNE and model.stage_lr == 1e-5 and model.stage_version == 1
    model.change_training_state("PRETRAIN", lr=0.5)
    assert model.training_state is TrainingState.PRETRAIN and model.stage_lr == 0.5 and model.stage_version == 2
    with pytest.raises(ValueError, match="unknown training state"):
        model.change_training_state("WARMUP")
    with pytest.raises(KeyError, match="unknown modality"):
        model.change_training_state(TrainingState.TRANSFER, "flair")


def test_transfer_keeps_the_unet_frozen_over_two_steps():
    """Fails without the feature: ``_toggle(self.gen, True)`` made every generator parameter trainable again after the first
    discriminator phase."""
    model, before, _, _, _, flags = _transfer_run()
    after = model.state_dict()
    unet = [k for k in after if k.startswith("gen.blocks.unet.")]
    assert len(unet) > 50
    for k in unet:
        assert torch.equal(after[k], before[k]), k
    for k in ("gen.blocks.bssfp.conv.weight", "gen.blocks.bssfp.bn.weight", "gen.blocks.bssfp.bn.bias",
              "discr.d1.bssfp.conv.weight", "discr.d2.conv.weight", "discr.d5.bn.weight", "discr.final.weight"):
        assert not torch.equal(after[k], before[k]), k
    for k in after:                                                             # the heads that are not selected stay unused
        if k.startswith(("gen.blocks.dwi-tensor.", "discr.d1.dwi-tensor.")):
            assert torch.equal(after[k], before[k]), k
    assert all(p.grad is None and not p.requires_grad for p in model.gen.blocks["unet"].parameters())
    assert not any(any(f) for f in flags)                                       # after EVERY step, not only the last
    assert all(p.requires_grad for p in model.gen.blocks["bssfp"].parameters())
    assert all(p.requires_grad for p in model.discr.parameters())
    frozen = {id(p) for p in model.gen.blocks["unet"].parameters()}
    for o in model.optimizers():
        assert not any(id(p) in frozen for g in o.param_groups for p in g["params"])
        assert o.param_groups[0]["lr"] == model.lr


def test_transfer_steps_equal_an_independent_loop():
    """bounds of test_gan_harness_with_oracle_modules_matches_oracle_step: logs rel 1e-6, parameters rtol 1e-5 / atol 1e-7"""
    model, _, logs, ref_logs, loop, _ = _transfer_run()
    for step in range(2):
        for k in LOG_NAMES:
            assert logs[step][k] == pytest.approx(ref_logs[step][k], rel=1e-6), (step, k)
    for net, ref in ((model.gen, loop.gen), (model.discr, loop.discr)):
        for (n, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
            assert torch.allclose(p, q, rtol=1e-5, atol=1e-7), n


def test_fine_tune_at_the_models_rate_equals_the_plain_step():
    plain, tuned = _oracle_model("bssfp", seed=3), _oracle_model("bssfp", seed=3)
    tuned.change_training_state(TrainingState.FINE_TUNE, lr=tuned.lr)
    assert _oracle_model("bssfp").change_training_state(TrainingState.FINE_TUNE).optimizers()[0].param_groups[0]["lr"] == 1e-5
    batch = synthetic_batch(2, 32, seed=9)
    for step in range(2):
        plain.training_step(batch, step)
        tuned.training_step(batch, step)
    for (n, p), (_, q) in zip(plain.named_parameters(), tuned.named_parameters()):
        assert torch.equal(p, q), n
    assert all(p.requires_grad for p in tuned.parameters()) and all(p.requires_grad for p in plain.parameters())


def test_modality_switch_selects_heads():
    model = _oracle_model("dwi-tensor")
    head, d1 = model.gen.blocks["dwi-tensor"], model.discr.d1["dwi-tensor"]
    model.change_training_state(TrainingState.TRANSFER, "t1w")
    assert model.input_modality == model.gen.input_modality == model.discr.modality == "t1w"
    assert model.gen.blocks[model.gen.input_modality] is head and model.discr.d1[model.discr.modality] is d1    # the shared 6-channel head
    model.change_training_state(TrainingState.TRANSFER, "bssfp")
    assert model.input_modality == model.gen.input_modality == model.discr.modality == "bssfp"
    assert model.gen.blocks["bssfp"] is not head and model.discr.d1["bssfp"] is not d1
    assert model.gen.blocks["bssfp"].conv.weight.shape[1] == 24 and model.discr.d1["bssfp"].conv.weight.shape[1] == 30
    assert model.unpack_batch(synthetic_batch(1, 8, seed=0))[0].shape[1] == 24


# ---- checkpoints and file names (tiny networks) -----------------------------------------------------------------------------------

def _tiny_model(modality="dwi-tensor", seed=0, **kw):
    torch.manual_seed(seed)
    return bSSFPToDWITensorModel(modality, gen=TinyGenerator(modality), discr=TinyDiscriminator(modality),
                                 optimizer_class=torch.optim.AdamW, batch_size=2, **kw).train()


def _tiny_kw(modality="dwi-tensor"):
    return dict(gen=TinyGenerator(modality), discr=TinyDiscriminator(modality), optimizer_class=torch.optim.AdamW)


@pytest.fixture
def cpu_metrics(monkeypatch):
    from unet_bssfp_amd import metrics
    monkeypatch.setattr(metrics, "reference_metric_fns", lambda: [])           # the metric kernels run on the GPU only


def test_checkpoint_round_trip_of_the_state(tmp_path):
    model = _tiny_model().change_training_state(TrainingState.TRANSFER, "bssfp")
    for i, batch in enumerate(TinyQueue("bssfp", 4, seed=1).batches(2)):
        model.training_step(batch, i)
    path = str(tmp_path / "t.ckpt")
    checkpoint.save_checkpoint(model, path, epoch=3)
    hp = torch.load(path, weights_only=True)["hyper_parameters"]               # plain types only
    assert hp["training_state"] == "TrainingState.TRANSFER" and type(hp["training_state"]) is str and hp["input_modality"] == "bssfp"
    back, info = checkpoint.load_from_checkpoint(path, **_tiny_kw())
    assert back.training_state is TrainingState.TRANSFER and back.input_modality == back.gen.input_modality == "bssfp"
    assert back.discr.modality == "bssfp" and back.stage_lr == model.lr and info["epoch"] == 3
    assert not any(p.requires_grad for p in back.gen.blocks["unet"].parameters())
    assert all(p.requires_grad for p in back.gen.blocks["bssfp"].parameters())
    for (k, v), (_, w) in zip(model.state_dict().items(), back.state_dict().items()):
        assert torch.equal(v, w), k
    for o, q in zip(model.optimizers(), back.optimizers()):                     # the same stage: its moments come back
        assert len(o.state) == len(q.state) > 0 and len(q.param_groups[0]["params"]) == len(o.param_groups[0]["params"])
        for s, t in zip(o.state.values(), q.state.values()):
            assert torch.equal(s["exp_avg"], t["exp_avg"])
    # the next stage from the same file: weights loaded, everything trainable, fresh optimisers at the thesis's rate
    nxt, _ = checkpoint.load_from_checkpoint(path, training_state=TrainingState.FINE_TUNE, **_tiny_kw())
    assert nxt.training_state is TrainingState.FINE_TUNE and nxt.input_modality == "bssfp" and nxt.stage_lr == 1e-5
    assert all(p.requires_grad for p in nxt.parameters())
    assert all(len(o.state) == 0 and o.param_groups[0]["lr"] == 1e-5 for o in nxt.optimizers())
    assert torch.equal(nxt.gen.blocks["unet"][0].weight, model.gen.blocks["unet"][0].weight)
    other, _ = checkpoint.load_from_checkpoint(path, training_state="TRANSFER", input_modality="t1w", **_tiny_kw())
    assert other.input_modality == other.gen.input_modality == other.discr.modality == "t1w"
    assert all(len(o.state) == 0 for o in other.optimizers())
    plain, _ = checkpoint.load_from_checkpoint(path, training_state=None, **_tiny_kw())
    assert plain.training_state is None and all(p.requires_grad for p in plain.parameters())


def test_a_file_without_the_key_loads_as_before(tmp_path):
    model = _tiny_model("bssfp")
    for i, batch in enumerate(TinyQueue("bssfp", 2, seed=1).batches(2)):
        model.training_step(batch, i)
    path = str(tmp_path / "plain.ckpt")
    checkpoint.save_checkpoint(model, path)
    hp = torch.load(path, weights_only=True)["hyper_parameters"]
    assert sorted(hp) == sorted(checkpoint.HPARAM_KEYS)                          # no state: the file is what it was
    back, _ = checkpoint.load_from_checkpoint(path, **_tiny_kw("bssfp"))
    assert back.training_state is None and back.stage_version == 0 and all(p.requires_grad for p in back.parameters())
    assert all(len(o.state) > 0 for o in back.optimizers())


def test_checkpoint_file_names_carry_the_state(tmp_path, cpu_metrics):
    model = _tiny_model().change_training_state(TrainingState.TRANSFER, "pc-bssfp")
    mc = ModelCheckpoint(str(tmp_path), stamp="")
    Trainer(max_epochs=1, callbacks=[mc], graph=False).fit(model, TinyQueue("pc-bssfp", 2, 1), TinyQueue("pc-bssfp", 2, 2))
    name = os.path.basename(mc.best_model_path)
    assert name.startswith("TrainingState.TRANSFER-pc-bssfp-epoch=00-val_loss=") and name.endswith(".ckpt")
    assert os.path.exists(mc.best_model_path)
    plain = ModelCheckpoint(str(tmp_path), stamp="")
    Trainer(max_epochs=1, callbacks=[plain], graph=False).fit(_tiny_model("bssfp"), TinyQueue("bssfp", 2, 1), TinyQueue("bssfp", 2, 2))
    assert os.path.basename(plain.best_model_path).startswith("bssfp-epoch=00-val_loss=")


def test_resume_inside_a_stage_and_the_state_mismatch_error(tmp_path, cpu_metrics):
    model = _tiny_model().change_training_state(TrainingState.TRANSFER, "bssfp")
    mc = ModelCheckpoint(str(tmp_path), save_last=True, stamp="")
    Trainer(max_epochs=1, callbacks=[mc], graph=False).fit(model, TinyQueue("bssfp", 4, 1), TinyQueue("bssfp", 2, 2))
    last = str(tmp_path / "last.ckpt")
    again = _tiny_model(seed=7).change_training_state(TrainingState.TRANSFER, "bssfp")
    trainer = Trainer(max_epochs=2, callbacks=[ModelCheckpoint(str(tmp_path / "b"), stamp="")], graph=False)
    trainer.fit(again, TinyQueue("bssfp", 4, 1), TinyQueue("bssfp", 2, 2), ckpt_path=last)
    assert [h["epoch"] for h in trainer.history][-1] == 1
    frozen = {id(p) for p in again.gen.blocks["unet"].parameters()}
    g_opt = again.optimizers()[0]
    assert len(g_opt.state) > 0 and not any(id(p) in frozen for p in g_opt.state)
    assert int(next(iter(g_opt.state.values()))["step"]) == 4                   # 2 restored + 2 of the second epoch
    for (k, v), (_, w) in zip(model.gen.blocks["unet"].state_dict().items(), again.gen.blocks["unet"].state_dict().items()):
        assert torch.equal(v, w), k
    for wrong in (_tiny_model("bssfp"), _tiny_model().change_training_state(TrainingState.FINE_TUNE, "bssfp")):
        with pytest.raises(RuntimeError, match="training state"):
            Trainer(max_epochs=2, graph=False).fit(wrong, TinyQueue("bssfp", 4, 1), TinyQueue("bssfp", 2, 2), ckpt_path=last)


def test_train_staged_runs_three_stages_from_best_to_best(tmp_path, cpu_metrics):
    from unet_bssfp_amd.train import train_staged
    torch.manual_seed(0)
    seen = []

    def queues(state, modality):
        seen.append((state, modality))
        return TinyQueue(modality, 4, seed=1), TinyQueue(modality, 2, seed=2)

    paths = train_staged(queues, "bssfp", str(tmp_path), max_epochs={"PRETRAIN": 2, "TRANSFER": 2, "FINE_TUNE": 1}, device="cpu",
                         batch_size=2, **_tiny_kw())
    assert seen == [(TrainingState.PRETRAIN, "dwi-tensor"), (TrainingState.TRANSFER, "bssfp"), (TrainingState.FINE_TUNE, "bssfp")]
    assert len(paths) == 3 and all(os.path.exists(p) for p in paths)
    names = [os.path.basename(p) for p in paths]
    assert names[0].startswith("TrainingState.PRETRAIN-dwi-tensor-") and names[1].startswith("TrainingState.TRANSFER-bssfp-")
    assert names[2].startswith("TrainingState.FINE_TUNE-bssfp-")
    ckpts = [torch.load(p, weights_only=True) for p in paths]
    assert [c["hyper_parameters"]["training_state"] for c in ckpts] == [str(s) for s in TrainingState]
    unet = [{k: v for k, v in c["state_dict"].items() if k.startswith("gen.blocks.unet.")} for c in ckpts]
    for k in unet[0]:                                                           # TRANSFER started from PRETRAIN's best and froze it
        assert torch.equal(unet[0][k], unet[1][k]), k
    assert any(not torch.equal(unet[1][k], unet[2][k]) for k in unet[1])        # FINE_TUNE trains the body again
    head = "gen.blocks.bssfp.conv.weight"
    assert not torch.equal(ckpts[0]["state_dict"][head], ckpts[1]["state_dict"][head])
    # stages listed individually: resume the workflow at TRANSFER from a given checkpoint
    more = train_staged(queues, "t1w", str(tmp_path / "again"), stages=["TRANSFER"], ckpt_path=paths[0], max_epochs=1, device="cpu",
                        batch_size=2, **_tiny_kw())
    assert len(more) == 1 and os.path.basename(more[0]).startswith("TrainingState.TRANSFER-t1w-")
    with pytest.raises(ValueError, match="stages"):
        train_staged(queues, "bssfp", str(tmp_path), stages=["FINE_TUNE", "TRANSFER"], device="cpu", **_tiny_kw())


# ---- two gloo ranks in TRANSFER ---------------------------------------------------------------------------------------------------

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker_transfer(rank, world, port, q):
    sys.path.insert(0, ROOT)
    from unet_bssfp_amd import ddp
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        torch.manual_seed(rank)                            # ranks start different; attach() broadcasts rank 0
        gen, discr = R.RefGenerator("dwi-tensor", dropout=0.0).train(), R.RefDiscriminator("dwi-tensor").train()
        model = bSSFPToDWITensorModel("dwi-tensor", gen=gen, discr=discr, optimizer_class=torch.optim.AdamW, lr=1e-3)
        ddp.attach(model)                                  # attached BEFORE the state change: the exchange must be rebuilt
        model.change_training_state(TrainingState.TRANSFER, "bssfp")
        frozen = list(gen.blocks["unet"].parameters())
        before = [p.detach().clone() for p in frozen]
        counts = [sum(b.numel for b in s.buckets) for s in (model.grad_sync_gen, model.grad_sync_discr)]
        want = [sum(p.numel() for p in gen.blocks["bssfp"].parameters()),
                sum(p.numel() for p in ddp.used_parameters(discr, "bssfp"))]
        assert counts == want, (counts, want)
        batch = synthetic_batch(2, 32, seed=50 + rank)
        logs = {}
        model._phase_gen(batch, logs)                      # training_step, with a look at the averaged gradients in between
        model._finish_grads("gen")
        grads = {n: p.grad.detach().clone() for n, p in gen.blocks["bssfp"].named_parameters()}
        assert all(p.grad is None for p in frozen)
        model._phase_gen_update_discr(batch, logs)
        model._finish_grads("discr")
        model._phase_discr_update()
        untouched = all(torch.equal(p, b) for p, b in zip(frozen, before)) and all(p.grad is None for p in frozen)
        digest = torch.stack([p.detach().double().sum() for p in model.parameters()])
        gathered = [torch.zeros_like(digest) for _ in range(world)]
        dist.all_gather(gathered, digest)
        assert all(torch.equal(g, gathered[0]) for g in gathered), "ranks diverged after the step"
        # as numpy arrays: pickled by value.  A tensor crosses the queue as a file descriptor served by THIS process, which may be
        # gone (destroy_process_group, exit) before the parent unpickles it: FileNotFoundError in q.get, now and then
        q.put((rank, "ok" if untouched else "FAIL: a frozen parameter moved", {n: g.numpy() for n, g in grads.items()}))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, f"FAIL: {e!r} {traceback.format_exc()}", None))
    finally:
        dist.destroy_process_group()


def test_transfer_on_two_gloo_ranks_exchanges_the_trainable_set_only():
    """as test_cpu_ddp.test_gan_step_data_parallel_matches_single_process_gloo: the averaged head gradients against a
    single-process emulation (rank 0's weights, per-rank batches and BatchNorm statistics), that file's bound (rtol 1e-5, atol 1e-7)"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_transfer, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
    assert all(r[1] == "ok" for r in res), [r[1] for r in res]
    threads = torch.get_num_threads()
    torch.set_num_threads(2)                              # as the workers: the bound is no allowance for another summation order
    try:
        total = _single_process_head_gradients()
    finally:
        torch.set_num_threads(threads)
    for n, want in total.items():
        for r in range(2):
            torch.testing.assert_close(torch.from_numpy(res[r][2][n]), want / 2, rtol=1e-5, atol=1e-7, msg=lambda m: f"rank {r} {n}: {m}")


def _single_process_head_gradients():
    """sum over the two ranks' batches of the generator-phase head gradients: rank 0's weights, per-rank BatchNorm statistics"""
    torch.manual_seed(0)
    gen, discr = R.RefGenerator("dwi-tensor", dropout=0.0).train(), R.RefDiscriminator("dwi-tensor").train()
    gen.input_modality = discr.modality = "bssfp"
    for p in list(discr.parameters()) + list(gen.blocks["unet"].parameters()):
        p.requires_grad_(False)
    total = None
    for r in range(2):
        d_r = copy.deepcopy(discr)                        # BatchNorm buffers are per rank
        x, y = R.synthetic_batch(2, 32, seed=50 + r)
        y_hat = gen(x)
        logits = d_r(x, y_hat)
        adv = torch.nn.functional.binary_cross_entropy_with_logits(logits, torch.ones_like(logits))
        gen.zero_grad()
        (adv + torch.nn.functional.l1_loss(y_hat, y) * 100.0).backward()
        assert all(p.grad is None for p in gen.blocks["unet"].parameters())
        g = {n: p.grad.clone() for n, p in gen.blocks["bssfp"].named_parameters()}
        total = g if total is None else {n: total[n] + g[n] for n in g}
    return total
