"""Host side of the fit loop (unet_bssfp_amd.trainer): the callback rules, epoch statistics on CPU tensors, checkpoints and
resume, and the patch queue's state at an epoch boundary.  No network runs a step here (a CPU oracle step at 32^3 takes over
10 s): the model is a ``bSSFPToDWITensorModel`` subclass with one-layer ``gen`` / ``discr`` whose steps set ``last_logs`` from a
script, and the queues yield dicts.  Lightning is absent, so parity with it is **unpinned**: these tests pin the rules the
docstrings of ``trainer.py`` state.
"""
import io
import json
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from unet_bssfp_amd import checkpoint
from unet_bssfp_amd.gan import bSSFPToDWITensorModel
from unet_bssfp_amd.trainer import EarlyStopping, EpochStats, ModelCheckpoint, Trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class StubQueue:
    """``n`` patches per epoch; batch ``i`` (counted over the queue's life) carries the value ``i``"""

    def __init__(self, n):
        self.n, self.count = n, 0

    def __len__(self):
        return self.n

    def batches(self, batch_size, **kw):
        left = self.n
        while left > 0:
            size = min(batch_size, left)
            left -= size
            self.count += 1
            yield {"v": torch.tensor(float(self.count)), "size": size}

    def state_dict(self):
        return {"count": self.count}

    def load_state_dict(self, state):
        self.count = int(state["count"])


class StubModel(bSSFPToDWITensorModel):
    """training_step: logs the batch's value and moves a weight by it; validation_step: logs the script's entry for the
    validation epoch (counted in a buffer of ``gen``, so that a checkpoint carries it)"""

    def __init__(self, script, batch_size=2, val_batches=1):
        gen, discr = torch.nn.Linear(2, 2), torch.nn.Linear(2, 1)
        gen.register_buffer("calls", torch.zeros(2, dtype=torch.long))
        super().__init__("bssfp", gen=gen, discr=discr, optimizer_class=torch.optim.AdamW, batch_size=batch_size)
        self.script, self.val_batches = script, val_batches

    def training_step(self, batch, batch_idx=0):
        assert self.training
        with torch.no_grad():
            self.gen.weight.add_(batch["v"] * 0.125)
            self.gen.calls[0] += 1
        self.last_logs = {"train_gen_loss": batch["v"].clone(), "train_discr_loss": (batch["v"] * 2).to(torch.float64)}

    def validation_step(self, batch, batch_idx=0):
        assert not self.training and not torch.is_grad_enabled()
        epoch = int(self.gen.calls[1]) // self.val_batches
        self.gen.calls[1] += 1
        self.last_logs = {k: torch.tensor(float(v[epoch])) for k, v in self.script.items()}


def _fit(tmp_path, script, max_epochs, callbacks, train_n=5, ckpt_path=None, log_path=None):
    torch.manual_seed(0 if ckpt_path is None else 1)             # (a resumed model's own initialisation must not matter)
    model = StubModel(script)
    tq, vq = StubQueue(train_n), StubQueue(2)
    trainer = Trainer(max_epochs=max_epochs, callbacks=callbacks, log_path=log_path)
    trainer.fit(model, tq, vq, ckpt_path=ckpt_path)
    return trainer, model


def f32(v) -> float:
    """the script's value as the step logs it: scalars travel as float32"""
    return float(torch.tensor(v, dtype=torch.float32))


def _files(d):
    return sorted(f for f in os.listdir(d) if f.endswith(".ckpt"))


# ---- callbacks: the worked examples of the docstrings ---------------------------------------------------------------------

def test_early_stopping_worked_example(tmp_path):
    es = EarlyStopping(patience=3)
    assert (es.monitor, es.mode, es.min_delta, es.check_finite) == ("val_gen_loss_recon", "min", 0.0, True)
    script = {"val_gen_loss_recon": [5, 4, 4, 4.5, 4, 1, 1, 1, 1, 1], "val_loss": [1] * 10}
    trainer, model = _fit(tmp_path, script, 10, [es])
    assert es.stopped_epoch == 4 and trainer.current_epoch == 4 and trainer.should_stop
    assert [h["epoch"] for h in trainer.history] == [0, 1, 2, 3, 4]            # five epochs run
    assert es.best_score == 4.0 and es.wait_count == 3
    assert trainer.global_step == 5 * 3 * 2                                    # 3 batches per epoch, two optimiser steps each
    assert model.training                                                      # validation leaves the model in train mode


def test_early_stopping_max_mode_and_min_delta(tmp_path):
    es = EarlyStopping("val_loss", patience=2, mode="max", min_delta=0.5)
    trainer, _ = _fit(tmp_path, {"val_loss": [1.0, 1.4, 1.5, 1.7, 9.0]}, 5, [es])
    assert es.stopped_epoch == 2 and es.best_score == 1.0 and len(trainer.history) == 3     # 1.4 and 1.5 do not beat 1.0 + 0.5


def test_model_checkpoint_worked_example(tmp_path):
    mc = ModelCheckpoint(str(tmp_path), save_top_k=2, stamp="S")
    assert (mc.monitor, mc.mode) == ("val_loss", "min")
    trainer, _ = _fit(tmp_path, {"val_loss": [0.5, 0.3, 0.4, 0.2, 0.6]}, 5, [mc])
    e1, e3 = "bssfp-epoch=01-val_loss=0.3000S.ckpt", "bssfp-epoch=03-val_loss=0.2000S.ckpt"
    assert _files(tmp_path) == [e1, e3]
    assert mc.best_model_path == str(tmp_path / e3) and mc.best_model_score == f32(0.2)
    assert mc.best_k_models == {str(tmp_path / e1): f32(0.3), str(tmp_path / e3): f32(0.2)}
    assert len(trainer.history) == 5


def test_default_stamp_is_the_construction_time(tmp_path):
    import datetime
    before = datetime.datetime.now()
    mc = ModelCheckpoint(str(tmp_path))
    assert mc.save_top_k == 10
    assert before <= datetime.datetime.fromisoformat(mc.stamp) <= datetime.datetime.now()
    _fit(tmp_path, {"val_loss": [0.25]}, 1, [mc])
    assert _files(tmp_path) == [f"bssfp-epoch=00-val_loss=0.2500{mc.stamp}.ckpt"]      # src/eval.py:335-338


def test_model_checkpoint_runs_after_early_stopping_and_nan_counts_as_inf(tmp_path):
    mc = ModelCheckpoint(str(tmp_path), save_top_k=1, stamp="")
    es = EarlyStopping("val_loss", patience=10)
    trainer, _ = _fit(tmp_path, {"val_loss": [float("nan"), 0.5, 0.25]}, 3, [mc, es])
    assert trainer.callbacks == [es, mc]
    # NaN with check_finite stops that epoch; the checkpoint of that epoch is still written, scored +inf
    assert es.stopped_epoch == 0 and len(trainer.history) == 1
    assert list(mc.best_k_models.values()) == [math.inf] and _files(tmp_path) == ["bssfp-epoch=00-val_loss=nan.ckpt"]
    ckpt = torch.load(mc.best_model_path, weights_only=True)
    assert ckpt["callbacks"]["EarlyStopping"]["stopped_epoch"] == 0          # the stop decision is in the file: it ran first


def test_nan_monitor_stops_that_epoch_and_is_beaten_by_any_number(tmp_path):
    es = EarlyStopping("val_gen_loss_recon", patience=10)
    mc = ModelCheckpoint(str(tmp_path), save_top_k=1, stamp="")
    script = {"val_gen_loss_recon": [1.0, float("nan"), 0.5], "val_loss": [float("nan"), 0.5, 0.1]}
    trainer, _ = _fit(tmp_path, script, 3, [es, mc])
    assert es.stopped_epoch == 1 and [h["epoch"] for h in trainer.history] == [0, 1]
    assert math.isnan(trainer.history[1]["val_gen_loss_recon"]) and trainer.history[1]["nonfinite"] == {"val_gen_loss_recon": 1}
    assert _files(tmp_path) == ["bssfp-epoch=01-val_loss=0.5000.ckpt"] and mc.best_model_score == 0.5
    es2 = EarlyStopping("val_gen_loss_recon", patience=10, check_finite=False)
    trainer2, _ = _fit(tmp_path, script, 3, [es2])
    assert len(trainer2.history) == 3 and es2.wait_count == 0 and es2.best_score == 0.5


def test_missing_monitor_raises(tmp_path):
    with pytest.raises(RuntimeError, match="val_gen_loss_recon"):
        _fit(tmp_path, {"val_loss": [1.0]}, 1, [EarlyStopping()])
    with pytest.raises(RuntimeError, match="val_loss"):
        _fit(tmp_path, {"val_gen_loss_recon": [1.0]}, 1, [ModelCheckpoint(str(tmp_path))])


def test_repeated_name_gets_a_version_suffix(tmp_path):
    for _ in range(3):
        _fit(tmp_path, {"val_loss": [0.5]}, 1, [ModelCheckpoint(str(tmp_path), stamp="T")])
    base = "bssfp-epoch=00-val_loss=0.5000T"
    assert _files(tmp_path) == sorted([base + ".ckpt", base + "-v1.ckpt", base + "-v2.ckpt"])


def test_callback_metrics_history_and_log_file(tmp_path):
    log = str(tmp_path / "log.jsonl")
    trainer, _ = _fit(tmp_path, {"val_loss": [0.5, 0.25]}, 2, [], train_n=5, log_path=log)
    # epoch 1: batches 4, 5, 6 of the queue, the ragged one included with the same weight (the plain mean over batches)
    assert trainer.callback_metrics == {"train_gen_loss": 5.0, "train_gen_loss_epoch": 5.0, "train_discr_loss": 10.0,
                                        "train_discr_loss_epoch": 10.0, "val_loss": 0.25}
    assert trainer.history[0] == {"epoch": 0, "global_step": 6, "train_gen_loss": 2.0, "train_discr_loss": 4.0, "val_loss": 0.5,
                                  "nonfinite": {}}
    assert [json.loads(line) for line in open(log)] == trainer.history
    dropped = Trainer(max_epochs=1, drop_last=True)
    q = StubQueue(5)
    dropped.fit(StubModel({"val_loss": [0.0]}), q)
    assert dropped.history[0]["train_gen_loss"] == 1.5 and dropped.global_step == 4 and q.count == 3


def test_log_file_is_strict_json_for_a_non_finite_mean(tmp_path):
    log = str(tmp_path / "log.jsonl")
    trainer, _ = _fit(tmp_path, {"val_loss": [float("nan"), float("inf")]}, 2, [], log_path=log)
    assert math.isnan(trainer.history[0]["val_loss"]) and trainer.history[1]["val_loss"] == math.inf     # history keeps the numbers

    def refuse(name):
        raise ValueError(name)
    lines = [json.loads(line, parse_constant=refuse) for line in open(log)]   # a strict reader: no NaN / Infinity tokens
    assert [e["val_loss"] for e in lines] == [None, None] and [e["nonfinite"] for e in lines] == [{"val_loss": 1}] * 2
    assert lines[0]["train_gen_loss"] == 2.0


def _worker_fit(rank, world, port, q, dirpath):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        open(os.path.join(dirpath, "bssfp-epoch=00-val_loss=0.5000N.ckpt"), "a").close()      # the first name is taken
        dist.barrier()
        mc = ModelCheckpoint(dirpath, save_top_k=2, stamp="N")
        trainer = Trainer(max_epochs=2, callbacks=[mc])
        torch.manual_seed(0)
        trainer.fit(StubModel({"val_loss": [0.5, 0.25]}), StubQueue(5), StubQueue(2))
        uneven = None
        try:
            Trainer(max_epochs=1).fit(StubModel({"val_loss": [0.5]}), StubQueue(5), StubQueue(2) if rank == 0 else None)
        except ValueError as e:
            uneven = str(e)
        q.put((rank, sorted(mc.best_k_models), mc.best_model_path, trainer.history, uneven))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, f"FAIL: {e!r} {traceback.format_exc()}", None, None, None))
    finally:
        dist.destroy_process_group()


def test_two_ranks_agree_on_checkpoint_names_and_on_queue_lengths_gloo(tmp_path):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_fit, args=(r, 2, port, q, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert all(not isinstance(r[1], str) for r in res), res
    names = [str(tmp_path / "bssfp-epoch=00-val_loss=0.5000N-v1.ckpt"), str(tmp_path / "bssfp-epoch=01-val_loss=0.2500N.ckpt")]
    assert res[0][1] == res[1][1] == names and res[0][2] == res[1][2] == names[1]      # chosen on rank 0, the same everywhere
    assert res[0][3] == res[1][3] and res[0][3][0]["train_gen_loss"] == 2.0              # both ranks: the means of the union
    assert all("differ in length" in r[4] for r in res)                                # a validation queue on one rank only
    assert _files(tmp_path) == sorted(os.path.basename(n) for n in names + [names[0].replace("-v1", "")])


# ---- epoch statistics ------------------------------------------------------------------------------------------------------

def test_epoch_stats_on_cpu_against_a_python_f64_loop():
    g = torch.Generator().manual_seed(0)
    keys = ["a", "b", "c"]
    stats = EpochStats(keys, "cpu")
    weights = [2.0, 0.0, 0.5, 3.25, 8.0]
    want, total = dict.fromkeys(keys, 0.0), 0.0
    for w in weights:
        vals = ((torch.rand(3, generator=g) - 0.5) * 1e3).float()
        logs = {"a": vals[0], "b": vals[1].double(), "c": vals[::2][1]}           # f64 and a strided view: converted with .float()
        stats.add(logs, w)
        for k in keys:
            want[k] += w * float(logs[k].float())
        total += w
    stats.reduce(None)                                                          # world size 1: nothing to do
    means, bad = stats.means()
    assert means == {k: want[k] / total for k in keys} and bad == dict.fromkeys(keys, 0)
    assert float(stats.acc[3]) == total
    stats.add({"a": torch.tensor(float("inf")), "b": torch.tensor(1.0), "c": torch.tensor(float("nan"))}, 1.0)
    means, bad = stats.means()
    assert means["a"] == math.inf and math.isnan(means["c"]) and math.isfinite(means["b"]) and bad == {"a": 1, "b": 0, "c": 1}
    with pytest.raises(ValueError, match="keys changed"):
        stats.add({"a": torch.tensor(1.0), "b": torch.tensor(1.0)}, 1.0)
    stats.reset()
    assert float(stats.acc.abs().sum()) == 0.0
    with pytest.raises(ValueError):
        EpochStats(["k%d" % i for i in range(33)], "cpu")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker_reduce(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    from unet_bssfp_amd.trainer import EpochStats as Stats
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        stats = Stats(["x", "y"], "cpu")
        for i in range(2 + rank):                                  # rank 0: two batches, rank 1: three
            stats.add({"x": torch.tensor(float(10 * rank + i)), "y": torch.tensor(float("nan") if (rank, i) == (1, 2) else 1.0)}, 4.0)
        stats.reduce(None)
        q.put((rank, stats.means()))
    except Exception as e:  # noqa: BLE001
        q.put((rank, f"FAIL: {e!r}"))
    finally:
        dist.destroy_process_group()


def test_epoch_stats_reduce_gives_every_rank_the_means_of_the_union_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_reduce, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    for rank, got in res:
        assert not isinstance(got, str), got
        means, bad = got
        assert means["x"] == (0 + 1 + 10 + 11 + 12) / 5 and math.isnan(means["y"]) and bad == {"x": 0, "y": 1}, (rank, got)


# ---- checkpoints and resume ------------------------------------------------------------------------------------------------

SCRIPT = {"val_loss": [0.5, 0.3, 0.4, 0.2], "val_gen_loss_recon": [5.0, 4.0, 4.0, 4.5]}


def _callbacks(d):
    return [EarlyStopping(patience=3), ModelCheckpoint(str(d), save_top_k=2, save_last=True, stamp="R")]


def test_trainer_checkpoint_loads_weights_only_and_through_load_checkpoint(tmp_path):
    trainer, model = _fit(tmp_path, SCRIPT, 2, _callbacks(tmp_path))
    path = str(tmp_path / "last.ckpt")
    ckpt = torch.load(path, weights_only=True)
    assert ckpt["epoch"] == 1 and ckpt["global_step"] == 12 and ckpt["pytorch-lightning_version"] == checkpoint.LIGHTNING_VERSION
    assert sorted(ckpt["callbacks"]) == ["EarlyStopping", "ModelCheckpoint"]
    assert ckpt["callbacks"]["EarlyStopping"] == {"best_score": 4.0, "wait_count": 0, "stopped_epoch": 0, "patience": 3}
    assert ckpt["callbacks"]["ModelCheckpoint"]["best_model_score"] == f32(0.3)
    assert ckpt["mi355"]["train_queue"] == {"count": 6} and ckpt["mi355"]["val_queue"] == {"count": 2}
    fresh = StubModel(SCRIPT)
    info = checkpoint.load_checkpoint(fresh, path)
    assert info["epoch"] == 1 and info["global_step"] == 12 and info["ignored_keys"] == []
    for (k, a), (_, b) in zip(model.state_dict().items(), fresh.state_dict().items()):
        assert torch.equal(a, b), k


def test_resume_equals_the_uninterrupted_run(tmp_path):
    whole, parts = tmp_path / "whole", tmp_path / "parts"
    t_whole, m_whole = _fit(whole, SCRIPT, 4, _callbacks(whole))
    _fit(parts, SCRIPT, 2, _callbacks(parts))
    cbs = _callbacks(parts)
    t_res, m_res = _fit(parts, SCRIPT, 4, cbs, ckpt_path=str(parts / "last.ckpt"))
    assert t_res.history == t_whole.history and [h["epoch"] for h in t_res.history] == [0, 1, 2, 3]
    assert t_res.global_step == t_whole.global_step == 24 and t_res.callback_metrics == t_whole.callback_metrics
    assert cbs[0].state_dict() == t_whole.callbacks[0].state_dict()
    rel = lambda cb, d: {os.path.relpath(p, d): s for p, s in cb.best_k_models.items()}      # noqa: E731
    assert rel(cbs[1], parts) == rel(t_whole.callbacks[1], whole)
    assert os.path.relpath(cbs[1].best_model_path, parts) == os.path.relpath(t_whole.callbacks[1].best_model_path, whole)
    assert cbs[1].best_model_score == t_whole.callbacks[1].best_model_score == f32(0.2)
    assert _files(parts) == _files(whole) == ["bssfp-epoch=01-val_loss=0.3000R.ckpt", "bssfp-epoch=03-val_loss=0.2000R.ckpt", "last.ckpt"]
    for (k, a), (_, b) in zip(m_whole.state_dict().items(), m_res.state_dict().items()):
        assert torch.equal(a, b), k


def test_resume_from_a_file_without_trainer_state_warns_and_starts_fresh(tmp_path):
    model = StubModel(SCRIPT)
    path = str(tmp_path / "plain.ckpt")
    checkpoint.save_checkpoint(model, path, epoch=0, global_step=6)
    es = EarlyStopping(patience=3)
    trainer = Trainer(max_epochs=2, callbacks=[es])
    with pytest.warns(UserWarning, match="start fresh"):
        trainer.fit(StubModel(SCRIPT), StubQueue(5), StubQueue(2), ckpt_path=path)
    assert [h["epoch"] for h in trainer.history] == [1] and trainer.global_step == 12 and es.best_score == 5.0


# ---- the patch queue's state at an epoch boundary --------------------------------------------------------------------------

def _patch_queue(seed):
    from unet_bssfp_amd import augment as A
    from unet_bssfp_amd import data as Q
    subs = [{"bssfp": {"data": torch.zeros(24, 1, 1, 1)}, "dwi-tensor": {"data": torch.zeros(6, 1, 1, 1)}} for _ in range(3)]
    return Q.PatchQueue(subs, "bssfp", max_length=4, samples_per_volume=2, sampler=Q.UniformSampler(32),
                        target_shape=(36, 48, 40), transform=A.reference_augmentation(), seed=seed)


def _rows(plan):
    return [(p.load.subject, p.load.epoch, p.load.fill, p.load.seed, p.origin) for p in plan]


def test_patch_queue_state_resumes_the_plan_at_an_epoch_boundary():
    whole = _patch_queue(11)
    epochs = [_rows(whole.next_plan(len(whole))) for _ in range(3)]
    assert [{r[1] for r in e} for e in epochs] == [{0}, {1}, {2}] and epochs[1] != epochs[2]
    first = _patch_queue(11)
    for _ in range(2):
        first.next_plan(len(first))
    state = first.state_dict()
    assert state["epoch"] == 1 and state["fill_count"] == 4 and state["generator"].dtype == torch.uint8
    buf = io.BytesIO()
    torch.save(state, buf)
    state = torch.load(io.BytesIO(buf.getvalue()), weights_only=True)                         # survives a weights_only round trip
    restored = _patch_queue(999)                                                              # another seed: the state decides
    restored.load_state_dict(state)
    assert _rows(restored.next_plan(len(restored))) == epochs[2]
    assert restored.epoch == 2 and restored.fill_count == 6


def test_patch_queue_state_is_refused_in_the_middle_of_an_epoch():
    q = _patch_queue(3)
    q.next_plan(1)
    with pytest.raises(RuntimeError, match="middle of an epoch"):
        q.state_dict()
    with pytest.raises(RuntimeError, match="middle of an epoch"):
        q.load_state_dict({"generator": torch.Generator().get_state(), "epoch": 0, "fill_count": 0})
    q.next_plan(len(q) - 1)
    assert q.state_dict()["epoch"] == 0
