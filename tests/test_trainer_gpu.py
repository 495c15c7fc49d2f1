"""The fit loop on the device (unet_bssfp_amd.trainer): the epoch-statistics kernel (csrc/epoch_stats.hip), the eager loop
against a hand-written one, the graph loop against the eager one bit for bit (the test of
``GraphedTrainingStep(preserve_state=True)``), resume, and the absence of host reads inside an epoch.

Subjects as in test_patch_queue.test_gpu_next_batch_feeds_a_graphed_training_step: raw extents (40, 52, 36) / (36, 44, 44),
target (36, 48, 40), patch 32, 24 + 6 channels; 3 training subjects x 2 samples at batch 4 (one full batch and a ragged tail
of 2), 1 validation subject.  ``DropoutState`` is process-wide: every run is finished and snapshotted before the next
model is built.  Runs that several tests compare against are made once and shared.
"""
import math

import pytest
import torch

from unet_bssfp_amd import _lib, ops
from unet_bssfp_amd.trainer import EarlyStopping, EpochStats, ModelCheckpoint, Trainer

DEV = "cuda:0"
pytestmark = pytest.mark.gpu

WEIGHTS = [1.0, 0.0, 2.5, 0.3, 4.0, 1e-3, 7.75]          # m = 7 calls: a zero, non-integers, inexact decimals


# ---- mi355_epoch_accumulate ------------------------------------------------------------------------------------------------

def _values(n, m, seed):
    """(m, n) float32, magnitudes log-uniform over 1e-8 .. 1e8, both signs"""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(m, n, generator=g, dtype=torch.float64) * 16 - 8)
    sign = torch.where(torch.rand(m, n, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign).float()


def _sources(n):
    """n scalars as views at odd element offsets of one larger tensor; with n > 1 the last slot is the first one's tensor"""
    big = torch.zeros(2 * n + 3, dtype=torch.float32, device=DEV)
    views = [big[2 * k + 1] for k in range(n)]
    if n > 1:
        views[n - 1] = views[0]
    return big, views


def _write(big, n, row):
    host = torch.zeros(big.numel())
    for k in range(n):
        host[2 * k + 1] = row[k]
    big.copy_(host)


def _run_sequence(n, vals, weights):
    big, views = _sources(n)
    table = ops.scalar_table(views)
    acc = torch.zeros(2 * n + 1, dtype=torch.float64, device=DEV)
    for row, w in zip(vals, weights):
        _write(big, n, row)
        ops.epoch_accumulate(table, n, w, acc)
    torch.cuda.synchronize()
    return acc


def _slot_value(row, n, k):
    return float(row[0] if (n > 1 and k == n - 1) else row[k])


@pytest.mark.parametrize("n", [1, 5, 32])
def test_epoch_accumulate_against_a_python_f64_loop(hip, n):
    m = len(WEIGHTS)
    vals = _values(n, m, seed=n)
    acc = _run_sequence(n, vals, WEIGHTS).cpu().tolist()
    total = 0.0
    for w in WEIGHTS:
        total += w
    assert acc[n] == total                                                     # exact: the same f64 additions in the same order
    for k in range(n):
        want, mass = 0.0, 0.0
        for row, w in zip(vals, WEIGHTS):
            want += w * _slot_value(row, n, k)
            mass += abs(w * _slot_value(row, n, k))
        # 2m roundings of acc += w * v, each at most half an ulp of a partial sum no larger than sum |w v|, fma or not
        err, bound = abs(acc[k] - want), m * 2.0 ** -52 * mass
        print(f"n={n} key={k}: |got - want| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (k, acc[k], want)
        assert acc[n + 1 + k] == 0.0


def test_epoch_accumulate_counts_non_finite_values_and_is_bit_identical_between_runs(hip):
    n, m = 5, len(WEIGHTS)
    clean = _values(n, m, seed=77)
    vals = clean.clone()
    vals[2, 1] = float("nan")
    vals[3, 2] = float("inf")
    vals[5, 2] = float("-inf")
    vals[4, 3] = float("-inf")
    weights = [w or 1.0 for w in WEIGHTS]                                      # (0 * inf would be one more NaN: keep the sums telling)
    a, b = _run_sequence(n, vals, weights), _run_sequence(n, vals, weights)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))               # two identical sequences: bit-identical
    ref = _run_sequence(n, clean, weights)
    got = a.cpu().tolist()
    assert got[n + 1:] == [0.0, 1.0, 2.0, 1.0, 0.0]
    assert math.isnan(got[1]) and math.isnan(got[2]) and got[3] == -math.inf   # carried as IEEE arithmetic carries them
    for k in (0, 4, n):                                                        # the other keys and the weight: untouched
        assert got[k] == float(ref[k])


def test_epoch_accumulate_refuses_bad_arguments_before_any_launch(hip):
    big, views = _sources(32)
    big.fill_(3.0)
    table = ops.scalar_table(views)
    acc = torch.arange(67, dtype=torch.float64, device=DEV)
    before = acc.clone()
    for n in (0, 33, -1):
        with pytest.raises(_lib.Mi355Error, match="epoch_accumulate"):
            ops.epoch_accumulate(table, n, 1.0, acc)
    holes = _lib.ScalarTable()
    holes.src[0] = views[0].data_ptr()                                         # slot 1 stays null
    with pytest.raises(_lib.Mi355Error, match="null pointer"):
        ops.epoch_accumulate(holes, 2, 1.0, acc)
    assert hip.mi355_epoch_accumulate(None, 1, 1.0, acc.data_ptr(), None) < 0
    assert hip.mi355_epoch_accumulate(table, 1, 1.0, None, None) < 0
    with pytest.raises(ValueError):
        ops.scalar_table(views + [views[0]])                                   # 33 slots
    with pytest.raises(ValueError):
        ops.epoch_accumulate(table, 32, 1.0, acc[:64])                         # acc too short for 2n + 1
    torch.cuda.synchronize()
    assert torch.equal(acc, before)


def test_epoch_accumulate_captured_once_and_replayed(hip):
    n, w = 5, 2.5
    vals = _values(n, 3, seed=5)
    big, views = _sources(n)
    table = ops.scalar_table(views)
    acc = torch.zeros(2 * n + 1, dtype=torch.float64, device=DEV)
    _write(big, n, vals[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        ops.epoch_accumulate(table, n, w, acc)                                 # the pointer table travels by value: capturable
    torch.cuda.synchronize()
    assert float(acc.abs().sum()) == 0.0                                       # a capture runs nothing
    for row in vals:
        _write(big, n, row)
        graph.replay()
    torch.cuda.synchronize()
    eager = _run_sequence(n, vals, [w] * 3)
    assert torch.equal(acc.view(torch.int64), eager.view(torch.int64))
    assert float(acc[n]) == 7.5


def test_epoch_stats_on_the_device_converts_and_caches(hip):
    stats = EpochStats(["a", "b"], DEV)
    a = torch.tensor([1.5], device=DEV)
    b = torch.tensor(2.0, device=DEV, dtype=torch.float64)                     # not f32: converted with .float()
    for _ in range(3):
        stats.add({"a": a, "b": b}, 4)
    assert len(stats._tables) <= 3
    assert stats.means() == ({"a": 1.5, "b": 2.0}, {"a": 0, "b": 0})
    with pytest.raises(ValueError, match="keys changed"):
        stats.add({"a": a}, 4)


# ---- fit -------------------------------------------------------------------------------------------------------------------

_CACHE = {}


def _subjects():
    if "subjects" not in _CACHE:
        g = torch.Generator().manual_seed(2)
        out = []
        for i in range(4):
            s = [(40, 52, 36), (36, 44, 44)][i % 2]
            out.append({"bssfp": {"data": (torch.rand((24,) + s, generator=g) - 0.3).to(DEV)},
                        "dwi-tensor": {"data": (torch.rand((6,) + s, generator=g) - 0.3).to(DEV)}})
        _CACHE["subjects"] = out
    return _CACHE["subjects"]


def _queues(transform=None):
    from unet_bssfp_amd import data as Q
    subs = _subjects()
    kw = dict(max_length=4, samples_per_volume=2, sampler=Q.UniformSampler(32), target_shape=(36, 48, 40), transform=transform)
    return Q.PatchQueue(subs[:3], "bssfp", seed=17, **kw), Q.PatchQueue(subs[3:], "bssfp", seed=18, **kw)


def _model(seed=4):
    import unet_bssfp_amd as M
    from unet_bssfp_amd.functional import DropoutState
    from unet_bssfp_amd.gan import bSSFPToDWITensorModel
    torch.manual_seed(seed)
    DropoutState.reset()
    gen, discr = M.Generator("bssfp", dropout=0.05), M.Discriminator("bssfp")
    model = bSSFPToDWITensorModel("bssfp", gen=gen.to(DEV), discr=discr.to(DEV), batch_size=4).train()
    DropoutState.base(torch.device(DEV))                     # drawn from the seeded CPU generator here, for every run alike
    return model


def _snapshot(model):
    from unet_bssfp_amd.functional import DropoutState
    torch.cuda.synchronize()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    moments, steps = [], []
    for o in model.optimizers():
        o.sync_step_counts()
        for p in o.param_groups[0]["params"]:
            st = o.state.get(p)
            if st:
                moments += [st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
                steps.append(int(st["step"]))
    return {"state": state, "moments": moments, "steps": steps, "dropout": int(DropoutState.base(torch.device(DEV)).item())}


def _assert_same(a, b):
    assert list(a["state"]) == list(b["state"])
    for k in a["state"]:
        assert torch.equal(a["state"][k], b["state"][k]), k                  # parameters, BatchNorm statistics and counters
    assert len(a["moments"]) == len(b["moments"]) > 0
    for i, (x, y) in enumerate(zip(a["moments"], b["moments"])):
        assert torch.equal(x, y), f"optimiser moment {i}"
    assert a["steps"] == b["steps"] and a["dropout"] == b["dropout"]


def _run(name):
    """2 epochs of the same start, made once: 'eager' and 'graph' through the Trainer, 'hand' through a loop written here"""
    if name in _CACHE:
        return _CACHE[name]
    model = _model()
    tq, vq = _queues()
    if name == "hand":
        history = []
        for epoch in range(2):
            entry = {}

            def account(sums, mass):
                for k, v in model.last_logs.items():                          # host reads, averaged in Python f64
                    sums[k] = sums.get(k, 0.0) + 4 * float(v)                 # weight = model.batch_size, the ragged batch too
                    mass[k] = mass.get(k, 0.0) + abs(4 * float(v))

            sums, mass, batches = {}, {}, 0
            for i, batch in enumerate(tq.batches(4)):
                model.training_step(batch, i)
                account(sums, mass)
                batches += 1
            entry.update({k: (s, mass[k], 4.0 * batches) for k, s in sums.items()})
            model.eval()
            sums, mass, batches = {}, {}, 0
            with torch.no_grad():
                for i, batch in enumerate(vq.batches(4)):
                    model.validation_step(batch, i)
                    account(sums, mass)
                    batches += 1
            model.train()
            entry.update({k: (s, mass[k], 4.0 * batches) for k, s in sums.items()})
            history.append(entry)
        out = (history, _snapshot(model), None)
    else:
        trainer = Trainer(max_epochs=2, graph=name == "graph")
        trainer.fit(model, tq, vq)
        assert (trainer.graphed_step is not None) == (name == "graph")
        out = (trainer.history, _snapshot(model), trainer)
    _CACHE[name] = out
    return out


def test_eager_fit_equals_a_hand_written_loop(hip):
    history, state, trainer = _run("eager")
    want, want_state, _ = _run("hand")
    assert trainer.global_step == 8 and [h["epoch"] for h in history] == [0, 1]
    for got, ref in zip(history, want):
        assert set(ref) == set(got) - {"epoch", "global_step", "nonfinite"} and got["nonfinite"] == {}
        assert "val_gen_loss_recon" in got and "val_loss" in got and "train_discr_loss" in got and "val_metric_SSIM" in got
        for k, (s, mass, total) in ref.items():
            m = round(total / 4)
            # the bound of the accumulate test (m 2^-52 sum |w v|) over sum w
            err, bound = abs(got[k] - s / total), m * 2.0 ** -52 * mass / total
            print(f"{k}: |got - want| = {err:.3e}, bound {bound:.3e}")
            assert err <= bound, (k, got[k], s / total)
    _assert_same(state, want_state)
    assert state["steps"] and set(state["steps"]) == {4}


def test_graph_fit_equals_eager_fit_bit_for_bit(hip):
    history, state, trainer = _run("graph")
    want, want_state, _ = _run("eager")
    assert trainer.global_step == 8
    _assert_same(state, want_state)
    assert history == want


def test_resumed_graph_fit_equals_the_uninterrupted_one(hip, tmp_path):
    whole_history, whole_state, _ = _run("graph")
    model = _model()
    tq, vq = _queues()
    first = Trainer(max_epochs=1, callbacks=[EarlyStopping(), ModelCheckpoint(str(tmp_path), save_last=True, stamp="")])
    first.fit(model, tq, vq)
    assert first.history == whole_history[:1]
    del model, first
    model = _model(seed=99)                                                    # a fresh model (other weights), fresh queues
    tq, vq = _queues()
    es = EarlyStopping()
    resumed = Trainer(max_epochs=2, callbacks=[es, ModelCheckpoint(str(tmp_path), stamp="")])
    resumed.fit(model, tq, vq, ckpt_path=str(tmp_path / "last.ckpt"))
    assert resumed.graphed_step is not None and resumed.global_step == 8
    assert [h["epoch"] for h in resumed.history] == [0, 1]
    assert resumed.history[1] == whole_history[1]                              # epoch 1 of both histories
    _assert_same(_snapshot(model), whole_state)
    assert es.best_score == min(h["val_gen_loss_recon"] for h in whole_history)


def test_a_trainer_that_holds_a_graph_rebuilds_it_when_the_state_behind_it_is_replaced(hip, tmp_path):
    """``fit`` again on a used trainer: ``FusedAdamW.load_state_dict`` replaces the moment tensors and the device step counters,
    and another model has other tensors altogether -- a graph captured before would go on updating the old ones."""
    from unet_bssfp_amd import checkpoint
    whole_history, whole_state, _ = _run("graph")
    model = _model()
    tq, vq = _queues()
    last = str(tmp_path / "last.ckpt")
    trainer = Trainer(max_epochs=1, callbacks=[EarlyStopping(), ModelCheckpoint(str(tmp_path), save_last=True, stamp="")])
    trainer.fit(model, tq, vq)
    g0 = trainer.graphed_step
    assert g0 is not None
    import shutil
    last = shutil.copy(last, str(tmp_path / "after_epoch_0.ckpt"))              # (last.ckpt itself is rewritten every epoch)
    # 1. resume on the SAME trainer, model and queues: equals the fresh-trainer resume, i.e. the uninterrupted run
    trainer.max_epochs = 2
    trainer.fit(model, tq, vq, ckpt_path=last)
    g1 = trainer.graphed_step
    assert g1 is not None and g1 is not g0
    assert [h["epoch"] for h in trainer.history] == [0, 1] and trainer.history[1] == whole_history[1]
    _assert_same(_snapshot(model), whole_state)
    # 2. nothing replaced: the graph is kept
    trainer.max_epochs = 0
    trainer.fit(model, tq, vq)
    assert trainer.graphed_step is g1
    # 3. a checkpoint loaded by the caller behind the graph: captured anew, and the LOADED counters and moments are the ones trained
    checkpoint.load_checkpoint(model, last)
    trainer.max_epochs = 1
    trainer.fit(model, *_queues())
    g2 = trainer.graphed_step
    assert g2 is not g1 and g2.model is model
    assert set(_snapshot(model)["steps"]) == {4}                               # 2 steps in the file + a replay + the eager tail
    # 4. another model: its own graph; the first model is left alone
    before = _snapshot(model)
    other = _model(seed=7)
    start = [p.detach().clone() for p in other.parameters()]
    trainer.fit(other, *_queues())
    assert trainer.graphed_step is not g2 and trainer.graphed_step.model is other
    assert any(not torch.equal(a, b) for a, b in zip(start, other.parameters()))
    after = _snapshot(model)
    assert all(torch.equal(before["state"][k], after["state"][k]) for k in before["state"])
    assert all(torch.equal(a, b) for a, b in zip(before["moments"], after["moments"]))


def test_sync_and_set_step_counts_keep_the_host_side_whole(hip):
    """replays advance only the device counter; both calls must leave ``state['step']`` AND the call count at it, or the next eager
    ``step()`` would leave the device-counter path for a host-side bias correction"""
    from unet_bssfp_amd.optim import FusedAdamW
    p = torch.nn.Parameter(torch.ones(8, device=DEV))
    opt = FusedAdamW([p], lr=1e-3)
    for _ in range(2):
        p.grad = torch.ones_like(p)
        opt.step()
    opt._step_dev[0].add_(3)                                                   # what three captured steps would have done
    opt.sync_step_counts()
    assert opt.state[p]["step"] == 5 and opt._calls[0] == 5
    opt._step_dev[0].add_(2)
    opt.set_step_counts(7)                                                     # no device read
    assert opt.state[p]["step"] == 7 and opt._calls[0] == 7
    twin = torch.nn.Parameter(p.detach().clone())
    topt = FusedAdamW([twin], lr=1e-3)
    import copy
    topt.load_state_dict(copy.deepcopy(opt.state_dict()))                      # a twin at step 7 by the documented route (a copy:
    #                                                                            load_state_dict keeps tensors that need no conversion)
    for q, o in ((p, opt), (twin, topt)):
        q.grad = torch.full_like(q, 0.5)
        o.step()
    assert opt.state[p]["step"] == 8 == opt._calls[0] and int(opt._step_dev[0]) == 8
    assert torch.equal(p, twin)


def test_preserve_state_refuses_e4m3_operands(hip):
    import unet_bssfp_amd as M
    from unet_bssfp_amd.gan import GraphedTrainingStep, synthetic_batch
    model = _model()
    M.set_compute_dtype(model.gen, M.compute_dtype_from_name("fp8"))
    before = _snapshot_params(model)
    with pytest.raises(NotImplementedError, match="e4m3"):
        GraphedTrainingStep(model, synthetic_batch(4, 32, seed=1, device=DEV), warmup=2, preserve_state=True)
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot_params(model)))       # refused before any warm-up step


def _snapshot_params(model):
    return [p.detach().clone() for p in model.parameters()]


@pytest.mark.parametrize("transform", [[], None], ids=["unaugmented", "default_augmentation"])
def test_no_host_read_inside_an_epoch(hip, transform):
    prev = torch.cuda.get_sync_debug_mode()
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            raised = False
        except RuntimeError:
            raised = True
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not raised:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not make .item() raise on this build")
    model = _model()
    tq, vq = _queues(transform=transform)
    trainer = Trainer(max_epochs=1, sync_debug=True)
    trainer.fit(model, tq, vq)
    assert torch.cuda.get_sync_debug_mode() == prev
    assert trainer.graphed_step is not None and trainer.global_step == 4
    entry = trainer.history[0]
    assert entry["nonfinite"] == {} and all(math.isfinite(v) for k, v in entry.items() if k != "nonfinite")
