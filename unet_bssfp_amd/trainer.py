"""The fit loop of the reference, without Lightning: epochs, validation, early stopping, top-k checkpoints.

The reference's whole training entry point is (src/train.py:15-77)::

    pl.Trainer(max_epochs=50, callbacks=[EarlyStopping('val_gen_loss_recon', patience=10),
                                         ModelCheckpoint(save_top_k=10, monitor='val_loss')]).fit(model, datamodule)

Lightning 2.2.1 is absent here, so parity with it is **unpinned**: the rules written in the docstrings below are the
contract, restated from Lightning's documented behaviour, and the tests pin them.

What the loop is made of:

* ``EpochStats``      every ``self.log(..., on_epoch=True, sync_dist=True)`` of the reference is an epoch mean.  The step's
                      scalars live in device tensors that a graph replay overwrites; ONE single-wave launch per step
                      (``mi355_epoch_accumulate``, csrc/epoch_stats.hip) adds them into f64 sums on the device, one
                      all-reduce and one device-to-host copy per epoch bring them home.  No host read inside an epoch.
* ``GraphedTrainingStep(preserve_state=True)``  the hipGraph step whose warm-up does not train (gan.py).
* ``PatchQueue.state_dict``  the feed's state at an epoch boundary (data.py).
* ``EarlyStopping``, ``ModelCheckpoint``, ``Trainer``  below.

Not built: Lightning's two sanity validation batches before the first epoch, the W&B logger, and resuming in the middle of
an epoch (a checkpoint is written at epoch boundaries only).  The thesis's PRETRAIN / TRANSFER / FINE_TUNE states are in
``stages.py`` and ``train.train_staged``; a captured step is dropped when the model's state changes.
Multi-rank ``fit`` is unmeasured on hardware.
"""
from __future__ import annotations

import datetime
import json
import math
import os
import re
import warnings
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import checkpoint as _ckpt

LAST_NAME = "last.ckpt"


def _world(group=None) -> int:
    import torch.distributed as dist
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


def _rank(group=None) -> int:
    import torch.distributed as dist
    return dist.get_rank(group) if dist.is_available() and dist.is_initialized() else 0


def _strict(v):
    """JSON has no NaN / Infinity: a non-finite number becomes null in the log file (``nonfinite`` names the keys)"""
    if isinstance(v, dict):
        return {k: _strict(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_strict(x) for x in v]
    return None if isinstance(v, float) and not math.isfinite(v) else v


class EpochStats:
    """Weighted epoch sums of named scalars, kept on ``device`` in f64: ``acc = [sum_k w v_k ..., sum w, non-finite counts ...]``.

    ``reset()`` zeroes; ``add(logs, weight)`` is one launch and no host read on the GPU (the same arithmetic with torch f64
    ops on CPU tensors, for host-side use); ``reduce(group)`` is one ``all_reduce(SUM)`` when the world size is above 1;
    ``means()`` is the object's single device-to-host copy per epoch.  ``keys=None`` adopts the keys of the first ``add`` after a
    ``reset``.  A non-finite value enters its sum as IEEE arithmetic carries it (the mean becomes NaN or inf, which is what
    ``EarlyStopping(check_finite=True)`` looks for) and is counted."""

    def __init__(self, keys: Optional[Sequence[str]] = None, device="cpu"):
        self.device = torch.device(device)
        self._fixed = keys is not None
        self.keys: Optional[Tuple[str, ...]] = None
        self.acc: Optional[torch.Tensor] = None
        self._tables: Dict[tuple, object] = {}
        if keys is not None:
            self._set_keys(keys)

    def _set_keys(self, keys):
        from ._lib import EPOCH_MAX_SCALARS
        keys = tuple(keys)
        if not 1 <= len(keys) <= EPOCH_MAX_SCALARS or len(set(keys)) != len(keys):
            raise ValueError(f"EpochStats takes 1..{EPOCH_MAX_SCALARS} distinct keys, got {keys}")
        self.keys = keys
        self.acc = torch.zeros(2 * len(keys) + 1, dtype=torch.float64, device=self.device)

    def reset(self):
        if not self._fixed:
            self.keys, self.acc = None, None
        elif self.acc is not None:
            self.acc.zero_()

    def add(self, logs: Dict[str, torch.Tensor], weight: float = 1.0):
        if self.keys is None:
            self._set_keys(logs.keys())
        if set(logs) != set(self.keys):
            raise ValueError(f"EpochStats.add: the logged keys changed within an epoch: {sorted(logs)} against {sorted(self.keys)}")
        n = len(self.keys)
        vals = []
        for k in self.keys:
            v = logs[k]
            if v.numel() != 1:
                raise ValueError(f"EpochStats.add: '{k}' is not a scalar: {tuple(v.shape)}")
            if v.dtype != torch.float32 or not v.is_contiguous():
                v = v.float().contiguous()
            vals.append(v)
        if self.device.type == "cuda":
            from . import ops
            ptrs = tuple(v.data_ptr() for v in vals)
            table = self._tables.get(ptrs)
            if table is None:
                if len(self._tables) >= 64:           # eager steps: fresh log tensors per step, addresses recur only by chance
                    self._tables.clear()
                table = self._tables[ptrs] = ops.scalar_table(vals)
            ops.epoch_accumulate(table, n, weight, self.acc)
            return
        v64 = torch.stack([v.reshape(()).to(torch.float64) for v in vals])
        self.acc[:n] += float(weight) * v64
        self.acc[n] += float(weight)
        self.acc[n + 1:] += (~torch.isfinite(v64)).to(torch.float64)

    def reduce(self, group=None):
        if self.acc is not None and _world(group) > 1:
            import torch.distributed as dist
            dist.all_reduce(self.acc, op=dist.ReduceOp.SUM, group=group)

    def means(self) -> Tuple[Dict[str, float], Dict[str, int]]:
        """({key: sum / total weight}, {key: number of non-finite values added}) as Python numbers"""
        if self.acc is None:
            return {}, {}
        host = self.acc.cpu().tolist()
        n = len(self.keys)
        total = host[n]
        means = {k: (host[i] / total if total != 0 else float("nan")) for i, k in enumerate(self.keys)}
        return means, {k: int(host[n + 1 + i]) for i, k in enumerate(self.keys)}


class EarlyStopping:
    """``pl.callbacks.EarlyStopping`` (src/train.py:19-20), evaluated once per validation epoch on the epoch mean of
    ``monitor`` (parity with Lightning 2.2.1 unpinned; this is the contract):

    * a non-finite monitor with ``check_finite`` stops the run at that epoch;
    * otherwise the epoch improved iff ``current < best - min_delta`` (``mode='max'``: ``current > best + min_delta``);
      ``best`` starts at +inf (-inf);
    * on improvement ``wait_count = 0``, otherwise ``wait_count += 1`` and the run stops when ``wait_count >= patience``;
    * a missing monitor key raises ``RuntimeError``.

    ``patience=3`` over the monitor values 5, 4, 4, 4.5, 4 stops after epoch 4 (``stopped_epoch == 4``, five epochs run)."""

    def __init__(self, monitor: str = "val_gen_loss_recon", patience: int = 10, mode: str = "min", min_delta: float = 0.0,
                 check_finite: bool = True):
        if mode not in ("min", "max"):
            raise ValueError(f"mode must be 'min' or 'max', got {mode!r}")
        self.monitor, self.patience, self.mode = monitor, int(patience), mode
        self.min_delta, self.check_finite = abs(float(min_delta)), check_finite
        self.best_score = math.inf if mode == "min" else -math.inf
        self.wait_count = 0
        self.stopped_epoch = 0

    def on_epoch_end(self, trainer, model):
        if self.monitor not in trainer.callback_metrics:
            raise RuntimeError(f"EarlyStopping: '{self.monitor}' is not among the epoch's metrics "
                               f"{sorted(trainer.callback_metrics)}")
        current = float(trainer.callback_metrics[self.monitor])
        stop = False
        if self.check_finite and not math.isfinite(current):
            stop = True
        else:
            improved = current < self.best_score - self.min_delta if self.mode == "min" else current > self.best_score + self.min_delta
            if improved:
                self.best_score, self.wait_count = current, 0
            else:
                self.wait_count += 1
                stop = self.wait_count >= self.patience
        if stop:
            self.stopped_epoch = trainer.current_epoch
            trainer.should_stop = True

    def state_dict(self) -> Dict:
        return {"best_score": float(self.best_score), "wait_count": int(self.wait_count), "stopped_epoch": int(self.stopped_epoch),
                "patience": int(self.patience)}

    def load_state_dict(self, state: Dict):
        self.best_score, self.wait_count = float(state["best_score"]), int(state["wait_count"])
        self.stopped_epoch = int(state.get("stopped_epoch", 0))


class ModelCheckpoint:
    """``pl.callbacks.ModelCheckpoint`` (src/train.py:21-27); runs after every validation epoch, after ``EarlyStopping``
    (parity with Lightning 2.2.1 unpinned; this is the contract):

    * the epoch's model is saved if fewer than ``save_top_k`` models are kept or if ``current`` beats the worst kept one; the
      worst is then deleted (``save_top_k=-1`` keeps all, ``0`` none); NaN counts as +inf for ``'min'`` (-inf for ``'max'``);
    * the file is named after the reference's files (src/eval.py:335-338):
      ``f"{modality}-epoch={epoch:02d}-val_loss={val_loss:.4f}{stamp}.ckpt"`` with the 0-based epoch and
      ``stamp = str(datetime.now())`` taken at construction; ``-v1``, ``-v2``, ... is appended if the name exists.
      ``filename`` replaces the part in front of the stamp with a Lightning-style template (``'{epoch:02d}-{val_loss:.4f}'``:
      every ``{name`` becomes ``name={name``; ``{modality}`` is replaced as is) and then ``stamp`` defaults to ``''``;
      a model in a training state (stages.py) gets the state in front, as the reference's files have it (src/train.py):
      ``TrainingState.TRANSFER-pc-bssfp-epoch=31-val_loss=...``;
    * ``save_last`` also writes ``last.ckpt`` every epoch;
    * ``best_model_path``, ``best_model_score``, ``best_k_models`` ({path: score}) as in Lightning.

    ``save_top_k=2`` over the ``val_loss`` values 0.5, 0.3, 0.4, 0.2, 0.6 leaves exactly the files of epochs 1 and 3;
    ``best_model_path`` is epoch 3's, ``best_model_score`` 0.2.  Files are written on rank 0 only."""

    def __init__(self, dirpath: str, filename: Optional[str] = None, monitor: str = "val_loss", mode: str = "min",
                 save_top_k: int = 10, save_last: bool = False, stamp: Optional[str] = None):
        if mode not in ("min", "max"):
            raise ValueError(f"mode must be 'min' or 'max', got {mode!r}")
        self.dirpath, self.filename, self.monitor, self.mode = str(dirpath), filename, monitor, mode
        self.save_top_k, self.save_last = int(save_top_k), save_last
        if stamp is None:
            stamp = str(datetime.datetime.now()) if filename is None else ""
        self.stamp = stamp
        self.best_k_models: Dict[str, float] = {}
        self.best_model_path, self.best_model_score = "", None
        self.last_model_path = ""

    def _worse(self, a: float, b: float) -> bool:
        return a > b if self.mode == "min" else a < b

    def _name(self, trainer, model) -> str:
        template = "{modality}-{epoch:02d}-{val_loss:.4f}" if self.filename is None else self.filename
        template = re.sub(r"\{(?!modality\b)([A-Za-z_][\w\-/]*)", r"\1={\1", template)
        values = dict(trainer.callback_metrics)
        values.update(epoch=trainer.current_epoch, modality=getattr(model, "input_modality", "model"))
        try:
            base = template.format(**values) + self.stamp
            state = getattr(model, "training_state", None)
            if state is not None:
                base = f"{state}-{base}"
        except KeyError as e:
            raise RuntimeError(f"ModelCheckpoint: {e} is not among the epoch's metrics {sorted(trainer.callback_metrics)}")
        path, v = os.path.join(self.dirpath, base + ".ckpt"), 0
        if trainer.is_global_zero:                  # rank 0 alone looks at the directory: it is the one that writes there
            while os.path.exists(path) or path in self.best_k_models:
                v += 1
                path = os.path.join(self.dirpath, f"{base}-v{v}.ckpt")
        return trainer.broadcast_from_zero(path)    # every rank keeps the same best_k_models / best_model_path

    def on_epoch_end(self, trainer, model):
        if self.monitor not in trainer.callback_metrics:
            raise RuntimeError(f"ModelCheckpoint: '{self.monitor}' is not among the epoch's metrics "
                               f"{sorted(trainer.callback_metrics)}")
        current = float(trainer.callback_metrics[self.monitor])
        if math.isnan(current):
            current = math.inf if self.mode == "min" else -math.inf
        k = self.save_top_k
        worst = None
        if self.best_k_models:
            worst = (max if self.mode == "min" else min)(self.best_k_models, key=self.best_k_models.get)
        keep = k != 0 and (k < 0 or len(self.best_k_models) < k or self._worse(self.best_k_models[worst], current))
        drop = None
        if keep:
            os.makedirs(self.dirpath, exist_ok=True)
            path = self._name(trainer, model)
            self.best_k_models[path] = current
            if k > 0 and len(self.best_k_models) > k:
                drop = worst
                del self.best_k_models[drop]
            best = (min if self.mode == "min" else max)(self.best_k_models, key=self.best_k_models.get)
            self.best_model_path, self.best_model_score = best, self.best_k_models[best]
            if trainer.is_global_zero:
                trainer.save_checkpoint(path, model)
                if drop is not None and os.path.exists(drop):
                    os.remove(drop)
        if self.save_last:
            self.last_model_path = os.path.join(self.dirpath, LAST_NAME)
            if trainer.is_global_zero:
                os.makedirs(self.dirpath, exist_ok=True)
                trainer.save_checkpoint(self.last_model_path, model)

    def state_dict(self) -> Dict:
        return {"monitor": self.monitor, "best_model_score": self.best_model_score, "best_model_path": self.best_model_path,
                "best_k_models": {p: float(s) for p, s in self.best_k_models.items()}, "last_model_path": self.last_model_path,
                "dirpath": self.dirpath}

    def load_state_dict(self, state: Dict):
        self.best_k_models = {str(p): float(s) for p, s in state.get("best_k_models", {}).items()}
        self.best_model_path = str(state.get("best_model_path", ""))
        score = state.get("best_model_score")
        self.best_model_score = None if score is None else float(score)
        self.last_model_path = str(state.get("last_model_path", ""))


class Trainer:
    """``pl.Trainer(max_epochs, callbacks).fit(model, datamodule)`` for the step harness (parity with Lightning unpinned).

    ``model``: ``training_step``, ``validation_step``, ``last_logs``, ``batch_size``, ``train()``, ``eval()``
    (``gan.bSSFPToDWITensorModel``).  A queue: ``batches(batch_size, **kw)`` and ``__len__`` (patches per epoch), plus
    ``state_dict`` / ``load_state_dict`` if it is to be resumed, plus ``next_batch(n, out=)`` for the graph path
    (``data.PatchQueue``).

    Per epoch:

    * train -- ``graph=True`` on a HIP model: ONE ``GraphedTrainingStep(preserve_state=True, group=group)`` built at the first
      epoch (after a checkpoint has been loaded) over a synthetic batch; each full batch is ``queue.next_batch(B, out=static)``,
      a replay and ``EpochStats.add``; a ragged last batch (``len(queue) % B``) goes through the eager
      ``model.training_step`` unless ``drop_last``.  ``graph=False``, or a CPU model: every batch through ``training_step``.
      The weight of every batch is ``model.batch_size``, ragged ones included, as the reference passes
      ``batch_size=self.batch_size`` to every ``self.log``: an epoch value is the plain mean over batches;
    * validate, if ``val_queue`` is given -- under ``model.eval()`` and ``torch.no_grad()``, ``validation_step`` on every
      batch, then ``model.train()``;
    * epoch end -- ``reduce(group)``, ``means()``; ``callback_metrics`` gets the validation keys under their own names and
      the training keys as ``k`` and ``k + '_epoch'``; one entry is appended to ``history`` (one line of strict JSON to
      ``log_path``: a non-finite mean is written as null);
      the callbacks run (``on_epoch_end``; ``ModelCheckpoint``s last), on every rank for the stop decision -- it derives
      from reduced numbers, so the ranks agree -- and on rank 0 for files.

    ``global_step`` counts optimiser steps, two per batch, as Lightning does under manual optimisation (unpinned).
    ``sync_debug=True`` runs the per-batch loops under ``torch.cuda.set_sync_debug_mode('error')`` and restores the previous
    mode: a host read inside an epoch raises.  Tested with ``transform=[]`` and with the queue's default augmentation; a caller's own
    transform list is as free of host reads as its stages are.

    A trainer may ``fit`` more than once.  The captured step of an earlier call is kept only for the same model, batch and
    patch shape and only while every tensor it updates is still the one it captured; ``fit(ckpt_path=...)``, another model,
    a checkpoint loaded in between or a ``change_training_state`` drop it, and it is rebuilt at the first epoch.

    Checkpoints are ``checkpoint.checkpoint_dict(model, epoch, global_step)`` with ``callbacks`` filled
    (``{'EarlyStopping': ..., 'ModelCheckpoint': ...}``) and ``mi355`` extended by ``train_queue`` / ``val_queue`` states and the
    history; they load through ``checkpoint.load_checkpoint`` and ``torch.load(weights_only=True)``.
    ``fit(ckpt_path=...)`` loads model, optimisers and dropout counter through ``load_checkpoint``, callback and queue state
    from the additions, and continues at ``epoch + 1``; a file without the additions resumes with fresh callbacks and queues
    and says so in a warning."""

    def __init__(self, max_epochs: int = 50, callbacks=(), graph: bool = True, drop_last: bool = False, group=None,
                 log_path: Optional[str] = None, sync_debug: bool = False):
        self.max_epochs, self.graph, self.drop_last, self.group = int(max_epochs), graph, drop_last, group
        self.log_path, self.sync_debug = log_path, sync_debug
        cbs = list(callbacks)
        self.callbacks = [c for c in cbs if not isinstance(c, ModelCheckpoint)] + [c for c in cbs if isinstance(c, ModelCheckpoint)]
        self.current_epoch = 0
        self.global_step = 0
        self.should_stop = False
        self.callback_metrics: Dict[str, float] = {}
        self.history: List[Dict] = []
        self.graphed_step = None
        self._graph_for = None
        self._queues: Dict[str, object] = {}
        self._steps_base: List[int] = []
        self._steps_since = 0

    @property
    def is_global_zero(self) -> bool:
        return _rank(self.group) == 0

    def broadcast_from_zero(self, obj):
        """``obj`` of the group's rank 0 on every rank (one object collective; nothing to do with one rank)"""
        if _world(self.group) > 1:
            import torch.distributed as dist
            box = [obj]
            dist.broadcast_object_list(box, src=0 if self.group is None else dist.get_global_rank(self.group, 0), group=self.group)
            obj = box[0]
        return obj

    # ---- checkpoints -------------------------------------------------------------------------------------------------
    def save_checkpoint(self, path: str, model) -> None:
        # (checkpoint_dict reads the optimisers' device step counters itself: FusedAdamW.sync_step_counts)
        ckpt = _ckpt.checkpoint_dict(model, self.current_epoch, self.global_step)
        ckpt["callbacks"] = {type(c).__name__: c.state_dict() for c in self.callbacks if hasattr(c, "state_dict")}
        for name, q in self._queues.items():
            if q is not None and hasattr(q, "state_dict"):
                ckpt["mi355"][name] = q.state_dict()
        ckpt["mi355"]["history"] = [dict(h) for h in self.history]
        torch.save(ckpt, path)

    def _resume(self, model, ckpt_path: str) -> int:
        ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)          # read once: model state and the additions
        info = _ckpt.apply_checkpoint(model, ckpt, path=ckpt_path)
        extra = ckpt.get("mi355") or {}
        states = ckpt.get("callbacks") or {}
        fresh = []
        for c in self.callbacks:
            if hasattr(c, "load_state_dict"):
                if type(c).__name__ in states:
                    c.load_state_dict(states[type(c).__name__])
                else:
                    fresh.append(type(c).__name__)
        for name, q in self._queues.items():
            if q is not None and hasattr(q, "load_state_dict"):
                if name in extra:
                    q.load_state_dict(extra[name])
                else:
                    fresh.append(name)
        if fresh:
            warnings.warn(f"{ckpt_path} carries no trainer state for {fresh}: they start fresh (model, optimisers and the "
                          "dropout counter were loaded)")
        self.history = [dict(h) for h in extra.get("history", [])]
        self.global_step = int(info["global_step"])
        return int(info["epoch"]) + 1

    # ---- the loops ---------------------------------------------------------------------------------------------------
    def _call(self, hook: str, model):
        for c in self.callbacks:
            fn = getattr(c, hook, None)
            if fn is not None:
                fn(self, model)

    class _SyncDebug:
        def __init__(self, on: bool):
            self.on = on and torch.cuda.is_available()

        def __enter__(self):
            if self.on:
                self.prev = torch.cuda.get_sync_debug_mode()
                torch.cuda.set_sync_debug_mode("error")

        def __exit__(self, *exc):
            if self.on:
                torch.cuda.set_sync_debug_mode(self.prev)
            return False

    @staticmethod
    def _device(model) -> torch.device:
        return next(model.parameters()).device

    @staticmethod
    def _graph_key(model, queue):
        """What a captured step is tied to: the model object, the batch and patch shape, and the ADDRESSES of every parameter,
        optimiser moment and device step counter (``FusedAdamW.load_state_dict`` replaces the latter two with new tensors), and
        the model's ``stage_version`` (``change_training_state`` changes which gradients a step computes)."""
        ptrs = [p.data_ptr() for p in model.parameters()]
        for o in model.optimizers():
            for st in o.state.values():
                ptrs += [v.data_ptr() for v in st.values() if isinstance(v, torch.Tensor)]
            ptrs += [t.data_ptr() for t in getattr(o, "_step_dev", {}).values()]
        return (id(model), model.batch_size, tuple(getattr(queue, "patch_size", ())), tuple(ptrs), getattr(model, "stage_version", 0))

    def _drop_graph(self):
        self.graphed_step, self._graph_for = None, None
        self._steps_base, self._steps_since = [], 0

    def _adopt_graph(self, model, queue):
        """A trainer may ``fit`` more than once.  The graph of an earlier call is replayed only if it is this model's, of this
        shape, and if no tensor it updates has been replaced since (a checkpoint loaded behind it, by ``fit(ckpt_path=...)``
        or by the caller); otherwise it is dropped and rebuilt at the first epoch.  A kept graph's step base is read afresh."""
        if self.graphed_step is None:
            return
        if self.graphed_step.model is not model or self.graphed_step.stale() or self._graph_for != self._graph_key(model, queue):
            self._drop_graph()
            return
        self._steps_base = [self._device_steps(o) for o in model.optimizers()]
        self._steps_since = 0

    def _build_graph(self, model, queue):
        from .gan import GraphedTrainingStep, synthetic_batch
        dev = self._device(model)
        patch = getattr(queue, "patch_size", None)
        if patch is None or not hasattr(queue, "next_batch"):
            raise TypeError("Trainer(graph=True) needs a queue with patch_size and next_batch(n, out=) (data.PatchQueue)")
        static = synthetic_batch(model.batch_size, tuple(patch), seed=0, modality=model.input_modality, device=dev)
        self.graphed_step = GraphedTrainingStep(model, static, warmup=2, group=self.group, preserve_state=True)
        # what the device step counters hold now, read once: from here on the trainer counts the steps itself
        self._steps_base = [self._device_steps(o) for o in model.optimizers()]
        self._steps_since = 0
        self._graph_for = self._graph_key(model, queue)

    @staticmethod
    def _device_steps(opt) -> int:
        counters = getattr(opt, "_step_dev", None)
        return int(next(iter(counters.values())).item()) if counters else 0

    def _host_step_counts(self, model):
        """graph replays advance the optimisers' device counters only: bring the host integers up to date, without a device
        read, before an eager step inside an epoch"""
        if self.graphed_step is not None:
            for o, base in zip(model.optimizers(), self._steps_base):
                if hasattr(o, "set_step_counts"):
                    o.set_step_counts(base + self._steps_since)

    def _train_epoch(self, model, queue, stats: EpochStats):
        B = model.batch_size
        full, tail = divmod(len(queue), B)
        use_graph = self.graph and self._device(model).type == "cuda"
        if use_graph and self.graphed_step is None and full:
            self._build_graph(model, queue)
        with self._SyncDebug(self.sync_debug):
            if use_graph:
                gs = self.graphed_step
                static = gs.instances[0][0] if gs is not None else None
                for _ in range(full):
                    queue.next_batch(B, out=static)
                    gs()
                    self._steps_since += 1
                    stats.add(model.last_logs, B)
                    self.global_step += 2
                if tail:
                    batch = queue.next_batch(tail)              # (dropped or not: the queue ends its epoch drained)
                    if not self.drop_last:
                        self._host_step_counts(model)
                        model.training_step(batch, full)
                        self._steps_since += 1
                        stats.add(model.last_logs, B)
                        self.global_step += 2
            else:
                for i, batch in enumerate(queue.batches(B)):
                    if self.drop_last and tail and i == full:
                        continue
                    model.training_step(batch, i)
                    stats.add(model.last_logs, B)
                    self.global_step += 2

    def _validate(self, model, queue, stats: EpochStats):
        model.eval()
        try:
            with torch.no_grad(), self._SyncDebug(self.sync_debug):
                for i, batch in enumerate(queue.batches(model.batch_size)):
                    model.validation_step(batch, i)
                    stats.add(model.last_logs, model.batch_size)
        finally:
            model.train()

    def _check_ranks(self, queues, device):
        """Every rank must run the same number of training and validation batches per epoch: the gradient exchange is
        collective, and so is the reduction of the epoch statistics, which a rank that added nothing would not enter."""
        if _world(self.group) > 1:
            import torch.distributed as dist
            lens = [-1 if q is None else len(q) for q in queues]
            n = torch.tensor(lens + [-v for v in lens], dtype=torch.int64, device=device)
            dist.all_reduce(n, op=dist.ReduceOp.MAX, group=self.group)
            hi, lo = n[:len(lens)].tolist(), [-v for v in n[len(lens):].tolist()]
            if hi != lo:
                raise ValueError(f"the ranks' queues differ in length: patches per epoch (train, val) from {lo} to {hi}")

    def fit(self, model, train_queue, val_queue=None, ckpt_path: Optional[str] = None):
        self._queues = {"train_queue": train_queue, "val_queue": val_queue}
        self.should_stop = False
        if ckpt_path:
            self._drop_graph()                       # a checkpoint is never loaded behind a captured graph
        start = self._resume(model, ckpt_path) if ckpt_path else 0
        self._adopt_graph(model, train_queue)
        device = self._device(model)
        self._check_ranks((train_queue, val_queue), device)
        model.train()
        train_stats, val_stats = EpochStats(None, device), EpochStats(None, device)
        for epoch in range(start, self.max_epochs):
            self.current_epoch = epoch
            train_stats.reset(), val_stats.reset()
            self._call("on_train_epoch_start", model)
            self._train_epoch(model, train_queue, train_stats)
            self._call("on_train_epoch_end", model)
            if val_queue is not None:
                self._call("on_validation_start", model)
                self._validate(model, val_queue, val_stats)
                self._call("on_validation_end", model)
            metrics: Dict[str, float] = {}
            nonfinite: Dict[str, int] = {}
            entry = {"epoch": epoch, "global_step": self.global_step}
            for stats, train in ((train_stats, True), (val_stats, False)):
                stats.reduce(self.group)
                means, bad = stats.means()
                entry.update(means)
                nonfinite.update({k: c for k, c in bad.items() if c})
                for k, v in means.items():
                    metrics[k] = v
                    if train:
                        metrics[k + "_epoch"] = v
            entry["nonfinite"] = nonfinite
            self.callback_metrics = metrics
            self.history.append(entry)
            if self.log_path and self.is_global_zero:
                with open(self.log_path, "a") as f:
                    f.write(json.dumps(_strict(entry), allow_nan=False) + "\n")
            self._call("on_epoch_end", model)
            if self.should_stop:
                break
        return self
