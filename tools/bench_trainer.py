"""trainer.Trainer: ms per training step inside ``fit`` next to the bare loop ``queue.next_batch(8, out=static); gs()`` over the SAME
captured step, model and queue, the epoch-statistics launch alone, and one validation batch.  8 x 24 x 64^3, bf16,
``reference_augmentation()``.  Device events, warm-up, interleaved rounds in one process; one JSON line per measurement
(median, quartiles, min and max over the rounds, ms) and one with the difference of the medians next to the bare loop's spread.

    python tools/bench_trainer.py [--reps 20] [--subjects 8]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_bssfp_amd as U                                               # noqa: E402
from unet_bssfp_amd import data as Q                                     # noqa: E402
from unet_bssfp_amd.gan import bSSFPToDWITensorModel                     # noqa: E402
from unet_bssfp_amd.trainer import EpochStats, Trainer                   # noqa: E402

DEV = "cuda:0"
BATCH = 8


class EpochTimer:
    """device events around the training loop of an epoch (validation and the epoch-end reduction stay outside)"""

    def __init__(self):
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def on_train_epoch_start(self, trainer, model):
        self.e0.record()

    def on_train_epoch_end(self, trainer, model):
        self.e1.record()

    def ms(self):
        self.e1.synchronize()
        return self.e0.elapsed_time(self.e1)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(what, v, **extra):
    q = statistics.quantiles(v, n=4)
    out = dict(what=what, median_ms=round(statistics.median(v), 4), p25_ms=round(q[0], 4), p75_ms=round(q[2], 4),
               min_ms=round(min(v), 4), max_ms=round(max(v), 4), reps=len(v), **extra)
    print(json.dumps(out), flush=True)
    return out


def main(reps, nsubjects):
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    subjects = [{"bssfp": {"data": torch.rand((24, 96, 128, 128), generator=g).to(DEV)},
                 "dwi-tensor": {"data": torch.rand((6, 96, 128, 128), generator=g).to(DEV)}} for _ in range(nsubjects)]
    queue = Q.PatchQueue(subjects, "bssfp", seed=3)                        # the reference's queue: 16 / 8 / 64^3, its augmentation
    val_queue = Q.PatchQueue(subjects[:1], "bssfp", seed=4)
    steps = len(queue) // BATCH
    model = bSSFPToDWITensorModel("bssfp", gen=U.Generator("bssfp", dropout=0.05), discr=U.Discriminator("bssfp"),
                                  batch_size=BATCH).to(DEV).train()
    U.set_compute_dtype(model, torch.bfloat16)
    timer = EpochTimer()
    trainer = Trainer(max_epochs=1, callbacks=[timer])

    def fit_epoch():
        trainer.fit(model, queue)                                          # one epoch per call; the graph is built by the first
        return timer.ms() / steps

    gs_holder = {}

    def bare_epoch():
        gs = gs_holder["gs"]
        static = gs.instances[0][0]

        def loop():
            for _ in range(steps):
                queue.next_batch(BATCH, out=static)
                gs()
        return timed(loop) / steps

    for _ in range(2):                                                     # warm-up: builds the graph, fills every cache
        fit_epoch()
    gs_holder["gs"] = trainer.graphed_step
    for _ in range(2):
        bare_epoch()

    stats = EpochStats(None, DEV)
    logs = dict(model.last_logs)

    def accumulate(n=100):
        def loop():
            for _ in range(n):
                stats.add(logs, BATCH)
        return timed(loop) / n

    val_batch = val_queue.next_batch(BATCH)

    def validation():
        model.eval()
        try:
            with torch.no_grad():
                return timed(lambda: model.validation_step(val_batch, 0))
        finally:
            model.train()

    accumulate(), validation()
    times = {"trainer_fit_step": [], "bare_loop_step": [], "epoch_accumulate_launch": [], "validation_batch": []}
    for _ in range(reps):                                                  # every variant once per round, in turn
        times["trainer_fit_step"].append(fit_epoch())
        times["bare_loop_step"].append(bare_epoch())
        times["epoch_accumulate_launch"].append(accumulate())
        times["validation_batch"].append(validation())
    res = {k: summary(k, v, steps_per_epoch=steps) for k, v in times.items()}
    fit, bare = res["trainer_fit_step"], res["bare_loop_step"]
    print(json.dumps(dict(what="trainer_minus_bare", difference_ms=round(fit["median_ms"] - bare["median_ms"], 4),
                          bare_interquartile_ms=round(bare["p75_ms"] - bare["p25_ms"], 4),
                          bare_range_ms=round(bare["max_ms"] - bare["min_ms"], 4))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--subjects", type=int, default=8)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    main(a.reps, a.subjects)
