"""Training states (unet_bssfp_amd.stages): ms per hipGraph-replayed training step in state ``None`` (the plain step), ``TRANSFER``
(the U-Net frozen: its data-gradient chain runs, its weight gradients, AdamW share and re-packs do not) and ``FINE_TUNE`` (the
plain step's launches at another rate).  8 x 24 x 64^3, bf16, dropout 0.05.  The three steps are captured in ONE process, from
the same seed; two warm-up rounds, then ``--reps`` rounds with every state once per round, in turn; device events; one JSON line
per state (median, quartiles, min and max over the rounds, ms) and one with the differences next to state None's own spread.

    python tools/bench_stages.py [--reps 20] [--replays 30] [--out profiles/stages_bench.json]
    python tools/bench_stages.py --only TRANSFER --replays 50      # one state alone, for a kernel trace of its launches
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_bssfp_amd as U                                               # noqa: E402
from unet_bssfp_amd.gan import GraphedTrainingStep, bSSFPToDWITensorModel, synthetic_batch   # noqa: E402
from unet_bssfp_amd.stages import TrainingState                          # noqa: E402

DEV = "cuda:0"
BATCH, SIZE = 8, 64
STATES = {"None": None, "TRANSFER": TrainingState.TRANSFER, "FINE_TUNE": TrainingState.FINE_TUNE}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(what, v, **extra):
    q = statistics.quantiles(v, n=4)
    return dict(what=what, median_ms=round(statistics.median(v), 4), p25_ms=round(q[0], 4), p75_ms=round(q[2], 4),
                min_ms=round(min(v), 4), max_ms=round(max(v), 4), reps=len(v), **extra)


def captured(state):
    torch.manual_seed(0)
    model = bSSFPToDWITensorModel("bssfp", gen=U.Generator("bssfp", dropout=0.05), discr=U.Discriminator("bssfp"),
                                  batch_size=BATCH).to(DEV).train()
    U.set_compute_dtype(model, torch.bfloat16)
    if state is not None:
        model.change_training_state(state, "bssfp")
    batch = synthetic_batch(BATCH, SIZE, seed=1234, device=DEV)
    return GraphedTrainingStep(model, batch, warmup=2)


def main(reps, replays, only, out):
    names = [only] if only else list(STATES)
    steps = {name: captured(STATES[name]) for name in names}

    def run(name):
        gs = steps[name]

        def loop():
            for _ in range(replays):
                gs()
        return timed(loop) / replays

    for _ in range(2):                                                     # warm-up rounds
        for name in names:
            run(name)
    times = {name: [] for name in names}
    for _ in range(reps):                                                  # every state once per round, in turn
        for name in names:
            times[name].append(run(name))
    lines = [summary(f"step_{name}", v, replays_per_round=replays, batch=BATCH, size=SIZE, dtype="bf16") for name, v in times.items()]
    if not only:
        res = {l["what"]: l for l in lines}
        base = res["step_None"]
        lines.append(dict(what="against_None",
                          transfer_minus_none_ms=round(res["step_TRANSFER"]["median_ms"] - base["median_ms"], 4),
                          fine_tune_minus_none_ms=round(res["step_FINE_TUNE"]["median_ms"] - base["median_ms"], 4),
                          none_interquartile_ms=round(base["p75_ms"] - base["p25_ms"], 4),
                          none_range_ms=round(base["max_ms"] - base["min_ms"], 4)))
    for l in lines:
        print(json.dumps(l), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--replays", type=int, default=30)
    ap.add_argument("--only", choices=list(STATES), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    main(a.reps, a.replays, a.only, a.out)
