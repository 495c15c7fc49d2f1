"""The captured 8 x 24 x 64^3 bf16 training step with and without the Perceptual term in its objective: what the reference's
``(L1 + 1e3 Perceptual) / 2 * recon_factor`` costs on top of the L1 objective.  Both models are built from the same seed and
replay one hipGraph each on the same static batch; device events, interleaved rounds in one process, one JSON line per variant.

    python tools/bench_perceptual_step.py [--reps 10] [--batch 8] [--size 64]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_bssfp_amd as U                                               # noqa: E402
from tools.bench_perceptual import random_net                            # noqa: E402
from unet_bssfp_amd import losses                                        # noqa: E402
from unet_bssfp_amd.gan import GraphedTrainingStep, bSSFPToDWITensorModel, synthetic_batch   # noqa: E402

DEV = "cuda:0"


def graphed(batch, batch_size, **kw):
    torch.manual_seed(0)
    model = bSSFPToDWITensorModel("bssfp", gen=U.Generator("bssfp", dropout=0.05), discr=U.Discriminator("bssfp"),
                                  batch_size=batch_size, **kw).to(DEV).train()
    U.set_compute_dtype(model, torch.bfloat16)
    return GraphedTrainingStep(model, batch, warmup=3)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=64)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    batch = synthetic_batch(a.batch, a.size, seed=5, device=DEV)
    net = random_net()
    steps = {"l1_objective": graphed(batch, a.batch),
             "l1_objective_divisor_2": graphed(batch, a.batch, recon_divisor=2),
             "reference_objective": graphed(batch, a.batch, extra_recon_terms=losses.reference_recon_terms(net))}
    times = {k: [] for k in steps}
    for r in range(3 + a.reps):                                           # 3 warm-up rounds of replays
        for k, gs in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                gs()
            e1.record()
            e1.synchronize()
            if r >= 3:
                times[k].append(e0.elapsed_time(e1) / 5)
    med = {}
    for k, v in times.items():
        med[k] = statistics.median(v)
        print(json.dumps(dict(what="training_step", variant=k, median_ms=round(med[k], 4), min_ms=round(min(v), 4),
                              max_ms=round(max(v), 4), reps=len(v), shape=[a.batch, 24, a.size, a.size, a.size])), flush=True)
    print(json.dumps(dict(what="perceptual_term_in_the_step", added_ms=round(med["reference_objective"] - med["l1_objective"], 4))),
          flush=True)
