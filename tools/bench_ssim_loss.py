"""losses.SSIMLoss: forward + backward time next to metrics.SSIMMetric and to the torch-composed term on the same tensors, and
the 8x64^3 training step with and without the term.  Device events, warm-up, interleaved rounds in one process; one JSON line per
measurement (median and min over the rounds, ms).

    python tools/bench_ssim_loss.py [--parts term,composed,step] [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import metrics_ref as MR                                     # noqa: E402  (the composed comparison only)
from unet_bssfp_amd import metrics as M                                  # noqa: E402
from unet_bssfp_amd.losses import SSIMLoss                               # noqa: E402

SHAPES = ((8, 6, 64, 64, 64), (1, 6, 128, 128, 128))


def rounds(fns, reps, warmup=3):
    """{name: [ms per call] * reps}: every variant once per round, in turn"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1))
    return out


def report(what, shape, times, **extra):
    for k, v in times.items():
        print(json.dumps(dict(what=what, shape=list(shape), variant=k, median_ms=round(statistics.median(v), 4),
                              min_ms=round(min(v), 4), reps=len(v), **extra)), flush=True)
    return {k: statistics.median(v) for k, v in times.items()}


def inputs(shape):
    g = torch.Generator().manual_seed(sum(shape))
    y = torch.rand(shape, generator=g)
    p = (y + 0.2 * torch.randn(shape, generator=g)).clamp(0, 1)
    return p.cuda().requires_grad_(True), y.cuda()


def bench_term(shape, reps, composed):
    p, y = inputs(shape)
    loss_fn, metric = SSIMLoss(3), M.SSIMMetric(3)

    def fwd_bwd(fn):
        p.grad = None
        fn(p, y).backward()

    fns = {"ssim_metric": lambda: metric(p, y), "ssim_loss_fwd": lambda: loss_fn(p.detach(), y),
           "ssim_loss_fwd_bwd": lambda: fwd_bwd(loss_fn)}
    def composed_term(a, b):
        with torch.device("cuda"):                                       # the oracle builds its window with factory calls
            return (1 - MR.ssim3d(a, b)).mean()

    if composed:
        fns["torch_composed_fwd_bwd"] = lambda: fwd_bwd(composed_term)
    med = report("term", shape, rounds(fns, reps))
    ratios = dict(loss_fwd_bwd_over_metric=round(med["ssim_loss_fwd_bwd"] / med["ssim_metric"], 3))
    if composed:
        ratios["torch_composed_over_loss_fwd_bwd"] = round(med["torch_composed_fwd_bwd"] / med["ssim_loss_fwd_bwd"], 2)
    print(json.dumps(dict(what="ratio", shape=list(shape), **ratios)), flush=True)


def bench_step(reps, batch_items=8, size=64, replays=10):
    import unet_bssfp_amd as U
    from unet_bssfp_amd.gan import GraphedTrainingStep, bSSFPToDWITensorModel, synthetic_batch
    batch = synthetic_batch(batch_items, size, seed=1234, device="cuda")

    def graphed(terms, fused):
        torch.manual_seed(0)
        model = bSSFPToDWITensorModel("bssfp", gen=U.Generator("bssfp", dropout=0.05), discr=U.Discriminator("bssfp"),
                                      extra_recon_terms=terms).cuda().train()
        U.set_compute_dtype(model, torch.bfloat16)
        model.fused_loss_heads = fused
        gs = GraphedTrainingStep(model, batch, warmup=2)
        return lambda: [gs() for _ in range(replays)]

    fns = {"default_fused_heads": graphed(None, True), "composed_heads_L1": graphed(None, False),
           "composed_heads_L1_SSIM": graphed({"SSIM": SSIMLoss(3)}, False)}
    times = {k: [t / replays for t in v] for k, v in rounds(fns, reps, warmup=5).items()}
    report("gan_step_bf16_hipgraph", (batch_items, size), times, replays_per_sample=replays)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="term,composed,step", help="comma list of term, composed (with term: the torch-composed comparison), step")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    parts = a.parts.split(",")
    for shape in SHAPES:
        if "term" in parts:
            bench_term(shape, a.reps, composed="composed" in parts)
    if "step" in parts:
        bench_step(a.reps)
