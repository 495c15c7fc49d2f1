"""What PReLU costs: one bf16 GAN training step (hipGraph replays, batch 8 x 64^3 by default) with a PReLU generator against the
LeakyReLU one, built and measured the way bench.py builds its flagship model, interleaved in rounds in ONE process.

    python tools/bench_prelu_step.py [--batch 8 --size 64 --steps 40 --rounds 3]      -> ms per step of both, per round
    python tools/bench_prelu_step.py --only prelu|leaky --eager --steps 20            -> one model alone: run this one under
        a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/bench_prelu_step.py --only ... --eager) and add up the
        normact_bwd_* / normact_small_* / slope_grad_sum rows of the two traces

Prints one JSON line per measurement.  Reads nothing but the package.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def build(act, batch, size, dev, eager=False):
    import unet_bssfp_amd as M
    from unet_bssfp_amd.gan import GraphedTrainingStep, bSSFPToDWITensorModel, synthetic_batch
    torch.manual_seed(0)           # (the process-wide dropout counter is shared by both captured steps: never reset here)
    gen = M.Generator("bssfp", dropout=0.05, act=act)
    model = bSSFPToDWITensorModel("bssfp", gen=gen, discr=M.Discriminator("bssfp"), batch_size=batch).to(dev).train()
    M.set_compute_dtype(model, torch.bfloat16)
    data = synthetic_batch(batch, size, seed=1234, device=dev)
    if eager:                      # (a kernel trace lists the launches of eager steps; a graph replay is one entry)
        count = [0]

        def step():
            model.training_step(data, count[0])
            count[0] += 1
        return step
    return GraphedTrainingStep(model, data, warmup=2)


def timed(step, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=("prelu", "leaky"), default=None)
    ap.add_argument("--eager", action="store_true", help="eager training steps instead of hipGraph replays (for kernel traces)")
    a = ap.parse_args()
    dev = "cuda:0"
    acts = {"leaky": None, "prelu": "PReLU"}
    names = [a.only] if a.only else ["leaky", "prelu"]
    steps = {n: build(acts[n], a.batch, a.size, dev, a.eager) for n in names}
    for n in names:                                   # warm up: clocks, caches
        timed(steps[n], 10)
    for r in range(a.rounds if not a.only else 1):
        for n in names:
            print(json.dumps({"round": r, "act": n, "mode": "eager" if a.eager else "hipgraph", "batch": a.batch, "size": a.size, "steps": a.steps,
                              "ms_per_step": round(timed(steps[n], a.steps), 4)}), flush=True)


if __name__ == "__main__":
    main()
