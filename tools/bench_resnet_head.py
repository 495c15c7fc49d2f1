"""ResNet input heads (Generator(head="resnet"), nn.ResidualUnit): what they cost, and what the fused tail launch is worth.

1. ms per hipGraph-replayed training step, 8 x 64^3, bf16, dropout 0.05: head "conv" (the reference's 1x1x1 head), "resnet" and
   "resnet" with ``fuse_tail = False`` (norm + act launch, 1x1x1 convolution, add), for 'dwi-tensor' (6 -> 24, projection residual) and
   'bssfp' (24 -> 24, identity residual), in state ``None`` and in ``TRANSFER``.  All steps are captured in ONE process from the same
   seed; two warm-up rounds, then ``--reps`` rounds with every configuration once per round, in turn; device events.
2. The tail launch alone (ops.restail_fwd, projection of 6 channels and identity) against ops.normact_fwd on the same z
   (8 x 64^3 rows of 32 bf16 channels), alternating in the same process (each window is one captured graph of ``--launches``
   launches), rotating over ``--buffers`` sets of tensors so that no launch finds its operands in the 256 MB memory-side cache.
   Bytes are counted from the shapes (z + y for normact_fwd; z + the padded x row + y for the tail) and set against the HBM
   figures of MI355X_MICROARCH.md (8 TB/s peak, about 6.3 TB/s achievable).

One JSON line per measurement (median, quartiles, min and max over the rounds) and one line per comparison next to the partner's own
spread.

    python tools/bench_resnet_head.py [--reps 10] [--replays 20] [--out profiles/resnet_head_bench.json]
    python tools/bench_resnet_head.py --only-kernel            # part 2 alone
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_bssfp_amd as U                                               # noqa: E402
from unet_bssfp_amd import ops                                           # noqa: E402
from unet_bssfp_amd.gan import GraphedTrainingStep, bSSFPToDWITensorModel, synthetic_batch   # noqa: E402
from unet_bssfp_amd.stages import TrainingState                          # noqa: E402

DEV = "cuda:0"
BATCH, SIZE = 8, 64
HBM_PEAK_TBS, HBM_ACHIEVABLE_TBS = 8.0, 6.3             # MI355X_MICROARCH.md, "HBM"
HEADS = {"conv": ("conv", True), "resnet": ("resnet", True), "resnet_unfused": ("resnet", False)}
STATES = {"None": None, "TRANSFER": TrainingState.TRANSFER}


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


def captured(head, fuse, modality, state):
    torch.manual_seed(0)
    gen = U.Generator(modality, dropout=0.05, head=head)
    for m in gen.modules():
        if isinstance(m, U.ResidualUnit):
            m.fuse_tail = fuse
    model = bSSFPToDWITensorModel(modality, gen=gen, discr=U.Discriminator(modality), batch_size=BATCH).to(DEV).train()
    U.set_compute_dtype(model, torch.bfloat16)
    if state is not None:
        model.change_training_state(state, modality)
    batch = synthetic_batch(BATCH, SIZE, seed=1234, modality=modality, device=DEV)
    return GraphedTrainingStep(model, batch, warmup=2)


def rounds(runs, reps):
    """runs: name -> callable returning ms; two warm-up rounds, then every name once per round, in turn"""
    for _ in range(2):
        for fn in runs.values():
            fn()
    times = {name: [] for name in runs}
    for _ in range(reps):
        for name, fn in runs.items():
            times[name].append(fn())
    return times


def bench_steps(reps, replays):
    lines = []
    for modality in ("dwi-tensor", "bssfp"):
        for sname, state in STATES.items():
            steps = {h: captured(head, fuse, modality, state) for h, (head, fuse) in HEADS.items()}

            def runner(gs):
                def loop():
                    for _ in range(replays):
                        gs()
                return lambda: timed(loop) / replays
            times = rounds({h: runner(gs) for h, gs in steps.items()}, reps)
            res = {h: summary(f"step_{modality}_{sname}_{h}", v, replays_per_round=replays, batch=BATCH, size=SIZE, dtype="bf16",
                              modality=modality, state=sname, head=h) for h, v in times.items()}
            lines += list(res.values())
            lines.append(dict(what=f"step_{modality}_{sname}_differences",
                              resnet_minus_conv_ms=round(res["resnet"]["median_ms"] - res["conv"]["median_ms"], 4),
                              fused_minus_unfused_ms=round(res["resnet"]["median_ms"] - res["resnet_unfused"]["median_ms"], 4),
                              unfused_interquartile_ms=round(res["resnet_unfused"]["p75_ms"] - res["resnet_unfused"]["p25_ms"], 4),
                              unfused_range_ms=round(res["resnet_unfused"]["max_ms"] - res["resnet_unfused"]["min_ms"], 4)))
            del steps
            torch.cuda.empty_cache()
    return lines


def bench_kernel(reps, launches, buffers):
    n, c, rows = BATCH, 32, BATCH * SIZE ** 3
    g = torch.Generator().manual_seed(0)
    sets = []
    for _ in range(buffers):
        z = (torch.randn(n, SIZE, SIZE, SIZE, c, generator=g) * 1.5).to(DEV, torch.bfloat16)
        x6 = torch.zeros(n, SIZE, SIZE, SIZE, 16)
        x6[..., :6] = torch.rand(n, SIZE, SIZE, SIZE, 6, generator=g)
        x24 = torch.zeros(n, SIZE, SIZE, SIZE, c)
        x24[..., :24] = torch.rand(n, SIZE, SIZE, SIZE, 24, generator=g)
        sets.append((z, x6.to(DEV, torch.bfloat16), x24.to(DEV, torch.bfloat16)))
    mean, rstd = torch.zeros(1, c, device=DEV), torch.ones(1, c, device=DEV)
    gamma, beta = (torch.rand(24, generator=g) + 0.5).to(DEV), (torch.rand(24, generator=g) - 0.5).to(DEV)
    rw, rb = ((torch.rand(24, 6, generator=g) - 0.5)).to(DEV), (torch.rand(24, generator=g) - 0.5).to(DEV)
    count = [0]

    def launch(kind):
        z, x6, x24 = sets[count[0] % buffers]
        count[0] += 1
        if kind == "normact_fwd":
            ops.normact_fwd(z, 1, mean, rstd, gamma, beta, 0.0)
        elif kind == "restail_proj6":
            ops.restail_fwd(z, x6, 1, mean, rstd, gamma, beta, 24, 6, rw, rb)
        else:
            ops.restail_fwd(z, x24, 1, mean, rstd, gamma, beta, 24, 24)

    def runner(kind):
        # the window's launches as one captured graph: the host's share of a ~50 us launch does not enter the time
        launch(kind)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(launches):
                launch(kind)
        return lambda: timed(graph.replay) / launches
    bytes_per_row = {"normact_fwd": 2 * c + 2 * c, "restail_proj6": 2 * c + 2 * 16 + 2 * c, "restail_identity": 2 * c + 2 * c + 2 * c}
    times = rounds({k: runner(k) for k in bytes_per_row}, reps)
    res = {}
    for k, v in times.items():
        nbytes = bytes_per_row[k] * rows
        s = summary(f"launch_{k}", v, launches_per_round=launches, rows=rows, channels=c, dtype="bf16", buffer_sets=buffers, bytes=nbytes)
        s["tb_per_s"] = round(nbytes / (s["median_ms"] * 1e-3) / 1e12, 3)
        s["share_of_hbm_peak_8tbs"] = round(s["tb_per_s"] / HBM_PEAK_TBS, 3)
        s["share_of_hbm_achievable_6p3tbs"] = round(s["tb_per_s"] / HBM_ACHIEVABLE_TBS, 3)
        res[k] = s
    base = res["normact_fwd"]
    lines = list(res.values())
    for k in ("restail_proj6", "restail_identity"):
        ratio = bytes_per_row[k] / bytes_per_row["normact_fwd"]
        allowed = ratio * base["median_ms"] + (base["max_ms"] - base["min_ms"])
        lines.append(dict(what=f"launch_{k}_against_normact_fwd", byte_ratio=ratio, time_ratio=round(res[k]["median_ms"] / base["median_ms"], 3),
                          allowed_ms=round(allowed, 4), measured_ms=res[k]["median_ms"], over_allowed_ms=round(max(0.0, res[k]["median_ms"] - allowed), 4),
                          normact_range_ms=round(base["max_ms"] - base["min_ms"], 4)))
    return lines


def main(a):
    lines = []
    if not a.only_kernel:
        lines += bench_steps(a.reps, a.replays)
    if not a.only_steps:
        lines += bench_kernel(a.reps, a.launches, a.buffers)
    for l in lines:
        print(json.dumps(l), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--launches", type=int, default=200, help="part 2: launches per timed window")
    ap.add_argument("--buffers", type=int, default=4, help="part 2: sets of tensors the launches rotate over")
    ap.add_argument("--only-kernel", action="store_true")
    ap.add_argument("--only-steps", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    main(args)
