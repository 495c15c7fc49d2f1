"""The rigid resampler and RandomMotion on the device (csrc/motion.hip) at the reference's shapes, device-event timing
after warm-up, one JSON line.  On a 24 x 96x128x128 and a 6-channel f32 volume, K = 2:
  - ``rigid_resample`` (channel minima + one launch) and the resampling launch alone with a given fill value;
  - fused ``RandomMotion.apply`` against the chained form (K + 1 stand-alone resamples and passes of ``axis_apply``,
    summed), interleaved call by call in the same run;
  - bytes moved, computed from shapes (one read + one write of the volume per launch that writes one; the f64 sum / min
    launch reads the volume once), and their share of the HBM peak (8 TB/s spec).
``--queue``: ms per 8 x (24 + 6) x 64^3 batch with the six-stage and the seven-stage transform at the natural p = 0.1 over
400 batches, and with all seven forced.  ``--step``: the bf16 8 x 64^3 graphed training step fed by the seven-stage queue
against the same step fed by the six-stage queue, alternated block by block.  Every figure is echoed on stderr as soon as
it exists."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_kspace import DEV, line, note, queue_lines, step_lines, subjects, timed  # noqa: E402
from unet_bssfp_amd import augment as A  # noqa: E402


def draw(seed=0):
    torch.manual_seed(seed)
    return A.RandomMotion().sample()


def stage_lines(res):
    mo = A.RandomMotion()
    p = draw()
    note(res, "times", [round(float(t), 4) for t in p.times])
    for c in (24, 6):
        x = torch.rand(c, 96, 128, 128, device=DEV)
        nbytes = x.numel() * 4
        tag = f"c{c}"
        ms = A.motion_matrices(p.degrees, p.translation, x.shape[1:])
        nb = len(A.motion_bands(p.times, x.shape[3]))
        line(res, f"{tag}_rigid_resample", timed(lambda: A.rigid_resample(x, ms[1])), 3, nbytes)
        line(res, f"{tag}_rigid_resample_given_fill", timed(lambda: A.rigid_resample(x, ms[1], fill=0.0)), 2, nbytes)
        # interleaved: fused, chained, fused, chained ... in one stream of calls, each timed by its own pair of events
        fused, chained = [], []
        for fn in (mo.apply, mo.apply_chained):
            for _ in range(3):
                fn(x, p)
        for _ in range(20):
            for fn, acc in ((mo.apply, fused), (mo.apply_chained, chained)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(x, p)
                e1.record()
                torch.cuda.synchronize()
                acc.append(e0.elapsed_time(e1))
        line(res, f"{tag}_motion_fused", float(np.mean(fused)), 3, nbytes)               # sum / min read, x read, y written
        line(res, f"{tag}_motion_chained", float(np.mean(chained)), 5 * nb + 3 * (nb - 1), nbytes)   # per image 3 + 2, per sum 3
        note(res, f"{tag}_fused_over_chained", round(float(np.mean(fused) / np.mean(chained)), 4))
        # the same pair back to back, as a queue issues them (no synchronisation between calls): alternating blocks of 20
        blocks = {"fused": [], "chained": []}
        for _ in range(3):
            blocks["fused"].append(timed(lambda: mo.apply(x, p), warmup=1))
            blocks["chained"].append(timed(lambda: mo.apply_chained(x, p), warmup=1))
        for name, v in blocks.items():
            note(res, f"{tag}_motion_{name}_back_to_back_ms", [round(t, 4) for t in v])
        note(res, f"{tag}_fused_over_chained_back_to_back", round(float(np.median(blocks["fused"]) / np.median(blocks["chained"])), 4))
        for name, fn in (("fused", mo.apply), ("chained", mo.apply_chained)):      # host time to enqueue one call
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                fn(x, p)
            note(res, f"{tag}_motion_{name}_host_enqueue_ms", round((time.perf_counter() - t0) / 20 * 1e3, 4))
            torch.cuda.synchronize()
        del x
        torch.cuda.empty_cache()


def forced_seven():
    tr = A.reference_full_transform()
    for t in tr:
        t.p = 1.0
    return tr


def queue_sets():
    return (("six_stage_p0.1", A.reference_training_transform(), 400),
            ("seven_stage_p0.1", A.reference_full_transform(), 400),
            ("seven_stage_forced", forced_seven(), 40))


def step_feeds():
    return {"six": A.reference_training_transform(), "seven": A.reference_full_transform()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queue", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--skip-stages", action="store_true")
    a = ap.parse_args()
    res = {"volume": "C x 96x128x128 f32"}
    if not a.skip_stages:
        stage_lines(res)
    if a.queue or a.step:
        subs = subjects(4)
        if a.queue:
            queue_lines(res, subs, queue_sets())
        if a.step:
            step_lines(res, subs, step_feeds())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
