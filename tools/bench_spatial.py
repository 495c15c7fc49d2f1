"""Spatial augmentation in the patch feed (csrc/spatial.hip) at the reference's shapes: 24 + 6 channels,
target 96x128x128, batches of 8 x 64^3, transform=[] so that only the gather is timed.  Device events around blocks of
batches after a warm-up; the variants alternate block by block inside one run, and each figure is the median over the
rounds with its run-to-run spread (min .. max).  One JSON line on stdout; every figure is echoed on stderr at once.
  (i)   plain     : the plain feed, the launch a queue without spatial stages takes;
  (ii)  flip      : a flip of all three axes in every load, fused into the gather;
  (iii) affine    : an affine in every load, fused into the gather;
  (iv)  chained   : the comparator made of the stand-alone pieces: per load and image crop_or_pad + rigid_resample into a
                    staging tensor, then the plain gather from it.  With 8 samples per volume and batches of 8 an epoch
                    has as many batches as loads, so one load (two images) is staged per batch.  rigid_resample gets a
                    given fill, which spares the comparator the channel-minimum pass that the fused form never runs.
``--raw D H W`` gives the subjects another raw extent than the target (then (iv) also pays a real crop / pad pass)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_kspace import DEV, note  # noqa: E402
from unet_bssfp_amd import augment as A  # noqa: E402
from unet_bssfp_amd import data as Q  # noqa: E402

TARGET = (96, 128, 128)


def subjects(n, raw):
    g = torch.Generator(device=DEV).manual_seed(0)
    return [{"bssfp": {"data": torch.rand(24, *raw, generator=g, device=DEV)},
             "dwi-tensor": {"data": torch.rand(6, *raw, generator=g, device=DEV)}} for _ in range(n)]


def block(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--raw", type=int, nargs=3, default=list(TARGET))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, default=16, help="batches per block")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    raw = tuple(a.raw)
    subs = subjects(4, raw)
    staged_subs = subjects(4, TARGET) if raw != TARGET else subs
    out = {name: {"data": torch.empty(8, c, 64, 64, 64, device=DEV)} for name, c in (("bssfp", 24), ("dwi-tensor_orig", 6))}

    def queue(s, **kw):
        return Q.PatchQueue(s, "bssfp", transform=[], seed=1, **kw)
    queues = {"plain": queue(subs),
              "flip": queue(subs, spatial=[A.RandomFlip(axes=(0, 1, 2), flip_probability=1.0)]),
              "affine": queue(subs, spatial=[A.RandomAffine()]),
              "chained": queue(staged_subs)}
    torch.manual_seed(0)
    matrix = A.affine_index_matrix(*A.RandomAffine().sample(), TARGET)
    turn = [0]

    def chained():
        sub = subs[turn[0] % len(subs)]
        turn[0] += 1
        staged = [A.rigid_resample(A.crop_or_pad(sub[name]["data"], TARGET), matrix, fill=0.0) for name in ("bssfp", "dwi-tensor")]
        queues["chained"].next_batch(8, out=out)
        return staged
    fns = {name: (lambda q=q: q.next_batch(8, out=out)) for name, q in queues.items() if name != "chained"}
    fns["chained"] = chained
    res = {"shapes": f"24 + 6 channels, raw {raw}, target {TARGET}, batch 8 x 64^3", "rounds": a.rounds, "batches_per_block": a.batches}
    for fn in fns.values():
        block(fn, 4)                                                  # warm-up
    times = {name: [] for name in fns}
    for _ in range(a.rounds):
        for name, fn in fns.items():                                  # the variants alternate inside the run
            times[name].append(block(fn, a.batches))
    for name, v in times.items():
        note(res, f"{name}_ms_per_batch", round(float(np.median(v)), 4))
        note(res, f"{name}_spread_ms", [round(float(min(v)), 4), round(float(max(v)), 4)])
    for name in ("flip", "affine", "chained"):
        note(res, f"{name}_over_plain", round(res[f"{name}_ms_per_batch"] / res["plain_ms_per_batch"], 3))
    note(res, "affine_over_chained", round(res["affine_ms_per_batch"] / res["chained_ms_per_batch"], 3))
    lo, hi = res["chained_spread_ms"]
    note(res, "affine_not_slower_than_chained_beyond_its_spread", bool(res["affine_ms_per_batch"] <= res["chained_ms_per_batch"] + (hi - lo)))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
