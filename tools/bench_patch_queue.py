"""Device patch queue (data.PatchQueue) at the reference's shapes: batches of 8 x (24 + 6) x 64^3 patches out of
96x128x128 subjects, device-event timing after warm-up.  Lines:
  - one fused launch per batch with no stage firing and with all three forced (bias field, noise, gamma);
  - bytes moved (patches written + read, computed from shapes) and their share of the HBM peak (8 TB/s spec,
    MI355X_MICROARCH.md) -- an upper bound: every timed batch is a fresh plan, but overlapping patches of one subject
    can still be served by the caches;
  - the same batch built by the chained path (crop_or_pad + the augmentation objects + extract_patches);
  - the bf16 8 x 64^3 graphed training step fed by next_batch(out=static batch) against the same step on its static
    batch, alternated block by block in one run.
Prints one JSON line.  ``--skip-step`` leaves the training-step lines out (the profile run)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unet_bssfp_amd import augment as A  # noqa: E402
from unet_bssfp_amd import data as Q  # noqa: E402
from unet_bssfp_amd.inference import extract_patches  # noqa: E402

HBM_PEAK = 8.0e12    # B/s, spec (MI355X_MICROARCH.md; 6.29 TB/s measured for a float4 copy)
DEV = "cuda:0"


def timed(fn, iters=20, warmup=3):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def subjects(n):
    g = torch.Generator(device=DEV).manual_seed(0)
    return [{"bssfp": {"data": torch.rand(24, 96, 128, 128, generator=g, device=DEV)},
             "dwi-tensor": {"data": torch.rand(6, 96, 128, 128, generator=g, device=DEV)}} for _ in range(n)]


def fresh_plans(q, rng, n, forced, batch=8):
    """n batches, each from two loads of the next pair of subjects (one straddle) at fresh origins, so that no batch
    re-reads what the previous one read; ``forced``: every stage fires"""
    plans, hi = [], [t - p for t, p in zip(q.target_shape, q.patch_size)]
    for k in range(n):
        loads = []
        for i in range(2):
            stages = ((q.transform[0], (rng.random(20) - 0.5).astype(np.float32) * 0.2),
                      (q.transform[1], (0.0, 0.05, int(rng.integers(0, 2 ** 62)))),
                      (q.transform[2], 1.1)) if forced else ()
            loads.append(Q.SubjectLoad(q.indices[(2 * k + i) % len(q.indices)], 0, k, 0, stages))
        plans.append([Q.PlannedPatch(loads[b % 2], tuple(int(rng.integers(0, h + 1)) for h in hi)) for b in range(batch)])
    return plans


def chained(q, plan, out):
    """crop_or_pad + augmentation objects + extract_patches, per subject load (the unfused path)"""
    for name, src, aug in (("bssfp", "bssfp", True), ("dwi-tensor_orig", "dwi-tensor", False)):
        parts, order = [], []
        for load in {id(p.load): p.load for p in plan}.values():
            x = A.crop_or_pad(q._by_index[load.subject][src]["data"], q.target_shape)
            if aug:
                for t, params in load.stages:
                    x = t.apply(x, params)
            mine = [b for b, p in enumerate(plan) if p.load is load]
            locs = np.array([list(plan[b].origin) + [o + s for o, s in zip(plan[b].origin, q.patch_size)] for b in mine])
            parts.append(extract_patches(x, locs, q.patch_size))
            order += mine
        out[name] = torch.cat(parts)[torch.from_numpy(np.argsort(order)).to(DEV)]
    return out


def step_lines(q, res, blocks=6, per_block=20):
    import unet_bssfp_amd as M
    from unet_bssfp_amd.gan import GraphedTrainingStep, bSSFPToDWITensorModel, synthetic_batch
    torch.manual_seed(0)
    model = bSSFPToDWITensorModel("bssfp", gen=M.Generator("bssfp", dropout=0.05), discr=M.Discriminator("bssfp")).to(DEV).train()
    M.set_compute_dtype(model, M.compute_dtype_from_name("bf16"))
    gstep = GraphedTrainingStep(model, synthetic_batch(8, 64, seed=1234, device=DEV), warmup=2)
    static = gstep.instances[0][0]

    def fed():
        q.next_batch(8, out=static)
        gstep()
    for _ in range(20):
        fed()
    torch.cuda.synchronize()
    ms = {"static": [], "fed": []}
    for blk in range(blocks):
        for name, fn in (("static", gstep), ("fed", fed)) if blk % 2 == 0 else (("fed", fed), ("static", gstep)):
            ms[name].append(timed(fn, iters=per_block, warmup=2))
    torch.cuda.synchronize()
    logs = torch.stack([v.reshape(()).float() for v in model.last_logs.values()])
    s, f = float(np.median(ms["static"])), float(np.median(ms["fed"]))
    res["step_8x64_static_ms"] = round(s, 3)
    res["step_8x64_fed_ms"] = round(f, 3)
    res["step_fed_over_static"] = round(f / s, 4)
    res["step_blocks_ms"] = {k: [round(v, 3) for v in vs] for k, vs in ms.items()}
    res["step_patches_per_s_fed"] = round(8 * 1000.0 / f, 1)
    res["step_logs_finite"] = bool(torch.isfinite(logs).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    subs = subjects(4)
    q = Q.PatchQueue(subs, "bssfp", seed=0)                 # reference defaults: 96x128x128, 64^3, max_length 16, 8 per volume
    rng = np.random.default_rng(0)
    pv = 64 ** 3
    written = 8 * (24 + 6) * pv * 4
    res = {"batch": "8 x (24 + 6) x 64^3 f32", "subjects": "4 x (24 + 6) x 96x128x128 f32", "measured": True}
    out = {"bssfp": {"data": torch.empty(8, 24, 64, 64, 64, device=DEV)},
           "dwi-tensor_orig": {"data": torch.empty(8, 6, 64, 64, 64, device=DEV)}}
    warmup, iters = 3, 20
    for name, forced in (("no_stage", False), ("all_stages", True)):
        plans = iter(fresh_plans(q, rng, warmup + iters, forced))
        ms = timed(lambda: q.gather(next(plans), out=out), iters=iters, warmup=warmup)
        res[f"fused_{name}_ms"] = round(ms, 4)
        # bytes computed from shapes over device time; overlapping patches of one subject can be served by the caches,
        # so this is an upper bound on the share of HBM bandwidth the batch uses
        res[f"fused_{name}_hbm_fraction_upper_bound"] = round(2 * written / (ms * 1e-3) / HBM_PEAK, 3)
        plan = fresh_plans(q, rng, 1, forced)[0]
        cout = {}
        ms_c = timed(lambda: chained(q, plan, cout), iters=5, warmup=1)
        res[f"chained_{name}_ms"] = round(ms_c, 3)
        res[f"chained_over_fused_{name}"] = round(ms_c / ms, 1)
        q.gather(plan, out=out)
        res[f"fused_equals_chained_{name}"] = all(torch.equal(out[k]["data"], cout[k]) for k in cout)
    res["bytes_written"] = written
    res["bytes_read_min"] = written                            # every patch voxel read once (computed, not counted)
    ms = timed(lambda: q.next_batch(8, out=out), iters=50)
    res["next_batch_reference_transform_ms"] = round(ms, 4)   # host plan + launch, p = 0.1 stages
    if not a.skip_step:
        step_lines(q, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
