"""DTI error table (eval.error_table) per subject: f32 channels-first tensors, R = 3, device-event timing after
warm-up.  Full mask (every voxel decomposed twice) and a ball mask (~52 % of the volume, voxels outside skip
the decompositions); ratio to two calc_scalar_maps calls on the same volume; the numpy oracle's time on the
96x128x128 input for the record.  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from unet_bssfp_amd import eval as E  # noqa: E402


def timed(fn, iters=10, warmup=3):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def subject(shape, seed=0):
    from oracle import dti_ref
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.from_numpy(np.moveaxis(dti_ref.synthetic_tensor_field((64, 64, 64), seed=seed), -1, 0).astype(np.float32)).cuda()
    reps = [1] + [-(-s // 64) for s in shape]
    target = t.repeat(*reps)[:, :shape[0], :shape[1], :shape[2]].contiguous()
    pred = target * (1 + 0.1 * torch.randn(target.shape, generator=g, device="cuda"))
    ps = torch.rand((3,) + tuple(shape), generator=g, device="cuda") ** 3
    ps /= ps.sum(0, keepdim=True)
    ax = [torch.linspace(-1, 1, s, device="cuda") for s in shape]
    zz, yy, xx = torch.meshgrid(*ax, indexing="ij")
    ball = ((zz ** 2 + yy ** 2 + xx ** 2) < 1.0).to(torch.uint8)
    return pred, target, ball, ps


def main():
    out = {"dtype": "f32", "layout": "channels_first", "nroi": 3}
    for name, shape in (("96x128x128", (96, 128, 128)), ("256^3", (256, 256, 256))):
        pred, target, ball, ps = subject(shape)
        nvox = ball.numel()
        full = torch.ones_like(ball)
        ms_full = timed(lambda: E.error_table(pred, target, full, ps, channels_first=True))
        ms_ball = timed(lambda: E.error_table(pred, target, ball, ps, channels_first=True))
        ms_maps = timed(lambda: (E.calc_scalar_maps(pred, channels_first=True), E.calc_scalar_maps(target, channels_first=True)))
        out[name] = {"ms_full_mask": round(ms_full, 3), "gvox_s_full_mask": round(nvox / ms_full / 1e6, 2),
                     "ms_ball_mask": round(ms_ball, 3), "ball_fraction": round(ball.float().mean().item(), 3),
                     "ms_two_scalar_maps": round(ms_maps, 3), "ratio_full_to_two_scalar_maps": round(ms_full / ms_maps, 3)}
        if name == "96x128x128":
            import dti_errors_ref as ref
            a = [np.moveaxis(x.cpu().numpy(), 0, -1) for x in (pred, target, ps)]
            m = ball.cpu().numpy()
            t0 = time.perf_counter()
            want, _ = ref.error_table(a[0], a[1], m, a[2])
            out[name]["numpy_oracle_s"] = round(time.perf_counter() - t0, 2)
            got = E.error_table(pred, target, ball, ps, channels_first=True).cpu().numpy()
            out[name]["max_rel_diff_vs_oracle"] = float(np.nanmax(np.abs(got - want) / np.abs(want)))
        del pred, target, ball, ps, full
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
