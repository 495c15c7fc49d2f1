"""RandomGhosting / RandomSpike / RandomBlur on the device (csrc/kspace.hip) at the reference's shapes, device-event
timing after warm-up, one JSON line.  Per stage, alone, on a 24 x 96x128x128 and a 6-channel f32 volume:
  - ghosting per axis, blur at a sigma with radius >= 1 (three passes), both spike paths (DC: one f64 sum + the wave add;
    DFT: three complex passes, the last one reducing, + the wave add);
  - bytes moved, computed from shapes (one read + one write of the volume per pass; a complex plane counts as a volume),
    and their share of the HBM peak (8 TB/s spec, MI355X_MICROARCH.md; 6.29 TB/s measured for a float4 copy);
  - with ``--comparators``, next to each, the same stage restated with torch.fft / F.conv1d on the GPU (a comparator
    only: the package itself uses neither).  Every figure is echoed on stderr as soon as it exists.
``--queue``: ms per 8 x (24 + 6) x 64^3 batch with the three-stage and the six-stage transform at the natural p = 0.1,
averaged over enough fills to see staging, and with every stage forced.  ``--step``: the bf16 8 x 64^3 graphed training
step fed by the six-stage queue against the same step fed by the three-stage queue, alternated block by block."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unet_bssfp_amd import augment as A  # noqa: E402
from unet_bssfp_amd import data as Q  # noqa: E402

HBM_PEAK = 8.0e12
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


def note(res, key, value):
    """record one figure and echo it on stderr at once, so that a run that is cut short still shows how far it got"""
    res[key] = value
    print(f"{key} = {value}", file=sys.stderr, flush=True)


def line(res, key, ms, volumes_moved, nbytes):
    note(res, key + "_ms", round(ms, 4))
    note(res, key + "_hbm_fraction", round(volumes_moved * nbytes / (ms * 1e-3) / HBM_PEAK, 3))


def fft_ghosting(x, n, axis, intensity):
    """comparator: the 1-D form through torch.fft along the axis"""
    s = torch.fft.fftshift(torch.fft.fft(x, dim=1 + axis), dim=1 + axis)
    m = torch.ones(x.shape[1 + axis], device=x.device)
    m[::n] = 1 - intensity
    m[x.shape[1 + axis] // 2] = 1
    shape = [1, 1, 1, 1]
    shape[1 + axis] = -1
    return torch.fft.ifft(torch.fft.ifftshift(s * m.view(shape), dim=1 + axis), dim=1 + axis).real


def fft_spike(x, pos, intensity):
    """comparator: the literal 3-D form through torch.fft (maximum by real part)"""
    s = torch.fft.fftshift(torch.fft.fftn(x, dim=(1, 2, 3)), dim=(1, 2, 3))
    idx = [int(np.floor(p * n)) for p, n in zip(pos, x.shape[1:])]
    flat = s.reshape(x.shape[0], -1)
    k = flat.real.argmax(1, keepdim=True)
    s[:, idx[0], idx[1], idx[2]] += flat.gather(1, k)[:, 0] * intensity
    return torch.fft.ifftn(torch.fft.ifftshift(s, dim=(1, 2, 3)), dim=(1, 2, 3)).real


def conv_blur(x, sigmas):
    """comparator: F.conv1d per axis on a padded volume (torch's 'reflect' does not repeat the edge voxel as scipy's does:
    a timing comparator, not a parity reference)"""
    for axis, sigma in enumerate(sigmas):
        r = A.blur_radius(sigma)
        if r == 0:
            continue
        t = torch.arange(-r, r + 1, device=x.device, dtype=torch.float32)
        w = torch.exp(-0.5 * t * t / (sigma * sigma))
        w = (w / w.sum()).view(1, 1, -1)
        y = x.movedim(1 + axis, -1)
        shp = y.shape
        y = F.pad(y.reshape(-1, 1, shp[-1]), (r, r), mode="reflect")
        x = F.conv1d(y, w).reshape(shp).movedim(-1, 1 + axis).contiguous()
    return x


def stage_lines(res, comparators):
    for c in (24, 6):
        x = torch.rand(c, 96, 128, 128, device=DEV)
        nbytes = x.numel() * 4
        tag = f"c{c}"
        gh, sp, bl = A.RandomGhosting(), A.RandomSpike(), A.RandomBlur()
        for axis in range(3):
            line(res, f"{tag}_ghosting_axis{axis}", timed(lambda: gh.apply(x, (5, axis, 0.7))), 2, nbytes)
            if comparators:
                note(res, f"{tag}_ghosting_axis{axis}_torch_fft_ms", round(timed(lambda: fft_ghosting(x, 5, axis, 0.7), iters=5, warmup=2), 4))
        m = {axis: A._upload(A.ghosting_matrix(x.shape[1 + axis], 5, 0.7), DEV) for axis in range(3)}
        for axis in range(3):                                         # the kernel alone: the matrix already on the device
            line(res, f"{tag}_axis_apply_axis{axis}", timed(lambda: A.axis_apply(x, m[axis], axis)), 2, nbytes)
        sig = (0.6, 1.5, 0.9)
        line(res, f"{tag}_blur_3_passes", timed(lambda: bl.apply(x, sig)), 6, nbytes)
        if comparators:
            note(res, f"{tag}_blur_conv1d_ms", round(timed(lambda: conv_blur(x, sig), iters=5, warmup=2), 4))
        pos = np.array([[0.31, 0.52, 0.77]])
        line(res, f"{tag}_spike_dc", timed(lambda: sp.apply(x, A.SpikeParams(0.05, pos, "dc"))), 3, nbytes)
        # DFT path: W pass 1 read + 2 written, H pass 2 + 2, D pass 2 read, wave add 1 + 1
        line(res, f"{tag}_spike_dft", timed(lambda: sp.apply(x, A.SpikeParams(0.05, pos, "dft")), iters=10), 11, nbytes)
        if comparators:
            note(res, f"{tag}_spike_torch_fft_ms", round(timed(lambda: fft_spike(x, pos[0], 0.05), iters=5, warmup=2), 4))
        del x
        torch.cuda.empty_cache()


def subjects(n):
    g = torch.Generator(device=DEV).manual_seed(0)
    return [{"bssfp": {"data": torch.rand(24, 96, 128, 128, generator=g, device=DEV)},
             "dwi-tensor": {"data": torch.rand(6, 96, 128, 128, generator=g, device=DEV)}} for _ in range(n)]


def forced_six():
    tr = A.reference_training_transform()
    for t in tr:
        t.p = 1.0
    return tr


def queue_lines(res, subs, sets=None):
    """``sets``: (name, transform, batches) per line; the default compares the three-stage and the six-stage transform"""
    out = {"bssfp": {"data": torch.empty(8, 24, 64, 64, 64, device=DEV)},
           "dwi-tensor_orig": {"data": torch.empty(8, 6, 64, 64, 64, device=DEV)}}
    if sets is None:
        sets = (("three_stage_p0.1", A.reference_augmentation(), 400),
                ("six_stage_p0.1", A.reference_training_transform(), 400),     # 400 batches = 200 fills
                ("six_stage_forced", forced_six(), 40))
    for name, tr, iters in sets:
        q = Q.PatchQueue(subs, "bssfp", transform=tr, seed=0)
        note(res, f"queue_{name}_ms_per_batch", round(timed(lambda: q.next_batch(8, out=out), iters=iters, warmup=4), 4))
        note(res, f"queue_{name}_fills", q.fill_count)


def step_lines(res, subs, feeds=None, blocks=6, per_block=20):
    """``feeds``: {name: transform, or None for the static batch}, in the order in which each is compared with the one
    before it; the default is static, three-stage, six-stage"""
    import unet_bssfp_amd as M
    from unet_bssfp_amd.gan import GraphedTrainingStep, bSSFPToDWITensorModel, synthetic_batch
    torch.manual_seed(0)
    model = bSSFPToDWITensorModel("bssfp", gen=M.Generator("bssfp", dropout=0.05), discr=M.Discriminator("bssfp")).to(DEV).train()
    M.set_compute_dtype(model, M.compute_dtype_from_name("bf16"))
    gstep = GraphedTrainingStep(model, synthetic_batch(8, 64, seed=1234, device=DEV), warmup=2)
    static = gstep.instances[0][0]
    if feeds is None:
        feeds = {"static": None, "three": A.reference_augmentation(), "six": A.reference_training_transform()}
    queues = {k: Q.PatchQueue(subs, "bssfp", transform=tr, seed=0) for k, tr in feeds.items() if tr is not None}

    def fed(q):
        q.next_batch(8, out=static)
        gstep()
    for _ in range(10):
        for q in queues.values():
            fed(q)
    torch.cuda.synchronize()
    runs = {k: (lambda q=queues[k]: fed(q)) if k in queues else gstep for k in feeds}
    ms = {k: [] for k in runs}
    names = list(runs)
    for blk in range(blocks):
        r = blk % len(names)
        for name in names[r:] + names[:r]:
            ms[name].append(timed(runs[name], iters=per_block, warmup=2))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    logs = torch.stack([v.reshape(()).float() for v in model.last_logs.values()])
    res["step_8x64_ms"] = {k: round(v, 3) for k, v in med.items()}
    res["step_blocks_ms"] = {k: [round(v, 3) for v in vs] for k, vs in ms.items()}
    for a, b in zip(names, names[1:]):
        res[f"step_{b}_over_{a}"] = round(med[b] / med[a], 4)
    res["step_logs_finite"] = bool(torch.isfinite(logs).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queue", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--skip-stages", action="store_true")
    ap.add_argument("--comparators", action="store_true", help="also time the torch.fft / F.conv1d restatements "
                    "(the first torch.fft call of each length builds its plan, which can take minutes)")
    a = ap.parse_args()
    res = {"volume": "C x 96x128x128 f32"}
    if not a.skip_stages:
        stage_lines(res, a.comparators)
    if a.queue or a.step:
        subs = subjects(4)
        if a.queue:
            queue_lines(res, subs)
        if a.step:
            step_lines(res, subs)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
