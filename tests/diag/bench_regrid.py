"""Microbenchmark of the regridding kernels: the cubic B-spline prefilter of 1 and 24 channels of a
176 x 240 x 256 volume (a 1 mm MP2RAGE-sized grid; the W, H and D passes apart, from calls that run one, two and three of
them), ``regrid`` of those onto 96 x 128 x 128 at each order, and order 1 at equal shape next to ``augment.rigid_resample`` on
the same tensor, which moves the same bytes.  Each as the hipEvent mean of ``--iters`` calls after warm-up with caller-owned
buffers: ms, algorithmic bytes per voxel (every source byte read once, every result byte written once) and their share of
the 8 TB/s HBM figure the project uses."""
import argparse, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from unet_bssfp_amd import _lib, augment as A, preprocess as P

ap = argparse.ArgumentParser()
ap.add_argument("--src", type=int, nargs=3, default=(176, 240, 256))
ap.add_argument("--dst", type=int, nargs=3, default=(96, 128, 128))
ap.add_argument("--channels", type=int, nargs="+", default=(1, 24))
ap.add_argument("--iters", type=int, default=300)
a = ap.parse_args()
src, dst = tuple(a.src), tuple(a.dst)
dev = "cuda:0"
HBM = 8000.0                                                # GB/s


def timed(name, fn, voxels, bytes_per_voxel, **extra):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    gbs = voxels * bytes_per_voxel / ms / 1e6
    print(json.dumps(dict(kernel=name, voxels=voxels, ms=round(ms, 4), bytes_per_voxel=round(bytes_per_voxel, 2),
                          achieved_gbs=round(gbs, 1), hbm_frac=round(gbs / HBM, 4), **extra)), flush=True)
    return ms


lib = _lib.load()
stream = torch.cuda.current_stream().cuda_stream
c_, s_ = np.cos(0.1), np.sin(0.1)
m = np.zeros((3, 4))                                        # a rotated, downsampling read about the centre: mostly inside
m[:, :3] = np.array([[c_, -s_, 0], [s_, c_, 0], [0, 0, 1.0]]) @ np.diag(np.asarray(src, np.float64) / np.asarray(dst, np.float64))
m[:, 3] = (np.asarray(src) - 1) / 2 - m[:, :3] @ ((np.asarray(dst) - 1) / 2)

for c in a.channels:
    svox, ovox = c * int(np.prod(src)), c * int(np.prod(dst))
    x = torch.rand((c,) + src, device=dev)
    coef = torch.zeros((c,) + src, dtype=torch.float64, device=dev)
    out = torch.zeros((c,) + dst, device=dev)
    t_all = timed("bspline_prefilter", lambda: P.bspline_coefficients(x, out=coef), svox, 12, channels=c, passes="W H D")
    if c * src[0] * src[1] <= 65536:                       # the passes apart: the same bytes as rows of one, two, three axes
        d, h, w = src
        one = lambda cc, dd, hh: _lib.check(lib.mi355_bspline_prefilter(x.data_ptr(), coef.data_ptr(), cc, dd, hh, w, stream))   # noqa: E731
        t_w = timed("bspline_prefilter", lambda: one(c * d * h, 1, 1), svox, 12, channels=c, passes="W")
        t_wh = timed("bspline_prefilter", lambda: one(c * d, 1, h), svox, 12, channels=c, passes="W H")
        print(json.dumps(dict(kernel="bspline_prefilter", channels=c, pass_ms=dict(W=round(t_w, 4), H=round(t_wh - t_w, 4),
                                                                                    D=round(t_all - t_wh, 4)),
                              note="H and D by difference; the W pass reads f32 and writes f64 (12 B / voxel), H and D read and "
                                   "write f64 in place (16 B / voxel and the start sum's second read)")))
        P.bspline_coefficients(x, out=coef)
    for how, source, sbytes in (("nearest", x, 4), ("linear", x, 4), ("bspline", coef, 8)):
        timed(f"regrid_{how}", lambda: P.regrid(source, m, dst, how, 0.0, out=out), ovox, 4 + sbytes * svox / ovox, channels=c,
              src=src, dst=dst, taps={"nearest": 1, "linear": 8, "bspline": 64}[how])
    del coef
    y = torch.rand((c,) + dst, device=dev)
    rot = np.concatenate([np.array([[c_, -s_, 0], [s_, c_, 0], [0, 0, 1.0]]), np.zeros((3, 1))], 1)
    rot[:, 3] = (np.asarray(dst) - 1) / 2 - rot[:, :3] @ ((np.asarray(dst) - 1) / 2)
    timed("regrid_linear_equal_shape", lambda: P.regrid(y, rot, dst, "linear", 0.0, out=out), ovox, 8, channels=c, shape=dst)
    timed("augment_rigid_resample", lambda: A.rigid_resample(y, rot, fill=0.0), ovox, 8, channels=c, shape=dst,
          note="f32 coordinates; allocates its result per call")
    del x, y, out
