"""Microbenchmark of the preprocessing kernels on one 96 x 128 x 128 volume: the OLS and WLS tensor fits
(N = 64 measurements -- an ASSUMPTION, the thesis does not state the direction count), phase_correct + assemble_bssfp
(12 cycles) and the range pass, each as ms per call, algorithmic bytes per voxel (fit: 4 N in + 4 per output) against the 8 TB/s
HBM figure the project uses, and the f64 numpy restatement on one CPU core beside it."""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from unet_bssfp_amd import preprocess as P
from tests import preprocess_ref as R

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, nargs=3, default=(96, 128, 128))
ap.add_argument("--meas", type=int, default=64)
ap.add_argument("--cycles", type=int, default=12)
ap.add_argument("--iters", type=int, default=300)
ap.add_argument("--cpu-voxels", type=int, default=20000)
a = ap.parse_args()
grid, n, p = tuple(a.grid), a.meas, a.cycles
nvox = int(np.prod(grid))
dev = "cuda:0"
HBM = 8000.0                                                # GB/s


def timed(name, fn, bytes_per_voxel, **extra):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    gbs = nvox * bytes_per_voxel / ms / 1e6
    print(json.dumps(dict(kernel=name, voxels=nvox, ms=round(ms, 4), gvox_per_s=round(nvox / ms / 1e6, 3),
                          bytes_per_voxel=bytes_per_voxel, achieved_gbs=round(gbs, 1), hbm_frac=round(gbs / HBM, 4), **extra)))
    return ms


b, g = R.scheme(n)
table = P.gradient_table(b, g)
design = R.design_matrix(b, g)
d6, s0 = R.tensor_field(4096, seed=1)
sig = torch.from_numpy(R.signals(d6, s0, design).astype(np.float32)).to(dev)                 # (4096, n)
dwi = sig[torch.randint(0, 4096, (nvox,), device=dev)].t().contiguous().reshape((n,) + grid)   # [N][D][H][W]
out = torch.zeros((6,) + grid, device=dev)
mask = (torch.rand(grid, device=dev) < 0.8).to(torch.uint8)
for method in ("ols", "wls"):
    ms = timed(f"dtifit_{method}", lambda: P.fit_tensor(dwi, table, method, out=out), 4 * n + 4 * 6, meas=n)
    print(json.dumps(dict(kernel=f"dtifit_{method}", f64_logs_per_s=round(nvox * n / ms / 1e6, 2), unit="G log / s")))
    timed(f"dtifit_{method}_masked_norm", lambda: P.fit_tensor(dwi, table, method, mask=mask, norm=(-1e-3, 3e-3), out=out),
          4 * n + 4 * 6 + 1, meas=n)
nii = dwi.movedim(0, -1).contiguous()
timed("dtifit_ols_interleaved_in", lambda: P.fit_tensor(nii, table, "ols", channels_first=False, out=out), 4 * n + 4 * 6, meas=n)
del nii

mag = torch.rand((p,) + grid, device=dev) * 1000
raw = torch.randint(0, 4096, (p,) + grid, device=dev).float()
re, im = torch.zeros_like(mag), torch.zeros_like(mag)
asm = torch.zeros((2 * p,) + grid, device=dev)
timed("bssfp_phase_correct", lambda: P.phase_correct(mag, raw, out=(re, im)), 2 * 8 * p + 8 * p, cycles=p,
      note="two reads of mag and phase (sums, then rotation) + re, im written")
timed("bssfp_assemble", lambda: P.assemble_bssfp(re, im, mask, (0.0, 1000.0), (-np.pi, np.pi), out=asm), 8 * p + 8 * p + 1, cycles=p)
timed("bssfp_assemble_one_cycle", lambda: P.assemble_bssfp(re, im, mask, (0.0, 1000.0), (-np.pi, np.pi), 0, out=asm), 8 + 8 * p + 1,
      cycles=p)
acc = P.RangeAccumulator(2 * p, P.bssfp_groups(2 * p), dev)
timed("channel_minmax", lambda: acc.update(asm, mask), 4 * 2 * p + 1, channels=2 * p)
t1 = torch.rand(grid, device=dev) * 3000
t1o = torch.zeros((6,) + grid, device=dev)
timed("normalize_channels_t1w", lambda: P.assemble_t1w(t1, mask, (0.0, 3000.0), out=t1o), 4 + 4 * 6 + 1, channels=6)

# the restatement on one CPU core
torch.set_num_threads(1)
s = sig.cpu().numpy().astype(np.float64)[np.random.default_rng(0).integers(0, 4096, a.cpu_voxels)]
t = time.perf_counter(); R.fit_ols(s, table.pinv); t_ols = time.perf_counter() - t
t = time.perf_counter(); R.fit_wls_cholesky(s, design, table.pinv); t_wls = time.perf_counter() - t
print(json.dumps(dict(cpu_restatement_voxels=a.cpu_voxels, meas=n, ols_s=round(t_ols, 4), ols_mvox_per_s=round(a.cpu_voxels / t_ols / 1e6, 4),
                      wls_cholesky_s=round(t_wls, 4), wls_mvox_per_s=round(a.cpu_voxels / t_wls / 1e6, 4),
                      kind="vectorised numpy, f64 (BLAS threads are not pinned by this script: run under OMP_NUM_THREADS=1)")))
