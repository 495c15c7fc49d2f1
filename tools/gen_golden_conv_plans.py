"""Records the host-side plan table tests/golden/conv_plans.npz (checked by tests/test_conv_plans_host.py).

    python tools/gen_golden_conv_plans.py LIB                 # re-record the expected results from the library LIB
    python tools/gen_golden_conv_plans.py LIB --capture       # (GPU) also re-capture the real descriptors first

The table pins what both convolution planners answer for the sweeps of tests/conv_plan_cases.py and for the de-duplicated
descriptors of one eager training step per configuration of tests/test_conv_audit.py (captured through ops.CONV_PROBE /
ops.WGRAD_PROBE; pointers stored as null / non-null).  Without --capture the descriptor rows already in the table are kept
and only the answers are recorded, which needs no GPU.  LIB is a build of the commit whose plans are to be pinned: a
refactoring records from its parent and must pass unchanged; a deliberate planner change re-records and shows the diff
(the script prints how many rows changed)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "conv_plans.npz")


def capture():
    """The distinct descriptors of one eager training step per audit configuration, as integer rows."""
    import torch
    import conv_plan_cases as P
    import unet_bssfp_amd as M
    from unet_bssfp_amd import ops
    from unet_bssfp_amd.gan import bSSFPToDWITensorModel, synthetic_batch
    from test_conv_audit import CONFIGS
    fwd, wgrad = set(), set()
    ops.CONV_PROBE = lambda pid, d, real: fwd.add(tuple(P.flatten(d))) and None
    ops.WGRAD_PROBE = lambda kind, d: wgrad.add(tuple(P.flatten(d))) and None
    for name, (dtype, n, s, _, _) in CONFIGS.items():
        torch.manual_seed(0)
        model = bSSFPToDWITensorModel("bssfp", gen=M.Generator("bssfp", dropout=0.0).to("cuda:0"),
                                      discr=M.Discriminator("bssfp").to("cuda:0")).train()
        M.set_compute_dtype(model, dtype)
        model.training_step(synthetic_batch(n, s, seed=1234, device="cuda:0"), 0)
        torch.cuda.synchronize()
        print(f"{name}: {len(fwd)} forward, {len(wgrad)} weight-gradient descriptors so far")
        del model
        torch.cuda.empty_cache()
    ops.CONV_PROBE = ops.WGRAD_PROBE = None
    return np.array(sorted(fwd), dtype=np.int64), np.array(sorted(wgrad), dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib", help="library whose plans are recorded")
    ap.add_argument("--capture", action="store_true", help="run the training steps on the GPU and replace the real descriptors")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import tools.diaglib as D
    D.use(a.lib)
    import conv_plan_cases as P
    from unet_bssfp_amd import _lib
    lib = _lib.load()
    old = dict(np.load(a.out)) if os.path.exists(a.out) else {}
    if a.capture:
        fwd_rows, wgrad_rows = capture()
    else:
        fwd_rows, wgrad_rows = old["fwd_real_desc"], old["wgrad_real_desc"]
    new = {
        "fwd_columns": np.array(P.columns(_lib.ConvDesc)), "wgrad_columns": np.array(P.columns(_lib.WgradDesc)),
        "fwd_real_desc": fwd_rows, "wgrad_real_desc": wgrad_rows,
        "fwd_real": P.table(lib, P.query_fwd, [P.unflatten(_lib.ConvDesc, r) for r in fwd_rows], 5),
        "wgrad_real": P.table(lib, P.query_wgrad, [P.unflatten(_lib.WgradDesc, r) for r in wgrad_rows], 2),
        "fwd_sweep": P.table(lib, P.query_fwd, P.fwd_sweep(), 5),
        "wgrad_sweep": P.table(lib, P.query_wgrad, P.wgrad_sweep(), 2),
    }
    for k in ("fwd_real", "wgrad_real", "fwd_sweep", "wgrad_sweep"):
        same = k in old and old[k].shape == new[k].shape
        changed = int((old[k] != new[k]).any(1).sum()) if same else len(new[k])
        print(f"{k}: {len(new[k])} rows, {changed} changed, {len(np.unique(new[k][:, 0]))} distinct plans / kinds")
    np.savez_compressed(a.out, **new)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
