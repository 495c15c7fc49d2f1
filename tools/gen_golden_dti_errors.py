"""Golden vectors for the DTI relative-error table (tests/golden/dti_errors.npz).  Build machine only.

Runs the reference's OWN functions of src/eval.py on small synthetic subjects: ``do_invert_dwi_tensor_norm``,
``do_calc_scalar_maps``, ``do_calc_diff_maps``, ``do_calc_error_avg`` and the probseg-preparation loop of
``calc_error_table``.  They are AST-extracted and exec'd in memory with a stand-in ``nib`` that keeps the
"files" as arrays (the real pandas writes the per-file CSVs into a temporary directory, read back here).
Nothing from the reference is written to the repository: only numbers go to the .npz.

``do_calc_diff_maps`` is called with the kinds it tests for ('azimuth', 'inclination'); the driver
``calc_diff_maps`` passes '_azimuth' / '_inclination', which would send the angles through the relative
formula -- part of the file-name plumbing this project does not mirror.

Case c1: 10x12x16, R = 3, normalised tensors + (min_v, max_v), f32 mask with 0.5 (-> uint8 0) and 2.0 voxels;
         every in-mask voxel rejection-sampled so that LAPACK's principal eigenvectors of pred and target have
         z >= 0.1 (the angle columns are then free of the sign convention); edge voxels: a target component
         exactly 0 with pred != 0 (inf -> 0), pred == target, probseg just below / at / above 1e-5, zero
         tensors (0/0 = NaN) outside the mask.
Case c2: 4x5x6, no de-normalisation, one zero tensor pair INSIDE the mask (NaN columns in every ROI).
Case c3: 4x5x6, ROI 1 below the 1e-5 threshold inside the mask (a 0/0 = NaN row).

Usage:  python tools/gen_golden_dti_errors.py [--ref /root/reference] [--out tests/golden]
"""
import argparse
import ast
import os
import sys
import tempfile
import typing

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLUMNS = ("dxx", "dxy", "dxz", "dyy", "dyz", "dzz", "md", "fa", "ad", "rd", "azimuth", "inclination")
MAPS = ("md", "fa", "ad", "rd", "azimuth", "inclination")
FUNCS = ("do_invert_dwi_tensor_norm", "do_calc_scalar_maps", "do_calc_diff_maps", "do_calc_error_avg")


class _Img:
    def __init__(self, data, affine=None, header=None):
        self.data, self.affine, self.header = np.array(data), affine, header

    def get_fdata(self, dtype=np.float64):
        return np.array(self.data, dtype=dtype)


class _Nib:
    """nibabel stand-in: load / save / Nifti1Image on an in-memory dict of arrays."""
    Nifti1Image = _Img

    def __init__(self):
        self.files = {}

    def load(self, fname):
        return self.files[fname]

    def save(self, img, fname):
        self.files[fname] = _Img(img.data)


def load_reference(ref_root):
    import pandas as pd
    path = os.path.join(ref_root, "src", "eval.py")
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in FUNCS]
    assert sorted(n.name for n in fns) == sorted(FUNCS), "reference layout changed"
    table_fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "calc_error_table")
    sub_loop = next(n for n in table_fn.body if isinstance(n, ast.For) and getattr(n.target, "id", "") == "sub")
    ps_loop = next(n for n in sub_loop.body if isinstance(n, ast.For) and getattr(n.target, "id", "") == "i")
    nib = _Nib()
    ns = {"np": np, "pd": pd, "nib": nib, "Tuple": typing.Tuple}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)          # in-memory only
    ps_code = compile(ast.Module(body=[ps_loop], type_ignores=[]), path, "exec")
    return ns, nib, ps_code


def reference_table(ref, pred, target, mask, probseg, min_v, max_v):
    """The reference's chain on one subject -> (R, 12) table, (12, ...) post-processed diff maps."""
    import pandas as pd
    ns, nib, ps_code = ref
    nib.files.clear()
    with tempfile.TemporaryDirectory() as tmp:
        name = os.path.join(tmp, "x_mod-bssfp_2024-01_{}-p1_state-s_sub-01_ses-1.nii.gz")
        nib.files[name.format("pred")] = _Img(pred)
        nib.files[name.format("target")] = _Img(target)
        mn, mx = (0.0, 1.0) if min_v is None else (min_v, max_v)           # x * 1 + 0: exact
        for kind in ("pred", "target"):
            ns["do_invert_dwi_tensor_norm"](name.format(kind), mn, mx)
            ns["do_calc_scalar_maps"](name.format(kind).replace(".nii.gz", "_denorm.nii.gz"))
        ns["do_calc_diff_maps"]((name.format("pred"), name.format("target"), ""))
        for k in MAPS:
            f = name.replace(".nii.gz", f"_{k}.nii.gz")
            ns["do_calc_diff_maps"]((f.format("pred"), f.format("target"), k))
        sub = "01"
        pns = {"np": np, "masks": {sub: np.asarray(mask, np.float64).astype(np.uint8)}, "sub": sub,
               "probseg": np.asarray(probseg, np.float64)}
        exec(ps_code, pns)
        diff = [name.format("diff")] + [name.replace(".nii.gz", f"_{k}.nii.gz").format("diff") for k in MAPS]
        table = np.full((probseg.shape[-1], 12), -1.0)
        for f in diff:
            ns["do_calc_error_avg"]((f, pns["masks"][sub], pns["probseg"]))
            csv = pd.read_csv(f.split(".nii.gz")[0] + "_rel_errors.csv")
            for r, roi in enumerate(("CSF", "GM", "WM")[:probseg.shape[-1]]):
                row = csv[csv["roi"] == roi]
                for c in COLUMNS:
                    if c in row:
                        table[r, COLUMNS.index(c)] = float(row[c].iloc[0])
        maps = np.concatenate([np.moveaxis(nib.files[f].data, -1, 0) for f in diff])      # saved as (..., k)
    assert (table != -1.0).all()
    return table, maps


def _spd(rng, n):
    a = rng.standard_normal((n, 3, 3))
    m = a @ np.swapaxes(a, -1, -2) * 3e-4 + np.eye(3) * 2e-4
    return np.stack([m[:, 0, 0], m[:, 0, 1], m[:, 0, 2], m[:, 1, 1], m[:, 1, 2], m[:, 2, 2]], -1)


def _ez(d):
    """z of LAPACK's principal eigenvector (the reference's eigh call)."""
    m = np.stack([d[..., [0, 1, 2]], d[..., [1, 3, 4]], d[..., [2, 4, 5]]], -2)
    return np.linalg.eigh(m, "U")[1][..., 2, 2]


def make_case(rng, shape, mask, min_v, max_v, edit):
    """pred/target (..., 6) f32 with LAPACK z >= 0.1 for both at every in-mask voxel, after `edit`."""
    n = int(np.prod(shape))
    t = _spd(rng, n)
    p = t * (1 + 0.1 * rng.standard_normal(t.shape))
    inside = np.asarray(mask).reshape(-1).astype(np.uint8) > 0

    def enc(x):
        return (x if min_v is None else (x - min_v) / (max_v - min_v)).astype(np.float32)

    def dec(x):
        return x.astype(np.float64) if min_v is None else x.astype(np.float64) * abs(max_v - min_v) + min_v

    pn, tn = enc(p), enc(t)
    for _ in range(1000):
        edit(pn, tn)
        bad = inside & ((_ez(dec(pn)) < 0.1) | (_ez(dec(tn)) < 0.1))
        if not bad.any():
            return pn.reshape(shape + (6,)), tn.reshape(shape + (6,))
        t2 = _spd(rng, int(bad.sum()))
        tn[bad] = enc(t2)
        pn[bad] = enc(t2 * (1 + 0.1 * rng.standard_normal(t2.shape)))
    raise RuntimeError("rejection sampling did not converge")


def ball(shape, r2=0.8):
    idx = np.stack(np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij"), -1)
    return ((idx ** 2).sum(-1) < r2)


def probseg_for(rng, shape, nroi=3):
    ps = rng.random(shape + (nroi,)) ** 3
    return (ps / ps.sum(-1, keepdims=True)).astype(np.float32)


def case1(rng):
    shape, min_v, max_v = (10, 12, 16), -2e-3, 6e-3
    mask = ball(shape).astype(np.float32).reshape(-1)
    ins = np.flatnonzero(mask > 0)
    outs = np.flatnonzero(mask == 0)
    mask[ins[5]] = 0.5                                           # astype(uint8) -> 0: outside
    mask[ins[6]] = 2.0
    ins = np.flatnonzero(mask.astype(np.uint8) > 0)

    def edit(pn, tn):
        tn[ins[0], 1] = 0.0                                      # |p - t| / 0 = inf -> 0
        pn[ins[0], 1] = 0.25
        tn[ins[1], 4] = 0.0
        pn[ins[1], 4] = 0.5
        pn[ins[2]] = tn[ins[2]]                                  # pred == target
        pn[outs[:4]] = 0.0                                       # 0/0 = NaN outside the mask
        tn[outs[:4]] = 0.0

    pred, target = make_case(rng, shape, mask, min_v, max_v, edit)
    ps = probseg_for(rng, shape).reshape(-1, 3)
    ps[ins[3], 0] = np.float32(0.99e-5)
    ps[ins[4], 0] = np.float32(1.01e-5)
    ps[ins[7], 1] = np.float32(1e-5)                             # f32(1e-5) < 1e-5 in f64: dropped
    ps[ins[8], 2] = np.float32(1e-5) * np.float32(1.0000001)
    return pred, target, mask.reshape(shape), ps.reshape(shape + (3,)), min_v, max_v


def case2(rng):
    shape = (4, 5, 6)
    mask = ball(shape, 1.5).astype(np.uint8).reshape(-1)
    ins = np.flatnonzero(mask)

    def edit(pn, tn):
        pn[ins[3]] = 0.0
        tn[ins[3]] = 0.0

    pred, target = make_case(rng, shape, mask, None, None, edit)
    return pred, target, mask.reshape(shape), probseg_for(rng, shape), None, None


def case3(rng):
    shape = (4, 5, 6)
    mask = ball(shape, 1.5).astype(np.uint8)
    pred, target = make_case(rng, shape, mask, None, None, lambda p, t: None)
    ps = probseg_for(rng, shape)
    ps[..., 1] = np.where(mask > 0, np.float32(5e-6), np.float32(0.3))
    return pred, target, mask, ps, None, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    ref = load_reference(a.ref)
    rng = np.random.default_rng(2024)
    out = {}
    for name, fn in (("c1", case1), ("c2", case2), ("c3", case3)):
        pred, target, mask, ps, min_v, max_v = fn(rng)
        with np.errstate(all="ignore"):
            table, maps = reference_table(ref, pred, target, mask, ps, min_v, max_v)
        out.update({f"{name}_pred": pred, f"{name}_target": target, f"{name}_mask": mask, f"{name}_probseg": ps,
                    f"{name}_minmax": np.array([] if min_v is None else [min_v, max_v]),
                    f"{name}_table": table, f"{name}_maps": maps})
        print(name, pred.shape, "NaN cells", int(np.isnan(table).sum()))
    np.savez_compressed(os.path.join(a.out, "dti_errors.npz"), **out)
    print("wrote", os.path.join(a.out, "dti_errors.npz"))


if __name__ == "__main__":
    main()
