"""Evaluation-side device ops.

``calc_scalar_maps`` is the GPU counterpart of the voxel loop of ``do_calc_scalar_maps``
(src/eval.py:73-135) with ``do_invert_dwi_tensor_norm`` (src/eval.py:39-47) optionally fused in
front.  The reference works file-to-file through nibabel (absent here); this mirror works on
device tensors -- the NIfTI load/save either side stays with the caller.

``error_table`` is the GPU counterpart of ``calc_diff_maps`` + ``calc_error_table`` /
``do_calc_error_avg`` (src/eval.py:154-192, 217-317): the per-tissue mean relative errors of the
tensor components, MD, FA, AD, RD and the principal direction, in one pass per subject.
``error_rows`` / ``write_error_csv`` lay the table out like the reference's CSV, and
``evaluate_subject`` runs it on a whole-volume prediction.
"""
from __future__ import annotations

import csv
import ctypes
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib

_DT = {torch.float32: 0, torch.float64: 2}
MAP_NAMES = ("fa", "md", "ad", "rd", "azimuth", "inclination", "rgb")
ERROR_COLUMNS = ("dxx", "dxy", "dxz", "dyy", "dyz", "dzz", "md", "fa", "ad", "rd", "azimuth", "inclination")
ROI_NAMES = ("CSF", "GM", "WM")


def calc_scalar_maps(data: torch.Tensor, min_v: Optional[float] = None, max_v: Optional[float] = None,
                     channels_first: bool = False) -> Dict[str, torch.Tensor]:
    """data: (..., 6) like the reference's NIfTI array, or (6, ...) with ``channels_first`` (a generator
    output without its batch axis); f32 or f64 on the GPU.  Returns the seven maps of the reference
    (``rgb`` is (..., 3)), in the dtype of ``data``.  ``min_v``/``max_v`` apply the inverse min-max
    normalisation x * |max - min| + min first."""
    if not data.is_cuda:
        raise _lib.Mi355Error("calc_scalar_maps runs on the GPU only (no CPU fallback)")
    if data.dtype not in _DT:
        raise _lib.Mi355Error(f"calc_scalar_maps: unsupported dtype {data.dtype}")
    if (min_v is None) != (max_v is None):
        raise ValueError("give both min_v and max_v or neither")
    data = data.contiguous()
    if channels_first:
        if data.shape[0] != 6:
            raise ValueError(f"expected 6 tensor components first, got shape {tuple(data.shape)}")
        spatial = tuple(data.shape[1:])
        nvox = data[0].numel()
        cs, vs = nvox, 1
    else:
        if data.shape[-1] != 6:
            raise ValueError(f"expected 6 tensor components last, got shape {tuple(data.shape)}")
        spatial = tuple(data.shape[:-1])
        nvox = data.numel() // 6
        cs, vs = 1, 6
    scale, offset = (1.0, 0.0) if min_v is None else (abs(float(max_v) - float(min_v)), float(min_v))
    out = {k: torch.empty(spatial, dtype=data.dtype, device=data.device) for k in MAP_NAMES[:-1]}
    out["rgb"] = torch.empty(spatial + (3,), dtype=data.dtype, device=data.device)
    _lib.check(_lib.load().mi355_dti_scalar_maps(
        data.data_ptr(), _DT[data.dtype], nvox, cs, vs, scale, offset,
        *[out[k].data_ptr() for k in MAP_NAMES], torch.cuda.current_stream().cuda_stream), "dti_scalar_maps")
    return out


def _denorm(min_v, max_v):
    if (min_v is None) != (max_v is None):
        raise ValueError("give both min_v and max_v or neither")
    return (1.0, 0.0) if min_v is None else (abs(float(max_v) - float(min_v)), float(min_v))


def error_table(pred: torch.Tensor, target: torch.Tensor, mask: torch.Tensor, probseg: torch.Tensor,
                min_v: Optional[float] = None, max_v: Optional[float] = None, channels_first: bool = False,
                return_maps: bool = False):
    """Mean relative errors of ``pred`` against ``target`` per tissue class -> (R, 12) float64 device tensor,
    columns ``ERROR_COLUMNS``, rows the R probability maps of ``probseg`` (the reference's CSF, GM, WM).

    pred, target: (..., 6) NIfTI order, or (6, ...) with ``channels_first``; f32 or f64 (the same for both).
    mask: (...) brain mask; a voxel counts where ``mask.to(torch.uint8) > 0`` (the reference's
    ``astype(np.uint8)``).  probseg: (..., R) or (R, ...) with ``channels_first``, f32 or f64, 1 <= R <= 4.
    ``min_v``/``max_v``: the inverse min-max normalisation applied before the MD/FA/AD/RD/angle maps (the
    tensor columns use the tensors as passed, the reference's "normalized" tensor errors).

    Per voxel: |p - t| / t (angles: (p - t) mod 360, the shorter way round), then |.|, 0 outside the mask,
    +inf -> 0.  NaN stays NaN: a 0/0 inside the mask makes that column NaN in EVERY row (probseg * NaN is
    NaN also where probseg is 0), as in the reference.  Weights: probseg where mask > 0 and probseg > 1e-5;
    a row whose weights sum to 0 is NaN.  The principal eigenvector has z >= 0 (``calc_scalar_maps``'
    convention), so the angle columns equal the reference's where LAPACK's eigenvector also has z > 0.

    ``return_maps``: also return {column: post-processed diff map (...)} in pred's dtype, the maps the
    reference writes back to disk.  Asynchronous (no host synchronisation); bit-identical between calls."""
    for name, t in (("pred", pred), ("target", target), ("mask", mask), ("probseg", probseg)):
        if not t.is_cuda:
            raise _lib.Mi355Error(f"error_table runs on the GPU only (no CPU fallback): {name} is on {t.device}")
    if pred.dtype not in _DT or target.dtype != pred.dtype:
        raise _lib.Mi355Error(f"error_table: pred/target must both be f32 or f64, got {pred.dtype} / {target.dtype}")
    if probseg.dtype not in _DT:
        raise _lib.Mi355Error(f"error_table: unsupported probseg dtype {probseg.dtype}")
    scale, offset = _denorm(min_v, max_v)
    if pred.shape != target.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} differ")
    if channels_first:
        if pred.dim() < 1 or pred.shape[0] != 6:
            raise ValueError(f"expected 6 tensor components first, got shape {tuple(pred.shape)}")
        spatial, ps_spatial, nroi = tuple(pred.shape[1:]), tuple(probseg.shape[1:]), probseg.shape[0] if probseg.dim() else 0
    else:
        if pred.dim() < 1 or pred.shape[-1] != 6:
            raise ValueError(f"expected 6 tensor components last, got shape {tuple(pred.shape)}")
        spatial, ps_spatial, nroi = tuple(pred.shape[:-1]), tuple(probseg.shape[:-1]), probseg.shape[-1] if probseg.dim() else 0
    if ps_spatial != spatial or tuple(mask.shape) != spatial:
        raise ValueError(f"spatial shapes differ: tensors {spatial}, mask {tuple(mask.shape)}, probseg {ps_spatial}")
    pred, target, probseg = pred.contiguous(), target.contiguous(), probseg.contiguous()
    mask = (mask if mask.dtype == torch.uint8 else mask.to(torch.uint8)).contiguous()
    nvox = 1
    for n in spatial:
        nvox *= n
    cs, vs = (nvox, 1) if channels_first else (1, 6)
    rs, pvs = (nvox, 1) if channels_first else (1, nroi)
    lib = _lib.load()
    ws_bytes = lib.mi355_dti_errors_workspace_bytes(nvox, nroi)
    if ws_bytes < 0:
        ws_bytes = 8                           # bad R: the call below rejects it with the library's message
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pred.device)
    table = torch.empty((max(nroi, 0), len(ERROR_COLUMNS)), dtype=torch.float64, device=pred.device)
    maps = None
    ptrs = None
    if return_maps:
        maps = {k: torch.empty(spatial, dtype=pred.dtype, device=pred.device) for k in ERROR_COLUMNS}
        ptrs = (ctypes.c_void_p * len(ERROR_COLUMNS))(*[maps[k].data_ptr() for k in ERROR_COLUMNS])
    _lib.check(lib.mi355_dti_errors(
        pred.data_ptr(), target.data_ptr(), _DT[pred.dtype], cs, vs, mask.data_ptr(),
        probseg.data_ptr(), _DT[probseg.dtype], rs, pvs, nvox, nroi, scale, offset,
        ws.data_ptr(), ws_bytes, table.data_ptr(), ptrs, torch.cuda.current_stream(pred.device).cuda_stream), "dti_errors")
    return (table, maps) if return_maps else table


def error_rows(table: torch.Tensor, modality: str, pred_id: str, sub: str, ses: str,
               roi_names: Sequence[str] = ROI_NAMES) -> List[dict]:
    """(R, 12) table -> one dict per ROI with the reference CSV's columns (modality, pred_id, sub, ses, roi,
    then ``ERROR_COLUMNS`` as Python floats)."""
    t = table.detach().to("cpu", torch.float64)
    if t.dim() != 2 or t.shape[1] != len(ERROR_COLUMNS) or t.shape[0] != len(roi_names):
        raise ValueError(f"table {tuple(t.shape)} does not match {len(roi_names)} ROI names x {len(ERROR_COLUMNS)} columns")
    rows = []
    for r, roi in enumerate(roi_names):
        row = {"modality": modality, "pred_id": pred_id, "sub": sub, "ses": ses, "roi": roi}
        row.update({c: float(v) for c, v in zip(ERROR_COLUMNS, t[r].tolist())})
        rows.append(row)
    return rows


def write_error_csv(rows: Sequence[dict], path: str) -> None:
    """Writes ``error_rows`` output (of one or more subjects) as CSV: modality, pred_id, sub, ses, roi, *ERROR_COLUMNS.
    Floats are written with repr (round-trip); NaN as ``nan``."""
    fields = ["modality", "pred_id", "sub", "ses", "roi", *ERROR_COLUMNS]
    with open(path, "w", newline="") as fh:
        w = csv.DictWriter(fh, fieldnames=fields)
        w.writeheader()
        for row in rows:
            w.writerow({k: (repr(v) if isinstance(v, float) else v) for k, v in row.items()})


def evaluate_subject(gen: torch.nn.Module, x: torch.Tensor, target: torch.Tensor, mask: torch.Tensor,
                     probseg: torch.Tensor, patch_size=64, patch_overlap=0, batch_size: int = 8,
                     overlap_mode: str = "crop", min_v: Optional[float] = None,
                     max_v: Optional[float] = None) -> torch.Tensor:
    """Whole-volume prediction of one subject (``inference.predict_volume(gen, x, ...)``: x (C, D, H, W) ->
    (6, D, H, W)), then ``error_table`` against target (6, D, H, W) with mask (D, H, W) and probseg
    (R, D, H, W) -> (R, 12) float64 device tensor.  The prediction is f32, so ``target`` must be f32 too."""
    from .inference import predict_volume
    _denorm(min_v, max_v)
    with torch.no_grad():
        pred = predict_volume(gen, x, patch_size, patch_overlap, batch_size, overlap_mode)
    return error_table(pred, target, mask, probseg, min_v, max_v, channels_first=True)
