"""``train_model`` of the reference (src/train.py:46-77) on the device feed and the fit loop of ``trainer.py``.

    python -m unet_bssfp_amd.train manifest.json

reads ``{"modality": ..., "dirpath": ..., "train": [{image name: NIfTI path, ...}, ...], "val": [...]}`` (optional:
``"max_epochs"``, ``"ckpt_path"``, ``"seed"``, ``"device"``), uploads every subject once (``data.subjects_from_nifti``)
and trains through two ``data.PatchQueue``s with the reference's arguments; like the reference's ``val_set``
(src/data_module.py:146-147) the validation queue augments as the training queue does.
"""
from __future__ import annotations

import json
import sys
from typing import Optional

from .trainer import EarlyStopping, ModelCheckpoint, Trainer


def train_model(train_queue, val_queue, modality: str, dirpath: str, ckpt_path: Optional[str] = None, max_epochs: int = 50,
                device="cuda:0", **model_kw) -> str:
    """Build (or load) the model, fit it under the reference's two callbacks with the reference's arguments
    (src/train.py:19-27: ``EarlyStopping('val_gen_loss_recon', patience=10)``, ``ModelCheckpoint(save_top_k=10,
    monitor='val_loss', mode='min')``) and return ``best_model_path``.  With ``ckpt_path`` the model comes from
    ``load_from_checkpoint`` and the fit starts at epoch 0 with fresh optimisers, callbacks and queues, as in the reference (:56-57, 63).
    To continue an interrupted run -- callbacks, queues, epoch counter -- use ``Trainer.fit(..., ckpt_path=...)``."""
    from .checkpoint import load_from_checkpoint
    from .gan import bSSFPToDWITensorModel
    if ckpt_path:
        model, _info = load_from_checkpoint(ckpt_path, device=device, **model_kw)
        model._optimizers = None             # Lightning's load_from_checkpoint restores no optimiser: configured anew
    else:
        model = bSSFPToDWITensorModel(modality, **model_kw).to(device)
    checkpoint_cb = ModelCheckpoint(dirpath, save_top_k=10, monitor="val_loss", mode="min")
    trainer = Trainer(max_epochs=max_epochs, callbacks=[EarlyStopping("val_gen_loss_recon", patience=10), checkpoint_cb])
    trainer.fit(model.train(), train_queue, val_queue)
    return checkpoint_cb.best_model_path


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 1:
        print(__doc__)
        return 2
    from .data import PatchQueue, subjects_from_nifti
    with open(argv[0]) as f:
        manifest = json.load(f)
    device, modality = manifest.get("device", "cuda:0"), manifest["modality"]
    seed = int(manifest.get("seed", 0))
    train = [subjects_from_nifti(files, device) for files in manifest["train"]]
    val = [subjects_from_nifti(files, device) for files in manifest["val"]]
    best = train_model(PatchQueue(train, modality, seed=seed), PatchQueue(val, modality, seed=seed + 1) if val else None,
                       modality, manifest["dirpath"], ckpt_path=manifest.get("ckpt_path"),
                       max_epochs=int(manifest.get("max_epochs", 50)), device=device)
    print(best)
    return 0


if __name__ == "__main__":
    sys.exit(main())
