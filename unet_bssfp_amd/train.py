"""``train_model`` of the reference (src/train.py:46-77) on the device feed and the fit loop of ``trainer.py``.

    python -m unet_bssfp_amd.train manifest.json

reads ``{"modality": ..., "dirpath": ..., "train": [{image name: NIfTI path, ...}, ...], "val": [...]}`` (optional:
``"max_epochs"``, ``"ckpt_path"``, ``"seed"``, ``"device"``, and the generator's ``"head"`` (``"conv"`` | ``"resnet"``) and
``"act"`` -- ``{"stages": [...], "head": "resnet", "act": "prelu"}`` is the thesis's network and workflow), uploads every subject once (``data.subjects_from_nifti``)
and trains through two ``data.PatchQueue``s with the reference's arguments; like the reference's ``val_set``
(src/data_module.py:146-147) the validation queue augments as the training queue does.

``"spatial"`` adds spatial augmentation in front of the reference's transform, for both queues: a list such as
``[{"type": "RandomFlip", "axes": [0, 1, 2]}, {"type": "RandomAffine", "degrees": 10, "scales": 0.1}]``, every other key
being a constructor argument of ``augment.RandomFlip`` / ``augment.RandomAffine``.  The ``'dwi-tensor'`` image is reoriented
with the volume; ``"tensor_rescale"`` -- a 6 x 2 list of per-component (min, max), or the path of a text file that holds one,
the layout of the reference's ``rescale_args_dwi.txt`` -- says that the tensors are stored normalised.

With ``"stages": ["PRETRAIN", "TRANSFER", "FINE_TUNE"]`` (any sub-list, in order) the manifest runs the thesis's staged
workflow instead (``train_staged``, stages.py): every stage gets queues of its own modality, starts from the previous stage's
best checkpoint (the first from ``"ckpt_path"``, if given) and the best paths are printed one per line.  ``"max_epochs"``
may then be a ``{stage name: epochs}`` object.
"""
from __future__ import annotations

import json
import sys
from typing import Dict, List, Optional, Sequence, Union

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


def train_staged(queues, modality: str, dirpath: str, stages: Optional[Sequence] = None, ckpt_path: Optional[str] = None,
                 max_epochs: Union[int, Dict] = 50, device="cuda:0", graph: bool = True, **model_kw) -> List[str]:
    """The thesis's staged workflow (Methods, "Training"; the state machine is not in the reference's ``src/``, parity unpinned):
    PRETRAIN on ``'dwi-tensor'`` (the DTI auto-encoder), TRANSFER on ``modality`` (only that modality's input block trains,
    the U-Net is frozen), FINE_TUNE on ``modality`` (everything at 1e-5).  Returns the stages' ``best_model_path``s in order.

    ``queues(state, stage_modality) -> (train_queue, val_queue)`` builds a stage's queues for that stage's modality; a mapping
    ``{state or its name: (train_queue, val_queue)}`` does as well.  ``stages``: the states to run, in order (default: all
    three) -- ``stages=['TRANSFER', 'FINE_TUNE'], ckpt_path=...`` resumes the workflow at TRANSFER from a given checkpoint.
    Every stage gets a fresh ``Trainer`` under the reference's two callbacks (src/train.py:19-27) and starts at epoch 0 from
    the previous stage's ``best_model_path`` with fresh optimisers (``load_from_checkpoint(path, training_state=...,
    input_modality=...)``); the first stage starts from ``ckpt_path`` or from a new model.  ``max_epochs``: one number, or
    ``{state or its name: epochs}``.  The file names carry the state (``TrainingState.TRANSFER-pc-bssfp-epoch=...``), so the
    stages share ``dirpath``."""
    from .checkpoint import load_from_checkpoint
    from .gan import bSSFPToDWITensorModel
    from .stages import PRETRAIN_MODALITY, STAGE_ORDER, TrainingState, parse_state

    def lookup(table, state, default=None):
        for key in (state, state.name, str(state)):
            if key in table:
                return table[key]
        if default is None:
            raise KeyError(f"train_staged: nothing given for {state}")
        return default

    states = [parse_state(s) for s in (STAGE_ORDER if stages is None else stages)]
    if not states or any(s is None for s in states) or sorted(states, key=STAGE_ORDER.index) != states or len(set(states)) != len(states):
        raise ValueError(f"train_staged: stages must be a non-empty sub-list of {[s.name for s in STAGE_ORDER]} in that order")
    paths, prev = [], ckpt_path
    for state in states:
        stage_modality = PRETRAIN_MODALITY if state is TrainingState.PRETRAIN else modality
        train_queue, val_queue = queues(state, stage_modality) if callable(queues) else lookup(queues, state)
        if prev:
            model, _info = load_from_checkpoint(prev, device=device, training_state=state, input_modality=stage_modality, **model_kw)
        else:
            model = bSSFPToDWITensorModel(stage_modality, **model_kw).to(device).change_training_state(state, stage_modality)
        epochs = max_epochs if isinstance(max_epochs, int) else lookup(max_epochs, state, 50)
        checkpoint_cb = ModelCheckpoint(dirpath, save_top_k=10, monitor="val_loss", mode="min")
        trainer = Trainer(max_epochs=int(epochs), graph=graph,
                          callbacks=[EarlyStopping("val_gen_loss_recon", patience=10), checkpoint_cb])
        trainer.fit(model.train(), train_queue, val_queue)
        prev = checkpoint_cb.best_model_path
        if not prev:
            raise RuntimeError(f"train_staged: {state} wrote no checkpoint (no validation queue?)")
        paths.append(prev)
        del trainer, model
    return paths


def spatial_from_manifest(manifest: Dict) -> Dict:
    """the ``spatial=`` / ``tensor_images=`` arguments of ``PatchQueue`` from the manifest keys ``"spatial"`` and
    ``"tensor_rescale"``; ``{}`` when neither is given"""
    import numpy as np
    from . import augment
    kw: Dict = {}
    if manifest.get("spatial"):
        kinds = {"RandomFlip": augment.RandomFlip, "RandomAffine": augment.RandomAffine}
        stages = []
        for entry in manifest["spatial"]:
            args = dict(entry)
            kind = args.pop("type", None)
            if kind not in kinds:
                raise ValueError(f'"spatial": unknown type {kind!r} (supported: {sorted(kinds)})')
            if isinstance(args.get("axes"), list):
                args["axes"] = tuple(args["axes"])
            stages.append(kinds[kind](**{k: tuple(v) if isinstance(v, list) else v for k, v in args.items()}))
        kw["spatial"] = stages
    if manifest.get("tensor_rescale") is not None:
        r = manifest["tensor_rescale"]
        kw["tensor_images"] = {"dwi-tensor": augment.check_tensor_rescale(np.loadtxt(r) if isinstance(r, str) else r)}
    return kw


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
    model_kw = {k: manifest[m] for m, k in (("head", "gen_head"), ("act", "gen_act")) if manifest.get(m) is not None}
    train = [subjects_from_nifti(files, device) for files in manifest["train"]]
    val = [subjects_from_nifti(files, device) for files in manifest["val"]]
    feed = spatial_from_manifest(manifest)
    if "stages" in manifest:
        epochs = manifest.get("max_epochs", 50)
        best = train_staged(lambda state, m: (PatchQueue(train, m, seed=seed, **feed),
                                              PatchQueue(val, m, seed=seed + 1, **feed) if val else None),
                            modality, manifest["dirpath"], stages=manifest["stages"], ckpt_path=manifest.get("ckpt_path"),
                            max_epochs=epochs if isinstance(epochs, dict) else int(epochs), device=device, **model_kw)
        print("\n".join(best))
        return 0
    best = train_model(PatchQueue(train, modality, seed=seed, **feed),
                       PatchQueue(val, modality, seed=seed + 1, **feed) if val else None,
                       modality, manifest["dirpath"], ckpt_path=manifest.get("ckpt_path"),
                       max_epochs=int(manifest.get("max_epochs", 50)), device=device, **model_kw)
    print(best)
    return 0


if __name__ == "__main__":
    sys.exit(main())
