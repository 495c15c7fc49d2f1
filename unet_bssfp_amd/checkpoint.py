"""Lightning-shaped checkpoints for the step harness -- SURVEY.md 8(f) rank 4 (format part).

The reference trains under ``pl.Trainer`` with ``ModelCheckpoint`` (src/train.py:21-27) and resumes with
``bSSFPToDWITensorModel.load_from_checkpoint(ckpt_path)`` (src/train.py:56-57).  A Lightning ``.ckpt`` is a
``torch.save``'d dict; the parts that matter here:

    'state_dict'        module state, keys prefixed by the LightningModule attribute: ``gen.*`` / ``discr.*``
                        (key table: SURVEY.md 8(b)); a reference checkpoint also carries
                        ``recon_criterion.*`` (MedicalNet weights of the Perceptual term) -- not loaded into the
                        model (listed under 'ignored_keys'); ``medicalnet_state_dict`` extracts them for
                        ``medicalnet.MedicalNetResNet10``
    'optimizer_states'  [gen AdamW state_dict, discr AdamW state_dict]   (configure_optimizers order, :359-361)
    'hyper_parameters'  what ``save_hyperparameters`` recorded (src/model.py:149): input_modality, lr,
                        batch_size, perceptual_factor, recon_factor; a model in a training state (stages.py) adds
                        'training_state' (a plain string, ``'TrainingState.TRANSFER'``) and 'stage_lr' -- absent without
                        a state, so such files are what they were; a model built with ``gen_head=`` / ``gen_act=`` adds
                        'gen_head' (a string) / 'gen_act' (a string, or a [name, {kwargs}] list) -- absent when not set
    'epoch', 'global_step', 'pytorch-lightning_version', 'lr_schedulers', 'callbacks', 'loops'

Files are read with ``torch.load(weights_only=True)`` only: nothing in the file is executed, and a
checkpoint whose pickle needs more than tensors and plain containers is refused by torch itself.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

LIGHTNING_VERSION = "2.2.1"          # requirements.txt:1 of the reference
HPARAM_KEYS = ("input_modality", "lr", "batch_size", "perceptual_factor", "recon_factor")
OPTIONAL_HPARAM_KEYS = ("gen_head", "gen_act")      # the generator's architecture (gan.bSSFPToDWITensorModel); written only when set
_OWN_PREFIXES = ("gen.", "discr.")


def _plain(v):
    """tensors to CPU, containers rebuilt from plain types: safe for weights_only loading"""
    if isinstance(v, torch.Tensor):
        return v.detach().cpu()
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


def checkpoint_dict(model, epoch: int = 0, global_step: int = 0) -> Dict:
    opts = model.optimizers()
    for o in opts:
        if hasattr(o, "sync_step_counts"):
            o.sync_step_counts()                     # device-side step counters -> state['step']
    extra = {}
    if next(model.gen.parameters()).is_cuda:
        from .functional import DropoutState
        dev = next(model.gen.parameters()).device
        extra["dropout_base"] = int(DropoutState.base(dev).item())
    hparams = {k: getattr(model, k) for k in HPARAM_KEYS}
    for k in OPTIONAL_HPARAM_KEYS:
        if getattr(model, k, None) is not None:
            hparams[k] = _plain(getattr(model, k))
    if getattr(model, "training_state", None) is not None:
        hparams["training_state"] = str(model.training_state)
        hparams["stage_lr"] = float(model.stage_lr)
    return {
        "epoch": int(epoch), "global_step": int(global_step), "pytorch-lightning_version": LIGHTNING_VERSION,
        "state_dict": _plain({k: v for k, v in model.state_dict().items() if k.startswith(_OWN_PREFIXES)}),
        "optimizer_states": [_plain(o.state_dict()) for o in opts],
        "lr_schedulers": [], "callbacks": {}, "loops": {},
        "hyper_parameters": hparams,
        "mi355": extra,
    }


def save_checkpoint(model, path: str, epoch: int = 0, global_step: int = 0) -> None:
    torch.save(checkpoint_dict(model, epoch, global_step), path)


def load_checkpoint(model, path: str, strict: bool = True, load_optimizers: bool = True) -> Dict:
    """Load a checkpoint written by ``save_checkpoint`` or by the reference's Lightning run into ``model``.
    Returns {'epoch', 'global_step', 'ignored_keys'}; keys outside gen./discr. (the reference's
    ``recon_criterion.*`` etc.) are listed, not loaded."""
    return apply_checkpoint(model, torch.load(path, map_location="cpu", weights_only=True), strict, load_optimizers, path)


def apply_checkpoint(model, ckpt: Dict, strict: bool = True, load_optimizers: bool = True, path: str = "checkpoint") -> Dict:
    """``load_checkpoint`` for a file that has been read already (the fit loop reads its own additions from the same dict)"""
    if "state_dict" not in ckpt:
        raise KeyError(f"{path}: not a Lightning-shaped checkpoint (no 'state_dict')")
    sd = ckpt["state_dict"]
    own = {k: v for k, v in sd.items() if k.startswith(_OWN_PREFIXES)}
    ignored = sorted(k for k in sd if not k.startswith(_OWN_PREFIXES))
    target = {k for k in model.state_dict() if k.startswith(_OWN_PREFIXES)}
    missing, unexpected = sorted(target - set(own)), sorted(set(own) - target)
    if strict and (missing or unexpected):
        raise RuntimeError(f"checkpoint does not match the model: missing {missing[:5]}... unexpected {unexpected[:5]}...")
    model.load_state_dict(own, strict=False)
    if next(model.gen.parameters()).is_cuda:
        from .functional import repack_weights
        repack_weights(model.gen), repack_weights(model.discr)
    if load_optimizers and ckpt.get("optimizer_states"):
        states = ckpt["optimizer_states"]
        # the optimisers of a training state (stages.py) cover that state's trainable parameters only
        stored = (ckpt.get("hyper_parameters") or {}).get("training_state")
        state = getattr(model, "training_state", None)
        if stored != (None if state is None else str(state)):
            raise RuntimeError(f"{path}: the checkpoint's optimiser state is that of training state {stored}, the model is in "
                               f"{state}; call model.change_training_state(...) first, or load the weights only "
                               "(load_optimizers=False, or load_from_checkpoint(path, training_state=...))")
        opts = model.optimizers()
        if len(states) != len(opts):
            raise RuntimeError(f"checkpoint has {len(states)} optimizer states, the model has {len(opts)} optimizers")
        for o, st in zip(opts, states):
            o.load_state_dict(st)
    base = (ckpt.get("mi355") or {}).get("dropout_base")
    if base is not None and next(model.gen.parameters()).is_cuda:
        from .functional import DropoutState
        DropoutState.base(next(model.gen.parameters()).device).fill_(int(base))
    return {"epoch": ckpt.get("epoch", 0), "global_step": ckpt.get("global_step", 0), "ignored_keys": ignored}


def medicalnet_state_dict(ckpt_or_path) -> Dict[str, torch.Tensor]:
    """The MedicalNet ResNet-10 weights a reference checkpoint carries under ``recon_criterion.<...>.``, without the prefix:
    ``MedicalNetResNet10().load_state_dict(medicalnet_state_dict(path))``.  The prefix is found by the stem's key: the one
    that ends in ``conv1.weight`` and has the shape (64, 1, 7, 7, 7).  ``KeyError`` if the checkpoint has no such network."""
    ckpt = ckpt_or_path
    if not isinstance(ckpt, dict):
        ckpt = torch.load(ckpt_or_path, map_location="cpu", weights_only=True)
    sd = ckpt.get("state_dict", ckpt)
    tail = "conv1.weight"
    stems = [k for k, v in sd.items() if k.startswith("recon_criterion.") and k.endswith(tail)
             and isinstance(v, torch.Tensor) and tuple(v.shape) == (64, 1, 7, 7, 7)]
    if not stems:
        raise KeyError("no MedicalNet ResNet-10 in the checkpoint: no key under 'recon_criterion.' ends in 'conv1.weight' "
                       "with shape (64, 1, 7, 7, 7)")
    prefix = stems[0][:-len(tail)]
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def load_from_checkpoint(path: str, device: Optional[str] = None, **overrides):
    """``bSSFPToDWITensorModel.load_from_checkpoint`` (src/train.py:57): rebuild the model from the stored
    hyper-parameters, then load weights and both optimizer states.  A stored training state (stages.py) is restored with
    its rate.  ``training_state=`` (a ``TrainingState``, its name, or ``None``) and ``input_modality=`` rebuild the model for
    the next stage instead: the weights are loaded, the state's rate is the table's unless ``stage_lr=`` is given, and the
    optimisers start fresh whenever the state, or the modality inside a state, differs from the stored one.  A stored ``gen_head`` /
    ``gen_act`` rebuilds the generator it describes; ``gen_head=`` / ``gen_act=`` override them, ``gen=`` replaces them."""
    from .gan import bSSFPToDWITensorModel
    from .stages import parse_state
    stored = dict(torch.load(path, map_location="cpu", weights_only=True).get("hyper_parameters") or {})
    hp = {k: v for k, v in stored.items() if k in HPARAM_KEYS + OPTIONAL_HPARAM_KEYS}
    stored_state = parse_state(stored.get("training_state"))
    state = parse_state(overrides.pop("training_state")) if "training_state" in overrides else stored_state
    same_stage = state is stored_state and overrides.get("input_modality", hp.get("input_modality")) == hp.get("input_modality")
    lr = overrides.pop("stage_lr", stored.get("stage_lr") if same_stage else None)
    if overrides.get("gen") is not None:           # a generator handed over replaces the stored description of one
        hp = {k: v for k, v in hp.items() if k not in OPTIONAL_HPARAM_KEYS}
    hp.update(overrides)
    if "input_modality" not in hp:
        raise KeyError(f"{path}: no 'input_modality' among the hyper-parameters; pass it explicitly")
    model = bSSFPToDWITensorModel(**hp)
    if device is not None:
        model = model.to(device)
    if state is not None:
        model.change_training_state(state, hp["input_modality"], lr=lr)
    # (without a state an ``input_modality=`` override keeps the optimiser state, as it always did)
    info = load_checkpoint(model, path, load_optimizers=same_stage or (state is None and stored_state is None))
    return model, info
