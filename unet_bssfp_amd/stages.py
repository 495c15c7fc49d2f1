"""Staged training: the thesis's PRETRAIN / TRANSFER / FINE_TUNE workflow (doc/thesis, Methods, section "Training").

The reference's files carry the traces -- ``eval.py`` calls ``model.change_training_state(TrainingState.FINE_TUNE, modality)``,
``train.py`` names a checkpoint ``TrainingState.TRANSFER-pc-bssfp-epoch=31-val_loss=...`` -- but the state machine itself is
not in its ``src/``.  Parity is therefore **unpinned**; the contract is the one written here and pinned by
tests/test_stages_host.py and tests/test_stages_gpu.py:

============  ==============================================================  =========================  ===================
state         generator                                                       discriminator              learning rate
============  ==============================================================  =========================  ===================
``PRETRAIN``  all trainable (the caller picks ``'dwi-tensor'``: auto-encoder)  all trainable              ``model.lr``
``TRANSFER``  ``gen.blocks['unet']`` frozen, ``gen.blocks[modality]`` trained  all trainable              ``model.lr``
``FINE_TUNE`` all trainable                                                   all trainable              ``model.fine_tune_lr``
============  ==============================================================  =========================  ===================

``None`` (no state) is the plain training step.  The modality heads that are not selected stay unused in every state.  The
frozen body of ``TRANSFER`` stays in ``train()`` mode: dropout runs, InstanceNorm has no running statistics, and the head's
BatchNorm belongs to the trained head.  A stage starts with fresh optimiser moments, as a Lightning run that begins with
``load_from_checkpoint`` does.

No kernel is specific to a state: ``TRANSFER`` runs the U-Net's data-gradient chain without its weight gradients, which
every backward function already offers through ``needs_input_grad``.
"""
from __future__ import annotations

import enum
from typing import List, Optional

import torch


class TrainingState(enum.Enum):
    """``str(TrainingState.TRANSFER) == 'TrainingState.TRANSFER'`` -- the prefix of the reference's checkpoint names."""
    PRETRAIN = "PRETRAIN"
    TRANSFER = "TRANSFER"
    FINE_TUNE = "FINE_TUNE"

    def __str__(self) -> str:
        return f"TrainingState.{self.name}"


FINE_TUNE_LR = 1e-5                 # the thesis's fine-tuning rate
PRETRAIN_MODALITY = "dwi-tensor"    # the auto-encoder stage: DTI in, DTI out
STAGE_ORDER = (TrainingState.PRETRAIN, TrainingState.TRANSFER, TrainingState.FINE_TUNE)


def parse_state(value) -> Optional[TrainingState]:
    """``None`` | ``TrainingState`` | ``'TRANSFER'`` | ``'TrainingState.TRANSFER'`` -> ``TrainingState`` or ``None``"""
    if value is None or isinstance(value, TrainingState):
        return value
    name = str(value).rsplit(".", 1)[-1]
    try:
        return TrainingState[name]
    except KeyError:
        raise ValueError(f"unknown training state {value!r} (choose from {[s.name for s in TrainingState]})") from None


def frozen_parameters(state: Optional[TrainingState], gen: torch.nn.Module) -> List[torch.nn.Parameter]:
    """The parameters that ``state`` keeps fixed: the shared body ``gen.blocks['unet']`` in ``TRANSFER``, none otherwise."""
    if state is not TrainingState.TRANSFER:
        return []
    return list(gen.blocks["unet"].parameters())


def stage_lr(state: Optional[TrainingState], lr: float, fine_tune_lr: float = FINE_TUNE_LR) -> float:
    return fine_tune_lr if state is TrainingState.FINE_TUNE else lr
