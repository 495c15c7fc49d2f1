"""Training / validation patch feed on the device -- the reference's ``train_dataloader`` / ``val_dataloader``.

The reference trains through (src/data_module.py:125-188)::

    CropOrPad((96, 128, 128), 0) -> Compose([...augmentations...], keep={'dwi-tensor': 'dwi-tensor_orig'})
        -> UniformSampler(64) -> Queue(max_length=16, samples_per_volume=8) -> DataLoader(batch_size=8)

Here the subjects stay in HBM as their RAW volumes (uploaded once) and ``PatchQueue.next_batch`` writes a whole batch
with ONE launch (``mi355_patch_queue_gather``): the crop/pad is index arithmetic, the augmentation stages that fired for
a patch's subject load run in registers, and the result equals ``extract_patches(chain(crop_or_pad(raw)))`` bit for bit.
The image-space members of the transform are fused (``augment.RandomBiasField``, ``RandomNoise``, ``RandomGamma``).  The
non-local members (``augment.RandomMotion``, ``RandomGhosting``, ``RandomSpike``, ``RandomBlur``) cannot run in the
registers of a gather: for a load in which one of them fired with an effect, the queue materialises ``chain(crop_or_pad(raw))`` up to and
including the LAST such stage once, with the stand-alone kernels, into a staging tensor of the target extent; the gather
reads that tensor as the load's source and fuses only the local stages that follow.  A staged tensor lives no longer than
the patches of its load.  ``RandomMotion`` draws one parameter set per augmented image of a load (as TorchIO does per
image of a subject), the other stages one per load.  Any other transform type raises ``TypeError``.

Spatial stages (``spatial=``: ``augment.RandomFlip``, ``RandomAffine``) sit in front of the ``keep`` copy and move every
image of a load alike; they are resampled inside the gather (``mi355_patch_queue_gather_spatial``), the
resampled volume is never materialised, and a diffusion-tensor image is reoriented voxel by voxel.

The plan -- which subjects fill the queue, the stages that fire and their parameters, the patch origins and their order
-- is host logic driven by the queue's own ``torch.Generator`` and needs no GPU (``next_plan``).  TorchIO is absent: the
structure follows its Queue (fill, shuffle, pop from the end), but its exact random streams are not reproduced
(**parity unpinned**).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, augment, nifti
from .inference import DATA, LOCATION, _triple

_STAGE_KIND = {augment.RandomBiasField: _lib.H["STAGE_BIAS_FIELD"], augment.RandomNoise: _lib.H["STAGE_NOISE"],
               augment.RandomGamma: _lib.H["STAGE_GAMMA"]}
_NONLOCAL = (augment.RandomMotion, augment.RandomGhosting, augment.RandomSpike, augment.RandomBlur)   # staged, never fused
_SIGN_PRESERVING = (augment.RandomBiasField, augment.RandomGamma, augment.RandomBlur)      # x >= 0 stays >= 0
_MAX_IMAGES = _lib.H["QUEUE_MAX_IMAGES"]
_SPATIAL = (augment.RandomFlip, augment.RandomAffine)                                        # resampled inside the gather


def subjects_from_nifti(files: Dict[str, str], device) -> Dict[str, Dict[str, torch.Tensor]]:
    """One subject ``{name: {'data': (C, D, H, W) f32}}`` from ``{name: path}``, uploaded once.  Like TorchIO's
    ``ScalarImage``, a 4-D file's last axis becomes the channel axis and a 3-D file gets one channel."""
    subject = {}
    for name, path in files.items():
        arr, _affine = nifti.load(path)
        if arr.ndim == 3:
            arr = arr[None]
        elif arr.ndim == 4:
            arr = np.moveaxis(arr, -1, 0)
        else:
            raise ValueError(f"{path}: expected a 3-D or 4-D image, got shape {arr.shape}")
        subject[name] = {DATA: torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).to(device)}
    return subject


def split_subjects(ids: Sequence, val_split: float = 0.1, test_split: float = 0.1, seed: int = 42):
    """``random_split(ids, [1 - t - v, v, t], Generator().manual_seed(seed))`` (src/data_module.py:70-75)
    -> (train, val, test) lists of ids."""
    ids = list(ids)
    parts = torch.utils.data.random_split(ids, [1 - test_split - val_split, val_split, test_split],
                                          torch.Generator().manual_seed(seed))
    return tuple([ids[i] for i in p.indices] for p in parts)


class UniformSampler:
    """``tio.data.UniformSampler(patch_size)``: every origin uniform in [0, target - patch] per axis (inclusive)."""

    def __init__(self, patch_size):
        self.patch_size = _triple(patch_size)
        if min(self.patch_size) <= 0:
            raise ValueError(f"patch size must be positive, got {self.patch_size}")

    def check(self, spatial_shape: Sequence[int]) -> None:
        if any(p > s for p, s in zip(self.patch_size, spatial_shape)):
            raise ValueError(f"Patch size {self.patch_size} cannot be larger than image size {tuple(spatial_shape)}")

    def draw(self, spatial_shape: Sequence[int], n: int, generator: torch.Generator) -> List[Tuple[int, int, int]]:
        self.check(spatial_shape)
        axes = [torch.randint(0, s - p + 1, (n,), generator=generator) for s, p in zip(spatial_shape, self.patch_size)]
        return [tuple(int(a[i]) for a in axes) for i in range(n)]


class SubjectLoad(NamedTuple):
    """One load of a subject into the queue: its position in the list given to the queue, the epoch, the running number
    of the fill that loaded it, the seed of the global CPU generator under which its stages were drawn, and the stages
    that fired as (transform, params); the params of a per-image stage (``RandomMotion``) are ``{image name: params}``
    for the modality and every kept source.  ``spatial``: the spatial stages that fired, drawn under ``seed + 1``."""
    subject: int
    epoch: int
    fill: int
    seed: int
    stages: tuple
    spatial: tuple = ()


class PlannedPatch(NamedTuple):
    load: SubjectLoad
    origin: Tuple[int, int, int]      # first voxel, padded (target_shape) coordinates


def _stages_of(transform) -> list:
    transform = list(transform)
    seen = set()
    for t in transform:
        if type(t) not in _STAGE_KIND and type(t) not in _NONLOCAL:
            raise TypeError(f"{type(t).__name__} cannot be fused into the patch queue (supported: RandomBiasField, "
                            "RandomNoise, RandomGamma, and staged: RandomMotion, RandomGhosting, RandomSpike, RandomBlur)")
        if type(t) in seen:
            raise TypeError(f"two {type(t).__name__} stages cannot be fused into one patch queue")
        seen.add(type(t))
    return transform


def _spatial_stages_of(spatial) -> list:
    spatial = list(spatial or ())
    seen = set()
    for t in spatial:
        if type(t) not in _SPATIAL:
            raise TypeError(f"{type(t).__name__} is no spatial stage of the patch queue (supported: RandomFlip, RandomAffine)")
        if type(t) in seen:
            raise TypeError(f"two {type(t).__name__} stages cannot be fused into one patch queue")
        seen.add(type(t))
    return spatial


class PatchQueue:
    """``tio.Queue(subjects_dataset, max_length, samples_per_volume, sampler)`` over device-resident subjects.

    ``subjects``: list of ``{name: {'data': (C, D, H, W) f32 tensor}}`` at any raw extent; each is cropped / padded to
    ``target_shape`` (``augment.crop_or_pad``) inside the gather.  A rank reads the shard ``subjects[rank::world]``, each
    epoch in a fresh permutation.  A fill loads the next ``min(max_length // samples_per_volume, left in the epoch)``
    subjects; for each load it draws the stages that fire and their parameters, then ``samples_per_volume`` origins;
    the list is shuffled and patches are popped from the end.  ``len()`` = patches per epoch.

    ``transform``: the augmentations applied per subject load in list order, fused into the gather or staged before it.  ``None`` (the
    default) means ``augment.reference_augmentation()``, the reference's training transform; ``[]`` augments nothing.
    The queue keeps no history: ``last_fill`` holds the loads of the current fill only.

    ``spatial``: ``augment.RandomFlip`` / ``RandomAffine`` stages that run in FRONT of the ``keep`` copy, i.e. TorchIO's
    ``Compose([spatial..., Compose([intensity...], keep=...)])``: a stage that fired moves every image of the load, the
    kept copy and the augmented target included, so input and target stay a pair.  The stages of a load compose into one
    matrix and the volume is resampled once, inside the gather (``mi355_patch_queue_gather_spatial``); a batch in which
    no load has an effective spatial stage takes the plain launch.  They are drawn under a seed derived from the load's
    own, not from the queue's generator, so a queue with and without ``spatial`` plans the same subjects, seeds,
    intensity stages and origins.  ``tensor_images = {source name: rescale or None}`` names the image whose six channels
    are a diffusion tensor, reoriented with the volume (``augment.tensor_reorientation``; a (6, 2) array of (min, max) for
    normalised data); the default is ``{'dwi-tensor': None}`` when the queue reads that image.  ``None`` or ``[]``
    (the default) changes nothing: the same draws, the same launch, the same bits."""

    def __init__(self, subjects: Sequence[Dict[str, Dict[str, torch.Tensor]]], modality: str, max_length: int = 16,
                 samples_per_volume: int = 8, sampler: Optional[UniformSampler] = None,
                 target_shape: Sequence[int] = (96, 128, 128), transform=None,
                 keep: Optional[Dict[str, str]] = None, seed: int = 0, rank: int = 0, world: int = 1,
                 padding_value: float = 0.0, spatial=None, tensor_images: Optional[Dict] = None):
        self.sampler = UniformSampler(64) if sampler is None else sampler
        self.target_shape = _triple(target_shape)
        if min(self.target_shape) <= 0:
            raise ValueError(f"target shape must be positive, got {self.target_shape}")
        self.sampler.check(self.target_shape)
        self.patch_size = self.sampler.patch_size
        self.transform = _stages_of(augment.reference_augmentation() if transform is None else transform)
        self.keep = {"dwi-tensor": "dwi-tensor_orig"} if keep is None else dict(keep)
        if samples_per_volume < 1 or max_length < samples_per_volume:
            raise ValueError(f"need 1 <= samples_per_volume <= max_length, got {samples_per_volume}, {max_length}")
        if world < 1 or not 0 <= rank < world:
            raise ValueError(f"bad rank {rank} of world {world}")
        self.modality, self.max_length, self.samples_per_volume = modality, int(max_length), int(samples_per_volume)
        self.padding_value = float(padding_value)
        everyone = list(subjects)
        self.indices = list(range(len(everyone)))[rank::world]      # this rank's shard (positions in ``subjects``)
        self.subjects = [everyone[i] for i in self.indices]
        self._by_index = dict(zip(self.indices, self.subjects))
        if not self.subjects:
            raise ValueError(f"rank {rank} of {world} has no subject")
        names = [modality] + list(self.keep)
        self.channels = {}
        for i, subj in enumerate(self.subjects):
            for name in names:
                if name not in subj:
                    raise ValueError(f"subject {i} of the shard has no image '{name}'")
                t = subj[name][DATA]
                if t.dim() != 4:
                    raise ValueError(f"subject {i} '{name}': expected (C, D, H, W), got {tuple(t.shape)}")
                if self.channels.setdefault(name, t.shape[0]) != t.shape[0]:
                    raise ValueError(f"image '{name}' has {t.shape[0]} channels in subject {i}, "
                                     f"{self.channels[name]} elsewhere")
        # RandomSpike takes its DC shortcut (M = sum(x)) only where no voxel can be negative; that is decided statically,
        # from the raw minima read once here, so that next_batch never waits for the device
        self.nonnegative: Dict[int, bool] = {}
        if any(type(t) is augment.RandomSpike for t in self.transform):
            for idx, subj in self._by_index.items():
                ok = True
                for name in names:
                    t = subj[name][DATA]
                    pads = any(n < g for n, g in zip(t.shape[1:], self.target_shape))
                    ok = ok and float(t.min()) >= 0 and (self.padding_value >= 0 or not pads)
                self.nonnegative[idx] = ok
        self._check_nonlocal()
        self.spatial = _spatial_stages_of(spatial)
        if tensor_images is None:
            tensor_images = {"dwi-tensor": None} if "dwi-tensor" in names else {}
        self.tensor_images = {name: augment.check_tensor_rescale(r) for name, r in dict(tensor_images).items()}
        self._channel_min: Dict[Tuple[int, str], torch.Tensor] = {}   # (subject, image) -> (C, 2) f64 (sum, min) on the device
        if self.spatial:
            for name in self.tensor_images:
                if name not in names:
                    raise ValueError(f"tensor image '{name}' is not among the images of the queue {names}")
                if self.channels[name] != 6:
                    raise ValueError(f"tensor image '{name}' has {self.channels[name]} channels; a diffusion tensor has 6 "
                                     "(dxx, dxy, dxz, dyy, dyz, dzz)")
            if len(self.tensor_images) > 1:
                raise ValueError(f"one tensor image per queue (a load carries one reorientation), got {list(self.tensor_images)}")
            # 'minimum' fills with the channel minima of crop_or_pad(raw): reduced on the device once per subject image,
            # here, so that next_batch only passes a pointer
            if any(t.fill is None for t in self.spatial):
                for idx, subj in self._by_index.items():
                    for name in dict.fromkeys(names):
                        if subj[name][DATA].is_cuda:
                            self._channel_minimum(idx, name)
        self._staged: Dict[int, Tuple[SubjectLoad, Dict[str, torch.Tensor]]] = {}   # id(load) -> (load, {image: tensor})
        self._gen = torch.Generator().manual_seed(int(seed))
        self.epoch = -1
        self._order: List[int] = []          # subjects left in the current epoch (next one at the end)
        self._patches: List[PlannedPatch] = []
        self.fill_count = 0                          # fills so far
        self.last_fill: List[SubjectLoad] = []       # the loads of the current fill, in load order

    def __len__(self):
        return len(self.subjects) * self.samples_per_volume

    # ---- state at an epoch boundary --------------------------------------------------------------------------------
    def _drained(self) -> bool:
        self._release_staged(())             # staging tensors of loads whose last patch has been gathered are dead
        return not self._patches and not self._order and not self._staged

    def state_dict(self) -> Dict:
        """``{'generator': uint8 tensor, 'epoch', 'fill_count'}`` -- all a queue carries from one epoch into the next.  Valid
        only when the queue is drained (no pending patch, no subject left in the epoch, nothing staged), which is where a
        whole number of epochs of ``batches()`` / ``next_plan(len(queue))`` leaves it; otherwise ``RuntimeError``: a queue in
        the middle of an epoch is not resumable.  A fresh queue over the same subjects and arguments that loads the state
        plans the following epochs identically: same subjects, load seeds, stages and origins."""
        if not self._drained():
            raise RuntimeError("PatchQueue.state_dict: the queue is in the middle of an epoch "
                               f"({len(self._patches)} patches pending, {len(self._order)} subjects left, "
                               f"{len(self._staged)} loads staged); its state is defined at epoch boundaries only")
        return {"generator": self._gen.get_state().clone(), "epoch": int(self.epoch), "fill_count": int(self.fill_count)}

    def load_state_dict(self, state: Dict) -> None:
        if not self._drained():
            raise RuntimeError("PatchQueue.load_state_dict: the queue is in the middle of an epoch")
        self._gen.set_state(torch.as_tensor(state["generator"], dtype=torch.uint8).cpu())
        self.epoch, self.fill_count = int(state["epoch"]), int(state["fill_count"])
        self.last_fill = []

    def _check_nonlocal(self) -> None:
        """what a staged stage cannot do is refused here, not at the first load in which the stage happens to fire"""
        limit = augment.AXIS_MAX_N
        for i, t in enumerate(self.transform):
            if type(t) is augment.RandomMotion:
                axes, what = (2,), "RandomMotion"
                if t.num_transforms + 1 > augment.MOTION_MAX_IMAGES:
                    raise ValueError(f"RandomMotion(num_transforms={t.num_transforms}): more than "
                                     f"{augment.MOTION_MAX_IMAGES - 1} transforms per image are not built on the device")
            elif type(t) is augment.RandomGhosting:
                axes, what = t.axes, "RandomGhosting"
            elif type(t) is augment.RandomBlur:
                axes, what = ((0, 1, 2) if augment.blur_radius(t.std_range[1]) > 0 else ()), "RandomBlur"
            elif type(t) is augment.RandomSpike:
                if t.num_spikes_range[1] > 1:
                    raise ValueError(f"RandomSpike(num_spikes={t.num_spikes_range}): more than one spike per load is not "
                                     "built on the device")
                dc_always = all(self.nonnegative.values()) and all(type(b) in _SIGN_PRESERVING for b in self.transform[:i])
                axes, what = (() if dc_always else (0, 1, 2)), "RandomSpike (DFT path)"
            else:
                continue
            for a in axes:
                if self.target_shape[a] > limit:
                    raise ValueError(f"{what} works along axis {a}, where the target extent {self.target_shape[a]} exceeds "
                                     f"{limit} (larger extents are not tiled)")

    # ---- host plan ---------------------------------------------------------------------------------------------
    def spike_path(self, subject: int, before: Sequence) -> str:
        """'dc' or 'dft' for a RandomSpike of a load of ``subject`` that runs after the stages ``before`` ((transform,
        params) pairs that fired): 'dc' only if every image of the subject is non-negative after crop/pad and every
        earlier stage keeps it so (bias field, gamma, blur); after motion, ghosting or noise, 'dft'"""
        ok = self.nonnegative.get(subject, False) and all(type(t) in _SIGN_PRESERVING for t, _ in before)
        return "dc" if ok else "dft"

    def _draw_stages(self, subject: int) -> Tuple[int, tuple]:
        """the stages that fire for one load, drawn like ``_Random.__call__`` (``rand(1) < p``, then ``sample()``)
        from the global CPU generator seeded from the queue's own generator; a spike's parameters get its path.  A
        per-image stage (``RandomMotion``) draws one set per augmented image, always for the modality and then each kept
        source, whether or not a batch will ask for the augmented target, so that a plan does not depend on that flag"""
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=self._gen))
        stages = []
        with torch.random.fork_rng(devices=[]):
            torch.default_generator.manual_seed(seed)
            for t in self.transform:
                if torch.rand(1).item() < t.p:
                    if t.per_image:
                        params = {name: t.sample() for name in self._augmented_names()}
                    else:
                        params = t.sample()
                    if type(t) is augment.RandomSpike:
                        params = params._replace(path=self.spike_path(subject, stages))
                    stages.append((t, params))
        return seed, tuple(stages)

    def _draw_spatial(self, seed: int) -> tuple:
        """the spatial stages that fire for a load whose intensity stages were drawn under ``seed``: drawn like them, but
        under ``seed + 1`` and never from the queue's generator, so that they leave every other draw where it was"""
        if not self.spatial:
            return ()
        fired = []
        with torch.random.fork_rng(devices=[]):
            torch.default_generator.manual_seed(seed + 1)
            for t in self.spatial:
                if torch.rand(1).item() < t.p:
                    fired.append((t, t.sample()))
        return tuple(fired)

    def _augmented_names(self) -> List[str]:
        """the images of a subject that a batch can ask for augmented: the modality, then each kept source"""
        return [self.modality] + [src for src in self.keep if src != self.modality]

    def _fill(self) -> None:
        if not self._order:
            self.epoch += 1
            self._order = [self.indices[int(i)] for i in torch.randperm(len(self.indices), generator=self._gen).flip(0)]
        n = min(self.max_length // self.samples_per_volume, len(self._order))
        loads, patches = [], []
        for _ in range(n):
            subject = self._order.pop()
            seed, stages = self._draw_stages(subject)
            load = SubjectLoad(subject, self.epoch, self.fill_count, seed, stages, self._draw_spatial(seed))
            loads.append(load)
            patches += [PlannedPatch(load, o) for o in
                        self.sampler.draw(self.target_shape, self.samples_per_volume, self._gen)]
        perm = torch.randperm(len(patches), generator=self._gen)
        self._patches = [patches[int(i)] for i in perm]
        self.last_fill = loads
        self.fill_count += 1

    def next_plan(self, batch_size: int = 8) -> List[PlannedPatch]:
        """the next ``batch_size`` patches of the queue (host only: no GPU work)"""
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        out = []
        for _ in range(batch_size):
            if not self._patches:
                self._fill()
            out.append(self._patches.pop())
        return out

    # ---- device gather -----------------------------------------------------------------------------------------
    def _images(self, augmented_target: bool):
        """(output name, source name, augmented) of every image a batch writes"""
        imgs = [(self.modality, self.modality, True)]
        for src, kept in self.keep.items():
            imgs.append((kept, src, False))
            if augmented_target and src != self.modality:
                imgs.append((src, src, True))
        if len(imgs) > _MAX_IMAGES:
            raise ValueError(f"a batch writes at most {_MAX_IMAGES} images, asked for {[i[0] for i in imgs]}")
        return imgs

    def _outputs(self, imgs, b: int, out, device):
        shapes = {name: (b, self.channels[src]) + self.patch_size for name, src, _ in imgs}
        if out is None:
            return {name: torch.empty(s, dtype=torch.float32, device=device) for name, s in shapes.items()}
        got = {}
        for name, s in shapes.items():
            if name not in out or not isinstance(out[name], dict) or DATA not in out[name]:
                raise ValueError(f"out= has no {{'{name}': {{'data': tensor}}}}")
            t = out[name][DATA]
            if tuple(t.shape) != s or t.dtype != torch.float32 or t.device != device or not t.is_contiguous():
                raise ValueError(f"out['{name}']: need a contiguous float32 {s} tensor on {device}, got "
                                 f"{t.dtype} {tuple(t.shape)} on {t.device}")
            got[name] = t
        spans = sorted((t.data_ptr(), t.data_ptr() + t.numel() * 4, name) for name, t in got.items())
        for (_, end, a), (start, _, bname) in zip(spans, spans[1:]):
            if start < end:
                raise ValueError(f"out['{a}'] and out['{bname}'] share memory: each written image needs its own tensor")
        return got

    @staticmethod
    def split_stages(load: SubjectLoad) -> Tuple[tuple, tuple]:
        """(staged, fused): the stages up to and including the last non-local one that has an effect, applied once
        into a staging tensor, and the local stages after it, fused into the gather.  A non-local stage without an
        effect (a blur whose three radii are 0, a ghosting or spike of intensity 0, a motion whose rotations and
        translations are all 0) is the identity and is dropped."""
        live = [(t, p) for t, p in load.stages if type(t) not in _NONLOCAL or t.has_effect(p)]
        last = max((i for i, (t, _) in enumerate(live) if type(t) in _NONLOCAL), default=-1)
        return tuple(live[:last + 1]), tuple(live[last + 1:])

    def spatial_transform(self, load: SubjectLoad) -> Optional[Tuple[np.ndarray, Optional[float]]]:
        """(M, fill) of a load: the 4 x 4 f64 product of its spatial stages in list order, in target coordinates, and what
        an outside voxel gets (None = the channel minimum); ``None`` if no stage fired with an effect.  A flip with no
        axis drawn and an affine with s = 1, zero angles and zero shift are dropped, as ``split_stages`` drops no-ops."""
        live = [(t, p) for t, p in load.spatial if t.has_effect(p)]
        if not live:
            return None
        fills = [t.fill for t, _ in live if isinstance(t, augment.RandomAffine)]    # a flip leaves no voxel outside
        return (augment.compose_index_matrices([t.matrix(p, self.target_shape) for t, p in live]),
                fills[0] if fills else 0.0)

    def _channel_minimum(self, subject: int, name: str) -> torch.Tensor:
        key = (subject, name)
        if key not in self._channel_min:
            x = augment.crop_or_pad(self._by_index[subject][name][DATA], self.target_shape, self.padding_value)
            self._channel_min[key] = augment.channel_sum_min(x)
        return self._channel_min[key]

    def _staged_source(self, load: SubjectLoad, staged: tuple, name: str) -> torch.Tensor:
        """chain(affine_resample(crop_or_pad(raw))) through ``staged`` for one image of one load, made once and kept while
        the load has patches (the resample only if a spatial stage of the load has an effect); a per-image stage applies
        the parameter set of the image it stages"""
        entry = self._staged.setdefault(id(load), (load, {}))[1]
        if name not in entry:
            x = augment.crop_or_pad(self._by_index[load.subject][name][DATA], self.target_shape, self.padding_value)
            sp = self.spatial_transform(load)
            if sp is not None:
                x = augment.affine_resample(x, sp[0], sp[1], self.tensor_images.get(name, augment.NOT_A_TENSOR))
            for t, params in staged:
                x = t.apply(x, params[name] if t.per_image else params)
            entry[name] = x
        return entry[name]

    def _release_staged(self, plan: Sequence[PlannedPatch]) -> None:
        """drop the staging tensors of loads that have no patch left, in this batch or in the queue"""
        if self._staged:
            live = {id(p.load) for p in plan} | {id(p.load) for p in self._patches}
            for key in [k for k in self._staged if k not in live]:
                del self._staged[key]

    @staticmethod
    def _load_struct(stages: tuple) -> _lib.QueueLoad:
        q = _lib.QueueLoad()
        q.nstages = len(stages)
        for s, (t, params) in enumerate(stages):
            q.stage[s] = _STAGE_KIND[type(t)]
            if isinstance(t, augment.RandomBiasField):
                coef = np.asarray(params, dtype=np.float32)
                q.bias_order = t.order
                for i, c in enumerate(coef):
                    q.bias_coef[i] = float(c)
            elif isinstance(t, augment.RandomNoise):
                q.noise_mean, q.noise_std, q.noise_seed = float(params[0]), float(params[1]), int(params[2])
            else:
                q.gamma = float(params)
        return q

    def gather(self, plan: Sequence[PlannedPatch], out=None, augmented_target: bool = False):
        """write the patches of ``plan`` (one launch, or one per chunk of MI355_MAX_PATCHES patches / MI355_QUEUE_MAX_LOADS
        loads, cut by the library): the plain gather, or the spatial one if a load of the plan has a spatial stage with an effect"""
        imgs = self._images(augmented_target)
        sources = {name: [self._by_index[p.load.subject][name][DATA] for p in plan] for _, name, _ in imgs}
        device = self._by_index[plan[0].load.subject][self.modality][DATA].device
        for name, ts in sources.items():
            for t in ts:
                if not t.is_cuda:
                    raise _lib.Mi355Error("the patch queue gathers on the GPU only (no CPU fallback)")
                if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
                    raise ValueError(f"subject image '{name}' must be a contiguous float32 tensor on {device}")
        outs = self._outputs(imgs, len(plan), out, device)
        slot: Dict[int, int] = {}
        loads: List[SubjectLoad] = []
        for p in plan:
            if id(p.load) not in slot:
                slot[id(p.load)] = len(loads)
                loads.append(p.load)
        nimg = len(imgs)
        self._release_staged(plan)
        split = [self.split_stages(l) for l in loads]
        qloads = (_lib.QueueLoad * len(loads))(*[self._load_struct(fused) for _, fused in split])
        qsrc = (_lib.QueueSource * (len(loads) * nimg))()
        for li, load in enumerate(loads):
            for j, (_, src, aug) in enumerate(imgs):
                t = self._by_index[load.subject][src][DATA]
                if aug and split[li][0]:          # a source of the target extent: the gather's crop/pad is the identity
                    t = self._staged_source(load, split[li][0], src)
                qsrc[li * nimg + j] = _lib.QueueSource(t.data_ptr(), *t.shape[1:])
        channels = (C.c_int32 * nimg)(*[self.channels[src] for _, src, _ in imgs])
        augmented = (C.c_int32 * nimg)(*[int(a) for _, _, a in imgs])
        ptrs = (C.c_void_p * nimg)(*[outs[name].data_ptr() for name, _, _ in imgs])
        pat = np.array([[slot[id(p.load)], *p.origin] for p in plan], dtype=np.int32)
        moved = [self.spatial_transform(l) for l in loads]
        if all(m is None for m in moved):
            _lib.check(_lib.load().mi355_patch_queue_gather(
                qloads, len(loads), qsrc, channels, augmented, ptrs, nimg, pat.ctypes.data_as(C.c_void_p), len(plan),
                *self.target_shape, *self.patch_size, self.padding_value, torch.cuda.current_stream(device).cuda_stream),
                "patch_queue_gather")
        else:
            # one launch serves the whole batch; a load without a spatial stage rides along with every image read as is,
            # and so does the staged image of a load that has one: its resample was done while staging
            qsp = (_lib.QueueSpatial * len(loads))()
            qrs = (_lib.QueueResampling * (len(loads) * nimg))()
            for li, load in enumerate(loads):
                if moved[li] is None:
                    continue
                m, fill = moved[li]
                qsp[li].m[:] = augment._rigid_rows(m).tolist()
                for name, rescale in self.tensor_images.items():
                    qsp[li].t6[:] = augment._tensor_rows(m, rescale).tolist()
                for j, (_, src, aug) in enumerate(imgs):
                    if aug and split[li][0]:
                        continue
                    cmin = self._channel_minimum(load.subject, src).data_ptr() if fill is None else None
                    qrs[li * nimg + j] = _lib.QueueResampling(cmin, 0.0 if fill is None else fill, 1)
            tensor = (C.c_int32 * nimg)(*[int(src in self.tensor_images) for _, src, _ in imgs])
            _lib.check(_lib.load().mi355_patch_queue_gather_spatial(
                qloads, qsp, len(loads), qsrc, qrs, channels, augmented, tensor, ptrs, nimg,
                pat.ctypes.data_as(C.c_void_p), len(plan), *self.target_shape, *self.patch_size, self.padding_value,
                torch.cuda.current_stream(device).cuda_stream), "patch_queue_gather_spatial")
        batch = {name: {DATA: outs[name]} for name, _, _ in imgs}
        ini = np.array([p.origin for p in plan], dtype=np.int64)
        batch[LOCATION] = torch.from_numpy(np.hstack([ini, ini + np.array(self.patch_size, dtype=np.int64)]))
        return batch

    def next_batch(self, batch_size: int = 8, out=None, augmented_target: bool = False):
        """``{modality: {'data'}, <kept>: {'data'}, 'location': (B, 6) int64}`` -- the layout ``unpack_batch`` reads;
        the augmented ``'dwi-tensor'`` too with ``augmented_target=True``.  With ``out=`` (e.g. the static batch of a
        ``GraphedTrainingStep``) the launch writes into those tensors: nothing is allocated or copied."""
        return self.gather(self.next_plan(batch_size), out=out, augmented_target=augmented_target)

    def batches(self, batch_size: int = 8, **kw):
        """one epoch's worth, like ``DataLoader(queue, batch_size)``: ceil(len / batch_size) batches"""
        left = len(self)
        while left > 0:
            n = min(batch_size, left)
            left -= n
            yield self.next_batch(n, **kw)
