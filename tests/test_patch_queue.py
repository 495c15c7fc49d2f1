"""Device patch queue (unet_bssfp_amd.data): the reference's train/val loader (src/data_module.py:125-188).

CPU: the host plan -- split, shards, epochs, fills, origins, stage rates and parameters, argument errors.
GPU: the fused gather (csrc/patch_queue.hip) against the chained path extract_patches(chain(crop_or_pad(raw))), bit for
bit, and the feed of a GraphedTrainingStep.  TorchIO is absent, so parity with its exact random streams is **unpinned**:
the tests pin the structure (TorchIO's Queue) and the equality with this package's own chained augmentations.
"""
import ctypes
from collections import Counter

import numpy as np
import pytest
import torch

from unet_bssfp_amd import augment as A
from unet_bssfp_amd import data as Q

DEV = "cuda:0"


def _subjects(n, shape=(2, 6, 7, 8), device="cpu", seed=0, extents=None):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        s = extents[i % len(extents)] if extents else shape[1:]
        out.append({"bssfp": {"data": (torch.rand((24,) + tuple(s), generator=g) - 0.3).to(device)},
                    "dwi-tensor": {"data": (torch.rand((6,) + tuple(s), generator=g) - 0.3).to(device)}})
    return out


def _cpu_queue(n=5, **kw):
    subs = [{"bssfp": {"data": torch.zeros(24, 1, 1, 1)}, "dwi-tensor": {"data": torch.zeros(6, 1, 1, 1)}} for _ in range(n)]
    kw.setdefault("target_shape", (10, 12, 14))
    kw.setdefault("sampler", Q.UniformSampler((4, 5, 6)))
    return Q.PatchQueue(subs, "bssfp", **kw)


# ---- CPU: host plan ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [10, 37])
def test_split_subjects_is_the_reference_random_split(n):
    ids = [f"sub-{i:03d}" for i in range(n)]
    parts = torch.utils.data.random_split(ids, [0.8, 0.1, 0.1], torch.Generator().manual_seed(42))
    want = tuple([ids[i] for i in p.indices] for p in parts)
    got = Q.split_subjects(ids)
    assert got == want
    assert sorted(sum(got, [])) == ids
    assert Q.split_subjects(ids, 0.2, 0.1, seed=7) == tuple(
        [ids[i] for i in p.indices] for p in torch.utils.data.random_split(ids, [0.7, 0.2, 0.1], torch.Generator().manual_seed(7)))


def test_epochs_load_every_subject_once_with_samples_per_volume_patches():
    q = _cpu_queue(5, max_length=16, samples_per_volume=8, seed=3)
    assert len(q) == 40
    orders = []
    for epoch in range(3):
        plan = q.next_plan(len(q))
        assert {p.load.epoch for p in plan} == {epoch}
        per_load = Counter(id(p.load) for p in plan)
        assert sorted(per_load.values()) == [8] * 5
        assert sorted(Counter(p.load.subject for p in plan).items()) == [(i, 8) for i in range(5)]
        loads = {id(p.load): p.load for p in plan}.values()
        fills = sorted({l.fill for l in loads})
        assert fills == list(range(3 * epoch, 3 * epoch + 3))         # fills of 2, 2, 1 subjects
        orders.append(tuple(frozenset(l.subject for l in loads if l.fill == f) for f in fills))
    assert len(set(orders)) > 1                                       # a fresh permutation per epoch


def _fill_sizes(plan):
    return sorted(Counter(l.fill for l in {id(p.load): p.load for p in plan}.values()).items())


def test_fills_hold_max_length_over_samples_per_volume_subjects():
    q = _cpu_queue(7, max_length=12, samples_per_volume=4, seed=1)
    assert len(q) == 28
    assert _fill_sizes(q.next_plan(28)) == [(0, 3), (1, 3), (2, 1)]   # the last fill takes what is left of the epoch
    assert q.fill_count == 3 and [l.fill for l in q.last_fill] == [2]
    first = q.next_plan(1)[0]
    assert q.fill_count == 4 and len(q.last_fill) == 3 and first.load in q.last_fill
    q = _cpu_queue(4, max_length=16, samples_per_volume=8)
    assert _fill_sizes(q.next_plan(len(q))) == [(0, 2), (1, 2)]
    # patches are popped from the end of the shuffled fill
    q = _cpu_queue(4, max_length=16, samples_per_volume=8, seed=5)
    q.next_plan(1)
    rest = list(q._patches)
    assert q.next_plan(15) == rest[::-1]


def test_the_queue_keeps_no_history():
    """a training loop pulls batches for days: the host plan must not grow with the number of fills"""
    import tracemalloc
    q = _cpu_queue(4, seed=6, max_length=16, samples_per_volume=8)   # reference transform: stages do fire
    tracemalloc.start()
    try:
        for _ in range(300):                                          # caches and tracemalloc's own first allocations
            q.next_plan(8)
        base = tracemalloc.get_traced_memory()[0]
        for _ in range(2000):
            q.next_plan(8)
        grown = tracemalloc.get_traced_memory()[0] - base
    finally:
        tracemalloc.stop()
    assert q.fill_count >= 1000 and len(q.last_fill) <= 2
    assert grown < 32 * 1024, grown                                   # keeping every fill's loads: ~450 KB here


def test_shards_over_three_ranks_are_disjoint_and_complete():
    seen = []
    for rank in range(3):
        q = _cpu_queue(10, rank=rank, world=3, samples_per_volume=2, max_length=4)
        assert q.indices == list(range(10))[rank::3]
        assert len(q) == 2 * len(q.indices)
        seen.append({p.load.subject for p in q.next_plan(len(q))})
        assert seen[-1] == set(q.indices)
    assert set.union(*seen) == set(range(10)) and sum(map(len, seen)) == 10


def test_origins_stay_in_bounds_and_reach_both_extremes():
    q = _cpu_queue(3, seed=11, transform=[])
    origins = np.array([p.origin for p in q.next_plan(3000)])
    hi = np.array([10 - 4, 12 - 5, 14 - 6])
    assert (origins >= 0).all() and (origins <= hi).all()
    assert (origins.min(0) == 0).all() and (origins.max(0) == hi).all()
    s = Q.UniformSampler(64)
    assert s.patch_size == (64, 64, 64)
    o = np.array(s.draw((96, 128, 128), 4000, torch.Generator().manual_seed(0)))
    assert o.min() == 0 and o.max(0).tolist() == [32, 64, 64]


def test_stages_fire_at_rate_p():
    p = 0.3
    tr = [A.RandomBiasField(p=p), A.RandomNoise(p=p, std=(0.01, 0.1)), A.RandomGamma(p=p)]
    q = _cpu_queue(2, max_length=1, samples_per_volume=1, transform=tr, seed=2)
    loads = [pl.load for pl in q.next_plan(3000)]
    assert len({id(l) for l in loads}) == 3000
    tol = 4.5 * np.sqrt(p * (1 - p) / 3000)
    for t in tr:
        rate = np.mean([any(s[0] is t for s in l.stages) for l in loads])
        assert abs(rate - p) < tol, (type(t).__name__, rate)
    for l in loads:                                                   # list order is kept
        kinds = [tr.index(s[0]) for s in l.stages]
        assert kinds == sorted(kinds)


def test_same_seed_same_plan_and_parameters_equal_a_chained_sample_sequence():
    def plan(seed):
        q = _cpu_queue(6, seed=seed, transform=[A.RandomBiasField(p=0.5), A.RandomNoise(p=0.5), A.RandomGamma(p=0.5)])
        return q, q.next_plan(60)

    q1, a = plan(9)
    _, b = plan(9)
    _, c = plan(10)

    def key(pl):
        return [(p.load.subject, p.load.seed, p.origin, [type(t).__name__ for t, _ in p.load.stages]) for p in pl]
    assert key(a) == key(b) and key(a) != key(c)
    fired = 0
    for load in {id(p.load): p.load for p in a}.values():
        torch.manual_seed(load.seed)                                  # the chain: _Random.__call__ for every transform
        want = []
        for t in q1.transform:
            if torch.rand(1).item() < t.p:
                want.append((t, t.sample()))
        assert [t for t, _ in load.stages] == [t for t, _ in want]
        for (_, got), (_, exp) in zip(load.stages, want):
            if isinstance(exp, np.ndarray):
                assert np.array_equal(got, exp)
            else:
                assert got == exp
        fired += len(want)
    assert fired > 0
    # the queue's draws leave the global generator alone
    torch.manual_seed(123)
    before = torch.rand(3)
    torch.manual_seed(123)
    _cpu_queue(3, seed=4).next_plan(20)
    assert torch.equal(torch.rand(3), before)


def test_bad_shapes_raise_value_error_and_unfusable_transforms_type_error():
    with pytest.raises(ValueError):
        Q.UniformSampler(0)
    with pytest.raises(ValueError):
        Q.UniformSampler((64, 64))
    with pytest.raises(ValueError):                                 # patch larger than the target
        _cpu_queue(2, target_shape=(10, 4, 14))
    with pytest.raises(ValueError):
        _cpu_queue(2, target_shape=(0, 12, 14))
    with pytest.raises(ValueError):
        _cpu_queue(2, max_length=4, samples_per_volume=8)
    with pytest.raises(ValueError):
        _cpu_queue(2, rank=3, world=3)
    with pytest.raises(ValueError):                                 # a channel count that changes between subjects
        Q.PatchQueue([{"bssfp": {"data": torch.zeros(24, 4, 4, 4)}, "dwi-tensor": {"data": torch.zeros(6, 4, 4, 4)}},
                      {"bssfp": {"data": torch.zeros(12, 4, 4, 4)}, "dwi-tensor": {"data": torch.zeros(6, 4, 4, 4)}}],
                     "bssfp", sampler=Q.UniformSampler(2), target_shape=(4, 4, 4))

    class RandomBlur(A._Random):
        pass
    with pytest.raises(TypeError):
        _cpu_queue(2, transform=[A.RandomNoise(), RandomBlur()])
    with pytest.raises(TypeError):
        _cpu_queue(2, transform=[A.RandomNoise(), A.RandomNoise()])
    with pytest.raises(TypeError):
        _cpu_queue(2, transform=[lambda s: s])


def test_gather_arguments_are_checked_on_the_host():
    from unet_bssfp_amd import _lib
    assert ctypes.sizeof(_lib.QueueLoad) == 184 and ctypes.sizeof(_lib.QueueSource) == 24
    lib = _lib.load()
    one = (ctypes.c_int32 * 1)(1)
    rc = lib.mi355_patch_queue_gather(None, 0, None, one, one, None, 1, None, 1, 8, 8, 8, 9, 8, 8, 0.0, None)
    assert rc < 0 and b"shape" in lib.mi355_last_error()
    rc = lib.mi355_patch_queue_gather(None, 0, None, one, one, None, 1, None, 1, 8, 8, 8, 4, 4, 4, 0.0, None)
    assert rc < 0 and b"null" in lib.mi355_last_error()
    assert lib.mi355_patch_queue_gather(None, 0, None, one, one, None, 1, None, 0, 8, 8, 8, 4, 4, 4, 0.0, None) == 0
    with pytest.raises(_lib.Mi355Error):                            # no CPU fallback
        _cpu_queue(2, transform=[]).next_batch(2)


def test_stage_boundary_is_never_contracted(tmp_path):
    """the bias product followed by the noise add, in ONE basic block (what a stage-mask template or an if-converted
    stage loop would give the fused kernel): gfx950 ISA must keep a separate multiply and add, no fma"""
    import os
    import re
    import subprocess
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unet_bssfp_amd", "csrc")
    src = tmp_path / "probe.hip"
    src.write_text('#include "augment_core.h"\n'
                   'extern "C" __global__ void probe(const float* x, float* out, float g, float mean) {\n'
                   '  out[threadIdx.x] = aug_noise_shift(aug_bias_apply(x[threadIdx.x], g), mean);\n}\n')
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", csrc,
                    str(src), "-o", str(tmp_path / "probe.s")], check=True, capture_output=True)
    isa = (tmp_path / "probe.s").read_text()
    body = isa[isa.index("probe:"):isa.index("s_endpgm")]
    ops = re.findall(r"\bv_(fma\w*|fmac\w*|mad\w*|pk_fma\w*|mul_f32\w*|add_f32\w*)", body)
    assert not [o for o in ops if o.startswith(("fma", "mad", "pk_fma"))], ops
    assert any(o.startswith("mul_f32") for o in ops) and any(o.startswith("add_f32") for o in ops), ops


def test_subjects_from_nifti_moves_the_fourth_axis_to_the_front(tmp_path):
    from unet_bssfp_amd import nifti
    vol4 = np.random.default_rng(0).random((5, 6, 7, 3)).astype(np.float32)
    vol3 = vol4[..., 0].copy()
    nifti.save(vol4, str(tmp_path / "a.nii.gz"))
    nifti.save(vol3, str(tmp_path / "b.nii"))
    s = Q.subjects_from_nifti({"dwi-tensor": str(tmp_path / "a.nii.gz"), "t1w": str(tmp_path / "b.nii")}, "cpu")
    assert s["dwi-tensor"]["data"].shape == (3, 5, 6, 7) and s["t1w"]["data"].shape == (1, 5, 6, 7)
    assert s["dwi-tensor"]["data"].dtype == torch.float32
    assert np.array_equal(s["dwi-tensor"]["data"][2].numpy(), vol4[..., 2])
    assert np.array_equal(s["t1w"]["data"][0].numpy(), vol3)


# ---- GPU: the fused gather -------------------------------------------------------------------------------------------

def _chained(q, plan, name, augmented):
    """extract_patches(chain(crop_or_pad(raw))) patch by patch: the unfused path the kernel must reproduce"""
    from unet_bssfp_amd.inference import extract_patches
    out = []
    for p in plan:
        x = A.crop_or_pad(q._by_index[p.load.subject][name]["data"], q.target_shape, q.padding_value)
        if augmented:
            for t, params in p.load.stages:
                x = t.apply(x, params)
        loc = np.array([list(p.origin) + [o + s for o, s in zip(p.origin, q.patch_size)]])
        out.append(extract_patches(x, loc, q.patch_size))
    return torch.cat(out)


def _check_batch(q, plan, batch, augmented_target=True):
    assert torch.equal(batch["bssfp"]["data"], _chained(q, plan, "bssfp", True))
    assert torch.equal(batch["dwi-tensor_orig"]["data"], _chained(q, plan, "dwi-tensor", False))
    if augmented_target:
        assert torch.equal(batch["dwi-tensor"]["data"], _chained(q, plan, "dwi-tensor", True))
    want = np.array([list(p.origin) + [o + s for o, s in zip(p.origin, q.patch_size)] for p in plan])
    assert batch["location"].dtype == torch.int64 and np.array_equal(batch["location"].numpy(), want)


_STAGE_SETS = {
    "none": [],
    "bias": [(A.RandomBiasField(), "bias")],
    "noise": [(A.RandomNoise(), "noise")],
    "gamma": [(A.RandomGamma(), "gamma")],
    "all": [(A.RandomBiasField(), "bias"), (A.RandomNoise(), "noise"), (A.RandomGamma(), "gamma")],
}


def _params(kind, rng):
    if kind == "bias":
        return (rng.random(20) - 0.5).astype(np.float32)
    if kind == "noise":
        return (float(rng.uniform(-0.1, 0.1)), float(rng.uniform(0.01, 0.1)), int(rng.integers(0, 2 ** 62)))
    return float(np.exp(rng.uniform(-0.3, 0.3)))


@pytest.mark.gpu
@pytest.mark.parametrize("patch", [(8, 12, 16), (5, 7, 9)])          # 16-byte rows / the per-voxel kernel
@pytest.mark.parametrize("stages", list(_STAGE_SETS))
def test_gpu_fused_batch_equals_the_chained_path(hip, patch, stages):
    target = (20, 24, 32)
    # crop D + pad H; the target itself; pad D + crop H and W with an odd raw W (unaligned source rows); a W pad with
    # 16-byte source rows (lanes that straddle the W border next to aligned ones); a W pad with an odd raw W
    extents = [(23, 19, 32), (20, 24, 32), (17, 27, 37), (20, 24, 28), (21, 22, 29)]
    subs = _subjects(len(extents), device=DEV, seed=len(stages), extents=extents)
    q = Q.PatchQueue(subs, "bssfp", sampler=Q.UniformSampler(patch), target_shape=target, transform=[])
    rng = np.random.default_rng(sum(patch) + len(stages))
    hi = [t - p for t, p in zip(target, patch)]
    plan = []
    for i in range(len(extents)):
        load = Q.SubjectLoad(i, 0, 0, 0, tuple((t, _params(kind, rng)) for t, kind in _STAGE_SETS[stages]))
        origins = [(0, 0, 0), tuple(hi), (0, hi[1], 1), (hi[0], 0, hi[2] - 1)]
        origins += [tuple(int(rng.integers(0, h + 1)) for h in hi) for _ in range(3)]
        plan += [Q.PlannedPatch(load, o) for o in origins]
    batch = q.gather(plan, augmented_target=True)
    _check_batch(q, plan, batch)


@pytest.mark.gpu
def test_gpu_batches_straddle_fills_and_long_calls_are_chunked(hip):
    target, patch = (20, 24, 32), (8, 12, 16)
    subs = _subjects(7, device=DEV, seed=5, extents=[(23, 19, 32), (20, 24, 32), (17, 27, 37)])
    tr = [A.RandomBiasField(p=0.5), A.RandomNoise(p=0.5), A.RandomGamma(p=0.5)]

    def queue():
        return Q.PatchQueue(subs, "bssfp", max_length=4, samples_per_volume=2, sampler=Q.UniformSampler(patch),
                            target_shape=target, transform=tr, seed=21)
    q, twin = queue(), queue()
    for bs in (3, 6, 5):                                              # fills of 4 patches: every batch mixes fills
        plan = twin.next_plan(bs)
        batch = q.next_batch(bs, augmented_target=True)
        assert len({p.load.subject for p in plan}) > 1
        _check_batch(q, plan, batch)
    # 61 patches of 7 subjects (about 30 loads) in one call: chunks cut at 4 loads
    plan = twin.next_plan(61)
    batch = q.next_batch(61, augmented_target=True)
    assert len({id(p.load) for p in plan}) > 4 and any(p.load.stages for p in plan)
    _check_batch(q, plan, batch)
    # 61 patches of 3 loads in one call: chunks cut at MI355_MAX_PATCHES (48) patches, the second one written at
    # patch 48 of every output
    rng = np.random.default_rng(3)
    hi = [t - p for t, p in zip(target, patch)]
    loads = [Q.SubjectLoad(i, 0, 0, 0, tuple((t, _params(kind, rng)) for t, kind in _STAGE_SETS["all"][:i + 1]))
             for i in range(3)]
    plan = [Q.PlannedPatch(loads[b % 3], tuple(int(rng.integers(0, h + 1)) for h in hi)) for b in range(61)]
    _check_batch(q, plan, q.gather(plan, augmented_target=True))
    # without augmented_target the augmented dwi-tensor is not produced
    assert set(q.next_batch(2)) == {"bssfp", "dwi-tensor_orig", "location"}


@pytest.mark.gpu
def test_gpu_out_feed_checks_and_no_host_sync(hip):
    from unet_bssfp_amd.gan import synthetic_batch
    patch = (8, 12, 16)
    subs = _subjects(3, device=DEV, seed=8, extents=[(23, 19, 32)])
    q = Q.PatchQueue(subs, "bssfp", sampler=Q.UniformSampler(patch), target_shape=(20, 24, 32), seed=1)
    out = {"bssfp": {"data": torch.empty(4, 24, *patch, device=DEV)}, "dwi-tensor_orig": {"data": torch.empty(4, 6, *patch, device=DEV)}}
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        q.next_batch(4)
        b = q.next_batch(4, out=out)
        q.next_batch(4, augmented_target=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert b["bssfp"]["data"] is out["bssfp"]["data"] and b["dwi-tensor_orig"]["data"] is out["dwi-tensor_orig"]["data"]
    bad = {"bssfp": {"data": torch.empty(4, 24, 8, 12, 15, device=DEV)}, "dwi-tensor_orig": out["dwi-tensor_orig"]}
    with pytest.raises(ValueError):
        q.next_batch(4, out=bad)
    with pytest.raises(ValueError):
        q.next_batch(4, out={**out, "bssfp": {"data": out["bssfp"]["data"].double()}})
    with pytest.raises(ValueError):
        q.next_batch(4, out={**out, "bssfp": {"data": out["bssfp"]["data"].cpu()}})
    alias = synthetic_batch(4, patch, seed=0, device=DEV)             # dwi-tensor and dwi-tensor_orig share one tensor
    alias["bssfp"]["data"] = out["bssfp"]["data"]
    q.next_batch(4, out=alias)                                        # fine while the augmented target is not written
    with pytest.raises(ValueError):
        q.next_batch(4, out=alias, augmented_target=True)


@pytest.mark.gpu
def test_gpu_next_batch_feeds_a_graphed_training_step(hip):
    import unet_bssfp_amd as M
    from unet_bssfp_amd.functional import DropoutState
    from unet_bssfp_amd.gan import GraphedTrainingStep, bSSFPToDWITensorModel, synthetic_batch

    torch.manual_seed(4)
    DropoutState.reset()
    gen, discr = M.Generator("bssfp", dropout=0.05), M.Discriminator("bssfp")
    model = bSSFPToDWITensorModel("bssfp", gen=gen.to(DEV), discr=discr.to(DEV)).train()
    subs = _subjects(5, device=DEV, seed=2, extents=[(40, 52, 36), (36, 44, 44)])
    kw = dict(max_length=4, samples_per_volume=2, sampler=Q.UniformSampler(32), target_shape=(36, 48, 40),
              transform=A.reference_augmentation(), seed=17)
    q, twin = Q.PatchQueue(subs, "bssfp", **kw), Q.PatchQueue(subs, "bssfp", **kw)
    gs = GraphedTrainingStep(model, synthetic_batch(2, 32, seed=1, device=DEV), warmup=2)
    static = gs.instances[0][0]
    x_ptr = static["bssfp"]["data"].data_ptr()
    for _ in range(3):
        q.next_batch(2, out=static)
        want = twin.next_batch(2)
        assert static["bssfp"]["data"].data_ptr() == x_ptr
        assert torch.equal(static["bssfp"]["data"], want["bssfp"]["data"])
        assert torch.equal(static["dwi-tensor_orig"]["data"], want["dwi-tensor_orig"]["data"])
        gs(0)
        logs = torch.stack([v.reshape(()).float() for v in model.last_logs.values()])
        assert torch.isfinite(logs).all()
