"""CPU-only tests of the host-side seam between autograd and the launches (``unet_bssfp_amd.functional``): what every
``ConvSpec.w_*`` packing hands to ``ops.weight_pack``, and the address-keyed hand-over tables."""
import inspect

import pytest
import torch

from unet_bssfp_amd import functional as Fn
from unet_bssfp_amd import ops

BF16 = torch.bfloat16
CLASSES8 = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
_WPACK_SIG = inspect.signature(ops.weight_pack)


@pytest.fixture
def recorder(monkeypatch):
    """ops.weight_pack / ops.amax_f32 replaced by recorders: (packs, amaxes).  A pack is recorded as the tuple
    (cout, cin, ks, s_co, s_ci, s_k, tbase, tstep, dtype, cinp, coutp, s2d_mode, s2d_cp, src_offset) of weight_pack's own
    parameters (defaults filled in), followed by the source, ``reuse`` and ``q_amax`` objects."""
    packs, amaxes = [], []

    def weight_pack(*args, **kwargs):
        b = _WPACK_SIG.bind(*args, **kwargs)
        b.apply_defaults()
        a = b.arguments
        packs.append((tuple(tuple(v) if isinstance(v, (list, tuple)) else v for v in (
            a["cout"], a["cin"], a["ks"], a["s_co"], a["s_ci"], a["s_k"], a["tbase"], a["tstep"], a["dtype"], a["cinp"],
            a["coutp"], a["s2d_mode"], a["s2d_cp"], a["src_offset"])), a["src"], a["reuse"], a["q_amax"]))
        ops.LAST_WPACK_DESC[0] = None
        return torch.empty((1,)), a["coutp"] or 32, a["cinp"] or 16

    def amax_f32(x, out=None):
        amaxes.append((x, out))
        return torch.ones((1,)) if out is None else out

    monkeypatch.setattr(ops, "weight_pack", weight_pack)
    monkeypatch.setattr(ops, "amax_f32", amax_f32)
    return packs, amaxes


def _cases():
    """(spec, weight shape, [(method, arguments after the weight, expected record)])"""
    conv3 = Fn.ConvSpec("conv", 5, 7, 3, 1, 1)
    conv4 = Fn.ConvSpec("conv", 5, 7, 4, 2, 1)
    dec = Fn.ConvSpec("deconv2", 6, 64, 2, 2, 0)
    k3, k4, k2 = (9, 3, 1), (16, 4, 1), (4, 2, 1)
    z, one, two = (0, 0, 0), (1, 1, 1), (2, 2, 2)
    m1, m2 = (-1, -1, -1), (-2, -2, -2)
    c3 = [
        ("w_fwd", (BF16, 16), (7, 5, 3, 135, 27, k3, z, one, BF16, 16, None, 0, 0, 0)),
        ("w_fwd", (torch.float32, 32), (7, 5, 3, 135, 27, k3, z, one, torch.float32, 32, None, 0, 0, 0)),
        ("w_dgrad_s1", (BF16, 16), (5, 7, 3, 27, 135, k3, two, m1, BF16, 16, None, 0, 0, 0)),
        ("w_fwd8", (16,), (7, 5, 3, 135, 27, k3, z, one, ops.FP8, 16, None, 0, 0, 0)),
        ("w_dgrad8", (16,), (5, 7, 3, 27, 135, k3, two, m1, ops.FP8, 16, None, 0, 0, 0)),
        ("w_fwd_part", (BF16, 16, 0, 2), (7, 2, 3, 135, 27, k3, z, one, BF16, 16, None, 0, 0, 0)),
        ("w_fwd_part", (BF16, 16, 2, 3), (7, 3, 3, 135, 27, k3, z, one, BF16, 16, None, 0, 0, 54)),
        ("w_dgrad_s1_part", (BF16, 16, 0, 2), (2, 7, 3, 27, 135, k3, two, m1, BF16, 16, None, 0, 0, 0)),
        ("w_dgrad_s1_part", (BF16, 16, 2, 3), (3, 7, 3, 27, 135, k3, two, m1, BF16, 16, None, 0, 0, 54)),
    ]
    c4 = [
        ("w_fwd_s2d", (BF16, 8), (7, 5, 2, 320, 64, k4, z, two, BF16, 64, None, 1, 8, 0)),
        ("w_dgrad_s2d", (BF16, 16, 8), (5, 7, 2, 64, 320, k4, two, m2, BF16, 16, 64, 2, 8, 0)),
        ("w_fwd_s2d_part", (BF16, 8, 0, 2), (7, 2, 2, 320, 64, k4, z, two, BF16, 64, None, 1, 8, 0)),
        ("w_fwd_s2d_part", (BF16, 8, 2, 3), (7, 3, 2, 320, 64, k4, z, two, BF16, 64, None, 1, 8, 128)),
        ("w_dgrad_s2d_part", (BF16, 16, 8, 0, 2), (2, 7, 2, 64, 320, k4, two, m2, BF16, 16, 64, 2, 8, 0)),
        ("w_dgrad_s2d_part", (BF16, 16, 8, 2, 3), (3, 7, 2, 64, 320, k4, two, m2, BF16, 16, 64, 2, 8, 128)),
    ]
    cd = [
        ("w_deconv_fwd_all", (BF16, 16), (64, 6, 1, 8, 512, k2, z, z, BF16, 16, 512, 2, 64, 0)),
        ("w_deconv_dgrad", (BF16, 64), (6, 64, 2, 512, 8, k2, z, one, BF16, 64, None, 0, 0, 0)),
    ]
    for cls in CLASSES8:
        tb = tuple(3 if p == 0 else 2 for p in cls)
        c4.append(("w_dgrad_s2", (BF16, 16, cls), (5, 7, 2, 64, 320, k4, tb, m2, BF16, 16, None, 0, 0, 0)))
        cd.append(("w_deconv_fwd", (BF16, 16, cls), (64, 6, 1, 8, 512, k2, cls, z, BF16, 16, None, 0, 0, 0)))
    return [(conv3, (7, 5, 3, 3, 3), c3), (conv4, (7, 5, 4, 4, 4), c4), (dec, (6, 64, 2, 2, 2), cd)]


PACKERS = ("w_fwd", "w_dgrad_s1", "w_fwd8", "w_dgrad8", "w_dgrad_s2", "w_deconv_fwd", "w_deconv_fwd_all", "w_deconv_dgrad",
           "w_fwd_s2d", "w_dgrad_s2d", "w_fwd_part", "w_dgrad_s1_part", "w_fwd_s2d_part", "w_dgrad_s2d_part")


def test_every_packer_hands_weight_pack_the_same_arguments(recorder):
    packs, amaxes = recorder
    seen = set()
    for spec, wshape, calls in _cases():
        w = torch.zeros(wshape)
        for name, args, want in calls:
            seen.add(name)
            fp8 = want[8] == ops.FP8
            del packs[:], amaxes[:]
            val = getattr(spec, name)(w, *args)
            assert len(packs) == 1, name
            got, src, reuse, q_amax = packs[0]
            assert got == want, (name, args)
            assert src.data_ptr() == w.data_ptr() and not src.requires_grad and reuse is None
            if fp8:                                   # the amax of the whole weight first, then the packing scaled with it
                assert len(amaxes) == 1 and amaxes[0][0].data_ptr() == w.data_ptr() and amaxes[0][1] is None
                assert len(val) == 4 and val[3] is q_amax and q_amax is not None
            else:
                assert not amaxes and q_amax is None and len(val) == 3
            # unchanged weight: served from the cache
            again = getattr(spec, name)(w, *args)
            assert len(packs) == 1 and len(amaxes) == int(fp8) and again[0] is val[0]
    assert seen == set(PACKERS)
    public = {n for n in vars(Fn.ConvSpec) if n.startswith("w_")}
    assert public == set(PACKERS)


def test_a_changed_weight_is_repacked_into_the_previous_buffer(recorder):
    packs, amaxes = recorder
    for spec, wshape, calls in _cases():
        w = torch.zeros(wshape)
        for name, args, want in calls:
            first = getattr(spec, name)(w, *args)
            del packs[:], amaxes[:]
            w.add_(1)
            getattr(spec, name)(w, *args)
            assert len(packs) == 1 and packs[0][0] == want and packs[0][2] is first[0], name
            if want[8] == ops.FP8:                   # the amax is rewritten in place as well (a captured graph points at it)
                assert len(amaxes) == 1 and amaxes[0][1] is first[3] and packs[0][3] is first[3]


# ------------------------------------------------------------------------------ hand-over tables
TABLES = {"Fp8Side": 32, "ColSumSide": 32, "LazyDx": 8, "LazyPool": 8, "PoolSide": 8, "FusedFinal": 8}


@pytest.fixture
def tables():
    """the six tables, empty before and after (tests that ran training steps in this process may have left entries)"""
    def empty():
        for name in TABLES:
            getattr(Fn, name).clear()
        Fn.PackMemo.clear()
        Fn.StepMemo.clear()
    empty()
    yield {name: getattr(Fn, name) for name in TABLES}
    empty()


def test_take_hands_the_payload_over_once(tables):
    for name in ("Fp8Side", "ColSumSide", "LazyDx", "LazyPool", "PoolSide"):
        table = tables[name]
        key, a, b = torch.zeros(2, 3), torch.ones(1), torch.ones(2)
        table.put(key, a, b)
        assert list(table._by_ptr) == [key.data_ptr()]
        got = table.take(key)
        assert isinstance(got, tuple) and len(got) == 2 and got[0] is a and got[1] is b
        assert table.take(key) is None and not table._by_ptr
        # the address alone is not enough: another shape under it is another tensor
        table.put(key, a)
        assert table.take(key.view(3, 2)) is None and not table._by_ptr
        # keep=True leaves the entry where it is
        table.put(key, a)
        assert table.take(key, keep=True)[0] is a and table.take(key, keep=True)[0] is a
        assert table.take(key)[0] is a and table.take(key, keep=True) is None
        assert table.enabled is True
        table.clear()


def test_an_entry_keeps_its_key_tensor_alive(tables):
    import weakref
    key = torch.zeros(4)
    ref = weakref.ref(key)
    tables["PoolSide"].put(key, torch.ones(1))
    del key
    assert ref() is not None
    tables["PoolSide"].clear()
    assert ref() is None


def test_a_full_table_is_emptied_before_the_next_entry(tables):
    for name, capacity in TABLES.items():
        table = tables[name]
        keys = [torch.zeros(1) for _ in range(capacity + 1)]
        w = torch.zeros(1)
        for i, k in enumerate(keys[:capacity]):
            table.put(k, w, w, w._version)
            assert len(table._by_ptr) == i + 1
        table.put(keys[capacity], w, w, w._version)
        assert list(table._by_ptr) == [keys[capacity].data_ptr()], name
        table.clear()


def test_begin_step_empties_every_table_and_both_memos(tables, monkeypatch):
    monkeypatch.setattr(Fn.DropoutState, "advance", classmethod(lambda cls, device: None))     # (device counters: no GPU here)
    monkeypatch.setattr(Fn.Fp8Scales, "advance", classmethod(lambda cls, device: None))
    keys = []
    for name in TABLES:
        keys.append(torch.zeros(3))
        tables[name].put(keys[-1], keys[-1], keys[-1], 0)
    x, act = torch.zeros(2), torch.zeros(5)
    Fn.PackMemo.put(x, 16, BF16, act)
    Fn.StepMemo.put((x, act), 7, act)
    assert Fn.PackMemo.get(x, 16, BF16) is act and Fn.StepMemo.get((x, act), 7) is act
    assert all(tables[name]._by_ptr for name in TABLES)
    Fn.begin_step(torch.device("cpu"))
    assert not any(tables[name]._by_ptr for name in TABLES)
    assert Fn.PackMemo.get(x, 16, BF16) is None and Fn.StepMemo.get((x, act), 7) is None
    assert not Fn.PackMemo._store and not Fn.StepMemo._store


def test_fused_final_serves_only_the_convolution_it_was_computed_for(tables):
    ff = tables["FusedFinal"]
    a, y, w = torch.zeros(2, 3), torch.ones(2, 1), torch.zeros(1, 3)
    assert ff.take(a, w) is None                              # nothing registered: the convolution launches itself
    ff.put(a, y, w, w._version)
    assert ff.take(a, w) is y and ff.take(a, w) is None
    ff.put(a, y, w, w._version)
    with pytest.raises(RuntimeError, match="not the one it was computed for"):
        ff.take(a, torch.zeros(1, 3))                         # a foreign weight
    assert not ff._by_ptr
    ff.put(a, y, w, w._version)
    w.add_(1)
    with pytest.raises(RuntimeError, match="not the one it was computed for"):
        ff.take(a, w)                                         # the same weight after an update
    ff.put(a, y, w, w._version)
    with pytest.raises(RuntimeError, match="not the one it was computed for"):
        ff.take(a.view(3, 2), w)                              # another tensor at the activation's address
