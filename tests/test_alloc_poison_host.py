"""tests/alloc_poison.py itself, on the CPU: the wrappers fill and restore, every (kind, dtype) pair gives the stated bit
pattern, the runner flags exactly the defects it exists for (and each poison kind catches the one the other is blind to), and
the static scan still sees every allocation site of the package."""
import collections
import threading

import numpy as np
import pytest
import torch

from tests import alloc_poison as AP
from tests.alloc_poison import poisoned, run_scenario, static_sites

REAL = (torch.empty, torch.empty_like, torch.Tensor.new_empty)


def _restored():
    return (torch.empty, torch.empty_like, torch.Tensor.new_empty) == REAL


# ------------------------------------------------------------------------------------------------ fill and restore
def test_fills_all_three_entry_points_and_restores():
    with poisoned("nan") as stats:
        assert not _restored()
        a = torch.empty((3, 5))
        b = torch.empty_like(a, dtype=torch.float64)
        c = a.new_empty((2, 2))
        d = torch.empty(7, dtype=torch.uint8)
        e = torch.empty((0,))                        # nothing to fill: not counted
    assert _restored()
    assert all(bool(torch.isnan(t).all()) for t in (a, b, c))
    assert b.dtype == torch.float64 and c.shape == (2, 2) and c.dtype == a.dtype
    assert d.tolist() == [0xFF] * 7 and e.numel() == 0
    assert stats.filled == 4 and stats.calls == 5


def test_restores_after_an_exception_and_does_not_nest():
    with pytest.raises(ZeroDivisionError):
        with poisoned("big"):
            assert not _restored()
            1 / 0
    assert _restored()
    with pytest.raises(RuntimeError, match="do not nest"):
        with poisoned("nan"):
            with poisoned("big"):
                pass
    assert _restored()
    with pytest.raises(ValueError):
        with poisoned("zero"):
            pass
    assert _restored()
    with poisoned("nan"):                           # still usable after all of the above
        assert bool(torch.isnan(torch.empty(2)).all())
    assert _restored()


def test_other_threads_see_the_poison():
    """autograd runs backward on a worker thread: the patch has to be process-wide"""
    seen = {}

    def worker():
        seen["plain"] = torch.empty(4)

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            seen["thread"] = threading.current_thread()
            seen["bwd"] = torch.empty_like(g)
            return g

    with poisoned("big") as stats:
        t = threading.Thread(target=worker)
        t.start()
        t.join()
        x = torch.ones(3, requires_grad=True)
        Fn.apply(x).sum().backward()
    assert seen["plain"].tolist() == [pytest.approx(3e38)] * 4
    assert seen["bwd"].tolist() == [pytest.approx(3e38)] * 3
    assert stats.filled >= 2
    assert _restored()


def test_parameters_are_not_poisoned_into_the_graph():
    """nn.Parameter(torch.empty(..)) followed by an initialiser, the package's construction idiom, works under poison"""
    with poisoned("nan"):
        p = torch.nn.Parameter(torch.empty(4, 3))
        torch.nn.init.constant_(p, 0.5)
    assert p.requires_grad and p.grad_fn is None and bool((p == 0.5).all())


# ------------------------------------------------------------------------------------------------ every kind and dtype
def _bits(t):
    return t.contiguous().view(torch.uint8).numpy().tobytes()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.float64, torch.complex64])
def test_nan_fills_floating_with_nan(dtype):
    with poisoned("nan"):
        t = torch.empty((5, 3), dtype=dtype)
    t = torch.view_as_real(t) if dtype.is_complex else t
    assert bool(torch.isnan(t).all())


@pytest.mark.parametrize("dtype, value", [(torch.float32, 3e38), (torch.bfloat16, 3e38), (torch.float64, 1e300),
                                          (torch.float16, 6e4), (torch.complex64, 3e38)])
def test_big_fills_floating_with_a_huge_finite_value(dtype, value):
    with poisoned("big"):
        t = torch.empty((5, 3), dtype=dtype)
    t = torch.view_as_real(t) if dtype.is_complex else t
    want = torch.tensor(value, dtype=torch.float64).to(t.dtype)          # the dtype's rounding of the stated value
    assert bool(torch.isfinite(t).all()) and bool((t == want).all())
    assert not bool(torch.isfinite(want * want))                        # huge: its square leaves the dtype
    assert abs(float(want) - value) <= value * 2.0 ** -8


def test_byte_patterns_read_as_stated():
    with poisoned("nan"):
        n = torch.empty(16, dtype=torch.uint8)
    with poisoned("big"):
        b = torch.empty(16, dtype=torch.uint8)
    assert _bits(n) == b"\xff" * 16 and _bits(b) == b"\x7e" * 16
    # a byte workspace read as f32 / f64: NaN under "nan", huge and finite under "big"
    assert np.isnan(np.frombuffer(_bits(n), np.float32)).all() and np.isnan(np.frombuffer(_bits(n), np.float64)).all()
    f32, f64 = np.frombuffer(_bits(b), np.float32), np.frombuffer(_bits(b), np.float64)
    assert np.isfinite(f32).all() and (f32 > 1e37).all() and np.isfinite(f64).all() and (f64 > 1e300).all()
    # as e4m3 (1-4-3, bias 7, no infinities): 0xFF = S.1111.111 is NaN, 0x7E = 0.1111.110 is 2^8 * 1.75 = 448
    e, m = (0x7E >> 3) & 0xF, 0x7E & 0x7
    assert 2.0 ** (e - 7) * (1 + m / 8) == 448.0
    assert (0xFF & 0x7F) == 0x7F
    if hasattr(torch, "float8_e4m3fn"):
        assert bool(torch.isnan(n.view(torch.float8_e4m3fn).float()).all())
        assert bool((b.view(torch.float8_e4m3fn).float() == 448.0).all())
    # as a max-pool window position: matches none of 0..7
    assert 0xFF not in range(8)


def test_bool_patterns():
    with poisoned("nan"):
        assert torch.empty(9, dtype=torch.bool).tolist() == [True] * 9
    with poisoned("big"):
        assert torch.empty(9, dtype=torch.bool).tolist() == [False] * 9


@pytest.mark.parametrize("kind", AP.KINDS)
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.int16, torch.int8])
def test_index_dtypes_raise(kind, dtype):
    with poisoned(kind):
        with pytest.raises(TypeError, match="never an index"):
            torch.empty(4, dtype=dtype)
        with pytest.raises(TypeError, match="never an index"):
            torch.empty_like(torch.zeros(4), dtype=dtype)
        with pytest.raises(TypeError, match="never an index"):
            torch.zeros(4).new_empty((0,), dtype=dtype)          # even with no element
    assert _restored()


# ------------------------------------------------------------------------------------------------ negative controls
def _writes_every_second_element():
    buf = torch.empty(64)
    buf[::2] = torch.arange(32, dtype=torch.float32)
    return {"sum": buf.sum()}                       # reads the 32 slots nobody wrote


def _multiplies_unwritten_by_zero():
    buf = torch.empty(64)
    return {"prod": buf * torch.zeros(64)}         # finite garbage x 0 = 0; NaN x 0 = NaN


def _amax_over_half_written():
    buf = torch.empty(64)
    buf[:32] = torch.linspace(-1.0, 1.0, 32)
    # fmaxf semantics, as the device amax kernels have them: a NaN operand is dropped
    return {"amax": torch.from_numpy(np.fmax.reduce(buf.abs().numpy())[None].copy())}


def _sound():
    buf = torch.empty(64)
    buf[:] = torch.arange(64, dtype=torch.float32)
    return {"sum": buf.sum(), "buf": buf}


def _caught_by(scenario, monkeypatch):
    # Unpoisoned, the controls would read whatever malloc hands out -- often the poison a test above left in a freed block.
    # Device memory in a test process is fresh zeros (or an earlier right answer): give the unpoisoned run exactly that.  The
    # poisoned runs wrap this function like the real one and fill over its zeros.
    monkeypatch.setattr(torch, "empty", lambda *a, **k: torch.zeros(*a, **k))
    with pytest.raises(AP.PoisonFinding) as err:
        run_scenario(scenario)
    return err.value.kinds


def test_runner_passes_a_sound_scenario():
    out = run_scenario(_sound)
    assert float(out["sum"]) == 2016.0


def test_negative_control_unwritten_slots_summed_is_caught_by_both(monkeypatch):
    assert _caught_by(_writes_every_second_element, monkeypatch) == {"nan", "big"}


def test_negative_control_times_zero_is_caught_only_by_nan(monkeypatch):
    assert _caught_by(_multiplies_unwritten_by_zero, monkeypatch) == {"nan"}


def test_negative_control_amax_is_caught_only_by_big(monkeypatch):
    assert _caught_by(_amax_over_half_written, monkeypatch) == {"big"}


def test_runner_needs_at_least_one_poisoned_allocation():
    with pytest.raises(AssertionError, match="allocated nothing"):
        run_scenario(lambda: {"x": torch.zeros(3)})


# ------------------------------------------------------------------------------------------------ sites
ISSUE_FILES = ("ops.py", "functional.py", "augment.py", "nn.py", "eval.py", "metrics.py", "data.py", "inference.py", "ddp.py",
               "gan.py")


def test_static_scan_finds_every_site():
    sites = static_sites()
    assert len(sites) >= 99, len(sites)
    count = collections.Counter(f for f, _ in sites)
    for name in ISSUE_FILES:
        assert count[name] >= 1, (name, dict(count))
    for f, line in sites:
        assert isinstance(f, str) and f.endswith(".py") and isinstance(line, int) and line >= 1


def test_logged_site_is_the_innermost_package_frame_and_matches_the_static_scan():
    """host-callable package code that allocates: the logged pairs are members of static_sites()"""
    from unet_bssfp_amd import nn as N
    log = set()
    with poisoned("nan", log):
        conv = N.Conv3d(2, 3, 3, padding=1)
        torch.empty(3)                               # from the test, not the package: not logged
    assert log and log <= set(static_sites()), (log, static_sites()[:5])
    assert {f for f, _ in log} == {"nn.py"}
    assert bool(torch.isfinite(conv.weight).all())   # the initialiser wrote every element over the poison
