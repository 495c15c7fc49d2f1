"""Poisoned allocations for tests: for the duration of a ``with poisoned(kind):`` block every ``torch.empty``,
``torch.empty_like`` and ``Tensor.new_empty`` allocates through the real function and then FILLS the result, so a kernel that
reads a slot it never wrote sees the poison instead of the zeros (or the previous call's right answer) that the caching
allocator happens to hand out in a test process.  Two poisons, because either alone has blind spots (DESIGN.md,
"Allocations are never zero-filled"):

  kind      floating                         uint8                                       bool
  "nan"     NaN                              0xFF (NaN as e4m3 / f32 / f64; window 255)  True
  "big"     3e38 (f32, bf16) 1e300 (f64)     0x7E (448 as e4m3; ~8e37 as f32)            False
            6e4 (f16)

``fmaxf`` and ordered comparisons drop a NaN (amax, max-pool, ``take = v > m``); a finite poison times a zero weight is 0 where
NaN x 0 is NaN.  A result that is bit-identical without poison and under both has neither blind spot.

Any other integer dtype raises: the poisons are values, never indices.  Whoever adds an index tensor allocated with
``torch.empty`` has to decide on purpose what a stale read of it may address.

A plain module (no conftest, no plugin): the tests import it."""
from __future__ import annotations

import ast
import contextlib
import os
import sys
import threading

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "unet_bssfp_amd")
ALLOC_NAMES = ("empty", "empty_like", "new_empty")

KINDS = ("nan", "big")
BIG = {torch.float32: 3e38, torch.bfloat16: 3e38, torch.float64: 1e300, torch.float16: 6e4}
BYTE = {"nan": 0xFF, "big": 0x7E}
BOOL = {"nan": True, "big": False}

_active = threading.Lock()          # one poisoned block at a time (the patch is process-wide: every thread sees it)


class Stats:
    """what a poisoned block did: ``filled`` allocations with at least one element were overwritten"""

    def __init__(self):
        self.filled = 0
        self.calls = 0


def fill_value(kind: str, dtype: torch.dtype):
    """the poison of ``kind`` for ``dtype`` (complex: the value of both parts); raises for a dtype that has none"""
    if kind not in KINDS:
        raise ValueError(f"unknown poison kind {kind!r}")
    if dtype.is_floating_point or dtype.is_complex:
        base = {torch.complex64: torch.float32, torch.complex128: torch.float64, torch.complex32: torch.float16}.get(dtype, dtype)
        if base not in BIG:
            raise TypeError(f"alloc_poison: no poison defined for {dtype}")
        return float("nan") if kind == "nan" else BIG[base]
    if dtype == torch.uint8:
        return BYTE[kind]
    if dtype == torch.bool:
        return BOOL[kind]
    raise TypeError(f"alloc_poison: torch.empty of integer dtype {dtype}: a poison is a value, never an index -- "
                    "decide what a stale read of this tensor may address before allocating it uninitialised")


def _fill(t: torch.Tensor, kind: str, stats: Stats) -> torch.Tensor:
    v = fill_value(kind, t.dtype)               # (raises for index dtypes even when the tensor is empty)
    stats.calls += 1
    if t.numel() == 0:
        return t
    with torch.no_grad():
        if t.dtype.is_complex:
            torch.view_as_real(t).fill_(v)
        else:
            t.fill_(v)
    stats.filled += 1
    return t


def _package_site():
    """(file name, line) of the innermost calling frame that lies inside the package, or None"""
    f = sys._getframe(2)
    while f is not None:
        name = f.f_code.co_filename
        if os.path.dirname(os.path.abspath(name)) == PKG_DIR:
            return (os.path.basename(name), f.f_lineno)
        f = f.f_back
    return None


@contextlib.contextmanager
def poisoned(kind: str, log=None):
    """Replace torch.empty / torch.empty_like / Tensor.new_empty by filling wrappers until the block ends (restored in
    ``finally``; the patch is seen by every thread, autograd's backward workers included).  log: a set that receives the
    (file name, line) of every call that comes from inside ``unet_bssfp_amd/``.  Yields a ``Stats``."""
    if kind not in KINDS:
        raise ValueError(f"unknown poison kind {kind!r}")
    if not _active.acquire(blocking=False):
        raise RuntimeError("alloc_poison.poisoned: blocks do not nest")
    real_empty, real_like, real_new = torch.empty, torch.empty_like, torch.Tensor.new_empty
    stats = Stats()

    def note():
        if log is not None:
            site = _package_site()
            if site is not None:
                log.add(site)

    def empty(*a, **k):
        note()
        return _fill(real_empty(*a, **k), kind, stats)

    def empty_like(*a, **k):
        note()
        return _fill(real_like(*a, **k), kind, stats)

    def new_empty(self, *a, **k):
        note()
        return _fill(real_new(self, *a, **k), kind, stats)

    try:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
        yield stats
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = real_empty, real_like, real_new
        _active.release()


def static_sites():
    """[(file name, line)], one entry per ``.empty(`` / ``.empty_like(`` / ``.new_empty(`` call in ``unet_bssfp_amd/*.py`` (two
    calls on one line: two equal entries), from an ast walk at call time, so line numbers never go stale.  The line is the one a
    frame reports while inside the call: what the wrappers log."""
    sites = []
    for name in sorted(os.listdir(PKG_DIR)):
        if not name.endswith(".py"):
            continue
        with open(os.path.join(PKG_DIR, name)) as fh:
            tree = ast.parse(fh.read(), name)
        for node in ast.walk(tree):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in ALLOC_NAMES:
                sites.append((name, node.lineno))
    return sorted(sites)


class PoisonFinding(AssertionError):
    """a scenario's result depends on the contents of freshly allocated memory (``kinds``: the poisons that showed it)"""

    def __init__(self, message, kinds):
        super().__init__(message)
        self.kinds = kinds


def run_scenario(scenario, log=None, sync=None):
    """The runner.  ``scenario()`` builds its own inputs and modules from fixed seeds and returns a flat dict of tensors.  It
    runs three times -- unpoisoned, under "nan", under "big" -- and every returned tensor has to be finite and bit-identical
    (torch.equal over whole tensors) in all three; each poisoned run has to have filled at least one allocation.  No tolerance.
    Raises PoisonFinding naming the tensors and the poison kinds that differ; returns the unpoisoned result.
    sync: called after each run (torch.cuda.synchronize for device scenarios)."""
    def once(kind):
        if kind is None:
            out, stats = scenario(), None
        else:
            with poisoned(kind, log) as stats:
                out = scenario()
                if sync is not None:
                    sync()
        if sync is not None:
            sync()
        assert isinstance(out, dict) and out, "a scenario returns a non-empty dict of tensors"
        return {k: v.detach().clone() for k, v in out.items()}, stats

    base, _ = once(None)
    problems, kinds = [], set()
    for name, t in base.items():
        if t.is_floating_point() and not bool(torch.isfinite(t).all()):
            problems.append(f"{name}: not finite without poison")
    for kind in KINDS:
        got, stats = once(kind)
        assert stats.filled >= 1, f"the scenario allocated nothing under poison {kind!r}: it tests nothing"
        assert got.keys() == base.keys(), (sorted(got), sorted(base))
        for name, t in got.items():
            ref = base[name]
            if t.is_floating_point() and not bool(torch.isfinite(t).all()):
                bad = int((~torch.isfinite(t)).sum())
                problems.append(f"{name}: {bad} of {t.numel()} not finite under {kind!r}")
                kinds.add(kind)
            elif t.shape != ref.shape or t.dtype != ref.dtype or not torch.equal(t, ref):
                diff = int((t != ref).sum()) if t.shape == ref.shape else -1
                problems.append(f"{name}: {diff} of {t.numel()} elements differ under {kind!r}")
                kinds.add(kind)
    if problems:
        raise PoisonFinding("result depends on uninitialised memory:\n  " + "\n  ".join(problems), frozenset(kinds))
    return base
