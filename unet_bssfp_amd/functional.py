"""Autograd operators of the path: each forward/backward is a sequence of C-ABI launches
(``ops``); torch.autograd only orders them and accumulates parameter gradients, so
``requires_grad_`` toggling (Lightning ``toggle_optimizer``, src/model.py:264,274), DDP hooks and
back-propagation through the discriminator into the generator (src/model.py:172,268) work as
with the reference's stock modules."""
from __future__ import annotations

import os
import weakref
from typing import NamedTuple, Optional

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops
from .gradsink import sink_grad, sink_of
from .ops import round_up

CLASSES8 = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]

_WEIGHT_EPOCH = 0


def bump_weight_epoch():
    """Called by optimisers that update parameters through raw pointers (no autograd version bump)."""
    global _WEIGHT_EPOCH
    _WEIGHT_EPOCH += 1


class LayerCache:
    """Packed-weight cache of one convolution (re-packed when the parameter changes)."""

    def __init__(self):
        self._store = {}          # key -> [tag, value, weight tensor, pack descriptor]

    @staticmethod
    def _tag(tensor):
        return (tensor._version, tensor.data_ptr(), tensor.device, _WEIGHT_EPOCH)

    def get(self, key, tensor: torch.Tensor, builder):
        """builder(reuse) -> (packed, coutp, cinp); `reuse` is the previous buffer (re-packed in place so
        that its address stays stable across steps -- a captured hipGraph keeps pointing at it)."""
        tag = self._tag(tensor)
        hit = self._store.get(key)
        if hit is not None and hit[0] == tag:
            return hit[1]
        val = builder(hit[1][0] if hit is not None else None)
        self._store[key] = [tag, val, tensor, ops.LAST_WPACK_DESC[0]]
        return val

    def stale(self):
        """Entries whose weights changed since they were packed (and whose buffers can be re-packed in place)."""
        return [e for e in self._store.values() if e[0] != self._tag(e[2]) and e[3] is not None and e[3].dst == e[1][0].data_ptr()
                and e[3].src - getattr(e[3], "_src_off", 0) == e[2].data_ptr()]

    def clear(self):
        self._store.clear()


def repack_weights(module: torch.nn.Module):
    """Re-pack, in a few batched launches, every packed-weight buffer of `module` that is out of date
    (call right after an optimiser step: the following forward/backward then finds all caches fresh)."""
    by_dtype = {}
    entries = []
    for m in module.modules():
        spec = getattr(m, "spec", None)
        if isinstance(spec, ConvSpec):
            for e in spec.cache.stale():
                by_dtype.setdefault(e[3].dtype, []).append(e[3])
                entries.append(e)
                if len(e[1]) > 3:                         # e4m3 packing: its per-tensor amax follows the new weights first
                    ops.amax_f32(e[2].detach(), out=e[1][3])
    for descs in by_dtype.values():
        ops.weight_pack_multi(descs)
    for e in entries:
        e[0] = LayerCache._tag(e[2])
    for m in module.modules():
        tables = getattr(m, "upcat_tables", None)
        if isinstance(tables, UpCatTables):
            tables.refresh()


_ZEROS = {}


def _cached_zeros(n: int, device) -> torch.Tensor:
    """Shared read-only zero vector (exact-zero bias gradients): no fill kernel per layer.  Sharing is safe
    because every contribution ever accumulated into it is itself zero."""
    key = (n, device)
    t = _ZEROS.get(key)
    if t is None:
        t = torch.zeros((n,), dtype=torch.float32, device=device)
        _ZEROS[key] = t
    return t


def _padded(vec: Optional[torch.Tensor], n: int, fill: float = 0.0) -> Optional[torch.Tensor]:
    if vec is None:
        return None
    v = vec.detach()
    if v.numel() == n:
        return v.contiguous()
    out = torch.full((n,), fill, dtype=torch.float32, device=v.device)
    out[: v.numel()] = v
    return out


# ====================================================================================== backward stages
def _new_s2d(shape, dtype, device):
    """A space-to-depth output tensor.  Not zero-filled: the pack / norm+act kernels write every (cell, block) slot, the
    out-of-volume blocks of the border cells included (elementwise_common.h: s2d_zero_siblings); tests/alloc_poison.py
    fills it, like every other allocation, with NaN and with a huge value to prove that."""
    return torch.empty(shape, dtype=dtype, device=device)


class StageBoundary:
    """Collects, during a forward pass, the activations at which the backward pass can be cut into two stages (late
    layers first, early layers second) so that the late stage's gradient bucket is exchanged while the early stage's
    backward kernels run (gan.GraphedTrainingStep).  Inactive unless ``begin()`` was called."""
    _active = None

    @classmethod
    def begin(cls):
        cls._active = []

    @classmethod
    def active(cls) -> bool:
        return cls._active is not None

    @classmethod
    def mark(cls, *tensors):
        if cls._active is not None:
            cls._active.extend(t for t in tensors if t is not None and t.requires_grad)

    @classmethod
    def end(cls):
        out, cls._active = cls._active or [], None
        return out


class SideStream:
    """Weight gradients of the SMALL layers (32^3 and below: kernels of 5 - 60 us that cannot fill 256 CUs) on a second HIP
    stream, beside the data-gradient chain they do not feed: a quarter of the step is kernels shorter than 25 us.  MEASURED
    SLOWER (see ``allowed``) and therefore off by default; kept as a switch because the test suite covers it.  (The same for the full-resolution layers was measured slower in round 1: two
    chip-filling kernels thrash each other's L2 and LDS.)  Opt-in per backward pass (``scope()``: the harness's
    ``manual_backward``), joined before the pass returns and before any gradient bucket is exchanged; works under hipGraph
    capture (fork / join become graph edges).  Tensors the side kernels read are kept alive until the join: the caching
    allocator would otherwise hand their memory to later kernels of the main stream."""
    enabled = False
    max_rows = 40000            # output positions (n d h w) up to which a layer's weight gradient goes to the side stream
    _stream = None
    _dirty = False
    _keep = []

    @classmethod
    def run(cls, fn, *keep):
        if cls._stream is None:
            cls._stream = torch.cuda.Stream()
        ev = torch.cuda.Event()
        ev.record()                                     # everything the side kernels read has been enqueued on the main stream
        cls._stream.wait_event(ev)
        with torch.cuda.stream(cls._stream):
            fn()
        cls._keep.extend(t for t in keep if t is not None)
        cls._dirty = True

    @classmethod
    def join(cls):
        if cls._dirty:
            ev = torch.cuda.Event()
            ev.record(cls._stream)
            torch.cuda.current_stream().wait_event(ev)
            cls._keep.clear()
            cls._dirty = False

    class scope:
        def __enter__(self):
            self.prev = SideStream.enabled
            SideStream.enabled = SideStream.allowed
            return self

        def __exit__(self, *exc):
            SideStream.join()
            SideStream.enabled = self.prev
            return False

    allowed = False             # OFF: measured 12.48 against 12.27 ms per step with it (interleaved A/B, round 3): the fork / join
                                # edges of ~70 small launches cost more than the overlap returns; bench.py --side-stream turns it on


class DeferredReduce:
    """Slab reductions of the weight-gradient launches, deferred and batched (round 4).  Every weight-gradient kernel writes f32
    partial sums (slabs) that a second launch sums into ``weight.grad`` -- ~30 launches of 7 - 23 us per step that nothing in
    the backward pass waits for: only the optimiser (and, under DDP, the bucket's all-reduce) reads a weight gradient.  Inside
    ``scope()`` (the harness's ``manual_backward``) the layers launch only their slab kernel (``mi355_conv_wgrad_partial``) and
    the reductions of up to ``max_jobs`` layers run as ONE launch (``mi355_wgrad_reduce_multi``): when that many are pending,
    when a layer contributes a second time in the pass, when the pending ones would complete an eagerly exchanged DDP bucket
    (its all-reduce has to be enqueued while backward kernels are still to come), and when the scope ends.  ``GradBuckets.written`` is called at
    the flush, so a bucket is exchanged only after its reductions have been enqueued.  Same kernels bodies and summation
    order per layer as the immediate form: bit-identical gradients (``test_deferred_weight_gradient_reduction_is_bit_identical``).
    Outside a scope (op-level use, ``loss.backward()`` on a bare network) nothing is deferred."""
    enabled = False
    allowed = True              # bench.py --immediate-reduce turns it off (A/B)
    max_jobs = 16               # one launch of mi355_wgrad_reduce_multi
    _jobs = []                  # (job, workspace) pairs: the workspace stays allocated until its reduction is enqueued
    _after = []                 # (sink, parameter): GradBuckets.written calls owed at the flush
    _params = set()
    launches = 0                # multi-launches so far (tests)

    @classmethod
    def wants(cls, sink, param, acc) -> bool:
        """True: this contribution may be deferred.  A second contribution to a parameter that still has a pending reduction
        flushes first (its ``fresh`` state is only advanced by ``written``) and runs immediately, accumulating."""
        if not cls.enabled or sink is None:
            return False
        if acc or id(param) in cls._params:
            cls.flush()
            return False
        return True

    @classmethod
    def add(cls, jobs, sink, param):
        cls._jobs.extend(jobs)
        cls._after.append((sink, param))
        cls._params.add(id(param))
        if len(cls._jobs) + 2 > cls.max_jobs or sink.completes_with(cls._after):    # (a layer adds at most two jobs)
            cls.flush()

    @classmethod
    def flush(cls):
        if not cls._jobs and not cls._after:
            return
        jobs, after = cls._jobs, cls._after
        cls._jobs, cls._after, cls._params = [], [], set()     # (written() may launch a bucket, whose launch flushes: re-entrant)
        ops.wgrad_reduce_multi(jobs)
        cls.launches += 1
        for sink, param in after:
            sink.written(param)

    class scope:
        def __enter__(self):
            self.prev = DeferredReduce.enabled
            DeferredReduce.enabled = DeferredReduce.allowed
            return self

        def __exit__(self, *exc):
            if exc[0] is None:
                DeferredReduce.flush()
            else:                                   # a failed backward pass: drop what is pending
                DeferredReduce._jobs, DeferredReduce._after, DeferredReduce._params = [], [], set()
            DeferredReduce.enabled = self.prev
            return False


# ====================================================================================== layout
class Fp8Scales:
    """Delayed per-tensor scaling of the e4m3 operands (BASELINE.json configs[4]).  An operand's scale 224 / amax has to be
    known when its PRODUCER writes it, if the producer is to write the e4m3 copy itself (no amax pass, no cast pass over the
    tensor): every (layer, operand role) owns a slot = (amax in use, amax being gathered) in one device table; kernels that
    write or cast an operand scale with the first and raise the second; ``advance`` (once per training step, on the device:
    part of a captured step) makes the gathered amax the one in use.  A slot's first step has no history: it takes the
    in-step amax pass (``primed`` is host state, it changes only between steps).  Values beyond twice the previous step's
    amax saturate at +-448 (e4m3 holds 448, the scale maps amax to 224)."""
    ROWS = 256
    _chunks = {}      # device -> [(table f32 [ROWS, 2], [slots], saturation record int32 [ROWS])]
    producer_side = True     # False: every operand takes the consumer-side cast (diagnostics / A-B)

    class Slot:
        __slots__ = ("use", "next", "primed", "touched", "sat")

        def __init__(self, row: torch.Tensor, sat: torch.Tensor):
            self.use, self.next = row[0:1], row[1:2]
            self.sat = sat                      # int32[1]: steps in which this operand saturated (a value clamped at +-448)
            self.primed = self.touched = False

    @classmethod
    def slot(cls, device) -> "Fp8Scales.Slot":
        chunks = cls._chunks.setdefault(device, [])
        if not chunks or len(chunks[-1][1]) == cls.ROWS:
            chunks.append((torch.zeros((cls.ROWS, 2), dtype=torch.float32, device=device), [],
                           torch.zeros((cls.ROWS,), dtype=torch.int32, device=device)))
        table, slots, sat = chunks[-1]
        s = cls.Slot(table[len(slots)], sat[len(slots): len(slots) + 1])
        slots.append(s)
        return s

    @classmethod
    def advance(cls, device):
        for table, slots, sat in cls._chunks.get(device, ()):
            if any(s.touched for s in slots):
                ops.fp8_scale_roll(table, len(slots), sat)
                for s in slots:
                    s.primed, s.touched = s.primed or s.touched, False

    @classmethod
    def primed_slots(cls, device) -> set:
        """slots with a history when the next step starts (primed, or touched by the step before: ``advance`` primes those)"""
        return {id(s) for _, slots, _ in cls._chunks.get(device, ()) for s in slots if s.primed or s.touched}

    @classmethod
    def check_capture(cls, device, primed_before: set):
        """``primed`` / ``touched`` are HOST flags that a hipGraph capture bakes into the captured launches (in-step amax pass or
        delayed scale; which slots ``advance`` rolls): a slot that was first used inside the capture -- created by it, or never
        primed by an eager step before it -- would replay its first-step form for ever.  GraphedTrainingStep runs at
        least two eager steps first; this is the check that they did prime everything the captured step touches."""
        bad = sum(1 for _, slots, _ in cls._chunks.get(device, ()) for s in slots if s.touched and id(s) not in primed_before)
        if bad:
            raise RuntimeError(f"fp8 delayed scaling: {bad} operand slot(s) were used for the first time inside a hipGraph capture; "
                               "run the step eagerly (at least twice) before capturing it")

    @classmethod
    def saturated_steps(cls, device=None) -> int:
        """Steps x slots in which an e4m3 operand saturated since the process started (values beyond twice the previous step's
        amax clamp at +-448 under delayed scaling): the overflow record VERDICT r3 asked for.  One host sync."""
        total = 0
        for dev, chunks in cls._chunks.items():
            if device is None or torch.device(dev) == torch.device(device):
                total += sum(int(sat[: len(slots)].sum()) for _, slots, sat in chunks)
        return total


class HandOver:
    """A table that hands tensors from the launch that wrote them to the autograd node that consumes them, keyed by the
    ADDRESS of the tensor they travel under (autograd hands tensors, not attributes, from one node to the next).  An entry
    keeps that tensor alive, so the address cannot come to mean another tensor while the entry exists.  Every table
    registers itself in ``per_step``: ``begin_step`` empties whatever is listed there."""
    per_step = []               # everything with a clear() that a new training step empties (the memos below join it)

    def __init__(self, doc: str, capacity: int = 8):
        self.__doc__, self.capacity = doc, capacity
        self.enabled = True     # read by the call sites only (bench.py's A/B switches)
        self._by_ptr = {}
        HandOver.per_step.append(self)

    def put(self, t: torch.Tensor, *payload):
        if len(self._by_ptr) >= self.capacity:     # (a loop that never starts a training step: nothing may pile up here)
            self._by_ptr.clear()
        self._by_ptr[t.data_ptr()] = (*payload, tuple(t.shape), t)

    def take(self, t: torch.Tensor, keep: bool = False) -> Optional[tuple]:
        """the payload registered under ``t`` (removed unless ``keep``), or None"""
        hit = self._by_ptr.get(t.data_ptr()) if keep else self._by_ptr.pop(t.data_ptr(), None)
        return hit[:-2] if hit is not None and hit[-2] == tuple(t.shape) else None

    def clear(self):
        self._by_ptr.clear()


class _CheckedHandOver(HandOver):
    """payload (y, weight, weight version): only the convolution it was computed for may take it"""

    def take(self, a: torch.Tensor, w: torch.Tensor):
        registered = a.data_ptr() in self._by_ptr
        hit = super().take(a)
        if registered and (hit is None or hit[1].data_ptr() != w.data_ptr() or hit[2] != w._version):
            # (the activation may not even have been written: never fall back to a launch that would read it)
            raise RuntimeError("FusedFinal: the convolution that takes the precomputed output is not the one it was computed for")
        return hit[0] if registered else None


Fp8Side = HandOver(
    """e4m3 copies on their way from the kernel that wrote them to the convolution that consumes them, keyed by the bf16
    tensor they mirror (autograd hands tensors, not attributes, from one node to the next).  An entry keeps its bf16 tensor
    alive, so the address cannot come to mean another tensor while the entry exists.  Emptied every step.""", capacity=32)

ColSumSide = HandOver(
    """Per-channel sums of a data gradient, emitted by the convolution launch that PRODUCED it (fused statistics epilogue),
    on their way to the node that needs them as a bias gradient (the transposed convolution under a skip concatenation:
    its bias gradient was a separate pass over the full-resolution gradient).  Keyed like Fp8Side; emptied every step.
    Payload: (partial sums, channel offset).""", capacity=32)

LazyDx = HandOver(
    """A data gradient that is never materialised: the 1x1x1 final convolution of the U-Net hands (dz, W) to the norm + act
    node that produced its input, whose backward kernels form da = dz @ W per row on the fly (ops.normact_bwd, implicit=)
    instead of reading a 134-MB tensor twice that a separate launch would have written.  The convolution's backward returns an
    UNINITIALISED placeholder of da's shape (allocation only) and registers the operands under it; only a node that was
    promised as the single consumer at forward time (ConvFn lazy_dx=True, set by BasicUNet) may receive it.""")

LazyPool = HandOver(
    """The gradient of an encoder level's output -- MaxPool3d(2)'s backward plus the skip connection's gradient -- never
    materialised (round 4): ``SkipPoolFn.backward`` returns an UNINITIALISED placeholder and registers (x, y, idx, d_pool,
    d_skip) under it; the norm + act node that produced the level's output forms da per row inside its two backward kernels
    (``ops.normact_bwd(pool=)``: the window positions recorded by the forward max-pool, one byte per pooled element).  That drops
    the max-pool backward launch (at 128^3 x 32: 134 MB + 134 MB read, 134 MB written) and the two reads of its result; the
    values are those the launch would have stored, bit for bit.  Only offered when the producer of the pooled tensor IS a
    NormActFn node (checked on the autograd graph at forward time) and the extents are even; a node that cannot use it (the
    small-tensor kernels, a space-to-depth output) materialises the gradient with the ordinary kernel.
    ``enabled``: bench.py --eager-pool-bwd turns it off (A/B).""")

PoolSide = HandOver(
    """MaxPool3d(2) of an activation that the norm + act launch producing it has already computed (ops.normact_fwd, pool=True):
    NormActFn.forward registers (y, idx) under the activation, SkipPoolFn.forward takes them instead of launching.
    ``enabled``: bench.py --separate-pool turns it off (A/B).""")

FusedFinal = _CheckedHandOver(
    """Output of a 1x1x1 convolution that the norm + act launch producing its input has already computed (ops.normact_fwd,
    final=): NormActFn.forward registers it under the activation, ConvFn.forward (lazy_dx=True: same single-consumer promise as
    LazyDx) takes it instead of launching.  The convolution stays an autograd node: its weight / bias gradients and the LazyDx
    hand-over are unchanged.""")


def fp8_operand(x: torch.Tensor, slot: "Fp8Scales.Slot", constant: bool = False) -> torch.Tensor:
    """The e4m3 copy of a convolution operand with the amax in ``slot.use``: the one its producer wrote if there is one;
    otherwise one cast pass with the previous step's amax (gathering this step's); on the slot's first step the in-step
    amax pass + cast.  constant: an input that enters several convolution calls of one step (the packed batch) is cast once."""
    hit = Fp8Side.take(x, keep=constant)
    if hit is not None:
        return hit[0]
    if slot.primed:
        x8 = ops.cast_fp8(x, slot.use, slot.next)
    else:
        ops.amax_act(x, out=slot.use)
        torch.maximum(slot.next, slot.use, out=slot.next)
        x8 = ops.cast_fp8(x, slot.use)
    slot.touched = True
    if constant:
        Fp8Side.put(x, x8)
    return x8


class PackMemo:
    """Packed form of constant NCDHW inputs, valid within ONE training step (``begin_step`` clears it at the start of every
    step, so a benchmark that feeds the same batch again still packs it each step).  An entry is tied to the tensor
    OBJECT (weak reference) and its version counter, never to an address."""
    _store = {}

    @classmethod
    def get(cls, x, cp, dtype):
        e = cls._store.get((id(x), cp, dtype))
        if e is not None and e[0]() is x and e[1] == x._version:
            return e[2]
        return None

    @classmethod
    def put(cls, x, cp, dtype, act):
        if len(cls._store) >= 8:
            cls._store.clear()
        cls._store[(id(x), cp, dtype)] = (weakref.ref(x), x._version, act)

    @classmethod
    def holds(cls, act) -> bool:
        """is ``act`` the packed form of a constant input of this step?"""
        return any(e[2].data_ptr() == act.data_ptr() for e in cls._store.values())

    @classmethod
    def clear(cls):
        cls._store.clear()


HandOver.per_step.append(PackMemo)


class PackFn(Function):
    """NCDHW f32 tensors -> one NDHWC activation (virtual torch.cat along channels + layout)."""

    @staticmethod
    def forward(ctx, cp, dtype, *srcs):
        s2d = cp < 0                     # cp < 0: write the space-to-depth tensor S(.) with |cp| channels per block
        cp = abs(cp)
        ctx.s2d = s2d
        n, _, d, h, w = srcs[0].shape
        ctx.dims = (d, h, w)
        epv = 4 if dtype == torch.float32 else 8
        ctx.split = None
        if len(srcs) > 1 and any(s.shape[1] % epv for s in srcs[:-1]):
            # channel boundaries that are not 16-byte aligned: concatenate first (boundary plumbing)
            ctx.split = [s.shape[1] for s in srcs]
            srcs = (torch.cat([s.detach().to(torch.float32) for s in srcs], dim=1),)
        if s2d:
            out = _new_s2d(ops.s2d_shape(n, d, h, w, cp), dtype, srcs[0].device)
        else:
            out = ops.new_act(n, d, h, w, cp, dtype, srcs[0].device)
        offs, off = [], 0
        if len(srcs) == 2:
            # torch.cat([x, y], 1) of the discriminator: both sources in one pass that writes whole rows
            s0, s1 = (t.detach().to(torch.float32).contiguous() for t in srcs)
            ops.pack2(s0, s1, out, 0, cp, s2d_cblk=cp if s2d else 0)
            ctx.offs = [(0, s0.shape[1]), (s0.shape[1], s1.shape[1])]
            return out
        for i, s in enumerate(srcs):
            c = s.shape[1]
            last = i == len(srcs) - 1
            s32 = s.detach().to(torch.float32).contiguous()
            if s2d:
                ops.pack_ncdhw_s2d(s32, out, cp, off, cp if last else off + c)
            else:
                ops.pack_ncdhw(s32, out, off, cp if last else off + c)
            offs.append((off, c))
            off += c
        ctx.offs = offs
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = ops.as_act(g)
        need = ctx.needs_input_grad[2:]
        if ctx.s2d:
            def unpack(c, off, cp=g.shape[4] // 8):
                return ops.unpack_ncdhw_s2d(g, c, ctx.dims, cp, off)
        else:
            def unpack(c, off):
                return ops.unpack_ncdhw(g, c, off)
        if ctx.split is not None:
            pieces = torch.split(unpack(sum(ctx.split), 0), ctx.split, dim=1)
            return (None, None, *[pc.contiguous() if need[i] else None for i, pc in enumerate(pieces)])
        return (None, None, *[unpack(c, off) if need[i] else None for i, (off, c) in enumerate(ctx.offs)])


class UnpackFn(Function):
    """NDHWC activation -> contiguous NCDHW f32 (the tensor handed back to the caller)."""

    @staticmethod
    def forward(ctx, act, c):
        ctx.meta = (act.shape[4], act.dtype)
        return ops.unpack_ncdhw(act, c, 0)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        cp, dtype = ctx.meta
        n, c, d, h, w = g.shape
        out = ops.new_act(n, d, h, w, cp, dtype, g.device)
        ops.pack_ncdhw(g.to(torch.float32).contiguous(), out, 0, cp)
        return out, None


class GenOutFn(Function):
    """The generator's NDHWC output -> (contiguous NCDHW f32 tensor handed to the caller, S(output) for the PatchGAN's first block:
    Discriminator reads ``y._mi355_s2d`` instead of packing the f32 tensor again).  Backward: ONE pass joins the loss head's NCDHW
    gradient and the PatchGAN's space-to-depth gradient into the NDHWC gradient of the final convolution (src/model.py:172, 268) --
    before: unpack S -> NCDHW f32, an add over the f32 tensors, pack NCDHW -> NDHWC."""

    @staticmethod
    def forward(ctx, act, c, cblk):
        act = ops.as_act(act)
        ctx.meta = (tuple(act.shape), act.dtype, c)
        ctx.set_materialize_grads(False)
        return ops.unpack_ncdhw(act, c, 0), ops.s2d_repack(act, cblk)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gs):
        shape, dtype, c = ctx.meta
        if gy is None and gs is None:
            return None, None, None
        out = torch.empty(shape, dtype=dtype, device=(gy if gy is not None else gs).device)
        ops.seam_grad(gy.to(torch.float32).contiguous() if gy is not None else None, ops.as_act(gs) if gs is not None else None, out, c, shape[1:4])
        return out, None, None


# ====================================================================================== conv
class ConvSpec:
    """Static description of one convolution layer (+ its packed-weight cache)."""

    def __init__(self, kind, cin, cout, ks, stride, pad):
        assert kind in ("conv", "deconv2")
        self.kind, self.cin, self.cout, self.ks, self.stride, self.pad = kind, cin, cout, ks, stride, pad
        self.cache = LayerCache()
        self._amax = {}             # cache key of an e4m3 packing -> its per-tensor max |w| (device f32[1], rewritten in place)
        self._fp8_slots = {}        # (role, device) -> Fp8Scales.Slot

    def fp8_slot(self, role: str, device) -> "Fp8Scales.Slot":
        """delayed-scaling state of this layer's e4m3 operand: role 'x' (forward input) or 'g' (incoming gradient)"""
        key = (role, device)
        if key not in self._fp8_slots:
            self._fp8_slots[key] = Fp8Scales.slot(device)
        return self._fp8_slots[key]

    # ---- packed weights --------------------------------------------------------------
    def _pack(self, key, w, geo, dtype, cinp, c_off=0, **opts):
        """One packing of ``w`` through the cache.  geo: ops.weight_pack's (cout, cin, ks, s_co, s_ci, s_k, tbase, tstep); c_off:
        first input channel of a channel slice (k^3 source elements each); opts: coutp, s2d_mode, s2d_cp.  dtype ops.FP8 (per-tensor
        scale 224 / max |w|): the amax pass runs first and the value is (packed, coutp, cinp, amax)."""
        def build(reuse):
            kw = dict(opts, reuse=reuse, src_offset=c_off * self.ks ** 3)
            if dtype != ops.FP8:
                return ops.weight_pack(w.detach(), *geo, dtype, cinp, **kw)
            amax = self._amax[key] = ops.amax_f32(w.detach(), out=self._amax.get(key))
            return (*ops.weight_pack(w.detach(), *geo, dtype, cinp, q_amax=amax, **kw), amax)
        return self.cache.get(key, w, build)

    def w_fwd(self, w, dtype, cinp):
        return self.w_fwd_part(w, dtype, cinp, 0, self.cin)

    def w_dgrad_s1(self, w, dtype, cinp):
        return self.w_dgrad_s1_part(w, dtype, cinp, 0, self.cin)

    def w_fwd8(self, w, cinp):
        return self.w_fwd(w, ops.FP8, cinp)

    def w_dgrad8(self, w, cinp):
        return self.w_dgrad_s1(w, ops.FP8, cinp)

    # channel slice [c_off, c_off + c_n) of a stride-1 weight: forward and data-gradient packings (UpCatConvFn's skip part)
    def w_fwd_part(self, w, dtype, cinp, c_off, c_n):
        k = self.ks
        return self._pack(("fwd", dtype, cinp, c_off, c_n), w,
                          (self.cout, c_n, k, self.cin * k ** 3, k ** 3, (k * k, k, 1), (0, 0, 0), (1, 1, 1)), dtype, cinp, c_off)

    def w_dgrad_s1_part(self, w, dtype, cinp, c_off, c_n):
        k = self.ks
        return self._pack(("dgrad", dtype, cinp, c_off, c_n), w,
                          (c_n, self.cout, k, k ** 3, self.cin * k ** 3, (k * k, k, 1), (k - 1,) * 3, (-1,) * 3), dtype, cinp, c_off)

    def w_dgrad_s2(self, w, dtype, cinp, cls):
        # k4 s2 p1 transposed: parity class p per dim uses taps {3,1} (p=0) or {2,0} (p=1)
        k = self.ks
        tb = tuple(3 if p == 0 else 2 for p in cls)
        return self._pack(("dgrad2", dtype, cinp, cls), w,
                          (self.cin, self.cout, 2, k ** 3, self.cin * k ** 3, (k * k, k, 1), tb, (-2,) * 3), dtype, cinp)

    def w_deconv_fwd(self, w, dtype, cinp, cls):
        # ConvTranspose3d weight (Cin, Cout, 2,2,2): class = output parity = tap
        return self._pack(("dfwd", dtype, cinp, cls), w, (self.cout, self.cin, 1, 8, self.cout * 8, (4, 2, 1), cls, (0, 0, 0)),
                          dtype, cinp)

    def w_deconv_fwd_all(self, w, dtype, cinp):
        # all 8 parity classes as ONE GEMM: column blk*Cout + co  <-  w[ci][co][(bd,bh,bw)]
        return self._pack(("dfwd_all", dtype, cinp), w, (self.cout, self.cin, 1, 8, self.cout * 8, (4, 2, 1), (0, 0, 0), (0, 0, 0)),
                          dtype, cinp, coutp=8 * self.cout, s2d_mode=2, s2d_cp=self.cout)

    def w_deconv_dgrad(self, w, dtype, cinp):
        return self._pack(("ddgrad", dtype, cinp), w, (self.cin, self.cout, 2, self.cout * 8, 8, (4, 2, 1), (0, 0, 0), (1, 1, 1)),
                          dtype, cinp)

    # k4 s2 p1 on a space-to-depth input (dense k2 s1): W'[j][co][blk*cp + c] = w[co][c][2j + b]
    def w_fwd_s2d(self, w, dtype, cp):
        return self.w_fwd_s2d_part(w, dtype, cp, 0, self.cin)

    def w_dgrad_s2d(self, w, dtype, cinp, cp):
        # dS[i][blk*cp + c] = sum_{j'} dz[i + j' - 1][co] * w[co][c][2(1-j') + b]
        return self.w_dgrad_s2d_part(w, dtype, cinp, cp, 0, self.cin)

    # channel slice [c_off, c_off + c_n) of the k4 s2 p1 weight in the space-to-depth packings (the PatchGAN's first block
    # split into the parts of cat([x, y], 1): SplitS2dConvFn)
    def w_fwd_s2d_part(self, w, dtype, cp, c_off, c_n):
        k = self.ks
        return self._pack(("fwd_s2d", dtype, cp, c_off, c_n), w,
                          (self.cout, c_n, 2, self.cin * k ** 3, k ** 3, (k * k, k, 1), (0, 0, 0), (2, 2, 2)), dtype, 8 * cp, c_off,
                          s2d_mode=1, s2d_cp=cp)

    def w_dgrad_s2d_part(self, w, dtype, cinp, cp, c_off, c_n):
        k = self.ks
        return self._pack(("dgrad_s2d", dtype, cinp, cp, c_off, c_n), w,
                          (c_n, self.cout, 2, k ** 3, self.cin * k ** 3, (k * k, k, 1), (2, 2, 2), (-2, -2, -2)), dtype, cinp, c_off,
                          coutp=8 * cp, s2d_mode=2, s2d_cp=cp)

    def out_extent(self, e):
        if self.kind == "deconv2":
            return 2 * e
        return (e + 2 * self.pad - self.ks) // self.stride + 1


def _conv_fwd_stats(want, x0, x1, wp, coutp, bias, ks, stride, pad, out, grid, real, cols=None, delta=None, **kw):
    """ops.conv_fwd with, if wanted, the fused per-tile channel statistics: the buffer ([tiles][2][cols], cols = coutp unless
    given) is sized by ops.conv_num_tiles for exactly this launch (kw: what both take -- fp8, addend, d2s).  Returns it, or None."""
    part = None
    if want:
        tiles, _ = ops.conv_num_tiles(x0, x1, wp, coutp, ks, stride, pad, out, grid, **kw)
        part = torch.empty((tiles, 2, cols or coutp), dtype=torch.float32, device=out.device)
    ops.conv_fwd(x0, x1, wp, coutp, bias, ks, stride, pad, out, grid, stats=part, real=real, delta=delta, **kw)
    return part


def _out_and_stats(ctx, out, part):
    """what the convolution nodes return: (out, statistics); without statistics an empty tensor stands in for them"""
    if part is None:
        part = torch.empty((0,), dtype=torch.float32, device=out.device)
    ctx.mark_non_differentiable(part)
    ctx.set_materialize_grads(False)      # no zero tensor (+ fill launch) for the statistics output in every backward
    return out, part


def _grad_target(p, deferrable=False):
    """Where a parameter gradient goes: (sink, tensor the kernels write, accumulate?, deferred jobs).  With gradient storage owned
    by the path (gradsink.GradBuckets) the kernels write -- or, for a second use of the parameter in this backward pass,
    accumulate -- straight into ``p.grad`` and autograd gets None; otherwise a fresh tensor goes back to autograd.  deferrable:
    the slab reductions of this contribution may be left to DeferredReduce (jobs is then a list for ops.conv_wgrad(defer=))."""
    sink = sink_of(p)
    if sink is None:
        return None, torch.empty_like(p, dtype=torch.float32), False, None
    jobs = [] if (deferrable and DeferredReduce.wants(sink, p, not sink.fresh(p))) else None
    return sink, sink_grad(p), not sink.fresh(p), jobs      # (fresh: read AFTER wants(), which may have flushed p's first contribution)


def _grad_done(sink, p, grad, jobs=None):
    """The launches that write ``grad`` (see _grad_target) are enqueued: owe or tell the sink; returns what autograd gets."""
    if jobs:
        DeferredReduce.add(jobs, sink, p)
    elif sink is not None:
        sink.written(p)
    else:
        return grad
    return None


def _bias_colsum_grad(bias, dz, cout):
    """A convolution's bias gradient, the per-channel sum of ``dz``: written (second use: added) into the parameter's gradient
    storage, or -- no sink -- a fresh vector of the ``cout`` real channels.  Returns what autograd gets."""
    if sink_of(bias) is None:
        return ops.colsum(dz)[:cout].contiguous()
    sink, db, acc, _ = _grad_target(bias)
    ops.colsum_into(dz, db, accumulate=acc)
    return _grad_done(sink, bias, db)


class ConvFn(Function):
    """z = conv(x0 | x1) + bias  (optionally with fused per-tile channel statistics)."""
    wgrad_first = False         # backward: weight gradient before the data gradient (bench.py --wgrad-first).  Measured: 10.018 against
                                # 10.007 ms per step in the default order (three interleaved rounds) -- no gain, off

    @staticmethod
    def forward(ctx, x0, x1, weight, bias, spec: ConvSpec, want_stats: bool, zero_bias_grad: bool = False,
                s2d_cp: int = 0, fp8: bool = False, lazy_dx: bool = False):
        # lazy_dx: the caller guarantees that x0 is the output of a (non-small, plain-layout) NormActFn node and has no other
        # consumer: a 1x1x1 convolution then leaves its data gradient to that node's backward kernels (LazyDx)
        x0 = ops.as_act(x0)
        x1 = ops.as_act(x1) if x1 is not None else None
        n, di, hi, wi, c0 = x0.shape
        c1 = x1.shape[4] if x1 is not None else 0
        dtype, dev = x0.dtype, x0.device
        cp = round_up(spec.cout, 16)
        ctx.s2d_cp = s2d_cp
        if s2d_cp:
            # x0 is S(a): the k4 s2 p1 convolution of a == dense k2 s1 p0 convolution of S(a)
            assert spec.kind == "conv" and spec.ks == 4 and spec.stride == 2 and spec.pad == 1 and x1 is None
            assert c0 == 8 * s2d_cp
            do_, ho, wo = di - 1, hi - 1, wi - 1
        else:
            do_, ho, wo = (spec.out_extent(e) for e in (di, hi, wi))
        out = ops.new_act(n, do_, ho, wo, cp, dtype, dev)
        part = None
        bp = bias.detach() if bias is not None else None
        if s2d_cp:
            wp, coutp, _ = spec.w_fwd_s2d(weight, dtype, s2d_cp)
            part = _conv_fwd_stats(want_stats, x0, None, wp, coutp, bp, 2, 1, (0, 0, 0), out, (do_, ho, wo), (spec.cin, spec.cout))
        elif (fp8 and spec.kind == "conv" and spec.ks == 3 and spec.stride == 1 and spec.pad == 1 and x1 is None
              and dtype == torch.bfloat16 and ops.conv_fp8_supported(x0, round_up(spec.cout, 32), out, (do_, ho, wo))):
            # BASELINE.json configs[4]: e4m3 operands (per-tensor scales) on the block-scaled MFMA, f32 accumulate, bf16 out
            wp, coutp, _, amax_w = spec.w_fwd8(weight, c0)
            slot = spec.fp8_slot("x", dev)
            # (the packed batch enters both generator passes of a training step: cast once; never memoised outside training)
            x8 = fp8_operand(x0, slot, constant=torch.is_grad_enabled() and not x0.requires_grad and PackMemo.holds(x0))
            part = _conv_fwd_stats(want_stats, x8, None, wp, coutp, bp, 3, 1, (1, 1, 1), out, (do_, ho, wo), (spec.cin, spec.cout),
                                   fp8=(slot.use, amax_w))
        elif lazy_dx and spec.kind == "conv" and spec.ks == 1 and (pre := FusedFinal.take(x0, weight)) is not None:
            out = pre                          # computed by the launch that produced x0 (ops.normact_fwd, final=)
        elif spec.kind == "conv":
            wp, coutp, _ = spec.w_fwd(weight, dtype, c0 + c1)
            part = _conv_fwd_stats(want_stats, x0, x1, wp, coutp, bp, spec.ks, spec.stride, (spec.pad,) * 3, out, (do_, ho, wo),
                                   (spec.cin, spec.cout))
        else:
            assert x1 is None and not want_stats
            if spec.cout % 64 == 0:
                # the 8 parity classes folded into the column index of one 1x1x1 GEMM (8*Cout columns)
                wp, coutp, _ = spec.w_deconv_fwd_all(weight, dtype, c0)
                ops.conv_fwd(x0, None, wp, coutp, bp, 1, 1, (0, 0, 0), out, (di, hi, wi), os=2,
                             real=(spec.cin, 8 * spec.cout), cls_cout=spec.cout)
            else:
                for cls in CLASSES8:
                    wp, coutp, _ = spec.w_deconv_fwd(weight, dtype, c0, cls)
                    ops.conv_fwd(x0, None, wp, coutp, bp, 1, 1, (0, 0, 0), out, (di, hi, wi), os=2, ooff=cls,
                                 real=(spec.cin, spec.cout))
        ctx.save_for_backward(x0, x1, weight)
        ctx.spec = spec
        ctx.fp8 = fp8
        ctx.lazy_dx = bool(lazy_dx and LazyDx.enabled and spec.kind == "conv" and spec.ks == 1 and spec.stride == 1 and x1 is None
                           and not s2d_cp and dtype == torch.bfloat16 and spec.cout <= 8 and spec.cin <= c0)
        ctx.has_bias = bias is not None
        ctx.bias_param, ctx.weight_param = bias, weight    # (their .grad may live in a GradBuckets buffer: gradsink.py)
        # a normalisation with batch/instance statistics follows: the mean subtraction cancels the bias,
        # so its gradient is identically zero and is returned as exact zeros (no reduction pass)
        ctx.zero_bias_grad = zero_bias_grad
        return _out_and_stats(ctx, out, part)

    @staticmethod
    @once_differentiable
    def backward(ctx, dz, _dpart):
        if dz is None:                        # the conv output did not reach the loss
            return (None,) * 10
        x0, x1, weight = ctx.saved_tensors
        spec: ConvSpec = ctx.spec
        dz = ops.as_act(dz)
        carried = ColSumSide.take(dz)           # per-channel sums of dz from the launch that produced it (bias gradient)
        n, di, hi, wi, c0 = x0.shape
        c1 = x1.shape[4] if x1 is not None else 0
        dtype, dev = x0.dtype, x0.device
        do_, ho, wo = dz.shape[1:4]
        cg = dz.shape[4]
        k = spec.ks
        dx0 = dx1 = dw = db = None
        need_dx = ctx.needs_input_grad[0] or (x1 is not None and ctx.needs_input_grad[1])
        if need_dx and ctx.lazy_dx:
            dx0 = ops.new_act(n, di, hi, wi, c0, dtype, dev)       # placeholder: never written, never read (LazyDx)
            LazyDx.put(dx0, dz, ctx.weight_param.detach())
        def dgrad(weight=weight):
            dxc = ops.new_act(n, di, hi, wi, c0 + c1, dtype, dev)
            # the second source of a skip concatenation comes from a transposed convolution whose bias gradient is the
            # per-channel sum of this data gradient: let the launch that writes it emit the sums (fused statistics)
            sums = None
            want_sums = (ColSumSide.enabled and x1 is not None and ctx.needs_input_grad[1] and spec.kind == "conv"
                         and spec.stride == 1 and not ctx.s2d_cp)
            if ctx.s2d_cp:
                wp, coutp, _ = spec.w_dgrad_s2d(weight, dtype, cg, ctx.s2d_cp)
                ops.conv_fwd(dz, None, wp, coutp, None, 2, 1, (1, 1, 1), dxc, (di, hi, wi), real=(spec.cout, spec.cin))
            elif (ctx.fp8 and spec.kind == "conv" and k == 3 and spec.stride == 1 and spec.pad == 1 and dtype == torch.bfloat16
                  and ops.conv_fp8_supported(dz, round_up(c0 + c1, 32), dxc, (di, hi, wi))):
                wp, coutp, _, amax_w = spec.w_dgrad8(weight, cg)
                slot = spec.fp8_slot("g", dev)
                sums = _conv_fwd_stats(want_sums, fp8_operand(dz, slot), None, wp, coutp, None, 3, 1, (1, 1, 1), dxc, (di, hi, wi),
                                       (spec.cout, spec.cin), fp8=(slot.use, amax_w))
            elif spec.kind == "conv" and spec.stride == 1:
                wp, coutp, _ = spec.w_dgrad_s1(weight, dtype, cg)
                sums = _conv_fwd_stats(want_sums, dz, None, wp, coutp, None, k, 1, (k - 1 - spec.pad,) * 3, dxc, (di, hi, wi),
                                       (spec.cout, spec.cin))
            elif spec.kind == "conv":
                if not (k == 4 and spec.stride == 2 and spec.pad == 1 and di % 2 == 0 and hi % 2 == 0 and wi % 2 == 0):
                    raise NotImplementedError("strided data gradient is implemented for k4 s2 p1 on even extents")
                for cls in CLASSES8:
                    wp, coutp, _ = spec.w_dgrad_s2(weight, dtype, cg, cls)
                    pad3 = tuple(1 if p == 0 else 0 for p in cls)
                    ops.conv_fwd(dz, None, wp, coutp, None, 2, 1, pad3, dxc, (di // 2, hi // 2, wi // 2), os=2, ooff=cls,
                                 real=(spec.cout, spec.cin))
            else:
                wp, coutp, _ = spec.w_deconv_dgrad(weight, dtype, cg)
                ops.conv_fwd(dz, None, wp, coutp, None, 2, 2, (0, 0, 0), dxc, (di, hi, wi), real=(spec.cout, spec.cin))
            dx0 = dxc[..., :c0] if c1 else dxc
            dx1 = dxc[..., c0:] if c1 else None
            if sums is not None:
                ColSumSide.put(dx1, sums, c0)
            return dx0, dx1

        run_dgrad = need_dx and not ctx.lazy_dx
        # (ConvFn.wgrad_first: both readers of dz -- it was just written by the norm backward -- back to back; measured, no gain)
        if run_dgrad and not ConvFn.wgrad_first:
            dx0, dx1 = dgrad()
            run_dgrad = False
        side = SideStream.enabled and n * do_ * ho * wo <= SideStream.max_rows
        if ctx.needs_input_grad[2]:
            weight = ctx.weight_param
            wsink, dwt, acc, defer = _grad_target(weight, deferrable=not side)

            def wgrad():
                if ctx.s2d_cp:
                    ops.conv_wgrad(x0, None, dz, (do_, ho, wo), 1, (0, 0, 0), 2, 1, (0, 0, 0), dwt, spec.cout, spec.cin,
                                   spec.cin * k ** 3, k ** 3, (k * k, k, 1), (0, 0, 0), (2, 2, 2), s2d_cp=ctx.s2d_cp, accumulate=acc,
                                   defer=defer)
                elif spec.kind == "conv":
                    ops.conv_wgrad(x0, x1, dz, (do_, ho, wo), 1, (0, 0, 0), k, spec.stride, (spec.pad,) * 3, dwt,
                                   spec.cout, spec.cin, spec.cin * k ** 3, k ** 3, (k * k, k, 1), (0, 0, 0), (1, 1, 1), accumulate=acc,
                                   defer=defer)
                elif dtype == torch.bfloat16 and spec.cout % 32 == 0 and cg == spec.cout:
                    # transposed conv: the 8 classes are 8*Cout GEMM columns of one k=1 weight-gradient launch
                    ops.conv_wgrad(x0, None, dz, (di, hi, wi), 1, (0, 0, 0), 1, 1, (0, 0, 0), dwt,
                                   spec.cout, spec.cin, 8, spec.cout * 8, (4, 2, 1), (0, 0, 0), (0, 0, 0),
                                   g_cls_cout=spec.cout, accumulate=acc, defer=defer)
                else:
                    assert defer is None or not defer
                    for cls in CLASSES8:                   # (eight launches into one workspace each: never deferred)
                        ops.conv_wgrad(x0, None, dz, (di, hi, wi), 2, cls, 1, 1, (0, 0, 0), dwt,
                                       spec.cout, spec.cin, 8, spec.cout * 8, (4, 2, 1), cls, (0, 0, 0), accumulate=acc)

            if side and wsink is not None:
                SideStream.run(wgrad, x0, x1, dz)
            else:
                wgrad()
            dw = _grad_done(wsink, weight, dwt, defer)
        if ctx.has_bias and ctx.needs_input_grad[3]:
            bias = ctx.bias_param
            bsink = sink_of(bias)
            if ctx.zero_bias_grad:                  # (with a sink: its slice of the bucket is zero and nobody ever writes it)
                db = _grad_done(bsink, bias, _cached_zeros(spec.cout, dev) if bsink is None else None)
            elif carried is not None or (side and bsink is not None):
                bsink, dbt, bacc, _ = _grad_target(bias)
                if carried is not None:
                    ops.colsum_from_parts(carried[0], carried[1], dbt, accumulate=bacc)
                else:
                    SideStream.run(lambda: ops.colsum_into(dz, dbt, accumulate=bacc), dz)
                db = _grad_done(bsink, bias, dbt)
            else:
                db = _bias_colsum_grad(bias, dz, spec.cout)
        if run_dgrad:
            dx0, dx1 = dgrad()
        return dx0, dx1, dw, db, None, None, None, None, None, None


class StepMemo:
    """Tensors computed once per training step and reused inside it, keyed by the objects they were computed from; emptied
    at the start of every step like PackMemo (``begin_step``).  Holds the x-part of the PatchGAN's first block
    (SplitS2dConvFn): the same batch x and the same discriminator weights enter D in the generator phase and in both calls
    of the discriminator phase (src/model.py:172,184-186)."""
    _store = {}

    @classmethod
    def get(cls, key_tensors, tag):
        e = cls._store.get(tuple(id(t) for t in key_tensors))
        if e is not None and all(r() is t for r, t in zip(e[0], key_tensors)) and e[1] == tag:
            return e[2]
        return None

    @classmethod
    def put(cls, key_tensors, tag, value):
        if len(cls._store) >= 8:
            cls._store.clear()
        cls._store[tuple(id(t) for t in key_tensors)] = ([weakref.ref(t) for t in key_tensors], tag, value)

    @classmethod
    def clear(cls):
        cls._store.clear()


HandOver.per_step.append(StepMemo)


class SplitS2dConvFn(Function):
    """z = Conv3d(k4, s2, p1)(cat([x, y], 1)) + bias with the two parts of the concatenation as separate space-to-depth
    operands sx = S(x) (constant: no gradient) and sy = S(y): the convolution is linear in its input, so
    z = conv(sx; W[:, :cx]) + conv(sy; W[:, cx:]) + bias.  The x-part is an f32 tensor computed ONCE per training step
    (StepMemo) and enters the y-part's launch as the accumulators' start value (conv_march2_kernel: `addend`): the
    PatchGAN's first block (src/model.py:72-73, 86-87) then costs one 24-channel convolution per step plus three 6-channel
    ones, instead of three 30-channel ones -- and S(x) is packed once instead of three times, the data gradient covers the 6
    y channels only, and the x-part of the weight gradient runs over x once (both halves of a stacked pair read the same
    x: ``xn``).  sx may hold fewer samples than sy (forward_pair stacks two calls over one x)."""

    sum_pair_gradients = True       # False: the x-part's weight gradient reads x once per half instead (`xn`; exact, twice the work)

    @staticmethod
    def forward(ctx, sx, sy, weight, bias, spec: ConvSpec, cx: int, cy: int, want_stats: bool):
        sx, sy = ops.as_act(sx), ops.as_act(sy)
        nx, ny = sx.shape[0], sy.shape[0]
        assert ny % nx == 0 and sx.shape[1:4] == sy.shape[1:4] and spec.cin == cx + cy
        di, hi, wi = sy.shape[1:4]
        grid = (di - 1, hi - 1, wi - 1)
        dtype, dev = sy.dtype, sy.device
        cpx, cpy = sx.shape[4] // 8, sy.shape[4] // 8
        cp = round_up(spec.cout, 16)
        tag = LayerCache._tag(weight)
        px = StepMemo.get((sx, weight), tag)
        if px is None:
            wpx, coutp, _ = spec.w_fwd_s2d_part(weight, dtype, cpx, 0, cx)
            px = torch.empty((nx, *grid, coutp), dtype=torch.float32, device=dev)
            ops.conv_fwd(sx, None, wpx, coutp, None, 2, 1, (0, 0, 0), px, grid, real=(cx, spec.cout))
            StepMemo.put((sx, weight), tag, px)
        wpy, coutp, _ = spec.w_fwd_s2d_part(weight, dtype, cpy, cx, cy)
        out = ops.new_act(ny, *grid, cp, dtype, dev)
        part = _conv_fwd_stats(want_stats, sy, None, wpy, coutp, bias.detach() if bias is not None else None, 2, 1, (0, 0, 0), out, grid,
                               (cy, spec.cout), addend=px)
        ctx.save_for_backward(sx, sy, weight)
        ctx.spec, ctx.cx, ctx.cy = spec, cx, cy
        ctx.bias_param, ctx.weight_param = bias, weight
        return _out_and_stats(ctx, out, part)

    @staticmethod
    @once_differentiable
    def backward(ctx, dz, _dpart):
        if dz is None:
            return (None,) * 8
        sx, sy, weight = ctx.saved_tensors
        spec, cx, cy = ctx.spec, ctx.cx, ctx.cy
        dz = ops.as_act(dz)
        ny, di, hi, wi, _ = sy.shape
        grid = tuple(dz.shape[1:4])
        dtype, dev = sy.dtype, sy.device
        cpx, cpy = sx.shape[4] // 8, sy.shape[4] // 8
        k = spec.ks
        dsy = dw = db = None
        if ctx.needs_input_grad[1]:
            wp, coutp, _ = spec.w_dgrad_s2d_part(weight, dtype, dz.shape[4], cpy, cx, cy)
            dsy = ops.new_act(ny, di, hi, wi, 8 * cpy, dtype, dev)
            ops.conv_fwd(dz, None, wp, coutp, None, 2, 1, (1, 1, 1), dsy, (di, hi, wi), real=(spec.cout, cy))
        if ctx.needs_input_grad[2]:
            weight = ctx.weight_param
            wsink, dwt, acc, defer = _grad_target(weight, deferrable=True)     # (x- and y-part: disjoint channel slices of dw)
            geo = (spec.cin * k ** 3, k ** 3, (k * k, k, 1), (0, 0, 0), (2, 2, 2))
            nx = sx.shape[0]
            if ny == 2 * nx and SplitS2dConvFn.sum_pair_gradients:
                # both halves of a stacked pair saw the SAME x: x (*) dz_a + x (*) dz_b = x (*) (dz_a + dz_b) -- half the x-part's
                # weight-gradient work for one pass over the two gradients (the sum is formed in f32 and rounded to bf16 once)
                ops.conv_wgrad(sx, None, torch.add(dz[:nx], dz[nx:]), grid, 1, (0, 0, 0), 2, 1, (0, 0, 0), dwt, spec.cout, cx, *geo,
                               s2d_cp=cpx, accumulate=acc, defer=defer)
            else:
                ops.conv_wgrad(sx, None, dz, grid, 1, (0, 0, 0), 2, 1, (0, 0, 0), dwt, spec.cout, cx, *geo, s2d_cp=cpx, accumulate=acc, n=ny,
                               defer=defer)
            ops.conv_wgrad(sy, None, dz, grid, 1, (0, 0, 0), 2, 1, (0, 0, 0), dwt, spec.cout, cy, *geo, s2d_cp=cpy, accumulate=acc,
                           dw_offset=cx * k ** 3, defer=defer)
            dw = _grad_done(wsink, weight, dwt, defer)
        if ctx.bias_param is not None and ctx.needs_input_grad[3]:
            db = _bias_colsum_grad(ctx.bias_param, dz, spec.cout)
        return None, dsy, dw, db, None, None, None, None


class UpCatTables:
    """What UpCatConvFn derives from the weights of one UpCat block (csrc/upcat.hip): the composite 4x4x4 kernel k4, its packing for
    the depth-to-space launch, the bias vector / border corrections, and k4's packing as the weight of the virtual
    Conv3d(co -> cl, k4, s2, p1) whose forward is the up-branch's data gradient.  Rebuilt IN PLACE (stable addresses: hipGraph
    replays) whenever one of the four parameters has changed (version counters / the optimiser epoch)."""

    def __init__(self):
        self.tag = None
        self.bufs = None
        self.wpk = None

    def stale(self, wd, bd, wc, bc) -> bool:
        return self.tag != tuple(LayerCache._tag(t) for t in (wd, wc, bd, bc) if t is not None)

    def get(self, wd, bd, wc, bc, ce, dtype):
        tag = tuple(LayerCache._tag(t) for t in (wd, wc, bd, bc) if t is not None)
        if tag != self.tag:
            self.bufs = ops.upcat_compose(wd.detach(), wc.detach(), bd.detach(), bc.detach() if bc is not None else None, ce, out=self.bufs)
            k4 = self.bufs[0]
            cl, co = k4.shape[:2]
            self.wpk = ops.weight_pack(k4, cl, co, 2, co * 64, 64, (16, 4, 1), (0, 0, 0), (2, 2, 2), dtype, cinp=8 * co, s2d_mode=1,
                                       s2d_cp=co, reuse=self.wpk[0] if self.wpk is not None else None)
            self.tag = tag
            self.args = (wd, bd, wc, bc, ce, dtype)
        return self.bufs, self.wpk

    def refresh(self):
        """after an optimiser step (repack_weights): rebuild now, so that the next forward finds everything fresh"""
        if self.tag is not None:
            self.get(*self.args)


class UpCatConvFn(Function):
    """z = Conv3d(ce + cu -> co, k3, p1)(cat([x_e, ConvTranspose3d(cl -> cu, k2, s2)(x_low)], 1)) + b_c  -- MONAI UpCat's
    upsample + concatenation + first convolution (BasicUNet at src/model.py:22-28) -- WITHOUT the up-sampled tensor: the two
    linear maps of the up-branch compose to one transposed convolution with a 4x4x4 kernel on the low-resolution tensor
    (csrc/upcat.hip: 8 taps instead of 27 per output voxel, `up` neither written nor read).  Launches:
      forward   skip part  P = conv3(x_e; W_c[:, :ce])                              (the layer's usual kernel, no bias)
                up part    z = convT4(x_low; K4) + P + biasp (+ border classes)     (conv_march2_kernel, depth-to-space mode)
      backward  dx_e = conv3^T(dz; W_c[:, :ce]);  S(dz);  dx_low = Kconv(S(dz));  dW_c[:, :ce] (usual kernel);
                dK4 = Kconv's weight gradient;  border sums of dz;  chain rule -> dW_d, dW_c[:, ce:], db_d.
    Even extents (skip = 2 x low), bf16.  The skip part P is rounded to bf16 once on its way into the second launch's accumulators (the
    unfused path rounded `up`, 64 channels of it, instead)."""

    @staticmethod
    def forward(ctx, x_e, x_low, wd, bd, wc, bc, spec_c: ConvSpec, tables: UpCatTables, want_stats: bool):
        x_e, x_low = ops.as_act(x_e), ops.as_act(x_low)
        n, D, H, W, ce = x_e.shape
        cl = x_low.shape[4]
        co = spec_c.cout
        assert tuple(x_low.shape[1:4]) == (D // 2, H // 2, W // 2) and wc.shape[1] == ce + wd.shape[1] and co % 32 == 0
        dtype, dev = x_e.dtype, x_e.device
        (k4, wp, biasp, delta), _ = tables.get(wd, bd, wc, bc, ce, dtype)
        wps, coutp, _ = spec_c.w_fwd_part(wc, dtype, ce, 0, ce)
        # (the skip part travels in bf16: as f32 -- an f32-output variant of conv_march_kernel, measured -- the fused forward took
        #  312 - 346 us instead of 234 - 240: 268 MB more to write and to read back)
        p_skip = ops.new_act(n, D, H, W, co, dtype, dev)
        ops.conv_fwd(x_e, None, wps, coutp, None, 3, 1, (1, 1, 1), p_skip, (D, H, W), real=(ce, co))
        out = ops.new_act(n, D, H, W, co, dtype, dev)
        grid = (D // 2, H // 2, W // 2)
        part = _conv_fwd_stats(want_stats, x_low, None, wp, 8 * co, biasp, 2, 1, (0, 0, 0), out, grid, (cl, 8 * co), cols=co, delta=delta,
                               addend=p_skip, d2s=True)
        ctx.save_for_backward(x_e, x_low, wd, wc, bd)
        ctx.spec_c, ctx.tables = spec_c, tables
        ctx.params = (wd, bd, wc, bc)
        return _out_and_stats(ctx, out, part)

    @staticmethod
    @once_differentiable
    def backward(ctx, dz, _dpart):
        if dz is None:
            return (None,) * 9
        x_e, x_low, wd, wc, bd = ctx.saved_tensors
        spec_c: ConvSpec = ctx.spec_c
        dz = ops.as_act(dz)
        n, D, H, W, ce = x_e.shape
        cl, co = x_low.shape[4], spec_c.cout
        cu = wd.shape[1]
        dtype, dev = x_e.dtype, x_e.device
        grid = (D // 2, H // 2, W // 2)
        (k4, _, _, _), wpk = ctx.tables.get(wd, bd, wc, ctx.params[3], ce, dtype)
        dx_e = dx_low = dwd = dbd = dwc = dbc = None
        if ctx.needs_input_grad[0]:
            wp, coutp, _ = spec_c.w_dgrad_s1_part(wc, dtype, dz.shape[4], 0, ce)
            dx_e = ops.new_act(n, D, H, W, ce, dtype, dev)
            ops.conv_fwd(dz, None, wp, coutp, None, 3, 1, (1, 1, 1), dx_e, (D, H, W), real=(co, ce))
        need_w = ctx.needs_input_grad[2] or ctx.needs_input_grad[4] or ctx.needs_input_grad[3]
        sg = ops.s2d_repack(dz) if (ctx.needs_input_grad[1] or need_w) else None      # S(dz): Kconv's operand, forward and weight gradient
        if ctx.needs_input_grad[1]:
            dx_low = ops.new_act(n, *grid, cl, dtype, dev)
            ops.conv_fwd(sg, None, wpk[0], wpk[1], None, 2, 1, (0, 0, 0), dx_low, grid, real=(co, cl))
        if need_w:
            wd_p, bd_p, wc_p, bc_p = ctx.params
            sk_c, dwc_t, acc_c, _ = _grad_target(wc_p)
            sk_d, dwd_t, acc_d, _ = _grad_target(wd_p)
            sk_b, dbd_t, acc_b, _ = _grad_target(bd_p)
            assert acc_c == acc_d == acc_b, "the UpCat block's parameters are used together"
            ops.conv_wgrad(x_e, None, dz, (D, H, W), 1, (0, 0, 0), 3, 1, (1, 1, 1), dwc_t, co, ce, (ce + cu) * 27, 27, (9, 3, 1),
                           (0, 0, 0), (1, 1, 1), accumulate=acc_c)
            dk4 = torch.empty_like(k4)
            ops.conv_wgrad(sg, None, x_low, grid, 1, (0, 0, 0), 2, 1, (0, 0, 0), dk4, cl, co, co * 64, 64, (16, 4, 1), (0, 0, 0), (2, 2, 2),
                           s2d_cp=co)
            esum = ops.border_sums(dz, co)
            ops.upcat_chain(dk4, wd.detach(), wc.detach(), bd.detach(), esum, ce, dwd_t, dwc_t, dbd_t, acc_c)
            dwc, dwd, dbd = _grad_done(sk_c, wc_p, dwc_t), _grad_done(sk_d, wd_p, dwd_t), _grad_done(sk_b, bd_p, dbd_t)
            if bc_p is not None and ctx.needs_input_grad[5]:
                # a normalisation follows: the mean subtraction cancels the convolution's bias, its gradient is exactly zero
                bsink = sink_of(bc_p)
                dbc = _grad_done(bsink, bc_p, _cached_zeros(co, dev) if bsink is None else None)
        return dx_e, dx_low, dwd, dbd, dwc, dbc, None, None, None


# ====================================================================================== norm + act
class NormCfg:
    def __init__(self, kind, channels, eps=1e-5, momentum=0.1, slope=1.0, p=0.0, act="leakyrelu"):
        """act: "leakyrelu" (``slope`` by value; 0 is ReLU, 1 the identity) or "prelu" (the slope is a trained parameter handed
        to NormActFn as ``alpha``; ``slope`` is not used)."""
        assert kind in ("instance", "batch", "none") and act in ("leakyrelu", "prelu")
        self.kind, self.channels, self.eps, self.momentum, self.slope, self.p = kind, channels, eps, momentum, slope, p
        self.act = act


class DropoutState:
    """Dropout randomness without host involvement per launch: one 64-bit step counter per device in
    device memory (seeded from torch's CPU generator, so torch.manual_seed governs it) plus a per-call
    salt.  ``advance()`` (once per training step: ``begin_step``) bumps the counter ON THE DEVICE, so a step captured
    in a hipGraph draws fresh masks at every replay."""
    _base = {}
    _salt = 0

    @classmethod
    def base(cls, device) -> torch.Tensor:
        t = cls._base.get(device)
        if t is None:
            t = torch.randint(0, 2 ** 40, (1,), dtype=torch.int64).to(device)
            cls._base[device] = t
        return t

    @classmethod
    def next_salt(cls) -> int:
        cls._salt += 1
        return cls._salt

    @classmethod
    def advance(cls, device):
        cls.base(device).add_(1)
        cls._salt = 0

    @classmethod
    def reset(cls):
        cls._base.clear()
        cls._salt = 0


def begin_step(device):
    """A training step begins: fresh dropout masks, constant inputs are packed afresh, nothing of the last step is left in a
    hand-over table, and the e4m3 scales gathered in the last step come into use."""
    DropoutState.advance(device)
    for table in HandOver.per_step:
        table.clear()
    Fp8Scales.advance(device)


class NormOpts(NamedTuple):
    """What a NormActFn node is asked for beyond norm + dropout + activation; a request it cannot serve (see forward) is dropped.
    bn_groups: BatchNorm statistics per consecutive sample group (two forward calls of the discriminator stacked along the
    batch: each group is normalised with its own batch statistics, the running statistics receive the groups' momentum updates
    in order -- exactly what two separate calls do).  emit8 / emit8_bwd: the fp8 convolution after this node / the fp8 data
    gradient of the convolution before it reads an e4m3 copy of a / dz: the kernel that writes the bf16 tensor writes the copy too."""
    s2d_out: bool = False       # return S(a), the space-to-depth tensor the next k4 s2 p1 block reads, instead of the plain a
    small: bool = False         # small tensor (ops.norm_is_small): statistics, norm, dropout and activation in ONE launch
    bn_groups: int = 1
    emit8: Optional["Fp8Scales.Slot"] = None
    emit8_bwd: Optional["Fp8Scales.Slot"] = None
    final: Optional[tuple] = None   # (weight, bias, skip_a) of the 1x1x1 convolution that is this node's ONLY consumer
    pool_after: bool = False    # the activation's only consumer is SkipPoolFn (nn.Down.forward_skip)


def _norm_statistics(z, part, conv_bias, cfg: NormCfg, training, running_mean, running_var, batches_tracked, bn_groups=1,
                     in_launch=False):
    """Where a norm node's statistics come from -> (groups, mean, rstd, batch_stats, running).  batch_stats: the batch's own
    (instance norm; BatchNorm in training mode or without running statistics) -- from the partials ``part`` the convolution's
    launch emitted (taken about ``conv_bias``) or a reduction over z, finalized per group; ``running``: the buffers that launch
    updates (running_mean, running_var, batches_tracked), or Nones.  in_launch: the caller's kernel computes batch statistics
    itself (the small-tensor launch): mean / rstd come back None, nothing is launched."""
    n, d, h, w, c = z.shape
    if cfg.kind == "none":
        return 1, None, None, False, (None,) * 3
    if cfg.kind == "batch" and not training and running_mean is not None:
        # eval mode: every sample is normalised with the SAME running statistics: one (1, c) mean / rstd row, one group --
        # whatever bn_groups says (a stacked forward_pair on a model in .eval(): ADVICE r3)
        mean = _padded(running_mean, c).reshape(1, c)
        rstd = torch.rsqrt(_padded(running_var, c, 1.0) + cfg.eps).reshape(1, c)
        return 1, mean, rstd, False, (None,) * 3
    groups = n if cfg.kind == "instance" else bn_groups
    assert n % groups == 0
    count = n * d * h * w // groups
    if count <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(z.shape)}")
    upd = cfg.kind == "batch" and training and running_mean is not None
    running = (running_mean, running_var, batches_tracked) if upd else (None,) * 3
    if in_launch:
        return groups, None, None, True, running
    if part is not None and part.numel() > 0:
        assert part.shape[2] == c, "fused statistics need coutp == padded channels"
        ppg = part.shape[0] // groups
        shift = conv_bias.detach() if conv_bias is not None else None
    else:
        (part, ppg), shift = ops.channel_stats(z, groups), None
    n_real = running_mean.numel() if upd else (shift.numel() if shift is not None else 0)
    mean, rstd = ops.norm_finalize(part, ppg, groups, c, count, shift, cfg.eps, running[0], running[1], cfg.momentum, n_real=n_real,
                                   batches_tracked=running[2])
    return groups, mean, rstd, True, running


def _affine_grad_target(gamma_p, beta_p, both: bool):
    """Where a norm's affine gradients go -> (sink, keyword arguments for the backward launch).  ``both`` wanted and in one sink:
    the kernels write (second use: add) them straight into the parameters' .grad storage (gradsink.py); else fresh vectors."""
    sink = sink_of(gamma_p) if (both and sink_of(beta_p) is sink_of(gamma_p)) else None
    if sink is None:
        return None, {}
    _, dg_t, acc, _ = _grad_target(gamma_p)
    return sink, dict(affine_into=(dg_t, sink_grad(beta_p)), accumulate=acc)


def _affine_grad_done(sink, gamma_p, beta_p, dgamma, dbeta, nch, need_g, need_b):
    """The backward launch is enqueued: tell the sink, or cut the fresh vectors to the ``nch`` real channels -> what autograd gets"""
    return (_grad_done(sink, gamma_p, dgamma[:nch].contiguous() if (dgamma is not None and need_g) else None),
            _grad_done(sink, beta_p, dbeta[:nch].contiguous() if (dbeta is not None and need_b) else None))


class NormActFn(Function):
    """a = LeakyReLU(Dropout(Norm(z)))  -- MONAI ADN "NDA" / BatchNorm3d + LeakyReLU; with cfg.act == "prelu" a = PReLU(...) and
    ``alpha`` (f32[1]) is its trained slope: read on the device by every launch, its gradient returned.  part / conv_bias: the
    convolution's fused statistics and the bias they were taken about (_norm_statistics); opts: NormOpts."""

    @staticmethod
    def _positional(cfg, training, running_mean, running_var, s2d_out=False, batches_tracked=None, small=False, bn_groups=1,
                    emit8=None, emit8_bwd=None, final=None, pool_after=False, alpha=None):
        """what followed conv_bias in the positional form from before NormOpts -> what follows it in forward"""
        return (alpha, running_mean, running_var, batches_tracked, cfg, training,
                NormOpts(s2d_out, small, bn_groups, emit8, emit8_bwd, final, pool_after))

    @classmethod
    def apply(cls, z, part, gamma, beta, conv_bias, *rest):
        # a NormCfg where forward has alpha (a tensor or None): a caller written for the positional form, which stays served
        if rest and isinstance(rest[0], NormCfg):
            rest = cls._positional(*rest)
        return super().apply(z, part, gamma, beta, conv_bias, *rest)

    @staticmethod
    def forward(ctx, z, part, gamma, beta, conv_bias, alpha, running_mean, running_var, batches_tracked, cfg: NormCfg, training,
                opts: NormOpts = NormOpts()):
        z = ops.as_act(z)
        n, d, h, w, c = z.shape
        if (cfg.act == "prelu") != (alpha is not None) or (alpha is not None and cfg.kind == "none"):
            raise ValueError("NormActFn: a PReLU node takes its slope as `alpha` (and a norm); a LeakyReLU node takes none")
        groups, mean, rstd, batch_stats, running = _norm_statistics(z, part, conv_bias, cfg, training, running_mean, running_var,
                                                                    batches_tracked, opts.bn_groups, in_launch=opts.small)
        # which launch: the one-launch small-tensor kernel (it needs batch statistics to compute), else the streaming kernel in ONE
        # of its forms -- S(a) out, + e4m3 copy, + final convolution, + max-pool, plain -- the first one asked for that it can serve.
        # The e4m3 copies and the final convolution exist for 32 bf16 channels in the plain layout only; a node that was ASKED for
        # the small kernel writes no e4m3 copy even where it falls back to the streaming one.
        small = opts.small and batch_stats
        bf16_32 = z.dtype == torch.bfloat16 and c == 32
        can8 = bf16_32 and not opts.small and not opts.s2d_out
        emit8 = opts.emit8 if (can8 and opts.emit8 is not None and opts.emit8.primed) else None
        ctx.emit8_bwd = opts.emit8_bwd if (can8 and opts.emit8_bwd is not None and opts.emit8_bwd.primed) else None
        # (the kernels guard gamma / beta's possibly shorter length; alpha is a pointer for them, never read on the host)
        gp, bp, ap = (t.detach() if t is not None else None for t in (gamma, beta, alpha))
        p = cfg.p if training else 0.0
        seed, seed_t = (DropoutState.next_salt(), DropoutState.base(z.device)) if p > 0.0 else (0, None)
        out = _new_s2d(ops.s2d_shape(n, d, h, w, c), z.dtype, z.device) if opts.s2d_out else None

        def launch(**form):
            return ops.normact_fwd(z, groups, mean, rstd, gp, bp, cfg.slope, p, seed, seed_t=seed_t, alpha=ap, **form)

        if small:
            # small tensor (low U-Net levels, last PatchGAN blocks)
            a, mean, rstd = ops.normact_small_fwd(z, groups, gp, bp, cfg.eps, cfg.slope, p, seed, seed_t, running[0], running[1],
                                                  cfg.momentum, running[2], out=out, s2d=opts.s2d_out, alpha=ap)
        elif opts.s2d_out:
            a = launch(out=out, s2d=True)
        elif emit8 is not None:
            a8 = torch.empty(z.shape, dtype=torch.uint8, device=z.device)
            a = launch(q8=(a8, emit8.use, emit8.next))
            emit8.touched = True
            Fp8Side.put(a, a8)
        elif opts.final is not None and bf16_32:
            # the 1x1x1 convolution computed in the same pass; without autograd (skip_a) the activation itself is not even written
            fw, fb, skip_a = opts.final          # (skip_a comes from the caller: in here grad mode is always off)
            y = ops.new_act(n, d, h, w, round_up(fw.shape[0], 16), z.dtype, z.device)
            a = launch(final=(fw.detach(), fb.detach() if fb is not None else None, y), skip_a=skip_a)
            FusedFinal.put(a, y, fw, fw._version)
        elif opts.pool_after and PoolSide.enabled and d % 2 == 0 and h % 2 == 0 and w % 2 == 0:
            # SkipPoolFn's MaxPool3d(2) in this launch (PoolSide); a statistics group is whole samples, so no window straddles two
            a, py, pidx = launch(pool=True)
            PoolSide.put(a, py, pidx)
        else:
            a = launch()
        ctx.small, ctx.s2d_out, ctx.seed_t = small, opts.s2d_out, seed_t
        ctx.affine_params, ctx.alpha_param = (gamma, beta), alpha
        ctx.save_for_backward(z, mean, rstd, gp, bp, ap)
        ctx.meta = (groups, cfg.slope, p, seed, batch_stats, gamma.numel() if gamma is not None else 0)
        return a

    @staticmethod
    @once_differentiable
    def backward(ctx, da):
        z, mean, rstd, gp, bp, ap = ctx.saved_tensors
        groups, slope, p, seed, batch_stats, nch = ctx.meta
        da = ops.as_act(da)
        lazy = LazyDx.take(da)                  # (dz, W) of the 1x1x1 convolution that consumed a: da is formed on the fly
        if lazy is not None:
            if ctx.small or ctx.s2d_out:
                raise RuntimeError("LazyDx placeholder reached a norm node that cannot form the gradient itself")
            da = None
        pool = None
        lp = LazyPool.take(da) if da is not None else None     # (x, y, idx, d_pool, d_skip): MaxPool3d(2) + skip consumed a
        if lp is not None:
            if ctx.small or ctx.s2d_out:
                da = ops.maxpool2_bwd(lp[0], lp[1], lp[3], lp[4])     # these kernels read a materialised gradient
            else:
                pool, da = (lp[2], lp[3]), lp[4]
        _, _, need_g, need_b, _, need_alpha = ctx.needs_input_grad[:6]
        want_affine = need_g or need_b
        gamma_p, beta_p = ctx.affine_params
        sink, kw = _affine_grad_target(gamma_p, beta_p, need_g and need_b and mean is not None)
        # PReLU: the slope's gradient comes out of the same launches, written (or accumulated) where the parameter's gradient lives;
        # the launches share one `accumulate` with the affine gradients -- where the two differ it goes through a scalar of its own
        alpha_p, asink, da_t, da_tmp = ctx.alpha_param, None, None, None
        if alpha_p is not None and need_alpha:
            asink, da_t, a_acc, _ = _grad_target(alpha_p)
            if a_acc != bool(kw.get("accumulate", False)):
                da_tmp = torch.zeros_like(da_t)
            kw.update(dalpha=da_t if da_tmp is None else da_tmp)
        kw.update(s2d=ctx.s2d_out, seed_t=ctx.seed_t, alpha=ap)
        if ctx.small:
            dz, dgamma, dbeta = ops.normact_small_bwd(z, da, groups, mean, rstd, gp, bp, slope, p, seed, batch_stats,
                                                      want_affine=want_affine, **kw)
        else:
            slot8 = ctx.emit8_bwd
            q8 = (torch.empty(z.shape, dtype=torch.uint8, device=z.device), slot8.use, slot8.next) if slot8 is not None else None
            dz, dgamma, dbeta = ops.normact_bwd(z, da, groups, mean, rstd, gp, bp, slope, p, seed, batch_stats,
                                                want_affine and mean is not None, q8=q8, implicit=lazy, pool=pool, **kw)
            if q8 is not None:
                slot8.touched = True
                Fp8Side.put(dz, q8[0])
        dg, dbt = _affine_grad_done(sink, gamma_p, beta_p, dgamma, dbeta, nch, need_g, need_b)
        dal = None
        if da_t is not None:
            if da_tmp is not None:
                da_t.add_(da_tmp) if a_acc else da_t.copy_(da_tmp)
            dal = _grad_done(asink, alpha_p, da_t)
        # z, part, gamma, beta, conv_bias, alpha; then running_mean, running_var, batches_tracked, cfg, training, opts
        return dz, None, dg, dbt, None, dal, None, None, None, None, None, None


class ResTailFn(Function):
    """y = ReLU(Norm(z)) + residual(x): the tail of nn.ResidualUnit (MONAI ResidualUnit, ADN "NDA", no activation after the sum) as
    ONE launch (ops.restail_fwd) instead of a norm + act launch, a 1x1x1 convolution and an add.  z: the last convolution's
    output, part: its fused statistics, x: the block's input; residual(x) = x when ``res_weight`` is None, else the 1x1x1
    convolution (res_weight, res_bias), ``res_spec`` its ConvSpec.  cfg: NormCfg with slope 0, no dropout; statistics as in
    NormActFn (_norm_statistics, one BatchNorm group).
    Backward: the existing launches -- ops.normact_bwd on z with da = dy (it recomputes the ReLU mask from z), the streaming
    1x1x1 weight gradient and a column sum for the residual convolution, and for x (when it needs one) dy itself or the 1x1x1
    data gradient."""

    @staticmethod
    def _positional(res_spec, cfg, training, running_mean, running_var, batches_tracked=None):
        """what followed res_bias in the earlier positional form -> what follows it in forward"""
        return running_mean, running_var, batches_tracked, res_spec, cfg, training

    @classmethod
    def apply(cls, *args):
        # a NormCfg where forward has running_var (a tensor or None): a caller written for the earlier order, which stays served
        if len(args) > 9 and isinstance(args[9], NormCfg):
            args = args[:8] + cls._positional(*args[8:])
        return super().apply(*args)

    @staticmethod
    def forward(ctx, z, part, x, gamma, beta, conv_bias, res_weight, res_bias, running_mean, running_var, batches_tracked,
                res_spec: Optional[ConvSpec], cfg: NormCfg, training):
        z, x = ops.as_act(z), ops.as_act(x)
        if cfg.kind == "none" or cfg.act != "leakyrelu" or cfg.slope != 0.0 or cfg.p != 0.0:
            raise ValueError("ResTailFn: a norm followed by ReLU, without dropout")
        groups, mean, rstd, batch_stats, _ = _norm_statistics(z, part, conv_bias, cfg, training, running_mean, running_var,
                                                              batches_tracked)
        gp, bp = gamma.detach(), beta.detach()
        rw = res_weight.detach() if res_weight is not None else None
        rb = res_bias.detach() if res_bias is not None else None
        cx = res_spec.cin if res_weight is not None else cfg.channels
        y = ops.restail_fwd(z, x, groups, mean, rstd, gp, bp, cfg.channels, cx, rw, rb)
        ctx.save_for_backward(z, x, mean, rstd, gp, bp)
        ctx.params = (gamma, beta, res_weight, res_bias)
        ctx.res_spec = res_spec
        ctx.meta = (groups, batch_stats, cfg.channels)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        z, x, mean, rstd, gp, bp = ctx.saved_tensors
        gamma_p, beta_p, rw_p, rb_p = ctx.params
        groups, batch_stats, nch = ctx.meta
        spec: Optional[ConvSpec] = ctx.res_spec
        dy = ops.as_act(dy)
        n, d, h, w, c = z.shape
        need_z, _, need_x, need_g, need_b, _, need_rw, need_rb = ctx.needs_input_grad[:8]
        dz = dg = dbt = dx = drw = drb = None
        if need_z or need_g or need_b:
            # norm + ReLU: exactly NormActFn's launches with slope 0 and no dropout
            sink, kw = _affine_grad_target(gamma_p, beta_p, need_g and need_b)
            dz, dgamma, dbeta = ops.normact_bwd(z, dy, groups, mean, rstd, gp, bp, 0.0, 0.0, 0, batch_stats, need_g or need_b, **kw)
            dg, dbt = _affine_grad_done(sink, gamma_p, beta_p, dgamma, dbeta, nch, need_g, need_b)
        if rw_p is None:
            dx = dy if need_x else None
        else:
            if need_x:
                wp, coutp, _ = spec.w_dgrad_s1(rw_p, z.dtype, c)
                dx = ops.new_act(n, d, h, w, x.shape[4], z.dtype, z.device)
                ops.conv_fwd(dy, None, wp, coutp, None, 1, 1, (0, 0, 0), dx, (d, h, w), real=(spec.cout, spec.cin))
            if need_rw:
                wsink, dwt, acc, defer = _grad_target(rw_p, deferrable=True)
                ops.conv_wgrad(x, None, dy, (d, h, w), 1, (0, 0, 0), 1, 1, (0, 0, 0), dwt, spec.cout, spec.cin, spec.cin, 1, (1, 1, 1),
                               (0, 0, 0), (1, 1, 1), accumulate=acc, defer=defer)
                drw = _grad_done(wsink, rw_p, dwt, defer)
            if rb_p is not None and need_rb:
                drb = _bias_colsum_grad(rb_p, dy, spec.cout)
        # z, part, x, gamma, beta, conv_bias, res_weight, res_bias; then the running buffers, res_spec, cfg, training
        return dz, None, dx, dg, dbt, None, drw, drb, None, None, None, None, None, None


# ====================================================================================== pool / loss
class MaxPoolFn(Function):
    @staticmethod
    def forward(ctx, x):
        x = ops.as_act(x)
        y = ops.maxpool2_fwd(x)
        ctx.save_for_backward(x, y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        return ops.maxpool2_bwd(x, y, ops.as_act(dy))


class SkipPoolFn(Function):
    """An encoder level's output is used twice: by the skip connection and by MaxPool3d(2) (MONAI BasicUNet).
    Returning both uses from ONE autograd node lets the backward see both gradients at once and sum them inside
    the max-pool backward kernel, instead of the engine launching a separate add over the full-resolution tensor."""

    @staticmethod
    def forward(ctx, x, lazy=False):
        """lazy: the caller found x's producer to be a NormActFn node (SkipPoolFn.apply_to): the backward may hand it a LazyPool
        placeholder instead of the materialised gradient."""
        x = ops.as_act(x)
        n, d, h, w, c = x.shape
        ctx.lazy = bool(lazy and LazyPool.enabled and d % 2 == 0 and h % 2 == 0 and w % 2 == 0)
        side = PoolSide.take(x)                 # (y, idx) written by the launch that wrote x
        if side is not None:
            y, idx = side
            ctx.save_for_backward(*((x, y, idx) if ctx.lazy else (x, y)))
        elif ctx.lazy:
            y, idx = ops.maxpool2_fwd(x, want_idx=True)
            ctx.save_for_backward(x, y, idx)
        else:
            y = ops.maxpool2_fwd(x)
            ctx.save_for_backward(x, y)
        ctx.set_materialize_grads(False)
        return x.view_as(x), y

    @staticmethod
    @once_differentiable
    def backward(ctx, d_skip, d_pool):
        if d_pool is None:
            return d_skip, None
        x, y = ctx.saved_tensors[:2]
        add = None
        if d_skip is not None:
            add = d_skip if d_skip.stride(4) == 1 and d_skip.dtype == x.dtype else ops.as_act(d_skip)
        if ctx.lazy:
            ph = torch.empty(x.shape, dtype=x.dtype, device=x.device)      # placeholder: never written, never read (LazyPool)
            LazyPool.put(ph, x, y, ctx.saved_tensors[2], ops.as_act(d_pool), add)
            return ph, None
        return ops.maxpool2_bwd(x, y, ops.as_act(d_pool), add), None

    @classmethod
    def apply_to(cls, x):
        """(skip, pooled) of an encoder level's output; offers the lazy gradient when x comes straight out of a norm + act node.
        The caller promises that x has no other consumer (BasicUNet.forward: a level's output goes to forward_skip only) -- autograd
        would otherwise add the uninitialised placeholder to the other consumer's gradient."""
        fnode = x.grad_fn
        return cls.apply(x, fnode is not None and type(fnode).__name__ == "NormActFnBackward")


class L1LossFn(Function):
    """torch.nn.L1Loss()(a, b) (mean reduction) on contiguous f32 tensors (src/model.py:126,136)."""

    @staticmethod
    def forward(ctx, a, b):
        a = a.contiguous()
        b = b.contiguous()
        ctx.save_for_backward(a, b)
        return ops.l1_fwd(a, b)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        da = ops.l1_bwd(a, b, g)
        return (da if ctx.needs_input_grad[0] else None, (-da) if ctx.needs_input_grad[1] else None)


def l1_loss(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return L1LossFn.apply(a, b)


class SSIM3dFn(Function):
    """Per-item Gaussian-window SSIM of contiguous f32 (B, C, D, H, W) tensors, (B, 1) f32, differentiable in ``a`` only
    (losses.SSIMLoss).  ``window``: the normalised 1-D profile, a host tensor.  The incoming per-item gradient stays on the
    device (ops.ssim3d_loss_bwd), so a step with this term captures into a hipGraph."""

    @staticmethod
    def forward(ctx, a, b, window, c1: float, c2: float):
        ssim, p = ops.ssim3d_loss_fwd(a, b, window, c1, c2)
        ctx.save_for_backward(a, b, p)
        ctx.window = window
        return ssim.float()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b, p = ctx.saved_tensors
        return ops.ssim3d_loss_bwd(a, b, p, g, ctx.window), None, None, None, None


class PerceptualFn(Function):
    """The MedicalNet Perceptual distance of contiguous f32 (B, C, D, H, W) tensors, f32 (), differentiable in ``y_hat`` only
    (losses.PerceptualLoss(differentiable=True)).  The forward is the extractor and tail pass of the metric path -- the same
    launches, so the same bits -- with the prediction's activations kept; the target's run keeps nothing.  The incoming
    gradient stays on the device (ops.medicalnet_tail_bwd), so a step with this term captures into a hipGraph."""

    @staticmethod
    def forward(ctx, y_hat, y, net):
        kept = {}
        fp, ft = net.features(y_hat, keep=kept), net.features(y)
        value, _item_sum, _mp, _mt = ops.medicalnet_tail(fp, ft, y_hat.shape[0], y_hat.shape[1])
        ctx.net, ctx.names = net, tuple(kept)
        ctx.save_for_backward(y_hat, ft, *kept.values())
        return value.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from .medicalnet import medicalnet_backward
        y_hat, ft, *saved = ctx.saved_tensors
        kept = dict(zip(ctx.names, saved))
        fp = kept["layer4.out"]
        g_feat = ops.medicalnet_tail_bwd(fp, ft, g.to(torch.float32).reshape(1).contiguous(), y_hat.shape[0], y_hat.shape[1])
        return medicalnet_backward(ctx.net, y_hat, kept, g_feat), None, None


class GanGenLossFn(Function):
    """The generator phase's loss head (src/model.py:126-137) as one launch each way on top of the L1 kernels:
    (adv + recon, [L1, recon, adv, adv + recon]) with adv = BCEWithLogits(logits, 1).mean() and recon = L1(y_hat, y) / divisor
    * factor.  In a graph replay a launch costs ~5 us whatever its size; the composed form is ~27 scalar-sized launches."""

    @staticmethod
    def forward(ctx, logits, y_hat, y, divisor: float, factor: float):
        logits, y_hat, y = logits.contiguous(), y_hat.contiguous(), y.contiguous()
        out = ops.gan_gen_loss_fwd(logits, y_hat, y, divisor, factor)
        ctx.save_for_backward(logits, y_hat, y)
        ctx.scale = (divisor, factor)
        ctx.mark_non_differentiable(out)
        return out[3], out

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        logits, y_hat, y = ctx.saved_tensors
        dlogits, gscale = ops.gan_gen_loss_bwd(logits, g, *ctx.scale)
        dy_hat = ops.l1_bwd(y_hat, y, gscale) if ctx.needs_input_grad[1] else None
        return dlogits if ctx.needs_input_grad[0] else None, dy_hat, None, None, None


class GanDiscrLossFn(Function):
    """The discriminator phase's loss (src/model.py:183-193): (BCEWithLogits(real, 1).mean() + BCEWithLogits(fake, 0).mean()) / 2
    in one launch each way.  ``real`` None: ``fake`` holds both logit maps stacked along the batch, fake first
    (Discriminator.forward_pair's single pass) -- the gradient is then one tensor, no slice / pad / add nodes."""

    @staticmethod
    def forward(ctx, fake, real):
        stacked = real is None
        fake = fake.contiguous()
        if stacked:
            half = fake.numel() // 2
            flat = fake.view(-1)
            f, r = flat[:half], flat[half:]
        else:
            real = real.contiguous()
            f, r = fake, real
        out = ops.gan_discr_loss_fwd(f, r)
        ctx.save_for_backward(fake, real)
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        fake, real = ctx.saved_tensors
        if real is None:
            d = torch.empty_like(fake)
            half = fake.numel() // 2
            ops.gan_discr_loss_bwd(fake.view(-1)[:half], fake.view(-1)[half:], g, d.view(-1)[:half], d.view(-1)[half:])
            return d, None
        df, dr = torch.empty_like(fake), torch.empty_like(real)
        ops.gan_discr_loss_bwd(fake, real, g, df, dr)
        return df, dr
