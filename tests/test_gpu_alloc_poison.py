"""No kernel reads memory that nobody wrote ("Allocations are never zero-filled").

Every byte of device memory of the package comes from ``torch.empty`` / ``empty_like`` / ``new_empty`` on the Python side, and
the kernels own "every slot is written by exactly one thread" contracts instead of zero-fills.  The parity tests run on the
caching allocator's memory -- fresh zeros, or the block an identical earlier call left behind -- so a kernel that reads a slot
it never wrote sees zero or last time's right answer there and passes.  Here every scenario runs three times: as it is, with
every fresh allocation filled with NaN, and filled with a huge finite value (tests/alloc_poison.py: why both).  All tensors a
scenario returns must be finite and BIT-IDENTICAL in the three runs: no tolerance, the kernels are deterministic (no atomics
but the order-independent amax atomicMax).  No CPU reference is computed in this file.

A scenario is a zero-argument function that builds its inputs and modules itself from fixed seeds and returns a flat dict of
tensors -- whole tensors, padded channels included.  Where a documented contract leaves a region unwritten AND unread, the
scenario returns the contractual region only, with a comment that cites the contract; nothing else is excluded.

The last test asserts that the scenarios together reached every allocation site of the package (an ``ast`` scan at test
time) but an explicit allowlist of at most five."""
import zlib

import numpy as np
import pytest
import torch

from tests.alloc_poison import run_scenario, static_sites
from tests.test_gpu_ops import CONV_CASES, S2D_PLANS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
DT = {F32: "f32", BF16: "bf16"}

SCENARIOS = {}          # id -> scenario
LOGGED = set()          # (file, line) of every package allocation the poisoned runs saw
RAN = set()             # ids whose test ran to its end

# allocation sites no scenario reaches: at most 5, each with its reason
ALLOWLIST = {
    "ddp.py": "the flat bucket of GradBuckets' multi-rank exchange: needs more than one rank (tests/test_gpu_ddp.py runs it)",
}


def scenario(name):
    def reg(fn):
        assert name not in SCENARIOS, name
        SCENARIOS[name] = fn
        return fn
    return reg


# ------------------------------------------------------------------------------------------------ helpers
def _pkg():
    from unet_bssfp_amd import functional as Fn, ops
    return Fn, ops


def seed(s=0):
    """fixed seeds; dropout masks repeat; nothing of an earlier run is left in a hand-over table or a step memo"""
    Fn, _ = _pkg()
    torch.manual_seed(s)
    Fn.DropoutState.reset()
    for table in Fn.HandOver.per_step:
        table.clear()


def rnd(*shape, lo=-0.5, scale=1.0):
    return (torch.rand(*shape, device=DEV) + lo) * scale


def rndn(*shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, device=DEV) * scale + shift


def act(x, dtype, cp=None):
    """NCDHW f32 device tensor -> NDHWC activation (channels padded to cp: the pack kernel writes the padding)"""
    _, ops = _pkg()
    n, c, d, h, w = x.shape
    cp = ops.round_up(c, 16) if cp is None else cp
    out = ops.new_act(n, d, h, w, cp, dtype, DEV)
    ops.pack_ncdhw(x.float().contiguous(), out, 0, cp)
    return out


def s2d(x, dtype, cp):
    """NCDHW f32 device tensor -> S(x), allocated like PackFn allocates it: NOT zero-filled"""
    Fn, ops = _pkg()
    n, c, d, h, w = x.shape
    out = Fn._new_s2d(ops.s2d_shape(n, d, h, w, cp), dtype, DEV)
    ops.pack_ncdhw_s2d(x.float().contiguous(), out, cp, 0, cp)
    return out


def grads(out, **named):
    """add the .grad of every named tensor / parameter that has one"""
    for k, t in named.items():
        if t is not None and t.grad is not None:
            out[k] = t.grad
    return out


def conv_layer(cins, cout, ks, stride, pad):
    from unet_bssfp_amd.nn import Conv3d
    return Conv3d(sum(cins), cout, ks, stride, pad).to(DEV)


# ------------------------------------------------------------------------------------------------ convolutions
def _conv_case(case, dtype):
    name, n, cins, cout, sp, ks, stride, pad = case

    def run():
        Fn, _ = _pkg()
        seed(zlib.crc32(name.encode()) % 1000)
        layer = conv_layer(cins, cout, ks, stride, pad)
        xs = [act(rnd(n, c, *sp, lo=-0.3), dtype).requires_grad_(True) for c in cins]
        z, part = Fn.ConvFn.apply(xs[0], xs[1] if len(xs) > 1 else None, layer.weight, layer.bias, layer.spec, True)
        z.backward(act(rnd(n, cout, *z.shape[1:4]), dtype))
        out = {"z": z, "stats": part}
        for i, x in enumerate(xs):
            out[f"dx{i}"] = x.grad
        return grads(out, dw=layer.weight, db=layer.bias)
    return run


for _case in CONV_CASES:
    for _dt in (F32, BF16):
        scenario(f"conv-{_case[0]}-{DT[_dt]}")(_conv_case(_case, _dt))


DECONV_CASES = [(64, 64, (2, 4, 8)), (128, 64, (4, 4, 4)), (64, 64, (64, 64, 33)), (128, 64, (32, 64, 65)), (64, 64, (8, 8, 32)),
                (128, 64, (4, 8, 64)), (256, 128, (8, 8, 8))]       # tests/test_gpu_ops.py::test_deconv_fwd_bwd


def _deconv_case(cin, cout, sp, dtype):
    def run():
        from unet_bssfp_amd.nn import ConvTranspose3d
        seed(2)
        layer = ConvTranspose3d(cin, cout, 2, 2).to(DEV)
        a = act(rnd(2, cin, *sp, lo=-0.4), dtype).requires_grad_(True)
        z = layer.forward_act(a)                                    # the strided output classes (os, ooff) or the 8 Cout GEMM
        z.backward(act(rnd(2, cout, *z.shape[1:4]), dtype))
        return grads({"z": z, "dx": a.grad}, dw=layer.weight, db=layer.bias)
    return run


for _c in DECONV_CASES:
    for _dt in (F32, BF16):
        scenario(f"deconv-{_c[0]}to{_c[1]}-{'x'.join(map(str, _c[2]))}-{DT[_dt]}")(_deconv_case(*_c, _dt))


K4S2_CASES = [(1, 30, 32, (8, 8, 32)), (2, 32, 64, (8, 8, 8)), (1, 64, 128, (4, 4, 4)), (2, 256, 32, (4, 4, 4))]


def _k4s2_s2d_case(n, cin, cout, sp, dtype):
    def run():
        Fn, ops = _pkg()
        seed(4)
        layer = conv_layer((cin,), cout, 4, 2, 1)
        cp = ops.round_up(cin, 16)
        s = s2d(rnd(n, cin, *sp, lo=-0.3), dtype, cp).requires_grad_(True)
        z, part = Fn.ConvFn.apply(s, None, layer.weight, layer.bias, layer.spec, True, False, cp)
        z.backward(act(rnd(n, cout, *z.shape[1:4]), dtype))
        return grads({"s": s, "z": z, "stats": part, "ds": s.grad}, dw=layer.weight, db=layer.bias)
    return run


for _c in K4S2_CASES:
    for _dt in (F32, BF16):
        scenario(f"k4s2_s2d-n{_c[0]}-{_c[1]}to{_c[2]}-{'x'.join(map(str, _c[3]))}-{DT[_dt]}")(_k4s2_s2d_case(*_c, _dt))
for _c in S2D_PLANS:                                                # the marching k2 kernel: bf16 only
    scenario(f"k4s2_s2d-n{_c[0]}-{_c[1]}to{_c[2]}-{'x'.join(map(str, _c[3]))}-bf16")(_k4s2_s2d_case(*_c, BF16))


def _split_s2d_case(ny, summed):
    def run():
        Fn, _ = _pkg()
        seed(6)
        Fn.StepMemo.clear()
        Fn.SplitS2dConvFn.sum_pair_gradients = summed
        try:
            cx, cy, cout, sp = 24, 6, 32, (64, 64, 64)
            layer = conv_layer((cx + cy,), cout, 4, 2, 1)
            sx, sy = s2d(rnd(1, cx, *sp, lo=-0.3), BF16, 32), s2d(rnd(ny, cy, *sp, lo=-0.3), BF16, 8).requires_grad_(True)
            z, part = Fn.SplitS2dConvFn.apply(sx, sy, layer.weight, layer.bias, layer.spec, cx, cy, True)     # x-part: f32 `addend`
            z2, _ = Fn.SplitS2dConvFn.apply(sx, sy, layer.weight, layer.bias, layer.spec, cx, cy, False)      # x-part from the memo
            z.backward(act(rnd(ny, cout, *z.shape[1:4]), BF16))
        finally:
            Fn.SplitS2dConvFn.sum_pair_gradients = True
            Fn.StepMemo.clear()
        return grads({"z": z, "z_memo": z2, "stats": part, "dsy": sy.grad}, dw=layer.weight, db=layer.bias)
    return run


for _ny, _summed in [(1, True), (2, True), (2, False)]:
    scenario(f"split_s2d-ny{_ny}-{'summed' if _summed else 'xn'}")(_split_s2d_case(_ny, _summed))


UPCAT_CASES = [(1, 32, 64, 64, 32, (24, 32, 64)), (2, 32, 64, 64, 32, (10, 24, 40)), (1, 64, 128, 64, 64, (16, 16, 32))]


def _upcat_case(n, ce, cl, cu, co, low):
    def run():
        Fn, _ = _pkg()
        from unet_bssfp_amd.nn import Conv3d, ConvTranspose3d
        seed(11)
        deconv, conv = ConvTranspose3d(cl, cu).to(DEV), Conv3d(ce + cu, co, 3, 1, 1).to(DEV)
        with torch.no_grad():
            deconv.bias.mul_(4.0)                                   # a deconv bias that matters at the border
        skip = tuple(2 * e for e in low)
        a_e, a_l = act(rnd(n, ce, *skip, lo=-0.3), BF16).requires_grad_(True), act(rnd(n, cl, *low, lo=-0.3), BF16).requires_grad_(True)
        tables = Fn.UpCatTables()
        z, part = Fn.UpCatConvFn.apply(a_e, a_l, deconv.weight, deconv.bias, conv.weight, conv.bias, conv.spec, tables, True)
        gz = rnd(n, co, *skip)
        z.backward(act(gz - gz.mean((2, 3, 4), keepdim=True), BF16))
        out = {"z": z, "stats": part, "dx_e": a_e.grad, "dx_low": a_l.grad}
        out.update({f"table{i}": t for i, t in enumerate(tables.bufs)})      # k4, its packing, bias vector, border corrections
        out["k4_pack"] = tables.wpk[0]
        return grads(out, dwd=deconv.weight, dbd=deconv.bias, dwc=conv.weight, dbc=conv.bias)
    return run


for _c in UPCAT_CASES:
    scenario(f"upcat-n{_c[0]}-ce{_c[1]}-cl{_c[2]}-{'x'.join(map(str, _c[5]))}")(_upcat_case(*_c))


def _genout_case(which):
    def run():
        Fn, _ = _pkg()
        seed(41)
        sp, n = (8, 12, 16), 2
        z = act(rnd(n, 6, *sp), BF16).requires_grad_(True)
        y, s = Fn.GenOutFn.apply(z, 6, 8)
        outs, gs = [], []
        if which != "discr_only":
            outs.append(y); gs.append(rnd(n, 6, *sp))
        if which != "loss_only":
            outs.append(s); gs.append(s2d(rnd(n, 6, *sp), BF16, 8))
        torch.autograd.backward(outs, gs)
        return {"y": y, "s": s, "dz": z.grad}
    return run


for _w in ("both", "loss_only", "discr_only"):
    scenario(f"genout-{_w}")(_genout_case(_w))


# ------------------------------------------------------------------------------------------------ norm + activation
def _normact_case(kind, n, c, sp, dtype, p, small=False, s2d_out=False, bn_groups=1, training=True):
    def run():
        Fn, ops = _pkg()
        seed(7)
        if small:
            assert ops.norm_is_small(n, *sp, c, bn_groups)
        bn = kind == "batch"
        z = act(rndn(n, c, *sp, scale=1.5, shift=0.7), dtype).requires_grad_(True)
        gamma = beta = None
        if kind != "none":
            gamma, beta = rnd(c, lo=0.5).requires_grad_(True), rnd(c).requires_grad_(True)
        rm, rv = (rnd(c), rnd(c, lo=0.5)) if bn else (None, None)
        nbt = torch.zeros((), dtype=torch.long, device=DEV) if bn else None
        cfg = Fn.NormCfg(kind, c, slope=0.1 if kind == "instance" else 0.2, p=p)
        a = Fn.NormActFn.apply(z, None, gamma, beta, None, None, rm, rv, nbt, cfg, training,
                               Fn.NormOpts(s2d_out=s2d_out, small=small, bn_groups=bn_groups))
        ga = rnd(n, c, *sp)
        a.backward(s2d(ga, dtype, z.shape[4]) if s2d_out else act(ga, dtype))
        out = {"a": a, "dz": z.grad}
        if bn:
            out.update(running_mean=rm, running_var=rv, batches_tracked=nbt)
        return grads(out, dgamma=gamma, dbeta=beta)
    return run


NORMACT_FORMS = [
    # id, kind, n, c, spatial, keyword arguments
    ("stream_in_n1", "instance", 1, 64, (16, 16, 32), {}),
    ("stream_in_n2", "instance", 2, 32, (4, 8, 8), {}),
    ("stream_bn_c24", "batch", 2, 24, (4, 4, 8), {}),                      # 24 real channels in 32: gamma / beta shorter than a row
    ("stream_bn_c512", "batch", 3, 512, (2, 2, 2), {}),
    ("stream_none", "none", 2, 32, (4, 4, 4), {}),
    ("small_s1", "instance", 2, 128, (4, 6, 8), dict(small=True)),         # register-resident, one row slot per thread
    ("small_s8", "instance", 1, 128, (16, 16, 16), dict(small=True)),      # eight row slots per thread
    ("small_s8_pred", "instance", 2, 64, (8, 12, 16), dict(small=True)),   # predicated slots, two groups one after the other
    ("small_bn_stream", "batch", 1, 64, (16, 16, 32), dict(small=True)),   # more than 4096 rows per group: the streaming form behind
    ("small_chunks_3", "instance", 3, 64, (4, 4, 4), dict(small=True)),    # >= 3 groups: the group-chunk backward (f64 scratch)
    ("small_chunks_8", "instance", 8, 128, (8, 8, 8), dict(small=True)),
    ("small_chunks_32", "instance", 32, 64, (2, 2, 2), dict(small=True)),  # more than 16 groups
    ("small_bn2", "batch", 2, 64, (16, 16, 16), dict(small=True, bn_groups=2)),
    ("small_bn2_n4", "batch", 4, 64, (8, 8, 8), dict(small=True, bn_groups=2)),
    ("stream_bn2", "batch", 4, 64, (8, 8, 8), dict(bn_groups=2)),
    ("eval_bn", "batch", 2, 32, (4, 4, 4), dict(training=False)),
    ("s2d_out", "batch", 2, 32, (4, 8, 8), dict(s2d_out=True)),
    ("s2d_out_ragged", "batch", 1, 32, (6, 10, 14), dict(s2d_out=True)),   # border cells with out-of-volume sibling blocks
    ("small_s2d_out", "batch", 2, 64, (4, 4, 8), dict(small=True, s2d_out=True)),
]

for _id, _kind, _n, _c, _sp, _kw in NORMACT_FORMS:
    for _dt in (F32, BF16):
        for _p in (0.0, 0.1):
            scenario(f"normact-{_id}-{DT[_dt]}-p{_p}")(_normact_case(_kind, _n, _c, _sp, _dt, _p, **_kw))


def _normact_pool_case(dtype, p, with_skip):
    """norm + act with the fused MaxPool3d(2) (PoolSide) and its lazy backward (LazyPool: the placeholder SkipPoolFn returns is
    never written and never read, functional.py: LazyPool)"""
    def run():
        Fn, _ = _pkg()
        seed(29)
        n, c, sp = 2, 32, (8, 12, 32)
        z = act(rndn(n, c, *sp, scale=1.5, shift=0.3), dtype).requires_grad_(True)
        gamma, beta = rnd(c, lo=0.5).requires_grad_(True), rnd(c).requires_grad_(True)
        cfg = Fn.NormCfg("instance", c, slope=0.1, p=p)
        a = Fn.NormActFn.apply(z, None, gamma, beta, None, None, None, None, None, cfg, True, Fn.NormOpts(pool_after=True))
        assert Fn.PoolSide._by_ptr, "the fused pool did not run"
        skip, pooled = Fn.SkipPoolFn.apply_to(a)
        dy = act(rndn(n, c, *(e // 2 for e in sp)), dtype)
        if with_skip:
            wide = act(rndn(n, 2 * c, *sp), dtype)
            torch.autograd.backward([skip, pooled], [wide[..., c:], dy])     # (a channel slice of a wider buffer, as in the U-Net)
        else:
            pooled.backward(dy)
        assert not Fn.LazyPool._by_ptr and not Fn.PoolSide._by_ptr
        return grads({"a": skip, "pooled": pooled, "dz": z.grad}, dgamma=gamma, dbeta=beta)
    return run


for _dt in (F32, BF16):
    for _p in (0.0, 0.1):
        for _ws in (True, False):
            scenario(f"normact-pool-{DT[_dt]}-p{_p}-{'skipgrad' if _ws else 'poolonly'}")(_normact_pool_case(_dt, _p, _ws))


def _normact_final_case(p, skip_a):
    """the fused final 1x1x1 convolution (FusedFinal) and, with autograd, its implicit data gradient (LazyDx: ConvFn.backward
    returns a placeholder that is never written and never read, functional.py: LazyDx)"""
    def run():
        Fn, _ = _pkg()
        seed(23)
        n, c, sp, k = 2, 32, (8, 12, 32), 6
        z = act(rndn(n, c, *sp, scale=1.5, shift=0.3), BF16).requires_grad_(not skip_a)
        gamma, beta = rnd(c, lo=0.5).requires_grad_(not skip_a), rnd(c).requires_grad_(not skip_a)
        w, b = rndn(k, c, 1, 1, 1, scale=0.2).requires_grad_(not skip_a), rndn(k, scale=0.3)
        cfg = Fn.NormCfg("instance", c, slope=0.1, p=p)
        spec = Fn.ConvSpec("conv", c, k, 1, 1, 0)
        with torch.set_grad_enabled(not skip_a):
            a = Fn.NormActFn.apply(z, None, gamma, beta, None, None, None, None, None, cfg, True, Fn.NormOpts(final=(w, b, skip_a)))
            y, _ = Fn.ConvFn.apply(a, None, w, b, spec, False, False, 0, False, True)
        if skip_a:
            # contract region: with skip_a the activation itself is not written, its only consumer is the fused convolution
            # (functional.py, NormActFn.forward: "without autograd (skip_a) the activation itself is not even written")
            return {"y": y}
        y.backward(act(rndn(n, k, *sp, scale=0.1), BF16))
        assert not Fn.LazyDx._by_ptr and not Fn.FusedFinal._by_ptr
        return grads({"a": a, "y": y, "dz": z.grad}, dgamma=gamma, dbeta=beta, dw=w)
    return run


for _p in (0.0, 0.1):
    for _sa in (False, True):
        scenario(f"normact-final-bf16-p{_p}-{'skip_a' if _sa else 'autograd'}")(_normact_final_case(_p, _sa))


# ------------------------------------------------------------------------------------------------ pooling
def _pool_case(sp, c, dtype):
    def run():
        _, ops = _pkg()
        seed(11)
        n = 2
        x = act(rndn(n, c, *sp), dtype)
        x[:, :2, :2, :2, :] = 0.0                              # ties
        y = ops.maxpool2_fwd(x)
        y2, idx = ops.maxpool2_fwd(x, want_idx=True)
        dy = act(rnd(n, c, *(e // 2 for e in sp), lo=0.0), dtype)
        wide = act(rndn(n, 2 * c, *sp), dtype)
        return {"y": y, "y_idx": y2, "idx": idx, "dx": ops.maxpool2_bwd(x, y, dy), "dx_add": ops.maxpool2_bwd(x, y, dy, wide[..., c:])}
    return run


for _sp, _c in (((4, 8, 8), 32), ((5, 7, 9), 16)):
    for _dt in (F32, BF16):
        scenario(f"pool-{'x'.join(map(str, _sp))}-{DT[_dt]}")(_pool_case(_sp, _c, _dt))


# ------------------------------------------------------------------------------------------------ loss and optimiser
@scenario("l1")
def _l1():
    from unet_bssfp_amd import l1_loss
    seed(13)
    a, b = rnd(2, 6, 9, 10, 11, lo=0.0).requires_grad_(True), rnd(2, 6, 9, 10, 11, lo=0.0).requires_grad_(True)
    loss = l1_loss(a, b)
    (loss * 50.0).backward()
    return {"loss": loss, "da": a.grad, "db": b.grad}


@scenario("gan_loss_heads")
def _gan_heads():
    from unet_bssfp_amd.functional import GanDiscrLossFn, GanGenLossFn
    seed(31)
    logits = rndn(2, 1, 4, 4, 4, scale=3.0).requires_grad_(True)
    y_hat, y = rnd(2, 6, 16, 24, 32, lo=0.0).requires_grad_(True), rnd(2, 6, 16, 24, 32, lo=0.0)
    total, parts = GanGenLossFn.apply(logits, y_hat, y, 1.0, 100.0)
    (total * 0.7).backward()
    fake, real = rndn(2, 1, 4, 4, 4, scale=2.0).requires_grad_(True), rndn(2, 1, 4, 4, 4, scale=2.0).requires_grad_(True)
    loss = GanDiscrLossFn.apply(fake, real)
    loss.backward()
    both = torch.cat([fake.detach(), real.detach()]).requires_grad_(True)
    loss_s = GanDiscrLossFn.apply(both, None)
    loss_s.backward()
    return {"gen_total": total, "gen_parts": parts, "dlogits": logits.grad, "dy_hat": y_hat.grad, "discr": loss, "dfake": fake.grad,
            "dreal": real.grad, "discr_stacked": loss_s, "dboth": both.grad}


@scenario("fused_adamw")
def _adamw():
    """two steps on gradients that the L1 backward kernel wrote into fresh (poisoned) memory; the second skips a parameter"""
    from unet_bssfp_amd import l1_loss
    from unet_bssfp_amd.optim import FusedAdamW
    seed(0)
    ps = [rndn(*s).requires_grad_(True) for s in [(32, 24, 3, 3, 3), (32,), (7,), (512, 256, 2, 2, 2)]]
    opt = FusedAdamW(ps, lr=1e-3)
    for step in range(2):
        for i, p in enumerate(ps):
            p.grad = None
            if not (step == 1 and i == 2):                     # a parameter without gradient is skipped
                (l1_loss(p, rndn(*p.shape)) * p.numel()).backward()
        opt.step()
    out = {f"p{i}": p.detach() for i, p in enumerate(ps)}
    for i, p in enumerate(ps):
        for k, v in opt.state.get(p, {}).items():
            if torch.is_tensor(v) and v.is_floating_point():
                out[f"state{i}_{k}"] = v
    return out


# ------------------------------------------------------------------------------------------------ fp8
@scenario("fp8_amax_cast_and_producer_copies")
def _fp8_ops():
    Fn, ops = _pkg()
    seed(3)
    n, c, sp = 2, 32, (4, 8, 16)
    x = act(rndn(n, c, *sp, scale=2.0), BF16)
    amax = ops.amax_act(x)
    x8 = ops.cast_fp8(x, amax)
    nxt = torch.zeros(1, dtype=torch.float32, device=DEV)
    x8d = ops.cast_fp8(x, amax * 0.5, nxt)                     # delayed scaling: some values saturate, amax gathered in the pass
    w_amax = ops.amax_f32(rndn(64, 32, 3, 3, 3))
    # producer side: the norm + act kernels write the e4m3 copy of a (forward) and of dz (backward) beside the bf16 tensor
    sa, sg = Fn.Fp8Scales.slot(DEV), Fn.Fp8Scales.slot(DEV)
    for s_, v in ((sa, 1.7), (sg, 0.031)):
        s_.use.fill_(v)
        s_.next.zero_()
        s_.primed = True
    z = act(rndn(n, c, *sp, scale=1.5, shift=0.3), BF16).requires_grad_(True)
    gamma, beta = rnd(c, lo=0.5).requires_grad_(True), rnd(c).requires_grad_(True)
    cfg = Fn.NormCfg("instance", c, slope=0.1, p=0.1)
    a = Fn.NormActFn.apply(z, None, gamma, beta, None, None, None, None, None, cfg, True, Fn.NormOpts(emit8=sa, emit8_bwd=sg))
    a8 = Fn.Fp8Side.take(a)[0]
    a.backward(act(rnd(n, c, *sp), BF16))
    (dz8, _, dz), = Fn.Fp8Side._by_ptr.values()                # (the copy travels under the tensor the backward kernel wrote)
    Fn.Fp8Side.clear()
    return grads({"amax": amax, "x8": x8, "x8_delayed": x8d, "amax_next": nxt, "w_amax": w_amax, "a": a, "a8": a8, "dz": dz,
                  "dz8": dz8, "amax_a": sa.next.clone(), "amax_dz": sg.next.clone()}, dgamma=gamma, dbeta=beta)


# ------------------------------------------------------------------------------------------------ whole steps
def _state(model, out, prefix=""):
    for name, p in model.named_parameters():
        out[f"{prefix}param/{name}"] = p.detach()
        if p.grad is not None:
            out[f"{prefix}grad/{name}"] = p.grad
    for name, b in model.named_buffers():
        out[f"{prefix}buffer/{name}"] = b
    return out


def _training_steps(mode):
    """two training steps of the GAN at 1 x 24 x 64^3 with generator dropout: the second has the delayed e4m3 scales primed (the
    producer-side copies run); DeferredReduce, the gradient sinks, PackMemo, LazyDx and LazyPool are all on this path"""
    def run():
        import unet_bssfp_amd as M
        from unet_bssfp_amd.gan import bSSFPToDWITensorModel, synthetic_batch
        seed(2)
        batch = synthetic_batch(1, 64, seed=11, device=DEV)
        model = bSSFPToDWITensorModel("bssfp", gen=M.Generator("bssfp", dropout=0.1).to(DEV), discr=M.Discriminator("bssfp").to(DEV)).train()
        M.set_compute_dtype(model, mode)
        out = {}
        for i in range(2):
            model.training_step(batch, i)
            for k, v in model.last_logs.items():
                out[f"log{i}/{k}"] = torch.as_tensor(v, device=DEV).detach().float().reshape(())
        return _state(model, out)
    return run


for _mode in ("f32", "bf16", "fp8"):
    scenario(f"training_steps-{_mode}")(_training_steps(_mode))


def _discriminator_case(modality, n, size, cin):
    """the PatchGAN on plain NCDHW tensors, the target requiring a gradient: PackFn's two-source space-to-depth pack and its
    backward (unpack_ncdhw_s2d), the space-to-depth norm outputs, and the stacked pair of the discriminator phase"""
    def run():
        import unet_bssfp_amd as M
        seed(7)
        d = M.Discriminator(modality).to(DEV).train()
        x, y = rnd(n, cin, size, size, size, lo=0.0), rnd(n, 6, size, size, size, lo=0.0).requires_grad_(True)
        logits = d(x, y)
        torch.nn.functional.binary_cross_entropy_with_logits(logits, torch.ones_like(logits)).backward()
        out = {"logits": logits, "dy": y.grad}
        both = d.forward_pair(x, rnd(n, 6, size, size, size, lo=0.0), y.detach(), stacked=True)
        both = both if isinstance(both, torch.Tensor) else torch.cat(list(both))
        both.mean().backward()
        out["pair_logits"] = both
        return _state(d, out)
    return run


scenario("discriminator-bssfp-n1-64")(_discriminator_case("bssfp", 1, 64, 24))
scenario("discriminator-t1w-n2-32")(_discriminator_case("t1w", 2, 32, 6))


@scenario("generator_odd_skip_extents")
def _odd_skip():
    import unet_bssfp_amd as M
    seed(7)
    g = M.Generator("bssfp", dropout=0.0).to(DEV).train()      # 40 -> 20 -> 10 -> 5 -> 2: the up-sampled 4 meets a skip of 5
    x, y = rnd(1, 24, 40, 24, 56, lo=0.0).requires_grad_(True), rnd(1, 6, 40, 24, 56, lo=0.0)
    y_hat = g(x)
    (y_hat - y).abs().mean().backward()
    return _state(g, {"y_hat": y_hat, "dx": x.grad})


@scenario("basic_unet_2d")
def _unet2d():
    from unet_bssfp_amd import BasicUNet
    seed(31)
    net = BasicUNet(spatial_dims=2, in_channels=1, out_channels=6, dropout=0.0).to(DEV).train()
    x, y = rnd(2, 1, 64, 64, lo=0.0), rnd(2, 6, 64, 64, lo=0.0)
    y_hat = net(x)
    (y_hat - y).abs().mean().backward()
    return _state(net, {"y_hat": y_hat})


# ------------------------------------------------------------------------------------------------ outside the step
def _predict_case(mode):
    def run():
        from unet_bssfp_amd import inference as I, nn as N
        seed(3)
        gen = N.Generator("bssfp").to(DEV)
        vol = rnd(24, 48, 64, 64, lo=0.0)
        return {"volume": I.predict_volume(gen, vol, 32, 8, batch_size=5, overlap_mode=mode)}
    return run


for _m in ("crop", "average"):
    scenario(f"predict_volume-{_m}")(_predict_case(_m))


def _metrics_case(shape):
    def run():
        from unet_bssfp_amd import metrics as M
        seed(5)
        p, y = rnd(*shape, lo=0.0), rnd(*shape, lo=0.0)
        out = {"mae": M.MAEMetric()(p, y), "mse": M.MSEMetric()(p, y), "psnr": M.PSNRMetric(1)(p, y),
               "ssim": M.SSIMMetric(3, data_range=1)(p, y)}
        if min(shape[2:]) >= 7:
            out["ssim_win7"] = M.SSIMMetric(3, win_size=7, kernel_sigma=1.0)(p, y)
        return out
    return run


for _s in [(2, 6, 32, 32, 32), (1, 6, 48, 40, 33), (3, 1, 11, 11, 11)]:
    scenario(f"metrics-{'x'.join(map(str, _s))}")(_metrics_case(_s))


def _ssim_loss_case(shape, win, sigma):
    def run():
        from unet_bssfp_amd.losses import SSIMLoss
        seed(9)
        x, y = rnd(*shape, lo=0.0).requires_grad_(True), rnd(*shape, lo=0.0)
        loss = SSIMLoss(3, win_size=win, kernel_sigma=sigma)(x, y)
        (loss * 3.5).backward()
        return {"loss": loss, "dx": x.grad}
    return run


for _s, _w, _sg in [((2, 3, 20, 17, 13), 11, 1.5), ((1, 2, 24, 9, 33), 7, 1.0)]:
    scenario(f"ssim_loss-{'x'.join(map(str, _s))}-win{_w}")(_ssim_loss_case(_s, _w, _sg))


@scenario("medicalnet_perceptual_and_fid")
def _medicalnet():
    from tests import medicalnet_ref as MR
    from unet_bssfp_amd import losses, metrics
    from unet_bssfp_amd.medicalnet import MedicalNetResNet10, medicalnet_distances
    seed(51)
    net = MedicalNetResNet10()
    net.load_state_dict(MR.random_init(MR.RefResNet10(), seed=11).state_dict(), strict=True)
    net = net.to(DEV)
    y = rndn(2, 2, 17, 20, 23, scale=1.5, shift=0.5)
    y_hat = y + 0.5 * rndn(*y.shape)
    value = losses.PerceptualLoss(net)(y_hat, y)
    _, fp, ft = medicalnet_distances(net, y_hat, y)
    return {"perceptual": value, "fid": metrics.FIDMedicalNet(net)(y_hat, y), "features_pred": fp, "features_target": ft}


def _dti_case(dtype, channels_first):
    def run():
        from unet_bssfp_amd import eval as E
        seed(17)
        sp = (5, 6, 7)

        def tensors():
            t = rnd(*sp, 6, scale=0.2)                          # (dxx, dxy, dxz, dyy, dyz, dzz): a dominant, distinct diagonal
            t[..., 0] += 1.0; t[..., 3] += 1.5; t[..., 5] += 2.0
            t = t.to(dtype)
            return t.movedim(-1, 0).contiguous() if channels_first else t
        pred, target = tensors(), tensors()
        mask = (rnd(*sp, lo=0.0) > 0.2)
        ps = rnd(*sp, 3, lo=0.0).to(dtype)
        ps = ps.movedim(-1, 0).contiguous() if channels_first else ps
        out = {f"map/{k}": v for k, v in E.calc_scalar_maps(pred, 0.1, 2.5, channels_first=channels_first).items()}
        table, maps = E.error_table(pred, target, mask, ps, 0.1, 2.5, channels_first=channels_first, return_maps=True)
        out["table"] = table
        out.update({f"err/{k}": v for k, v in maps.items()})
        out["table_only"] = E.error_table(pred, target, mask, ps, channels_first=channels_first)
        return out
    return run


for _dt, _cf in [(torch.float64, False), (F32, True)]:
    scenario(f"dti-{'f64' if _dt == torch.float64 else 'f32'}-{'cf' if _cf else 'cl'}")(_dti_case(_dt, _cf))


@scenario("augmentations")
def _augment():
    from unet_bssfp_amd import augment as A
    seed(19)
    x = rnd(3, 12, 20, 24, lo=0.0)                              # (C, D, H, W); non-negative: the spike takes the 'dc' path from the data
    signed = x - 0.4                                            # ... and the three-DFT path
    rng = np.random.default_rng(7)
    bias = A.RandomBiasField(order=3)
    out = {"bias": bias.apply(x, rng.uniform(-0.5, 0.5, 20).astype(np.float32)),
           "gamma": A.RandomGamma().apply(x, 1.2),
           "noise": A.RandomNoise().apply(x, (0.05, 0.1, 1234567)),
           "ghosting": A.RandomGhosting().apply(x, (5, 2, 0.7)),
           "blur": A.RandomBlur().apply(x, (1.2, 0.0, 0.8)),
           "spike_dc": A.RandomSpike().apply(x, A.SpikeParams(1.5, rng.random((1, 3)))),
           "spike_dft": A.RandomSpike().apply(signed, A.SpikeParams(0.7, rng.random((1, 3)))),
           "sum_min": A.channel_sum_min(signed), "spectrum_max": A.spectrum_max_device(signed)}
    mo = A.RandomMotion(num_transforms=2)
    params = A.MotionParams(np.array([0.3, 0.7], np.float32), rng.uniform(-10, 10, (2, 3)).astype(np.float32),
                            rng.uniform(-3, 3, (2, 3)).astype(np.float32))
    out["motion"] = mo.apply(x, params)
    out["motion_chained"] = mo.apply_chained(x, params)
    out["resample"] = A.rigid_resample(x, A.motion_matrices(params.degrees, params.translation, x.shape[1:])[1])
    return out


@scenario("patch_queue_fill")
def _patch_queue():
    from unet_bssfp_amd import data as Q
    seed(1)
    extents = [(23, 19, 32), (20, 24, 32), (17, 27, 37)]
    subs = [{"bssfp": {"data": rnd(24, *s, lo=-0.3)}, "dwi-tensor": {"data": rnd(6, *s, lo=-0.3)}} for s in extents]
    q = Q.PatchQueue(subs, "bssfp", sampler=Q.UniformSampler((8, 12, 16)), target_shape=(20, 24, 32), seed=1)
    batch = q.next_batch(6, augmented_target=True)
    return {name: v["data"] for name, v in batch.items() if isinstance(v, dict) and "data" in v}


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_result_does_not_depend_on_fresh_memory(hip, name):
    run_scenario(SCENARIOS[name], log=LOGGED, sync=torch.cuda.synchronize)
    RAN.add(name)


def test_runner_flags_a_read_of_unwritten_device_memory(hip):
    """the harness itself, on the device: a sum over a buffer of which only every second element was written"""
    from tests.alloc_poison import PoisonFinding

    def half_written():
        buf = torch.empty(256, device=DEV)
        buf[::2] = 1.0
        return {"sum": buf.sum()}
    with pytest.raises(PoisonFinding) as err:
        run_scenario(half_written, sync=torch.cuda.synchronize)
    assert err.value.kinds == {"nan", "big"}


def test_every_allocation_site_was_poisoned(hip):
    """the scenarios above, together, allocate at every torch.empty / empty_like / new_empty call of the package"""
    if RAN != set(SCENARIOS):
        pytest.skip("only part of the module was selected (or a scenario failed): site coverage needs every scenario")
    assert len(ALLOWLIST) <= 5
    sites = set(static_sites())
    allowed = {s for s in sites if s[0] in ALLOWLIST}
    assert len(allowed) <= 5, sorted(allowed)
    # (LOGGED also holds package lines that construct torch modules, whose constructors allocate: not sites of the package)
    assert len(LOGGED & sites) >= 50, "the logger and the scan do not speak of the same lines"
    missing = sites - allowed - LOGGED
    assert not missing, f"allocation sites no scenario reached: {sorted(missing)}"
