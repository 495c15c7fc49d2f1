"""In-situ audit of every convolution and weight-gradient launch of the real training step (GPU).

ops.CONV_PROBE / ops.WGRAD_PROBE snapshot each launch's operands (and every output range that is also read or only partly
written) before it runs, and after it compare the result with the descriptor-level reference of tests/conv_audit_ref.py on
the SAME operands: the only legitimate differences are the final rounding and the f32 summation order.  Bounds (derived, see
conv_audit_ref; tests/test_conv_audit_ref.py shows that each subtle corruption fails them), A = sum |x w| per element:
  * bf16 / e4m3 outputs: |y - r64| <= 1/2 spacing_bf16(y) + 2^-14 A at sampled voxels, twice that against the full f32
    reference everywhere; f32 outputs: 2^-14 A;
  * fused statistics per sample: sum within 2^-12 sqrt(P sum (z - b)^2), sum of squares within 2^-12 relative;
  * weight gradients per tap: rel-L2 <= 2^-13 and max error <= 2^-10 max |ref|;
  * everything outside the written region is bit-unchanged.
One eager training step per configuration (BASELINE.json sizes), weight-gradient reductions immediate, no graph capture.
The census (launches and worst err/bound per plan id / wgrad kind) goes to conv_audit.log, beside test_gpu_bf16.py's parity log.
"""
import math
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_audit_ref as R  # noqa: E402
from test_gpu_bf16 import LOG as _PARITY_LOG  # noqa: E402  (the suite's log directory)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOG = os.path.join(os.path.dirname(_PARITY_LOG), "conv_audit.log")
_ESIZE = {torch.float32: 4, torch.bfloat16: 2, torch.uint8: 1}


def _log(line):
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as fh:
            fh.write(line + "\n")
    except OSError:
        pass


def _host(ptr, nelem, dtype):
    """Copy nelem elements of `dtype` starting at a device pointer to the host (a non-owning view of the caller's memory)."""
    nbytes = int(nelem) * _ESIZE[dtype]
    st = torch._C._construct_storage_from_data_pointer(int(ptr), torch.device(DEV), nbytes)
    t = torch.empty(0, dtype=torch.uint8, device=DEV).set_(st, 0, (nbytes,), (1,))
    return t.cpu().view(dtype)


def _scalar(ptr):
    return float(_host(ptr, 1, torch.float32)[0]) if ptr else None


def _family(pid):
    """Kernel family from the plan id (10000 ks + 1000 halo + 100 shape + 10 vt + ct)."""
    from unet_bssfp_amd import ops
    p = ops.decode_plan_id(pid)
    names = {ops.SHAPE_MARCH: "march", ops.SHAPE_MARCHG: "marchg", ops.SHAPE_LOWG_W16: "lowg", ops.SHAPE_LOWG_W8: "lowg",
             ops.SHAPE_MARCH2: "march2", ops.SHAPE_RU: "ru"}
    return names.get(p.shape, f"k{p.ks} shape {p.shape}") if p.halo else f"k{p.ks} shape {p.shape}"


def _pair(a):
    return tuple(int(v) for v in a)


class Audit:
    """The probes of one configuration: census[key] = [launches, worst err/bound]."""

    def __init__(self, name, seed):
        self.name, self.seed = name, seed
        self.census, self.probed, self.audited = {}, 0, 0
        self.e4m3 = 0
        self.sec = 0.0

    def _note(self, key, worst):
        c = self.census.setdefault(key, [0, 0.0])
        c[0] += 1
        c[1] = max(c[1], worst)
        self.audited += 1
        assert worst <= 1.0, f"{self.name}: launch {key} exceeds its bound: err/bound = {worst:.3f}"

    # ---------------------------------------------------------------- forward launches
    def conv(self, pid, d, real):
        from unet_bssfp_amd import _lib
        import ctypes as C
        self.probed += 1
        torch.cuda.synchronize()
        t0 = time.time()
        et = R.elem_type(d.dtype)
        nx = d.n * d.di * d.hi * d.wi
        width = d.coutp // 8 if d.d2s else (d.cls_cout if d.cls_cout else d.coutp)
        cx = d.c0 + d.c1
        cinp = -(-cx // 16) * 16
        taps = 8 if d.d2s else d.ks ** 3
        nbias = d.nbias if d.nbias > 0 else d.coutp
        na = (d.add_n if d.add_n > 0 else d.n) * d.dy * d.hy * d.wy
        ns = R.SimpleNamespace(
            x0=_host(d.x0, R.act_extent(nx, d.c0, d.ld0), et), c0=d.c0, ld0=d.ld0,
            x1=_host(d.x1, R.act_extent(nx, d.c1, d.ld1), et) if d.x1 and d.c1 else None, c1=d.c1, ld1=d.ld1,
            n=d.n, di=d.di, hi=d.hi, wi=d.wi, do_=d.do_, ho=d.ho, wo=d.wo, ks=d.ks, stride=d.stride, pad=_pair(d.pad),
            wp=_host(d.wp, cinp * taps * d.coutp, et), coutp=d.coutp, bias=_host(d.bias, nbias, torch.float32) if d.bias else None,
            nbias=d.nbias, ldy=d.ldy, cstore=d.cstore, dy=d.dy, hy=d.hy, wy=d.wy, os=d.os, ooff=_pair(d.ooff), dtype=d.dtype,
            cls_cout=d.cls_cout, q_amax_x=_scalar(d.q_amax_x), q_amax_w=_scalar(d.q_amax_w),
            addend=_host(d.addend, R.act_extent(na, width, d.ld_add), torch.bfloat16 if d.add_bf16 else torch.float32) if d.addend else None,
            ld_add=d.ld_add, add_n=d.add_n, y_f32=d.y_f32, d2s=d.d2s, delta=_host(d.delta, 27 * width, torch.float32) if d.delta else None,
            add_bf16=d.add_bf16)
        yt = torch.float32 if (d.y_f32 or d.dtype == R.F32) else torch.bfloat16
        ny = d.n * d.dy * d.hy * d.wy
        y_ext = R.act_extent(ny, d.cstore, d.ldy)
        y_before = _host(d.y, y_ext, yt)
        tiles, tps = C.c_int32(0), C.c_int32(0)
        _lib.check(_lib.load().mi355_conv_num_tiles(C.byref(d), C.byref(tiles), C.byref(tps)), "conv_num_tiles")
        tiles, tps = tiles.value, tps.value
        if d.dtype == R.FP8:
            self.e4m3 += 1
        self.sec += time.time() - t0

        def after():
            torch.cuda.synchronize()
            t1 = time.time()
            y_after = _host(d.y, y_ext, yt)
            stats = _host(d.stats_part, tiles * 2 * width, torch.float32).view(tiles, 2, width) if d.stats_part else None
            ref = R.conv_fwd_ref(ns)
            written = ref.written.reshape(-1)
            pad = d.ldy - d.cstore
            ya = torch.nn.functional.pad(y_after, (0, pad)).view(ny, d.ldy)
            yb = torch.nn.functional.pad(y_before, (0, pad)).view(ny, d.ldy)
            ib = torch.int32 if yt == torch.float32 else torch.int16
            worst = 0.0
            # untouched: unwritten voxels and the channels [cstore, ldy) of written ones, bit for bit
            if not torch.equal(ya[~written].view(ib), yb[~written].view(ib)) or \
                    not torch.equal(ya[written][:, d.cstore:].view(ib), yb[written][:, d.cstore:].view(ib)):
                worst = math.inf
            y = ya[:, : d.cstore].float().view(d.n, d.dy, d.hy, d.wy, d.cstore)
            idx = R.sample_positions(ref.written, nrand=4096, seed=self.seed + self.audited)
            ref64 = R.conv_fwd_sampled(ns, idx)
            worst = max(worst, R.fwd_errors(y, yt, ref, ref64, idx))
            if stats is not None:
                st_ref, cnt = R.stats_ref(ref.acc, ref.written, d.n, width)
                got = stats.double()
                if tps > 0:
                    assert tiles == tps * d.n
                    got = got.view(d.n, tps, 2, width).sum(1)
                    worst = max(worst, R.stats_errors(got, st_ref, cnt, d.cstore))
                else:                                    # tiles span samples: the totals only
                    worst = max(worst, R.stats_errors(got.sum(0, keepdim=True), st_ref.sum(0, keepdim=True), cnt * d.n, d.cstore))
            self._note(("conv", pid, d.dtype), worst)
            self.sec += time.time() - t1

        return after

    # ---------------------------------------------------------------- weight-gradient launches
    def wgrad(self, kind, d):
        self.probed += 1
        torch.cuda.synchronize()
        t0 = time.time()
        et = R.elem_type(d.dtype)
        xn = d.xn if d.xn > 0 else d.n
        nx = xn * d.di * d.hi * d.wi
        ng = d.n * d.gd * d.gh * d.gw
        ns = R.SimpleNamespace(
            x0=_host(d.x0, R.act_extent(nx, d.c0, d.ld0), et), c0=d.c0, ld0=d.ld0,
            x1=_host(d.x1, R.act_extent(nx, d.c1, d.ld1), et) if d.x1 and d.c1 else None, c1=d.c1, ld1=d.ld1,
            n=d.n, di=d.di, hi=d.hi, wi=d.wi, g=_host(d.g, R.act_extent(ng, d.cg, d.ldg), et), cg=d.cg, ldg=d.ldg,
            do_=d.do_, ho=d.ho, wo=d.wo, gd=d.gd, gh=d.gh, gw=d.gw, gs=d.gs, goff=_pair(d.goff), ks=d.ks, stride=d.stride,
            pad=_pair(d.pad), cout=d.cout, cin=d.cin, s_co=d.s_co, s_ci=d.s_ci, s_k=_pair(d.s_k), tbase=_pair(d.tbase),
            tstep=_pair(d.tstep), accumulate=d.accumulate, dtype=d.dtype, s2d_cp=d.s2d_cp, g_cls_cout=d.g_cls_cout, xn=d.xn)
        cols = 8 * d.g_cls_cout if d.g_cls_cout else d.cg
        span = R.wgrad_span(ns, d.c0 + d.c1, cols)
        before = _host(d.dw, span, torch.float32)
        self.sec += time.time() - t0

        def after():
            torch.cuda.synchronize()
            t1 = time.time()
            got = _host(d.dw, span, torch.float32)
            g32 = R.wgrad_gemm(ns)
            g64 = R.wgrad_gemm(ns, R.wgrad_check_taps(d.ks), torch.float64)
            self._note(("wgrad", kind, d.dtype), R.wgrad_errors(ns, got, before, g32, g64))
            self.sec += time.time() - t1

        return after


CONFIGS = {
    # name: (compute dtype, N, edge, families of conv plans, wgrad kinds that must appear)
    "bf16_1x128": (torch.bfloat16, 1, 128, {"march", "marchg", "lowg", "march2"}, {2, 3, 4}),
    "bf16_8x64": (torch.bfloat16, 8, 64, {"march", "marchg", "lowg", "march2"}, {2, 3, 4}),
    "fp8_1x160": ("fp8", 1, 160, {"march", "marchg", "lowg", "march2"}, {2, 3, 4}),
    "f32_1x64": (torch.float32, 1, 64, set(), set()),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_conv_and_wgrad_launch_of_a_training_step_matches_the_reference(hip, name):
    import unet_bssfp_amd as M
    from unet_bssfp_amd import functional as Fn
    from unet_bssfp_amd import ops
    from unet_bssfp_amd.gan import bSSFPToDWITensorModel, synthetic_batch
    dtype, n, s, families, kinds = CONFIGS[name]
    torch.manual_seed(0)
    gen, discr = M.Generator("bssfp", dropout=0.0), M.Discriminator("bssfp")
    model = bSSFPToDWITensorModel("bssfp", gen=gen.to(DEV), discr=discr.to(DEV)).train()
    M.set_compute_dtype(model, dtype)
    batch = synthetic_batch(n, s, seed=1234, device=DEV)
    audit = Audit(name, seed=s)
    t0 = time.time()
    allowed = Fn.DeferredReduce.allowed
    Fn.DeferredReduce.allowed = False              # every weight gradient reduced at its own launch
    ops.CONV_PROBE, ops.WGRAD_PROBE = audit.conv, audit.wgrad
    try:
        model.training_step(batch, 0)
        torch.cuda.synchronize()
    finally:
        ops.CONV_PROBE = ops.WGRAD_PROBE = None
        Fn.DeferredReduce.allowed = allowed
    wall = time.time() - t0
    assert all(torch.isfinite(p).all() for p in model.parameters())
    _log(f"== {name}: {audit.probed} launches probed, {audit.audited} audited, {wall:.1f} s ({audit.sec:.1f} s in the audit)")
    for key in sorted(audit.census, key=str):
        cnt, worst = audit.census[key]
        what = f"plan {key[1]} ({_family(key[1])})" if key[0] == "conv" else f"wgrad kind {key[1]}"
        _log(f"  {what:28s} dtype {key[2]}  launches {cnt:4d}  worst err/bound {worst:.3f}")
    # census: nothing skipped, the families each configuration must contain
    assert audit.probed == audit.audited and audit.audited > 0, (audit.probed, audit.audited)
    fams = {_family(k[1]) for k in audit.census if k[0] == "conv"}
    assert families <= fams, (families - fams, fams)
    got_kinds = {k[1] for k in audit.census if k[0] == "wgrad"}
    assert kinds <= got_kinds, (kinds - got_kinds, got_kinds)
    if dtype == "fp8":
        assert audit.e4m3 > 0
    del model, gen, discr
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------- weight decoder
def _bfq(x):
    return x.to(torch.bfloat16).float()


@pytest.mark.parametrize("case", ["fwd", "dgrad_flipped", "s2d_mode1", "s2d_mode2", "fp8"])
def test_weight_pack_decodes_to_its_source(hip, case):
    """mi355_weight_pack's output, decoded by the audit's decoder, is the source element the header names for every GEMM
    index (bf16-rounded; fp8: the e4m3 cast of w * 224 / amax)."""
    from unet_bssfp_amd import ops
    g = torch.Generator().manual_seed(31)
    if case in ("fwd", "fp8"):
        src = torch.randn(40, 24, 3, 3, 3, generator=g)
        geo = dict(cout=40, cin=24, ks=3, s_co=24 * 27, s_ci=27, s_k=(9, 3, 1), tbase=(0, 0, 0), tstep=(1, 1, 1))
        extra = {}
    elif case == "dgrad_flipped":
        src = torch.randn(40, 24, 3, 3, 3, generator=g)
        geo = dict(cout=24, cin=40, ks=3, s_co=27, s_ci=24 * 27, s_k=(9, 3, 1), tbase=(2, 2, 2), tstep=(-1, -1, -1))
        extra = {}
    elif case == "s2d_mode1":                               # k4 s2 p1 weight as the dense k2 weight of S(a), 8 real channels per block
        src = torch.randn(32, 8, 4, 4, 4, generator=g)
        geo = dict(cout=32, cin=8, ks=2, s_co=8 * 64, s_ci=64, s_k=(16, 4, 1), tbase=(0, 0, 0), tstep=(2, 2, 2))
        extra = dict(s2d_mode=1, s2d_cp=16, cinp=128)
    else:                                                   # ConvTranspose3d(k2, s2) [cin][cout][2][2][2]: classes as GEMM columns
        src = torch.randn(32, 64, 2, 2, 2, generator=g)
        geo = dict(cout=64, cin=32, ks=1, s_co=8, s_ci=64 * 8, s_k=(4, 2, 1), tbase=(0, 0, 0), tstep=(0, 0, 0))
        extra = dict(s2d_mode=2, s2d_cp=64, coutp=512)
    srcd = src.to(DEV).contiguous()
    if case == "fp8":
        amax = ops.amax_f32(srcd)
        wp, coutp, cinp = ops.weight_pack(srcd, geo["cout"], geo["cin"], geo["ks"], geo["s_co"], geo["s_ci"], geo["s_k"],
                                          geo["tbase"], geo["tstep"], ops.FP8, q_amax=amax)
    else:
        wp, coutp, cinp = ops.weight_pack(srcd, geo["cout"], geo["cin"], geo["ks"], geo["s_co"], geo["s_ci"], geo["s_k"],
                                          geo["tbase"], geo["tstep"], torch.bfloat16, **extra)
    exp = R.pack_expect(src, geo["cout"], geo["cin"], coutp, cinp, geo["ks"], geo["s_co"], geo["s_ci"], geo["s_k"], geo["tbase"],
                        geo["tstep"], extra.get("s2d_mode", 0), extra.get("s2d_cp", 0))
    taps = geo["ks"] ** 3
    if case == "fp8":
        a = float(amax.cpu()[0])
        got = R.decode_wp(wp.cpu().reshape(-1), R.FP8, cinp, taps, coutp)          # the stored e4m3 values, unscaled
        scale = torch.tensor(224.0, dtype=torch.float32) / torch.tensor(a, dtype=torch.float32)
        assert torch.equal(got, (exp * scale).to(torch.float8_e4m3fn).float())
        assert a == float(src.abs().max())
    else:
        got = R.decode_wp(wp.cpu().reshape(-1), R.BF16, cinp, taps, coutp)
        assert torch.equal(got, _bfq(exp))


def test_upcat_compose_d2s_packing_decodes_to_the_composed_kernel(hip):
    """wp_d2s of mi355_upcat_compose: class b = (bd, bh, bw), tap e <-> kernel index 3 - b - 2 e per axis of k4 [cl][co][4][4][4]."""
    from unet_bssfp_amd import ops
    g = torch.Generator().manual_seed(32)
    cl, cu, ce, co = 32, 16, 16, 32
    wd = torch.randn(cl, cu, 2, 2, 2, generator=g).to(DEV)
    wc = torch.randn(co, ce + cu, 3, 3, 3, generator=g).to(DEV)
    bd = torch.randn(cu, generator=g).to(DEV)
    bc = torch.randn(co, generator=g).to(DEV)
    k4, wp, _, _ = ops.upcat_compose(wd, wc, bd, bc, ce)
    k4 = k4.cpu()
    got = R.decode_wp(wp.cpu().reshape(-1), R.BF16, cl, 8, 8 * co)
    exp = torch.zeros(8, 8 * co, cl)
    for blk in range(8):
        b = ((blk >> 2) & 1, (blk >> 1) & 1, blk & 1)
        for t in range(8):
            e = ((t >> 2) & 1, (t >> 1) & 1, t & 1)
            kk = tuple(3 - 2 * ee - bb for ee, bb in zip(e, b))
            exp[t, blk * co:(blk + 1) * co] = k4[:, :, kk[0], kk[1], kk[2]].t()
    assert torch.equal(got, _bfq(exp))
