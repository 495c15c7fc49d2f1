"""The cases of the weight-gradient bit pin: tools/gen_golden_wgrad_bits.py records them, tests/test_wgrad_bits_gpu.py replays them
and tests/test_wgrad_bits_host.py checks on the host that every case still lands on the kernel it exists for.  Each of the six
slab-writing kernel families of csrc/wgrad*.h and each slab-reduction form runs at the smallest shape where its edges are live
(partial tiles, footprints and segments, channel tails on either operand, both x sources of a concatenation, unequal stage
counts), and dw is reduced to the SHA-256 of its bytes plus its f64 sum and absolute maximum.

Inputs come from the integer hash ``values`` of medicalnet_bits_cases (no RNG); every call runs on poisoned fresh memory
(tests/alloc_poison.py), so a slab element that is read without having been written moves the hash.

A case is (name, dtype, n, x extent, c0, c1, cg, ks, stride, pad, descriptor extras, plan kind, slabs).  The slab count is what
mi355_conv_wgrad_workspace implies; with it the rules of make_reduce_job (csrc/wgrad_reduce.h) fix the reduction form named in
the row's comment -- the C ABI does not expose the form."""
import ctypes as C

import torch

import conv_plan_cases as P
from alloc_poison import poisoned
from medicalnet_bits_cases import DEV, digest, values

F32, BF16 = "f32", "bf16"
GENERIC, TILE, MARCH, POINTWISE, MARCH2 = 0, 1, 2, 3, 4          # mi355_conv_wgrad_plan_kind
S2D_GEO = dict(s_k=(16, 4, 1), s_ci=64, tstep=(2, 2, 2))          # dw[co][c][4][4][4] behind a dense k2 on a space-to-depth operand
DENSE = dict(cin_less=6, cout=500)                                # real extents below the padded ones: nci and cout tails

CASES = [
    # ---- wgrad_kernel<T, KS, TPW>
    ("generic_f32_k3", F32, 2, (3, 5, 9), 32, 16, 16, 3, 1, 1, {}, GENERIC, 32),                   # generic reduce (32 x 8)
    ("generic_k4s2", BF16, 2, (6, 8, 10), 16, 0, 32, 4, 2, 1, {}, GENERIC, 24),                    # generic reduce
    ("generic_k3s2", BF16, 2, (5, 7, 9), 32, 0, 16, 3, 2, 1, {}, GENERIC, 24),                     # generic reduce (> 16 slabs)
    ("generic_gs2", BF16, 2, (4, 5, 9), 16, 0, 16, 2, 1, 0, dict(gs=2, goff=(1, 0, 1)), GENERIC, 24),   # generic reduce
    # (a bf16 k1 on g's own grid is a tile plan: g holds one plane more than the grid, which keeps the case on wgrad_kernel<.., 1, 1>)
    ("generic_xn", BF16, 4, (3, 4, 9), 16, 0, 16, 1, 1, 0, dict(xn=2, g_ext=(4, 4, 9)), GENERIC, 48),  # generic reduce (< 128 slabs)
    # ---- wgrad_bf16_kernel<KS, TD, TH, TW>
    ("tile_k3_w32", BF16, 2, (3, 5, 19), 32, 32, 48, 3, 1, 1, {}, TILE, 8),                        # dense 27 taps, 2 channels per block
    ("tile_k3_w16", BF16, 2, (3, 9, 7), 16, 0, 16, 3, 1, 1, {}, TILE, 8),                          # dense 27 taps, 2 channels per block
    ("tile_k1", BF16, 2, (3, 5, 19), 48, 0, 16, 1, 1, 0, {}, TILE, 32),                            # generic reduce (> 16 slabs)
    ("tile_k2_p0", BF16, 2, (4, 6, 20), 32, 0, 32, 2, 1, 0, {}, TILE, 8),                          # generic reduce (k2)
    ("tile_k2_p1", BF16, 2, (3, 5, 7), 16, 0, 16, 2, 1, 1, {}, TILE, 4),                           # generic reduce (k2)
    ("tile_s2d", BF16, 1, (5, 5, 9), 64, 0, 32, 2, 1, 0, dict(s2d_cp=8, cin=6, **S2D_GEO), TILE, 2),     # s2d reduce, partial channel block
    ("dense27_8", BF16, 1, (4, 4, 4), 256, 0, 512, 3, 1, 1, DENSE, TILE, 2),                       # dense 27 taps, 8 channels per block
    ("dense27_4", BF16, 1, (4, 4, 4), 128, 0, 512, 3, 1, 1, DENSE, TILE, 2),                       # dense 27 taps, 4 channels per block
    ("dense1_8", BF16, 1, (4, 4, 4), 256, 0, 512, 1, 1, 0, DENSE, TILE, 8),                        # dense 1 tap, 8 channels per block
    ("dense1_4", BF16, 1, (4, 4, 4), 128, 0, 512, 1, 1, 0, DENSE, TILE, 8),                        # dense 1 tap, 4 channels per block
    ("cls_small", BF16, 2, (3, 5, 6), 32, 0, 32, 1, 1, 0, dict(g_cls_cout=32), TILE, 16),          # generic reduce, class scatter
    # ---- wgrad_deconv_kernel
    ("cls_deconv4", BF16, 2, (2, 4, 32), 64, 0, 32, 1, 1, 0, dict(g_cls_cout=32), TILE, 8),        # generic reduce, class scatter
    ("cls_deconv4_two_tiles", BF16, 2, (4, 8, 64), 64, 0, 32, 1, 1, 0, dict(g_cls_cout=32), TILE, 64),   # generic reduce, class scatter
    # ---- the marching kernels: two d-segments (5 + 4 planes; 3 + 2), partial h and w footprints
    ("march", BF16, 2, (9, 9, 33), 32, 16, 48, 3, 1, 1, {}, MARCH, 16),                            # dense 27 taps, 2 channels per block
    ("march2", BF16, 2, (6, 10, 34), 32, 0, 48, 2, 1, 0, {}, MARCH2, 16),                          # generic reduce (k2)
    # ---- wgrad_pw_kernel: 135 135 voxels = 2111 stages of 64 and one of 31 over 1024 waves, which run 3 or 2 stages each
    ("pointwise_16_32", BF16, 1, (33, 63, 65), 16, 0, 32, 1, 1, 0, {}, POINTWISE, 256),            # narrow generic reduce (8 x 32)
    ("pointwise_32_16", BF16, 1, (33, 63, 65), 32, 0, 16, 1, 1, 0, {}, POINTWISE, 256),            # narrow generic reduce (8 x 32)
]
NAMES = tuple(c[0] for c in CASES)
WAYS = ("set", "accumulate", "set_deferred", "accumulate_deferred")


class Case:
    def __init__(self, row):
        (self.name, self.dtype, self.n, self.ext, self.c0, self.c1, self.cg, self.ks, self.stride, self.pad, extra, self.kind,
         self.nslabs) = row
        extra = dict(extra)
        self.geo = {k: extra.pop(k) for k in ("s_k", "s_ci", "tstep") if k in extra}
        if "cin_less" in extra:
            extra["cin"] = self.c0 + self.c1 - extra.pop("cin_less")
        self.extra = extra

    def desc(self):
        """the descriptor with dummy pointers (the planner reads no memory) and this case's dw geometry"""
        d = P.wgrad_desc(self.n, self.ext, self.c0, self.c1, self.cg, self.ks, self.stride, self.pad, P.F32 if self.dtype == F32 else P.BF16,
                         **({"g_ext": tuple(2 * e for e in self.ext)} if self.extra.get("g_cls_cout") else {}), **self.extra)
        if self.extra.get("g_cls_cout"):                         # dw[ci][co][2][2][2]: the class picks the tap
            d.s_co, d.s_ci = 8, d.cout * 8
            d.s_k, d.tstep = (C.c_int64 * 3)(4, 2, 1), (C.c_int32 * 3)(0, 0, 0)
        if self.geo:
            d.s_ci = self.geo["s_ci"]
            d.s_co = d.cin * d.s_ci
            d.s_k, d.tstep = (C.c_int64 * 3)(*self.geo["s_k"]), (C.c_int32 * 3)(*self.geo["tstep"])
        return d

    def slab_bytes(self, d):
        cinp = (d.c0 + d.c1 + 31) // 32 * 32
        coutp = 8 * d.g_cls_cout if d.g_cls_cout else (d.cg + 31) // 32 * 32
        return d.ks ** 3 * cinp * coutp * 4


def case(name):
    return Case(CASES[NAMES.index(name)])


def run(name, kind="nan"):
    """[(name/way, (sha256, sum, absmax))] for the four WAYS: ops.conv_wgrad into a dw pre-filled with NaN (accumulate=False) and
    with 0.5 (accumulate=True), at once and through defer= with one ops.wgrad_reduce_multi for both.  kind: the poison."""
    from unet_bssfp_amd import ops
    c = case(name)
    d = c.desc()
    dt = torch.float32 if c.dtype == F32 else torch.bfloat16
    salt = 200 + 4 * NAMES.index(name)
    xn = d.xn if d.xn else d.n
    x0 = values((xn, d.di, d.hi, d.wi, d.c0), salt).to(dt).to(DEV)
    x1 = values((xn, d.di, d.hi, d.wi, d.c1), salt + 1).to(dt).to(DEV) if d.c1 else None
    g = values((d.n, d.gd, d.gh, d.gw, d.cg), salt + 2).to(dt).to(DEV)
    k = d.ks if not c.geo else 4
    shape = (d.cin, d.cout, 2, 2, 2) if d.g_cls_cout else (d.cout, d.cin, k, k, k)

    def call(accumulate, defer):
        dw = torch.full(shape, 0.5 if accumulate else float("nan"), dtype=torch.float32, device=DEV)
        ops.conv_wgrad(x0, x1, g, (d.do_, d.ho, d.wo), d.gs, tuple(d.goff), d.ks, d.stride, tuple(d.pad), dw, d.cout, d.cin, d.s_co,
                       d.s_ci, tuple(d.s_k), tuple(d.tbase), tuple(d.tstep), accumulate=accumulate, s2d_cp=d.s2d_cp,
                       g_cls_cout=d.g_cls_cout, n=d.n, defer=defer)
        return dw
    with poisoned(kind):
        jobs = []
        out = [call(False, None), call(True, None), call(False, jobs), call(True, jobs)]
        assert len(jobs) == 2
        ops.wgrad_reduce_multi(jobs)
        torch.cuda.synchronize()
    return [(f"{name}/{way}", digest(t)) for way, t in zip(WAYS, out)]
