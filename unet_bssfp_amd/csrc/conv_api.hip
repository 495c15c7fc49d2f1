// Host dispatch of the implicit-GEMM convolution kernels (C ABI: mi355_conv_fwd).
#include <algorithm>
#include "conv_kernels.h"
#include "conv_march.h"
#include "conv_marchg.h"
#include "conv_march2.h"

namespace {

// Kernel families of the halo plans.  The values are the `shape` digit(s) of mi355_conv_plan_id and may not change (7 and 8
// were experiments -- row reuse inside conv_halo_kernel with register staging: 216 VGPRs or spills, slower -- and 3, a 4x4x32
// tile with 4 subtiles per wave for thin-Cout bf16 layers, was never chosen by the planner; none of the three has a kernel).
enum ConvShape : int {
  kWide = 0,      // conv_halo_kernel 2x4x32, 2 subtiles per wave
  kMid = 1,       // 2x8x16, 2
  kSmall = 2,     // 4x8x8, 2
  kMid1 = 4,      // 2x4x16, 1 subtile per wave   } more workgroups at the low levels
  kSmall1 = 5,    // 2x8x8, 1                     }
  kWide8 = 6,     // 4x4x32, 8 waves x 2 subtiles: 25 % less halo traffic than 2x4x32 at the same occupancy
  kRu = 9,        // conv_ru_kernel: 4x4x32, 4 waves, row-reuse loop, halo by LDS-DMA
  kMarch = 10,    // conv_march_kernel: 16x32 footprint marching along d, 32 input channels resident
  kMarchG = 11,   // conv_marchg_kernel<ROWS>: 4 ROWS x 32 footprint marching along d, input channels in 32-channel groups,
                  //   weights streamed through an LDS ring; vt = ROWS
  kLowG16 = 12,   // conv_lowg_kernel: 512-voxel tiles 4x8x16 x 64 output channels, weights through LDS once per workgroup
  kLowG8 = 13,    //   ... 8x8x8
  kMarch2 = 14,   // conv_march2_kernel<ROWS>: dense 2x2x2 on wide tensors (the PatchGAN on space-to-depth operands); vt = ROWS
};

struct Plan {
  bool halo;
  int shape;      // halo plans: a ConvShape; 0 otherwise
  int vt, ct;
  int tiles_d, tiles_h, tiles_w;
  long long tiles;
  int tiles_per_sample;
  int seg_len, nseg;          // marching kernels: output planes per workgroup segment, segments per sample
  int ksplit, rpb;            // split-K factor (1 = off) and rows per reduce block
  long long stat_rows;        // rows of stats_part ( = tiles, or reduce blocks under split-K )
  bool pointwise, wg_stats;   // persistent 1x1x1 kernel; its statistics as one row per workgroup
  int stat_rows_per_sample;
};

struct Tile { int d, h, w, vt; };     // output voxels of a workgroup's tile, subtiles per wave
Tile tile_of(int shape) {
  switch (shape) {
    case kWide: return {2, 4, 32, 2};
    case kMid: return {2, 8, 16, 2};
    case kSmall: return {4, 8, 8, 2};
    case kMid1: return {2, 4, 16, 1};
    case kSmall1: return {2, 8, 8, 1};
    case kWide8: return {4, 4, 32, 2};
    case kRu: return {4, 4, 32, 4};
    case kLowG16: return {4, 8, 16, 4};
    default: return {8, 8, 8, 4};       // kLowG8 (the marching kernels set their own extents: set_tile_extents)
  }
}

int gcd_i(long long a, long long b) { while (b) { long long t = a % b; a = b; b = t; } return (int)a; }

// Plan overrides for A/B runs (they act only in the diagnostic build): MI355_CONV_SHAPE=<0|6|9|10|11>, MI355_CONV_CT=<1|2>,
// MI355_CONV_KSPLIT=<n>
MI355_PLANNER_CONSTANT(forced_ct, "MI355_CONV_CT", 0)
MI355_PLANNER_CONSTANT(forced_ksplit, "MI355_CONV_KSPLIT", 0)
MI355_PLANNER_CONSTANT(forced_shape, "MI355_CONV_SHAPE", -1)
// planner constants (sweeps: tools/sweep_plan.sh)
MI355_PLANNER_CONSTANT(tune_mg_minwg, "MI355_MG_MINWG", 192)
MI355_PLANNER_CONSTANT(tune_mg_fix, "MI355_MG_FIX", 900)
MI355_PLANNER_CONSTANT(tune_march_minwg, "MI355_MARCH_MINWG", 128)
MI355_PLANNER_CONSTANT(tune_ks_target, "MI355_KS_TARGET", 1024)
MI355_PLANNER_CONSTANT(tune_low_min, "MI355_LOW_MIN", 512)
MI355_PLANNER_CONSTANT(tune_lowg, "MI355_LOWG", 1)                   // 0: the low levels stay on conv_halo_kernel
MI355_PLANNER_CONSTANT(tune_lowg_target, "MI355_LOWG_TARGET", 256)
MI355_PLANNER_CONSTANT(tune_lowg_minch, "MI355_LOWG_MINCH", 4)       // least 16-channel chunks
// widest row the low-level plans take
// (20: the 20^3 level of a 160^3 volume -- BASELINE configs[4] -- is 2.56x its own work in conv_marchg_kernel's 16 x 32 footprints;
//  1x24x160^3 step, interleaved A/B of the diagnostic build: 16 -> 18.45 ms, 20 -> 17.90, 40 -> 18.03: profiles/r04c_ab_160_lowg_maxw.txt)
MI355_PLANNER_CONSTANT(tune_lowg_maxw, "MI355_LOWG_MAXW", 20)
MI355_PLANNER_CONSTANT(tune_gather_split, "MI355_GATHER_SPLIT", 1)

// ------------------------------------------------------------------------------------------------ predicates and searches
bool zero3(const int32_t* v) { return v[0] == 0 && v[1] == 0 && v[2] == 0; }

// Plain output grid with padding p: the grid is y itself (yscale 1; depth-to-space: every yscale-th voxel class of y), unit
// step, no offset, and the same padding p on every side.
bool plain_grid(const mi355_conv_desc* d, int p, int yscale = 1) {
  return d->os == 1 && zero3(d->ooff) && d->pad[0] == p && d->pad[1] == p && d->pad[2] == p &&
         d->dy == yscale * d->do_ && d->hy == yscale * d->ho && d->wy == yscale * d->wo;
}
// ... which is the whole stride-1 output of the input with padding p, stored in 16-byte pieces (the marching kernels' layers)
bool plain_full_grid(const mi355_conv_desc* d, int p) {
  const int grow = 2 * p - (d->ks - 1);
  return plain_grid(d, p) && d->do_ == d->di + grow && d->ho == d->hi + grow && d->wo == d->wi + grow && (d->cstore & 7) == 0;
}

// Fits 32-bit byte offsets: every tensor of the launch (two-byte inputs, y of y_bytes per element, the addend of add_bytes)
bool fits_32bit_offsets(const mi355_conv_desc* d, int y_bytes, int add_bytes) {
  const long long nvi = (long long)d->n * d->di * d->hi * d->wi, nvo = (long long)d->n * d->dy * d->hy * d->wy, lim = 1ll << 31;
  return nvi * d->ld0 * 2 < lim && nvi * (d->c1 ? d->ld1 : 0) * 2 < lim && nvo * d->ldy * y_bytes < lim &&
         (!d->addend || nvo * d->ld_add * add_bytes < lim);
}

// d-segment search of the marching kernels: `depth` output planes are cut into 1 .. 64 segments of len_rule(ceil(depth / ns))
// planes; fp footprints x segments workgroups run in rounds of `round`, each costing cost(len).  Returns the cheapest length
// among the cuts with at least min_wg workgroups (the first of equals: the longest), 0 if there is none.
template <typename LenRule, typename Cost>
int best_segment_len(int depth, long long fp, int round, long long min_wg, LenRule len_rule, Cost cost) {
  long long best = -1; int best_len = 0;
  for (int ns = 1; ns <= depth && ns <= 64; ++ns) {
    const int len = len_rule(ceil_div(depth, ns)), segs = ceil_div(depth, len);
    if (fp * segs < min_wg) continue;
    const long long c = (fp * segs + round - 1) / round * cost(len);
    if (best < 0 || c < best) { best = c; best_len = len; }
  }
  return best_len;
}
int any_len(int len) { return len; }

void set_segments(const mi355_conv_desc* d, Plan* p, int shape, int len, int rows) {
  p->shape = shape;
  p->seg_len = len;
  p->nseg = ceil_div(d->do_, len);
  p->vt = rows;
}

// workgroups of a halo-tile plan
long long count_wgs(const mi355_conv_desc* d, int shape, int ct) {
  const Tile t = tile_of(shape);
  return (long long)ceil_div(d->do_, t.d) * ceil_div(d->ho, t.h) * ceil_div(d->wo, t.w) * d->n * (d->coutp / (32 * ct));
}

// ------------------------------------------------------------------------------------------------ one function per family
// march2, 8-row footprints, two workgroups per CU (512 per round).  Cost per workgroup and 32-channel group: (len + 1) input
// planes of fixed overhead + len output planes of 2 x 4 x 2 ROWS MFMAs (32 per wave).
constexpr int kMarch2Rows = 2;
long long march2_footprints(const mi355_conv_desc* d) {
  return (long long)d->n * ceil_div(d->ho, 4 * kMarch2Rows) * ceil_div(d->wo, 32) * (d->coutp / 32);
}
long long march2_cost(int len) { return (len + 1) * 500ll + (long long)len * 1024; }

// Dense k2 on wide bf16 tensors in whole 32-channel groups, plain output grid, padding 0 (forward on S(a)) or 1 (its data
// gradient): the marching k2 kernel when its footprints x d-segments fill (most of) the chip and the rows are not mostly
// tile padding.
bool plan_march2(const mi355_conv_desc* d, Plan* p) {
  const int pd = d->pad[0];
  const bool ok = d->dtype == MI355_DT_BF16 && d->ks == 2 && d->c0 % 32 == 0 && d->c1 % 32 == 0 && (pd == 0 || pd == 1) &&
                  plain_full_grid(d, pd) && d->wo >= 32 && fits_32bit_offsets(d, d->y_f32 ? 4 : 2, 4) && d->add_n >= 0 &&
                  forced_shape() != 0;
  if (!ok) return false;
  // (rows x columns the tiles cover against the ones that exist: S-layout gradients are 2^k + 1 wide)
  const int th = ceil_div(d->ho, 4 * kMarch2Rows), tw = ceil_div(d->wo, 32);
  if ((long long)th * 8 * tw * 32 * 2 > 3ll * d->ho * d->wo) return false;
  const int len = best_segment_len(d->do_, march2_footprints(d), 512, 128, any_len, march2_cost);
  if (!len) return false;
  set_segments(d, p, kMarch2, len, kMarch2Rows);
  return true;
}

// march2 in depth-to-space mode (transposed k4 s2 p1 convolution): the descriptor asks for this kernel, so it is validated
// instead of tested.  The segment search wants half a round of workgroups; a volume too small for that takes the shortest
// segments on offer (workgroups only grow with the number of segments, so then no cut reaches half a round).
int plan_march2_d2s(const mi355_conv_desc* d, Plan* p) {
  MI355_REQUIRE(d->dtype == MI355_DT_BF16 && d->ks == 2 && d->c0 % 32 == 0 && d->c1 == 0 && d->coutp % 256 == 0 && plain_grid(d, 0, 2) &&
                    d->do_ == d->di && d->ho == d->hi && d->wo == d->wi && d->cstore <= d->coutp / 8 && (d->cstore & 7) == 0 &&
                    !d->y_f32 && d->add_n >= 0,
                "conv: bad depth-to-space descriptor");
  MI355_REQUIRE(fits_32bit_offsets(d, 2, d->add_bf16 ? 2 : 4), "conv: depth-to-space tensors exceed 32-bit byte offsets");
  int len = best_segment_len(d->do_, march2_footprints(d), 512, 256, any_len, march2_cost);
  if (!len) len = ceil_div(d->do_, d->do_ < 64 ? d->do_ : 64);
  set_segments(d, p, kMarch2, len, kMarch2Rows);
  return MI355_OK;
}

// march: <= 32 input channels in one source, plain output grid: the marching kernel, when its footprints x d-segments fill at
// least half the chip (e4m3 operands have no other kernel).
bool plan_march(const mi355_conv_desc* d, Plan* p) {
  const int f = forced_shape();
  if (!(f < 0 || f == kMarch) || !fits_32bit_offsets(d, 2, 4) || d->c1 != 0 || d->c0 != 32 || !plain_full_grid(d, 1)) return false;
  const long long fp = (long long)d->n * ceil_div(d->ho, kMarchFH) * ceil_div(d->wo, kMarchFW) * (d->coutp / 32);
  // segment length L: the grid should be whole 256-workgroup rounds, each workgroup marches L + 2 input planes;
  // L = 2 (mod 3), L >= 5 takes the kernel's straight-line path (conv_march.h), so only such L are proposed
  // unless the volume is too shallow
  const bool deep = d->do_ >= 5;
  const int len = best_segment_len(d->do_, fp, 256, 0,
                                   [deep](int len) { if (deep) { if (len < 5) len = 5; len += (2 - len % 3 + 3) % 3; } return len; },
                                   [](int len) { return (long long)len + 2; });
  if (fp * ceil_div(d->do_, len) < tune_march_minwg() && f != kMarch && d->dtype != MI355_DT_FP8) return false;
  set_segments(d, p, kMarch, len, 4);
  return true;
}

// marchg: more than 32 input channels (whole 32-channel groups per source), plain output grid: the group-marching kernel.
// Cost model per workgroup: (len + 2) input planes of fixed overhead (three block hand-overs per 32-channel group,
// ~900 cycles) + len output planes of MFMA work (54 x 32 cycles per footprint row); ROWS = 4 unless only the
// 8-row footprints can fill the chip.
bool plan_marchg(const mi355_conv_desc* d, Plan* p) {
  const int f = forced_shape();
  if (!(f < 0 || f == kMarchG) || !fits_32bit_offsets(d, 2, 4) || d->dtype != MI355_DT_BF16 || d->c0 % 32 != 0 || d->c1 % 32 != 0 ||
      d->c0 + d->c1 <= 32 || !plain_full_grid(d, 1))
    return false;
  for (int rows = 4; rows >= 2; rows -= 2) {
    const long long fp = (long long)d->n * ceil_div(d->ho, 4 * rows) * ceil_div(d->wo, 32) * (d->coutp / 32);
    const int len = best_segment_len(d->do_, fp, 256, f == kMarchG ? 0 : tune_mg_minwg(), any_len,      // must fill (most of) the chip
                                     [rows](int len) { return (len + 2) * (long long)tune_mg_fix() + (long long)len * 1728 * rows; });
    if (len) { set_segments(d, p, kMarchG, len, rows); return true; }
  }
  return false;
}

// ru / wide8 / wide: wide bf16 3x3x3 layers that do not march: the row-reuse + LDS-DMA kernel when its 4x4x32 tiles fill the
// chip, else 8-wave 4x4x32 tiles / the plain 2x4x32 tile.
int pick_ru_wide8(const mi355_conv_desc* d, int ct) {
  const int f = forced_shape();
  const int wide = count_wgs(d, kWide8, ct) >= 1024 ? kWide8 : kWide;
  const long long c9 = count_wgs(d, kRu, ct);
  int pick = (ct == 1 ? c9 >= 1024 : c9 >= 512) ? kRu : wide;
  if (f == kWide) pick = kWide;
  else if (f == kWide8) pick = wide;
  else if (f == kRu) pick = kRu;
  if (pick == kRu && !fits_32bit_offsets(d, 2, 4)) pick = wide;
  return pick;
}

// the plain wide tile at the 32^3 level
void thin_out_wide(const mi355_conv_desc* d, Plan* p) {
  // one 64-channel tile per workgroup leaves <= 1 workgroup per CU on a long K loop; 32-channel tiles double the
  // workgroups (measured 128->64: 40 -> 30 us, 128->128: 48 -> 41 us)
  if (p->ct == 2 && count_wgs(d, kWide, 2) < 512 && forced_ct() != 2) p->ct = 1;
  // ... and when even that leaves <= 2 workgroups per CU, half-width tiles (2x4x16, one subtile per wave) double
  // them again: -0.1 ms per step in the interleaved A/B (256->128 at 32^3: 98 -> 91 us, 128->64: 31 -> 26 us)
  if (p->ct == 1 && d->ks == 3 && count_wgs(d, kWide, 1) <= 512) p->shape = kMid1;
}

// lowg: low levels in bf16: 512-voxel tiles x 64 output channels, weights through LDS once per workgroup (conv_lowg_kernel)
bool lowg_eligible(const mi355_conv_desc* d) {
  return tune_lowg() && d->dtype == MI355_DT_BF16 && d->ks == 3 && d->coutp % 64 == 0 && (d->c0 + d->c1) >= 16 * tune_lowg_minch() &&
         (long long)d->n * d->do_ * d->ho * d->wo >= 256 && d->wo <= tune_lowg_maxw();
}

// the low-level tiles: few tiles -> favour more, smaller workgroups (the K loop is long, the grid is not)
void plan_low_tiles(const mi355_conv_desc* d, Plan* p) {
  p->shape = d->wo > 8 ? kMid : kSmall;
  if (count_wgs(d, p->shape, p->ct) < tune_low_min()) p->ct = 1;
  if (count_wgs(d, p->shape, p->ct) < tune_low_min()) p->shape = p->shape == kMid ? kMid1 : kSmall1;
}

// tile extents and subtiles of the chosen halo plan
void set_tile_extents(const mi355_conv_desc* d, Plan* p) {
  if (p->shape == kMarch || p->shape == kMarchG || p->shape == kMarch2) {      // (vt = footprint rows / 4 was set with the plan)
    p->ct = 1;
    p->tiles_d = p->nseg;
    p->tiles_h = ceil_div(d->ho, p->shape == kMarch ? kMarchFH : 4 * p->vt);
    p->tiles_w = ceil_div(d->wo, p->shape == kMarch ? kMarchFW : 32);
  } else {
    const Tile t = tile_of(p->shape);
    p->vt = t.vt;
    p->tiles_d = ceil_div(d->do_, t.d);
    p->tiles_h = ceil_div(d->ho, t.h);
    p->tiles_w = ceil_div(d->wo, t.w);
  }
  p->tiles_per_sample = p->tiles_d * p->tiles_h * p->tiles_w;
  p->tiles = (long long)p->tiles_per_sample * d->n;
}

// gather: 128 vt output positions per workgroup, any ks / stride / output grid
void plan_gather(const mi355_conv_desc* d, Plan* p) {
  const long long per = (long long)d->do_ * d->ho * d->wo;
  const long long m = per * d->n;
  p->vt = (m >= 128 * 2 * 512) ? 2 : 1;
  const int wg = 128 * p->vt;
  p->tiles = (m + wg - 1) / wg;
  p->tiles_per_sample = (per % wg == 0) ? (int)(per / wg) : 0;
  p->tiles_d = p->tiles_h = p->tiles_w = 0;
  p->shape = 0;
}

// pointwise: full-resolution 1x1x1 convs with <= 32 channels either side: persistent streaming kernel
bool pointwise_eligible(const mi355_conv_desc* d, const Plan& p) {
  return !p.halo && d->dtype == MI355_DT_BF16 && !d->cls_cout && d->ks == 1 && d->stride == 1 && p.vt == 2 &&
         (d->c0 + d->c1) / 16 <= 2 && d->c1 == 0 && d->coutp == 32 && plain_grid(d, 0);
}

int validate(const mi355_conv_desc* d) {
  MI355_REQUIRE(d && d->x0 && d->wp && d->y, "conv: null pointer");
  MI355_REQUIRE(d->dtype == MI355_DT_F32 || d->dtype == MI355_DT_BF16 || d->dtype == MI355_DT_FP8, "conv: bad dtype %d", d->dtype);
  MI355_REQUIRE(d->dtype != MI355_DT_FP8 || (d->q_amax_x && d->q_amax_w), "conv: fp8 operands need q_amax_x / q_amax_w");
  MI355_REQUIRE(d->c0 > 0 && d->c0 % 16 == 0 && d->c1 >= 0 && d->c1 % 16 == 0, "conv: channels must be multiples of 16 (c0=%d c1=%d)", d->c0, d->c1);
  MI355_REQUIRE(d->c1 == 0 || d->x1, "conv: c1 > 0 without x1");
  MI355_REQUIRE(d->ld0 >= d->c0 && (d->c1 == 0 || d->ld1 >= d->c1), "conv: ld < channels");
  const int epv = d->dtype == MI355_DT_F32 ? 4 : (d->dtype == MI355_DT_FP8 ? 16 : 8);
  MI355_REQUIRE(d->ld0 % epv == 0 && (d->c1 == 0 || d->ld1 % epv == 0), "conv: ld must keep rows 16-byte aligned");
  MI355_REQUIRE(d->coutp > 0 && d->coutp % 32 == 0, "conv: coutp %% 32 != 0");
  MI355_REQUIRE(d->cstore > 0 && d->cstore <= d->coutp && d->ldy >= d->cstore, "conv: bad cstore/ldy");
  MI355_REQUIRE(d->ks >= 1 && d->ks <= 4 && d->stride >= 1 && d->stride <= 2, "conv: unsupported ks=%d stride=%d", d->ks, d->stride);
  MI355_REQUIRE(d->n > 0 && d->di > 0 && d->hi > 0 && d->wi > 0 && d->do_ > 0 && d->ho > 0 && d->wo > 0, "conv: empty extent");
  MI355_REQUIRE(d->os >= 1, "conv: os < 1");
  MI355_REQUIRE(d->cls_cout == 0 || (d->ks == 1 && d->stride == 1 && d->os == 2 && d->cls_cout % 64 == 0 &&
                                     d->coutp == 8 * d->cls_cout && d->cstore <= d->cls_cout && !d->stats_part && zero3(d->ooff)),
                "conv: bad transposed-conv class folding (cls_cout=%d)", d->cls_cout);
  const int hi_off = d->cls_cout ? 1 : 0;     // classes reach offset 1 in every dimension
  MI355_REQUIRE((d->do_ - 1) * d->os + d->ooff[0] + hi_off < d->dy && (d->ho - 1) * d->os + d->ooff[1] + hi_off < d->hy &&
                    (d->wo - 1) * d->os + d->ooff[2] + hi_off < d->wy && d->ooff[0] >= 0 && d->ooff[1] >= 0 && d->ooff[2] >= 0,
                "conv: output grid exceeds the output tensor");
  return MI355_OK;
}

// split the contraction `ks` ways over blockIdx.z; a second kernel combines the partial sums
void set_split(const mi355_conv_desc* d, Plan* p, long long ks) {
  p->ksplit = (int)ks;
  const long long per = (long long)d->do_ * d->ho * d->wo;
  // rows per reduce block: divides the per-sample position count (statistics groups) and leaves >= ~512 blocks
  const long long cblocks = (d->coutp + 1023) / 1024;
  int rpb = 64;
  while (rpb > 1 && (per % rpb != 0 || (per / rpb) * d->n * cblocks < 512)) rpb >>= 1;
  p->rpb = gcd_i(per, rpb);
  p->stat_rows_per_sample = (int)(per / p->rpb);
  p->stat_rows = (long long)p->stat_rows_per_sample * d->n;
}

// Validation, the priority order among the families, and the split-K decision.
int make_plan(const mi355_conv_desc* d, Plan* p) {
  if (int rc = validate(d)) return rc;
  p->ct = (d->coutp % 64 == 0) ? 2 : 1;
  p->seg_len = p->nseg = 0;
  p->halo = ((d->ks == 3 || d->ks == 2) && d->stride == 1);
  if (p->halo) {
    if (forced_ct() == 1) p->ct = 1;
    bool march2 = d->d2s != 0;
    if (march2) { if (int rc = plan_march2_d2s(d, p)) return rc; }
    else march2 = plan_march2(d, p);
    MI355_REQUIRE(march2 || !d->addend, "conv: addend needs the marching k2 plan (bf16, ks 2, 32-channel groups, wide rows)");
    MI355_REQUIRE(d->d2s || (!d->delta && !d->add_bf16), "conv: delta / add_bf16 belong to the depth-to-space mode");
    const bool lowg = lowg_eligible(d);
    if (march2) {                                              // (planned above)
    } else if (d->wo > 16 && !lowg) {                          // the wide levels: march, marchg, then ru / wide8 / wide
      p->shape = kWide;
      if ((d->dtype == MI355_DT_BF16 || d->dtype == MI355_DT_FP8) && d->ks == 3 && !plan_march(d, p) && !plan_marchg(d, p))
        p->shape = pick_ru_wide8(d, p->ct);
      if (p->shape == kWide) thin_out_wide(d, p);
    } else if (lowg) {
      p->shape = d->wo > 8 ? kLowG16 : kLowG8;
      p->ct = 2;
    } else {
      plan_low_tiles(d, p);
    }
    set_tile_extents(d, p);
  } else {
    plan_gather(d, p);
  }
  MI355_REQUIRE(p->halo || (!d->addend && !d->y_f32 && !d->d2s), "conv: addend / y_f32 / d2s need the marching k2 plan");
  MI355_REQUIRE(!d->y_f32 || (p->halo && p->shape == kMarch2), "conv: y_f32 is implemented by the marching k2 kernel");
  MI355_REQUIRE(d->dtype != MI355_DT_FP8 || (p->halo && p->shape == kMarch),
                "conv: the fp8 path covers 3x3x3 stride-1 layers with 32 input channels in one source and a plain output grid");
  MI355_REQUIRE(p->tiles < (1ll << 31), "conv: too many tiles");
  p->ksplit = 1; p->rpb = 0;
  p->stat_rows = p->tiles; p->stat_rows_per_sample = p->tiles_per_sample;
  if (d->d2s) { p->stat_rows *= 8; p->stat_rows_per_sample *= 8; }     // one statistics row per (tile, output class)
  p->pointwise = pointwise_eligible(d, *p);
  p->wg_stats = p->pointwise && d->n == 1 && p->tiles > 2048;       // one statistics row per (persistent) workgroup
  if (p->wg_stats) { p->stat_rows = 2048; p->stat_rows_per_sample = 2048; }
  const long long wgs = p->tiles * (d->coutp / (32 * p->ct));
  const int nchunks = (d->c0 + d->c1) / 16;
  if (!p->halo && !d->cls_cout && d->os == 1 && zero3(d->ooff) && tune_gather_split()) {
    // gather kernel with few output positions and a long contraction (the transposed convolutions' data gradients at the
    // 16^3 / 8^3 levels: 128 dependent (tap, chunk) steps in 32 workgroups, 64 us for 1 GFLOP): split the (tap, chunk) pairs
    const long long nit = (long long)d->ks * d->ks * d->ks * nchunks;
    if (wgs <= 128 && nit >= 32) {
      const long long ks = std::min({(256 + wgs - 1) / wgs, nit / 8, 32ll});
      if (ks >= 2) set_split(d, p, ks);
    }
  }
  if (p->halo && p->shape != kMarch && p->shape != kMarchG && p->shape != kMarch2) {      // (the marching kernels walk the whole contraction themselves)
    // few output positions and a long contraction (8^3 / 16^3 U-Net levels, low PatchGAN levels): the
    // grid cannot fill 256 CUs and every workgroup streams its weights at one L2/HBM latency per tap
    // group => split the contraction over blockIdx.z and combine in a second kernel
    const int fk = forced_ksplit();
    const bool lowg = p->shape == kLowG16 || p->shape == kLowG8;       // one workgroup per CU: aim at 256 of them, down to one chunk each
    if ((fk == 0 && (lowg ? wgs < tune_lowg_target() : ((wgs < 256 && nchunks >= 8) || (wgs <= 512 && nchunks >= 16)))) || fk > 1) {   // (32^3 x 128 ch measured slower split)
      // low-level plan: the LARGEST split that still fits one round of tune_lowg_target() workgroups (rounded up, 60 workgroups -- the
      // 20^3 level of a 160^3 volume -- became 5 x 60 = 300: a second round for 44 of them; 24 at 10^3 became 264).  Same splits as
      // before wherever the count divides 256 (every low level of a 128^3 or 64^3 volume); 160^3: 17.99 -> 17.67 ms with the target
      // swept to the same effect (profiles/r04c_ab_lowg_target.txt)
      long long ks = lowg ? std::max(1ll, (long long)tune_lowg_target() / wgs) : (tune_ks_target() + wgs - 1) / wgs;
      if (fk > 1) ks = fk;
      ks = std::min({ks, (long long)(lowg ? nchunks : nchunks / 2), 32ll});
      if (ks >= 2) set_split(d, p, ks);
    }
  }
  return MI355_OK;
}

// ------------------------------------------------------------------------------------------------ launches
template <typename T, int KS, int TD, int TH, int TW>
void launch_halo_tile(const ConvArgs& a, int ct, dim3 grid, hipStream_t st) {
  if (ct == 2) conv_halo_kernel<T, KS, TD, TH, TW, 2><<<grid, dim3(256), conv_halo_lds<T, KS, TD, TH, TW, 2, 4>(), st>>>(a);
  else conv_halo_kernel<T, KS, TD, TH, TW, 1><<<grid, dim3(256), conv_halo_lds<T, KS, TD, TH, TW, 1, 4>(), st>>>(a);
}

template <typename T, int KS>
int launch_halo_tiles(const ConvArgs& a, const Plan& p, dim3 grid, hipStream_t st) {
  switch (p.shape) {
    case kWide: launch_halo_tile<T, KS, 2, 4, 32>(a, p.ct, grid, st); break;
    case kMid: launch_halo_tile<T, KS, 2, 8, 16>(a, p.ct, grid, st); break;
    case kSmall: launch_halo_tile<T, KS, 4, 8, 8>(a, p.ct, grid, st); break;
    case kMid1: launch_halo_tile<T, KS, 2, 4, 16>(a, p.ct, grid, st); break;
    case kSmall1: launch_halo_tile<T, KS, 2, 8, 8>(a, p.ct, grid, st); break;
    default: mi355_set_error("conv: no kernel for plan %d/%d", p.shape, p.ct); return MI355_ERR_UNSUPPORTED;
  }
  return MI355_OK;
}

// the families that exist for two-byte operands only (the planner admits no other type to them)
int launch_halo_bf16(const mi355_conv_desc* d, const Plan& p, const ConvArgs& a, dim3 grid, hipStream_t st) {
  const dim3 block(256);
  switch (p.shape) {
    case kWide8: {
      constexpr int lds = conv_halo_lds<bf16_t, 3, 4, 4, 32, 2, 8>();
      if (p.ct == 2) conv_halo_kernel<bf16_t, 3, 4, 4, 32, 2, 8><<<grid, dim3(512), lds, st>>>(a);
      else conv_halo_kernel<bf16_t, 3, 4, 4, 32, 1, 8><<<grid, dim3(512), lds, st>>>(a);
      break;
    }
    case kRu:
      if (p.ct == 2) conv_ru_kernel<2><<<grid, block, kRuLds, st>>>(a);
      else conv_ru_kernel<1><<<grid, block, kRuLds, st>>>(a);
      break;
    case kMarch: {
      const MarchArgs m{p.seg_len, p.nseg, p.tiles_h, p.tiles_w, d->q_amax_x, d->q_amax_w};
      if (d->dtype == MI355_DT_FP8) {
        if (int rc = raise_lds_limit<conv_march_kernel<true>>("conv_march", MarchCfg<true>::LDS)) return rc;
        conv_march_kernel<true><<<grid, block, MarchCfg<true>::LDS, st>>>(a, m);
      } else {
        if (int rc = raise_lds_limit<conv_march_kernel<false>>("conv_march", MarchCfg<false>::LDS)) return rc;
        conv_march_kernel<false><<<grid, block, MarchCfg<false>::LDS, st>>>(a, m);
      }
      break;
    }
    case kMarchG: {
      const MarchArgs m{p.seg_len, p.nseg, p.tiles_h, p.tiles_w, nullptr, nullptr};
      if (p.vt == 4) {
        if (int rc = raise_lds_limit<conv_marchg_kernel<4>>("conv_marchg", MarchGCfg<4>::LDS)) return rc;
        conv_marchg_kernel<4><<<grid, block, MarchGCfg<4>::LDS, st>>>(a, m);
      } else {
        if (int rc = raise_lds_limit<conv_marchg_kernel<2>>("conv_marchg", MarchGCfg<2>::LDS)) return rc;
        conv_marchg_kernel<2><<<grid, block, MarchGCfg<2>::LDS, st>>>(a, m);
      }
      break;
    }
    case kLowG16:
      if (int rc = raise_lds_limit<conv_lowg_kernel<4, 8, 16>>("conv_lowg", LowGCfg<4, 8, 16>::LDS)) return rc;
      conv_lowg_kernel<4, 8, 16><<<grid, block, LowGCfg<4, 8, 16>::LDS, st>>>(a);
      break;
    case kLowG8:
      if (int rc = raise_lds_limit<conv_lowg_kernel<8, 8, 8>>("conv_lowg", LowGCfg<8, 8, 8>::LDS)) return rc;
      conv_lowg_kernel<8, 8, 8><<<grid, block, LowGCfg<8, 8, 8>::LDS, st>>>(a);
      break;
    default: {      // kMarch2
      const March2Args m{p.seg_len, p.nseg, p.tiles_h, p.tiles_w, d->addend, d->ld_add, d->y_f32, d->add_n, d->add_bf16, d->delta};
      if (d->d2s) {
        if (int rc = raise_lds_limit<conv_march2_kernel<kMarch2Rows, true>>("conv_march2", March2Cfg<kMarch2Rows>::LDS)) return rc;
        conv_march2_kernel<kMarch2Rows, true><<<grid, block, March2Cfg<kMarch2Rows>::LDS, st>>>(a, m);
      } else {
        if (int rc = raise_lds_limit<conv_march2_kernel<kMarch2Rows, false>>("conv_march2", March2Cfg<kMarch2Rows>::LDS)) return rc;
        conv_march2_kernel<kMarch2Rows, false><<<grid, block, March2Cfg<kMarch2Rows>::LDS, st>>>(a, m);
      }
    }
  }
  return MI355_OK;
}

template <typename T>
int launch(const mi355_conv_desc* d, const Plan& p, hipStream_t st) {
  ConvArgs a;
  a.x0 = (const char*)d->x0; a.x1 = (const char*)d->x1;
  a.c0 = d->c0; a.c1 = d->c1; a.ld0 = d->ld0; a.ld1 = d->ld1;
  a.n = d->n; a.di = d->di; a.hi = d->hi; a.wi = d->wi;
  a.do_ = d->do_; a.ho = d->ho; a.wo = d->wo;
  a.ks = d->ks; a.stride = d->stride;
  a.pd = d->pad[0]; a.ph = d->pad[1]; a.pw = d->pad[2];
  a.wp = (const char*)d->wp; a.coutp = d->coutp; a.bias = d->bias;
  a.y = (char*)d->y; a.ldy = d->ldy; a.cstore = d->cstore;
  a.dy = d->dy; a.hy = d->hy; a.wy = d->wy; a.os = d->os;
  a.od = d->ooff[0]; a.oh = d->ooff[1]; a.ow = d->ooff[2];
  a.stats = d->stats_part;
  a.tiles_d = p.tiles_d; a.tiles_h = p.tiles_h; a.tiles_w = p.tiles_w;
  a.nchunks = (d->c0 + d->c1) / 16;
  a.m_total = (long long)d->n * d->do_ * d->ho * d->wo;
  a.ksplit = p.ksplit;
  a.cls_cout = d->cls_cout;
  a.nbias = d->nbias > 0 ? d->nbias : d->coutp;
  a.kslab = (float*)d->workspace;
  if (p.ksplit > 1) {
    const long long need = (long long)p.ksplit * a.m_total * d->coutp * 4;
    MI355_REQUIRE(d->workspace && d->workspace_bytes >= need, "conv: split-K workspace too small (%lld < %lld)",
                  (long long)d->workspace_bytes, need);
  }
  const dim3 grid((unsigned)p.tiles, (unsigned)(d->coutp / (32 * p.ct)), (unsigned)p.ksplit), block(256);
  constexpr bool two_byte = sizeof(T) == 2;
  if (p.halo) {
    int rc = MI355_OK;
    if (p.shape <= kSmall1) rc = d->ks == 3 ? launch_halo_tiles<T, 3>(a, p, grid, st) : launch_halo_tiles<T, 2>(a, p, grid, st);
    else if constexpr (two_byte) rc = launch_halo_bf16(d, p, a, grid, st);
    if (rc) return rc;
  } else if (two_byte && p.pointwise) {
    const int ntiles = (int)p.tiles;
    const dim3 g1((unsigned)(ntiles < 2048 ? ntiles : 2048));
    if (a.nchunks == 1) pointwise_conv_kernel<1><<<g1, block, 0, st>>>(a, ntiles, p.wg_stats ? 1 : 0);
    else pointwise_conv_kernel<2><<<g1, block, 0, st>>>(a, ntiles, p.wg_stats ? 1 : 0);
  } else if (two_byte && d->cls_cout && p.vt == 2 && a.nchunks <= 8 && d->c1 == 0 && (d->cstore & 7) == 0) {
    // transposed-conv forward, Cin <= 128: one workgroup per 256 voxels loops over all column blocks
    const dim3 g1((unsigned)p.tiles);
    if (a.nchunks <= 4) deconv_fwd_kernel<4><<<g1, block, 0, st>>>(a);
    else deconv_fwd_kernel<8><<<g1, block, 0, st>>>(a);
  } else {
    if (p.vt == 2) {
      if (p.ct == 2) conv_gather_kernel<T, 2, 2><<<grid, block, 0, st>>>(a);
      else conv_gather_kernel<T, 2, 1><<<grid, block, 0, st>>>(a);
    } else {
      if (p.ct == 2) conv_gather_kernel<T, 1, 2><<<grid, block, 0, st>>>(a);
      else conv_gather_kernel<T, 1, 1><<<grid, block, 0, st>>>(a);
    }
  }
  if (p.ksplit > 1) {
    int rc = mi355_check_launch("conv_fwd");
    if (rc) return rc;
    conv_ksplit_reduce_kernel<T><<<dim3((unsigned)p.stat_rows, (unsigned)((d->coutp + 1023) / 1024)), dim3(256), 0, st>>>(a, p.rpb);
    return mi355_check_launch("conv_ksplit_reduce");
  }
  return mi355_check_launch("conv_fwd");
}

}  // namespace

extern "C" int mi355_conv_plan_id(const mi355_conv_desc* d) {
  Plan p;
  int rc = make_plan(d, &p);
  if (rc) return rc;
  return 10000 * d->ks + 1000 * (p.halo ? 1 : 0) + 100 * p.shape + 10 * p.vt + p.ct;
}

extern "C" int mi355_conv_plan_seg_len(const mi355_conv_desc* d) {
  Plan p;
  int rc = make_plan(d, &p);
  if (rc) return rc;
  return p.seg_len;
}

extern "C" int mi355_conv_num_tiles(const mi355_conv_desc* d, int32_t* tiles, int32_t* tiles_per_sample) {
  Plan p;
  int rc = make_plan(d, &p);
  if (rc) return rc;
  if (tiles) *tiles = (int32_t)p.stat_rows;
  if (tiles_per_sample) *tiles_per_sample = p.stat_rows_per_sample;
  return MI355_OK;
}

extern "C" int64_t mi355_conv_workspace_bytes(const mi355_conv_desc* d) {
  Plan p;
  if (make_plan(d, &p)) return -1;
  if (p.ksplit <= 1) return 0;
  return (int64_t)p.ksplit * d->n * d->do_ * d->ho * d->wo * d->coutp * 4;
}

extern "C" int mi355_conv_fwd(const mi355_conv_desc* d, void* stream) {
  Plan p;
  int rc = make_plan(d, &p);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == MI355_DT_F32) return launch<float>(d, p, st);
  return launch<bf16_t>(d, p, st);
}
