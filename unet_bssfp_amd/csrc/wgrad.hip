// Weight gradient of the implicit-GEMM convolutions (C ABI: mi355_conv_wgrad, mi355_conv_wgrad_partial, mi355_wgrad_reduce_multi).
//   dw[tap][ci][co] = sum_{n,p} x[n, p*stride + tap - pad, ci] * g[n, p*gs + goff, co]
// Two passes.  A slab-writing kernel computes, per 32 x 32 (ci, co) tile, partial sums over disjoint sets of output positions into
// f32 slabs [tap][cinp][coutp] of the workspace; a reduction adds the slabs in a fixed order (deterministic) and scatters into the
// torch weight layout, at once or -- mi355_conv_wgrad_partial -- later, for many layers in one launch.  The kernels live in the
// wgrad_*.h headers by family; this file is their translation unit: planner (wplan), one launch function per kind, C entry points.
#include "wgrad_tile.h"
#include "wgrad_march.h"
#include "wgrad_pw.h"
#include "wgrad_reduce.h"
#include <cstring>
#include <vector>
namespace {
// which kernel writes the slabs: the values mi355_conv_wgrad_plan_kind returns
enum WKind : int {
  kWGeneric = 0,   // wgrad_kernel: any dtype / ks / stride / g grid
  kWTile = 1,      // wgrad_bf16_kernel (deconv4: wgrad_deconv_kernel): bf16, stride 1, g on the grid of the outputs
  kWMarch = 2,     // wgrad_march_kernel: 3x3x3, padding 1, same extents, wide rows
  kWPointwise = 3, // wgrad_pw_kernel: streaming 1x1x1, one (ci, co) tile
  kWMarch2 = 4,    // wgrad_march2_kernel: dense 2x2x2, padding 0, wide rows
};

struct WPlan { int ks, tpw, tap_groups, ci_tiles, co_tiles, splits, cinp32, coutp32; long long rows;
               int kind; bool deconv4; int shape, tiles_d, tiles_h, tiles_w, ntiles, nslabs;
               int seg_len, nseg; long long nv; };          // nv: voxels of x
constexpr int kWTD[2] = {2, 2}, kWTH[2] = {4, 8}, kWTW[2] = {32, 16};       // the tile shapes of wgrad_bf16_kernel
// planner constant of the tile path as a diagnostic-build knob (tools/sweep_plan.sh)
MI355_PLANNER_CONSTANT(tune_wg_target, "MI355_WG_TARGET", 512)
constexpr long long kSlabCap = 256ll << 20;        // the slab workspace stays below ~256 MiB

// d-segments of the two marching kernels (th x tw footprints per sample): the depth is cut into 1 .. depth / min_len segments of
// ceil(depth / ns) planes (cuts whose last segment would be empty are skipped); whole rounds of 256 workgroups (one per CU),
// cost = rounds x (planes per segment + pipeline fill); one slab per footprint and segment, under the workspace cap.
void set_wgrad_segments(const mi355_wgrad_desc* d, WPlan* p, int th, int tw, int min_len, long long slab_bytes) {
  const long long fp = (long long)d->n * th * tw, base = fp * p->ci_tiles * p->co_tiles;
  long long best = -1; int best_ns = 1;
  for (int ns = 1; ns <= d->do_ / min_len; ++ns) {
    const int L = ceil_div(d->do_, ns);
    if ((long long)(ns - 1) * L >= d->do_) continue;
    const long long wgs = base * ns, cost = ((wgs + 255) / 256) * (L + 3);
    if (ns * fp * slab_bytes > kSlabCap) break;
    if (best < 0 || cost < best) { best = cost; best_ns = ns; }
  }
  p->nseg = best_ns;
  p->seg_len = ceil_div(d->do_, best_ns);
  p->tiles_h = th; p->tiles_w = tw;
  p->nslabs = d->n * th * tw * best_ns;
}

int wplan(const mi355_wgrad_desc* d, WPlan* p) {
  MI355_REQUIRE(d && d->x0 && d->g && d->dw, "wgrad: null pointer");
  MI355_REQUIRE(d->dtype == MI355_DT_F32 || d->dtype == MI355_DT_BF16, "wgrad: bad dtype");
  MI355_REQUIRE(d->ks >= 1 && d->ks <= 4, "wgrad: unsupported ks=%d", d->ks);
  MI355_REQUIRE(d->c0 > 0 && d->c0 % 16 == 0 && d->c1 % 16 == 0 && d->cg % 16 == 0, "wgrad: channels must be multiples of 16");
  MI355_REQUIRE(d->c1 == 0 || (d->x1 && d->c0 % 32 == 0), "wgrad: concat split must be a multiple of 32");
  MI355_REQUIRE(d->cin <= d->c0 + d->c1 && d->cout <= d->cg, "wgrad: real extents exceed padded ones");
  MI355_REQUIRE(d->s2d_cp == 0 || (d->s2d_cp % 8 == 0 && d->c1 == 0 && d->c0 == 8 * d->s2d_cp && d->cin <= d->s2d_cp),
                "wgrad: bad space-to-depth operand");
  MI355_REQUIRE(d->xn >= 0 && (d->xn == 0 || d->n % d->xn == 0), "wgrad: xn must divide n");
  *p = WPlan{};                 // kind kWGeneric
  p->ks = d->ks;
  p->tpw = d->ks == 1 ? 1 : (d->ks == 3 ? 9 : 8);
  const int nt = d->ks * d->ks * d->ks;
  p->tap_groups = (nt + p->tpw - 1) / p->tpw;
  p->cinp32 = ((d->c0 + d->c1 + 31) / 32) * 32;
  p->coutp32 = d->g_cls_cout > 0 ? 8 * d->g_cls_cout : ((d->cg + 31) / 32) * 32;
  p->ci_tiles = p->cinp32 / 32;
  p->co_tiles = p->coutp32 / 32;
  p->rows = (long long)d->n * d->do_ * d->ho;
  p->nv = (long long)d->n * d->di * d->hi * d->wi;
  long long wgs = (long long)p->ci_tiles * p->co_tiles * p->tap_groups;
  long long s = 2048 / wgs;
  if (s < 1) s = 1;
  const long long max_s = (p->rows + 3) / 4;
  if (s > max_s) s = max_s;
  const long long slab_bytes = (long long)nt * p->cinp32 * p->coutp32 * 4;
  while (s > 1 && s * 4 * slab_bytes > kSlabCap) s /= 2;
  p->splits = (int)s;
  p->nslabs = p->splits * 4;
  // tile path: bf16, stride 1, g on the same grid as the outputs
  const bool cls = d->g_cls_cout > 0;
  MI355_REQUIRE(!cls || (d->dtype == MI355_DT_BF16 && d->ks == 1 && d->stride == 1 && d->g_cls_cout % 32 == 0 &&
                         d->cg >= d->g_cls_cout && d->gd == 2 * d->do_ && d->gh == 2 * d->ho && d->gw == 2 * d->wo &&
                         d->c1 == 0 && d->cout <= d->g_cls_cout),
                "wgrad: bad transposed-conv class folding");
  const bool tile = d->dtype == MI355_DT_BF16 && d->stride == 1 && d->ld0 % 8 == 0 && (d->c1 == 0 || d->ld1 % 8 == 0) && d->ldg % 8 == 0 &&
                    (cls || (d->ks <= 3 && d->gs == 1 && d->goff[0] == 0 && d->goff[1] == 0 && d->goff[2] == 0 &&
                             d->gd == d->do_ && d->gh == d->ho && d->gw == d->wo));
  if (!tile) return MI355_OK;
  p->kind = kWTile;
  p->shape = d->wo > 16 ? 0 : 1;
  p->tiles_d = ceil_div(d->do_, kWTD[p->shape]);
  p->tiles_h = ceil_div(d->ho, kWTH[p->shape]);
  p->tiles_w = ceil_div(d->wo, kWTW[p->shape]);
  p->ntiles = p->tiles_d * p->tiles_h * p->tiles_w * d->n;
  const int wsl = d->ks == 1 ? 4 : 1;                     // slabs per workgroup
  // transposed conv at the wide levels: 4 column tiles per workgroup (wgrad_deconv_kernel)
  p->deconv4 = cls && p->shape == 0 && p->co_tiles % kDeconvNco == 0 && d->do_ % 2 == 0 && d->ho % 4 == 0 && d->wo % 32 == 0;
  const long long cot = p->deconv4 ? p->co_tiles / kDeconvNco : p->co_tiles;
  long long sp = tune_wg_target() / ((long long)p->ci_tiles * cot);      // ~2 workgroups per CU (256, 1024 measured slower)
  if (sp < 1) sp = 1;
  if (sp > p->ntiles) sp = p->ntiles;
  while (sp > 1 && sp * wsl * slab_bytes > kSlabCap) sp /= 2;
  p->splits = (int)sp;
  p->nslabs = d->ks == 1 ? p->splits * 4 : p->splits;
  if (cls) return MI355_OK;
  // the refinements of the tile path address with 32-bit byte offsets (the first two take one x tensor: ld1 counts for the third only)
  const bool off32 = p->nv * std::max(d->ld0, d->ldg) * 2 < (1ll << 31), off32_x1 = off32 && p->nv * d->ld1 * 2 < (1ll << 31);
  const bool pad0 = d->pad[0] == 0 && d->pad[1] == 0 && d->pad[2] == 0, pad1 = d->pad[0] == 1 && d->pad[1] == 1 && d->pad[2] == 1;
  if (d->ks == 1 && d->c1 == 0 && d->c0 <= 32 && d->cg <= 32 && pad0 && d->di == d->do_ && d->hi == d->ho && d->wi == d->wo &&
      d->s2d_cp == 0 && d->xn == 0 && p->nv >= (1ll << 17) && off32) {
    // streaming 1x1x1 kernel: one (ci, co) tile, plain tensors on one grid, many voxels
    p->kind = kWPointwise;
    p->splits = 256;
    p->nslabs = 256;
  } else if (d->ks == 2 && d->c1 == 0 && pad0 && d->di == d->do_ + 1 && d->hi == d->ho + 1 && d->wi == d->wo + 1 && d->wo >= 32 &&
             d->do_ >= 4 && d->xn == 0 && off32) {
    // marching k2 kernel: dense 2x2x2, padding 0, x one larger than the grid, wide rows
    p->kind = kWMarch2;
    set_wgrad_segments(d, p, ceil_div(d->ho, kW2FH), ceil_div(d->wo, kW2FW), 2, slab_bytes);
  } else if (d->ks == 3 && pad1 && d->di == d->do_ && d->hi == d->ho && d->wi == d->wo && d->wo >= 32 && d->do_ >= 8 && off32_x1) {
    // marching kernel: 3x3x3, padding 1, same extents, wide rows
    p->kind = kWMarch;
    set_wgrad_segments(d, p, ceil_div(d->ho, kWmFH), ceil_div(d->wo, kWmFW), 4, slab_bytes);
  }
  return MI355_OK;
}

// ---- one launch function per kind
template <typename T>
void launch_generic(const WgradArgs& a, const WPlan& p, hipStream_t st) {
  dim3 grid(p.splits, p.ci_tiles, p.co_tiles * p.tap_groups), block(256);
  switch (p.ks) {
    case 1: hipLaunchKernelGGL((wgrad_kernel<T, 1, 1>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((wgrad_kernel<T, 2, 8>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((wgrad_kernel<T, 3, 9>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((wgrad_kernel<T, 4, 8>), grid, block, 0, st, a); break;
  }
}

template <int KS>
void launch_tile_ks(const WgradArgs& a, const WPlan& p, hipStream_t st) {
  const dim3 grid(p.splits, p.ci_tiles, p.co_tiles);
  constexpr int lds0 = ((kWTD[0] + KS - 1) * (kWTH[0] + KS - 1) * (kWTW[0] + KS - 1) + kWTD[0] * kWTH[0] * kWTW[0]) * 64;
  constexpr int lds1 = ((kWTD[1] + KS - 1) * (kWTH[1] + KS - 1) * (kWTW[1] + KS - 1) + kWTD[1] * kWTH[1] * kWTW[1]) * 64;
  if (p.shape == 0) wgrad_bf16_kernel<KS, kWTD[0], kWTH[0], kWTW[0]><<<grid, dim3(256), lds0, st>>>(a, p.tiles_d, p.tiles_h, p.tiles_w, p.ntiles);
  else wgrad_bf16_kernel<KS, kWTD[1], kWTH[1], kWTW[1]><<<grid, dim3(256), lds1, st>>>(a, p.tiles_d, p.tiles_h, p.tiles_w, p.ntiles);
}
void launch_tile(const WgradArgs& a, const WPlan& p, hipStream_t st) {
  if (p.deconv4) {
    const dim3 grid(p.splits, p.ci_tiles, p.co_tiles / kDeconvNco);
    wgrad_deconv_kernel<<<grid, dim3(256), (1 + kDeconvNco) * 256 * 64, st>>>(a, p.tiles_d, p.tiles_h, p.tiles_w, p.ntiles);
  } else if (p.ks == 3) launch_tile_ks<3>(a, p, st);
  else if (p.ks == 2) launch_tile_ks<2>(a, p, st);
  else launch_tile_ks<1>(a, p, st);
}

template <auto Kernel>
int launch_marching(const char* name, int lds, const WgradArgs& a, const WPlan& p, hipStream_t st) {
  const int rc = raise_lds_limit<Kernel>(name, lds);
  if (rc) return rc;
  const WMarchArgs m{p.seg_len, p.nseg, p.tiles_h, p.tiles_w, p.nslabs, p.ci_tiles, p.co_tiles};
  hipLaunchKernelGGL(Kernel, dim3(((p.nslabs + 7) / 8) * 8 * p.ci_tiles * p.co_tiles), dim3(256), lds, st, a, m);
  return MI355_OK;
}

int launch_pointwise(const WgradArgs& a, const WPlan& p, hipStream_t st) {
  const int rc = raise_lds_limit<wgrad_pw_kernel>("wgrad_pw", kPwLds);
  if (rc) return rc;
  wgrad_pw_kernel<<<dim3(256), dim3(256), kPwLds, st>>>(a, p.nv, (int)((p.nv + 63) / 64));
  return MI355_OK;
}
int64_t workspace_bytes(const WPlan& p) { return (int64_t)p.nslabs * p.ks * p.ks * p.ks * p.cinp32 * p.coutp32 * 4; }

int conv_wgrad_impl(const mi355_wgrad_desc* d, mi355_wreduce_job* deferred, void* stream) {
  WPlan p;
  int rc = wplan(d, &p);
  if (rc) return rc;
  const int64_t need = workspace_bytes(p);
  MI355_REQUIRE(d->workspace && d->workspace_bytes >= need, "wgrad: workspace too small (%lld < %lld)",
                (long long)d->workspace_bytes, (long long)need);
  MI355_REQUIRE((d->do_ - 1) * d->gs + d->goff[0] < d->gd && (d->ho - 1) * d->gs + d->goff[1] < d->gh &&
                    (d->wo - 1) * d->gs + d->goff[2] < d->gw, "wgrad: grid exceeds g");
  hipStream_t st = (hipStream_t)stream;
  WgradArgs a;
  a.x0 = (const char*)d->x0; a.x1 = (const char*)d->x1;
  a.c0 = d->c0; a.c1 = d->c1; a.ld0 = d->ld0; a.ld1 = d->ld1;
  a.n = d->n; a.di = d->di; a.hi = d->hi; a.wi = d->wi;
  a.g = (const char*)d->g; a.cg = d->cg; a.ldg = d->ldg;
  a.do_ = d->do_; a.ho = d->ho; a.wo = d->wo;
  a.gd = d->gd; a.gh = d->gh; a.gw = d->gw; a.gs = d->gs;
  a.god = d->goff[0]; a.goh = d->goff[1]; a.gow = d->goff[2];
  a.stride = d->stride; a.pd = d->pad[0]; a.ph = d->pad[1]; a.pw = d->pad[2];
  a.slab = d->workspace; a.cinp = p.cinp32; a.coutp = p.coutp32;
  a.splits = p.splits; a.tap_groups = p.tap_groups; a.rows = p.rows;
  a.g_cls_cout = d->g_cls_cout;
  a.xn = d->xn > 0 ? d->xn : d->n;
  MI355_REQUIRE(a.xn == d->n || (p.kind != kWMarch && !p.deconv4), "wgrad: xn is not supported by this plan");
  switch (p.kind) {
    case kWPointwise: rc = launch_pointwise(a, p, st); break;
    case kWMarch2: rc = launch_marching<wgrad_march2_kernel>("wgrad_march2", kW2Lds, a, p, st); break;
    case kWMarch: rc = launch_marching<wgrad_march_kernel>("wgrad_march", kWmLds, a, p, st); break;
    case kWTile: launch_tile(a, p, st); break;
    default:      // kWGeneric
      if (d->dtype == MI355_DT_F32) launch_generic<float>(a, p, st);
      else launch_generic<bf16_t>(a, p, st);
  }
  if (rc) return rc;
  rc = mi355_check_launch("conv_wgrad");
  if (rc) return rc;
  RedJob job;
  make_reduce_job(d, p.nslabs, p.cinp32, p.coutp32, &job);
  if (deferred) {
    static_assert(sizeof(RedJob) <= sizeof(mi355_wreduce_job), "mi355_wreduce_job is too small");
    memset(deferred, 0, sizeof(*deferred));
    memcpy(deferred, &job, sizeof(job));
    return MI355_OK;
  }
  return launch_reduce_single(job, st);
}
}  // namespace

extern "C" int64_t mi355_conv_wgrad_workspace(const mi355_wgrad_desc* d) {
  WPlan p;
  return wplan(d, &p) ? -1 : workspace_bytes(p);
}

extern "C" int mi355_conv_wgrad_plan_kind(const mi355_wgrad_desc* d) {
  WPlan p;
  return wplan(d, &p) ? -1 : p.kind;
}
extern "C" int mi355_conv_wgrad(const mi355_wgrad_desc* d, void* stream) { return conv_wgrad_impl(d, nullptr, stream); }
extern "C" int mi355_conv_wgrad_partial(const mi355_wgrad_desc* d, mi355_wreduce_job* job, void* stream) {
  MI355_REQUIRE(job, "wgrad_partial: null job");
  return conv_wgrad_impl(d, job, stream);
}

extern "C" int mi355_wgrad_reduce_multi(const mi355_wreduce_job* jobs, int32_t n, void* stream) {
  MI355_REQUIRE(n >= 0 && (n == 0 || jobs), "wgrad_reduce_multi: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  std::vector<RedJob> light, heavy;           // the generic form's jobs run in the light kernel (wgrad_reduce.h)
  for (int j = 0; j < n; ++j) {
    RedJob job;
    memcpy(&job, jobs + j, sizeof(job));
    MI355_REQUIRE(job.magic == kRedMagic && job.kind >= kRedGeneric && job.kind <= kRedS2d && job.gx > 0 && job.gy > 0,
                  "wgrad_reduce_multi: job %d was not filled by mi355_conv_wgrad_partial", j);
    (job.kind == kRedGeneric ? light : heavy).push_back(job);
  }
  for (int pass = 0; pass < 2; ++pass) {
    const std::vector<RedJob>& v = pass == 0 ? light : heavy;
    for (size_t j0 = 0; j0 < v.size(); j0 += kRedChunk) {
      WreduceMulti m;
      m.n = (int)std::min<size_t>(kRedChunk, v.size() - j0);
      long long blocks = 0;
      for (int j = 0; j < kRedChunk; ++j) {
        const RedJob& job = v[j0 + std::min(j, m.n - 1)];                // (unused entries repeat the last job; never selected)
        m.a[j] = job.q; m.kind[j] = job.kind; m.gx[j] = job.gx;
        m.first[j] = (int)blocks;
        if (j < m.n) blocks += pass == 0 ? (((long long)job.q.ntaps * job.q.cinp * job.q.coutp + kLightF4 * 4 - 1) / (kLightF4 * 4)) : (long long)job.gx * job.gy;
      }
      m.first[kRedChunk] = (int)blocks;
      MI355_REQUIRE(blocks > 0 && blocks < (1ll << 31), "wgrad_reduce_multi: bad block count");
      if (pass == 0) wgrad_reduce_multi_light_kernel<<<dim3((unsigned)blocks), dim3(256), 0, st>>>(m);
      else wgrad_reduce_multi_kernel<<<dim3((unsigned)blocks), dim3(256), 0, st>>>(m);
      const int rc = mi355_check_launch("wgrad_reduce_multi");
      if (rc) return rc;
    }
  }
  return MI355_OK;
}
