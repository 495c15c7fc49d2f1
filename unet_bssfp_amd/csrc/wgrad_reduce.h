// Second pass of the weight gradient: the slabs [nslabs][tap][cinp][coutp] the kernels of wgrad_tile.h, wgrad_march.h and wgrad_pw.h
// wrote are added in slab order (deterministic) and scattered into the torch weight layout.  Three forms as __device__ bodies over a
// caller-provided LDS area and block coordinates: the single-layer kernels and the two batched kernels run the same code.
#pragma once
#include "common.h"
namespace {
struct WreduceArgs {
  const float* slab; int nslabs; int ntaps, ks, cinp, coutp;
  float* dw; int cout, cin;
  long long s_co, s_ci, s_k0, s_k1, s_k2;
  int tb0, tb1, tb2, ts0, ts1, ts2;
  int accumulate;
  int s2d_cp;
  int co_cls;            // >0: co index is blk*co_cls + co, blk selects the destination tap
};
// slabs are written once and read once: non-temporal loads keep them from displacing the activations the next
// kernels re-read (-0.04 ms per step, 3 of 3 interleaved rounds)
__device__ __forceinline__ float4 ld_once(const float* p) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  const f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}
constexpr int kRedLdsFloats = 32 * (4 * 64 + 1);                     // the largest form (space-to-depth patch): 32.1 KB

// Generic form.  256 threads = 32 float4 groups (128 consecutive elements, 512 B per slab row) x 8 slab lanes;
// 4 independent 16-B loads in flight per thread, fixed-order LDS combine (deterministic).
// (A variant with 16 slab lanes x 8 loads in flight and 64-element blocks looked equal in the micro-benchmark
// but cost 0.3 ms per training step in the interleaved A/B -- twice the blocks, half the row length per block.)
// F4 float4 groups x SL slab lanes per block (F4 * SL = 256): 32 x 8 for ordinary layers; 8 x 32 when a layer has
// so few weights (1x1x1 convs: 1024 elements under 2048 slabs) that 128-element blocks would leave 8 blocks.
template <int F4, int SL>
__device__ __forceinline__ void wgrad_reduce_body(const WreduceArgs& a, const int bx, float* smem) {
  static_assert(F4 * SL == 256, "block shape");
  float4 (*red)[F4] = reinterpret_cast<float4 (*)[F4]>(smem);         // [SL][F4]
  const long long per = (long long)a.ntaps * a.cinp * a.coutp;        // multiple of 1024
  const int e = threadIdx.x % F4, sl = threadIdx.x / F4;
  const long long idx = ((long long)bx * F4 + e) * 4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (idx < per) {
    const float* base = a.slab + idx;
    int k = sl;
    for (; k + 3 * SL < a.nslabs; k += 4 * SL) {
      const float4 v0 = ld_once(base + (long long)k * per);
      const float4 v1 = ld_once(base + (long long)(k + SL) * per);
      const float4 v2 = ld_once(base + (long long)(k + 2 * SL) * per);
      const float4 v3 = ld_once(base + (long long)(k + 3 * SL) * per);
      s.x += (v0.x + v1.x) + (v2.x + v3.x); s.y += (v0.y + v1.y) + (v2.y + v3.y);
      s.z += (v0.z + v1.z) + (v2.z + v3.z); s.w += (v0.w + v1.w) + (v2.w + v3.w);
    }
    for (; k < a.nslabs; k += SL) {
      const float4 v = *reinterpret_cast<const float4*>(base + (long long)k * per);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  red[sl][e] = s;
  __syncthreads();
  if (sl != 0 || idx >= per) return;
#pragma unroll
  for (int q = 1; q < SL; ++q) {
    const float4 v = red[q][e];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  const float f[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long id = idx + j;
    int co = (int)(id % a.coutp);
    int ci = (int)((id / a.coutp) % a.cinp);
    const int tap = (int)(id / ((long long)a.coutp * a.cinp));
    int blk = 0;
    if (a.s2d_cp) { blk = ci / a.s2d_cp; ci = ci % a.s2d_cp; }
    if (a.co_cls) { blk = co / a.co_cls; co = co % a.co_cls; }
    if (co >= a.cout || ci >= a.cin || blk >= 8) continue;
    const int td = tap / (a.ks * a.ks), th = (tap / a.ks) % a.ks, tw = tap % a.ks;
    const long long dst = co * a.s_co + ci * a.s_ci + (a.tb0 + a.ts0 * td + (blk >> 2)) * a.s_k0 +
                          (a.tb1 + a.ts1 * th + ((blk >> 1) & 1)) * a.s_k1 + (a.tb2 + a.ts2 * tw + (blk & 1)) * a.s_k2;
    if (a.accumulate) a.dw[dst] += f[j]; else a.dw[dst] = f[j];
  }
}
template <int F4, int SL>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const WreduceArgs a) {
  __shared__ float4 red[SL * F4];
  wgrad_reduce_body<F4, SL>(a, blockIdx.x, reinterpret_cast<float*>(red));
}

// Dense form.  Few slabs, many weights (the 8^3 / 16^3 levels: 2-16 slabs of up to 28 MB): the cost is the WRITE side --
// consecutive slab elements are consecutive output channels, 27*cin floats apart in dw[co][ci][taps], so the
// generic form scatters 4-byte stores (measured 176 us for 512->512).  Here a block owns all taps of an
// 8 (ci) x 32 (co) patch, sums the slabs in order (128-B read segments) and turns the patch through LDS so
// that every output-channel row is written as one contiguous run of 8 * taps floats.
// CIB = input channels per block (8, 4 or 2: fewer when the patch count would not fill the chip); the 8 / CIB
// thread groups of a channel split the taps.
// Round 4: 16-byte loads along co (a thread owns 4 consecutive output channels of (ci, tap)s), every slab's loads of a thread issued
// before the first add (nslabs <= 16: up to 64 loads in flight; the 4-byte form with one slab at a time read its 14 - 56 MB of
// slabs at 1.4 TB/s: 16 - 27 us per layer).  Summation in slab order: bit-identical to the form it replaces.
template <int NT, int CIB>
__device__ __forceinline__ void wgrad_reduce_dense_body(const WreduceArgs& a, const int bx, const int by, float* tile) {
  constexpr int ROW = CIB * NT + 1;                       // LDS row of one output channel: [ci][tap] (+1: odd stride)
  constexpr int ITEMS = CIB * NT;                         // (ci, tap) pairs of the patch; 8 threads (co quads) per pair
  constexpr int PER = (ITEMS + 31) / 32;                  // pairs per thread
  static_assert(32 * ROW <= kRedLdsFloats, "LDS area");
  const int t = threadIdx.x, cq = t & 7, grp = t >> 3;    // co quad, pair lane (32 of them)
  const int ci0 = bx * CIB, co0 = by * 32;
  const long long per = (long long)NT * a.cinp * a.coutp;
  const long long tstride = (long long)a.cinp * a.coutp;
  float4 s[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) s[i] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int item = grp + i * 32;
    if (item < ITEMS) {
      const int ci_l = item / NT, tap = item - ci_l * NT;
      const float* base = a.slab + (long long)tap * tstride + (long long)(ci0 + ci_l) * a.coutp + co0 + cq * 4;
      for (int k0 = 0; k0 < a.nslabs; k0 += 4) {          // four slabs' loads in flight per pair, added in slab order
        float4 v[4];
#pragma unroll
#ifdef WGRAD_NT_DENSE
        for (int j = 0; j < 4; ++j) v[j] = k0 + j < a.nslabs ? ld_once(base + (long long)(k0 + j) * per) : make_float4(0.f, 0.f, 0.f, 0.f);
#else
        for (int j = 0; j < 4; ++j) v[j] = k0 + j < a.nslabs ? *reinterpret_cast<const float4*>(base + (long long)(k0 + j) * per) : make_float4(0.f, 0.f, 0.f, 0.f);
#endif
#pragma unroll
        for (int j = 0; j < 4; ++j) { s[i].x += v[j].x; s[i].y += v[j].y; s[i].z += v[j].z; s[i].w += v[j].w; }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int item = grp + i * 32;
    if (item < ITEMS) {
      const int ci_l = item / NT, tap = item - ci_l * NT;
      float* d = tile + (cq * 4) * ROW + ci_l * NT + tap;
      d[0] = s[i].x; d[ROW] = s[i].y; d[2 * ROW] = s[i].z; d[3 * ROW] = s[i].w;
    }
  }
  __syncthreads();
  const int nci = min(CIB, a.cin - ci0);          // valid input channels of this patch
  if (nci <= 0) return;
  const int run = nci * NT;
  for (int r = 0; r < 32; ++r) {
    const int co = co0 + r;
    if (co >= a.cout) break;
    float* dst = a.dw + (long long)co * a.s_co + (long long)ci0 * a.s_ci;
    for (int j = t; j < run; j += 256) {
      const float v = tile[r * ROW + j];
      if (a.accumulate) dst[j] += v; else dst[j] = v;
    }
  }
}
template <int NT, int CIB>
__global__ __launch_bounds__(256) void wgrad_reduce_dense_kernel(const WreduceArgs a) {
  __shared__ float tile[32 * (CIB * NT + 1)];
  wgrad_reduce_dense_body<NT, CIB>(a, blockIdx.x, blockIdx.y, tile);
}

// Space-to-depth form.  The PatchGAN k4 s2 layers computed on space-to-depth tensors: slab rows are (j, blk * cp + c) with 8 dense
// taps j and 8 parity blocks blk, and dw[co][c][kd][kh][kw] has kd = 2 jd + bd (likewise h, w): for one (co, c)
// the 8 x 8 (j, blk) values are the 64 contiguous taps of the 4x4x4 kernel.  The generic form scattered them as
// 4-byte stores (101 us for the 256->512 layer, whose "reduce" has a single slab); here a block turns a
// 4 (c) x 32 (co) x 64 patch through LDS and writes 256 contiguous floats per output channel.
__device__ __forceinline__ void wgrad_reduce_s2d_body(const WreduceArgs& a, const int bx, const int by, float* tile) {
  constexpr int CB = 4, ROW = CB * 64 + 1;
  static_assert(32 * ROW <= kRedLdsFloats, "LDS area");
  const int t = threadIdx.x, co_l = t & 31, j = t >> 5;                    // j = dense tap of the k2 formulation
  const int c0 = bx * CB, co0 = by * 32;
  const long long per = (long long)8 * a.cinp * a.coutp;
  float s[8][CB];
#pragma unroll
  for (int b = 0; b < 8; ++b)
#pragma unroll
    for (int c = 0; c < CB; ++c) s[b][c] = 0.f;
  const float* base = a.slab + ((long long)j * a.cinp + c0) * a.coutp + co0 + co_l;
  for (int k = 0; k < a.nslabs; ++k) {
    const float* p = base + (long long)k * per;
#pragma unroll
    for (int b = 0; b < 8; ++b)
#pragma unroll
      for (int c = 0; c < CB; ++c) s[b][c] += p[((long long)b * a.s2d_cp + c) * a.coutp];
  }
  const int jd = j >> 2, jh = (j >> 1) & 1, jw = j & 1;
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const int tap = (2 * jd + (b >> 2)) * 16 + (2 * jh + ((b >> 1) & 1)) * 4 + (2 * jw + (b & 1));
#pragma unroll
    for (int c = 0; c < CB; ++c) tile[co_l * ROW + c * 64 + tap] = s[b][c];
  }
  __syncthreads();
  const int nc = min(CB, a.cin - c0);
  if (nc <= 0) return;
  const int run = nc * 64;
  for (int r = 0; r < 32; ++r) {
    const int co = co0 + r;
    if (co >= a.cout) break;
    float* dst = a.dw + (long long)co * a.s_co + (long long)c0 * a.s_ci;
    for (int i = t; i < run; i += 256) {
      const float v = tile[r * ROW + i];
      if (a.accumulate) dst[i] += v; else dst[i] = v;
    }
  }
}
__global__ __launch_bounds__(256) void wgrad_reduce_s2d_kernel(const WreduceArgs a) {
  __shared__ float tile[kRedLdsFloats];
  wgrad_reduce_s2d_body(a, blockIdx.x, blockIdx.y, tile);
}

// Slab reductions of up to kRedChunk layers in ONE launch (mi355_wgrad_reduce_multi): a step has ~30 weight-gradient
// launches, each followed by a 7 - 23 us reduction of its slabs that nothing but the optimiser (or the bucket's all-reduce)
// waits for; deferred to the end of a backward segment they are one launch.  Block -> (job, block of the job) through
// the prefix table; each job runs the form (and so the summation order) its own launch would: bit-identical results.
constexpr int kRedChunk = 16;
enum { kRedGeneric = 0, kRedGenericNarrow, kRedDense27_8, kRedDense27_4, kRedDense27_2, kRedDense1_8, kRedDense1_4, kRedDense1_2, kRedS2d };
struct WreduceMulti { WreduceArgs a[kRedChunk]; int kind[kRedChunk], gx[kRedChunk], first[kRedChunk + 1]; int n; };
// The jobs of the generic form (the marching kernels' 64 - 256 slabs per layer: most of the bytes) in a kernel of their own: 56 registers
// and 4 KB of LDS instead of the union's 166 / 32 KB -- 8 waves per SIMD instead of 3 to keep the slab reads in flight.
// (all jobs in the union kernel: slower; 64 / 128 float4 groups per light block: another summation order -- r04b_ab_deferred_reduce.txt)
constexpr int kLightF4 = 32;
__global__ __launch_bounds__(256) void wgrad_reduce_multi_light_kernel(const WreduceMulti m) {
  __shared__ float4 red[256];
  const int b = blockIdx.x;
  int j = 0;
  while (j + 1 < m.n && b >= m.first[j + 1]) ++j;
  wgrad_reduce_body<kLightF4, 256 / kLightF4>(m.a[j], b - m.first[j], reinterpret_cast<float*>(red));
}
__global__ __launch_bounds__(256) void wgrad_reduce_multi_kernel(const WreduceMulti m) {
  __shared__ float smem[kRedLdsFloats];
  const int b = blockIdx.x;
  int j = 0;
  while (j + 1 < m.n && b >= m.first[j + 1]) ++j;
  const int local = b - m.first[j], gx = m.gx[j];
  const int bx = local % gx, by = local / gx;
  const WreduceArgs& a = m.a[j];
  switch (m.kind[j]) {
    case kRedGeneric: wgrad_reduce_body<32, 8>(a, local, smem); break;
    case kRedGenericNarrow: wgrad_reduce_body<8, 32>(a, local, smem); break;
    case kRedDense27_8: wgrad_reduce_dense_body<27, 8>(a, bx, by, smem); break;
    case kRedDense27_4: wgrad_reduce_dense_body<27, 4>(a, bx, by, smem); break;
    case kRedDense27_2: wgrad_reduce_dense_body<27, 2>(a, bx, by, smem); break;
    case kRedDense1_8: wgrad_reduce_dense_body<1, 8>(a, bx, by, smem); break;
    case kRedDense1_4: wgrad_reduce_dense_body<1, 4>(a, bx, by, smem); break;
    case kRedDense1_2: wgrad_reduce_dense_body<1, 2>(a, bx, by, smem); break;
    default: wgrad_reduce_s2d_body(a, bx, by, smem); break;
  }
}

constexpr int kRedMagic = 0x52454431;                                 // "RED1"
struct RedJob { WreduceArgs q; int kind, gx, gy, magic; };            // what mi355_wreduce_job holds
// the reduction of a layer's nslabs slabs [ks^3][cinp][coutp] in d->workspace into d->dw: its arguments, form and grid
void make_reduce_job(const mi355_wgrad_desc* d, const int nslabs, const int cinp, const int coutp, RedJob* job) {
  WreduceArgs& q = job->q;
  q.slab = d->workspace; q.nslabs = nslabs; q.ks = d->ks; q.ntaps = d->ks * d->ks * d->ks;
  q.cinp = cinp; q.coutp = coutp;
  q.dw = d->dw; q.cout = d->cout; q.cin = d->cin;
  q.s_co = d->s_co; q.s_ci = d->s_ci; q.s_k0 = d->s_k[0]; q.s_k1 = d->s_k[1]; q.s_k2 = d->s_k[2];
  q.tb0 = d->tbase[0]; q.tb1 = d->tbase[1]; q.tb2 = d->tbase[2];
  q.ts0 = d->tstep[0]; q.ts1 = d->tstep[1]; q.ts2 = d->tstep[2];
  q.accumulate = d->accumulate;
  q.s2d_cp = d->s2d_cp;
  q.co_cls = d->g_cls_cout;
  job->magic = kRedMagic;
  const long long per = (long long)q.ntaps * q.cinp * q.coutp;
  const bool base0 = q.tb0 == 0 && q.tb1 == 0 && q.tb2 == 0;
  const bool dense = !q.s2d_cp && !q.co_cls && q.s_k2 == 1 && q.s_k1 == d->ks && q.s_k0 == d->ks * d->ks && q.s_ci == q.ntaps &&
                     base0 && q.ts0 == 1 && q.ts1 == 1 && q.ts2 == 1;
  if (dense && q.nslabs <= 16 && (d->ks == 3 || d->ks == 1) && q.cinp % 8 == 0 && q.coutp % 32 == 0) {
    // input channels per block: as many as keep >= 512 blocks in flight
    const long long cob = q.coutp / 32;
    const int cib = (q.cinp / 8) * cob >= 512 ? 8 : ((q.cinp / 4) * cob >= 512 ? 4 : 2);
    job->gx = q.cinp / cib; job->gy = (int)cob;
    job->kind = (d->ks == 3 ? kRedDense27_8 : kRedDense1_8) + (cib == 8 ? 0 : (cib == 4 ? 1 : 2));
    return;
  }
  const bool s2d_dense = q.s2d_cp > 0 && !q.co_cls && d->ks == 2 && q.s_k2 == 1 && q.s_k1 == 4 && q.s_k0 == 16 && q.s_ci == 64 &&
                         base0 && q.ts0 == 2 && q.ts1 == 2 && q.ts2 == 2 &&
                         q.cinp == 8 * q.s2d_cp && q.s2d_cp % 4 == 0 && q.coutp % 32 == 0;
  if (s2d_dense && q.nslabs <= 8) {
    job->kind = kRedS2d; job->gx = q.s2d_cp / 4; job->gy = q.coutp / 32;
    return;
  }
  job->gy = 1;
  if (per <= 16384 && q.nslabs >= 128) { job->kind = kRedGenericNarrow; job->gx = (int)((per + 31) / 32); }
  else { job->kind = kRedGeneric; job->gx = (int)((per + 127) / 128); }
}

int launch_reduce_single(const RedJob& job, hipStream_t st) {
  const WreduceArgs& q = job.q;
  const dim3 grid((unsigned)job.gx, (unsigned)job.gy);
  switch (job.kind) {
    case kRedGeneric: wgrad_reduce_kernel<32, 8><<<grid, dim3(256), 0, st>>>(q); return mi355_check_launch("wgrad_reduce");
    case kRedGenericNarrow: wgrad_reduce_kernel<8, 32><<<grid, dim3(256), 0, st>>>(q); return mi355_check_launch("wgrad_reduce");
    case kRedDense27_8: wgrad_reduce_dense_kernel<27, 8><<<grid, dim3(256), 0, st>>>(q); break;
    case kRedDense27_4: wgrad_reduce_dense_kernel<27, 4><<<grid, dim3(256), 0, st>>>(q); break;
    case kRedDense27_2: wgrad_reduce_dense_kernel<27, 2><<<grid, dim3(256), 0, st>>>(q); break;
    case kRedDense1_8: wgrad_reduce_dense_kernel<1, 8><<<grid, dim3(256), 0, st>>>(q); break;
    case kRedDense1_4: wgrad_reduce_dense_kernel<1, 4><<<grid, dim3(256), 0, st>>>(q); break;
    case kRedDense1_2: wgrad_reduce_dense_kernel<1, 2><<<grid, dim3(256), 0, st>>>(q); break;
    default: wgrad_reduce_s2d_kernel<<<grid, dim3(256), 0, st>>>(q); return mi355_check_launch("wgrad_reduce_s2d");
  }
  return mi355_check_launch("wgrad_reduce_dense");
}
}  // namespace
