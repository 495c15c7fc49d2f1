// Slab-writing weight-gradient kernels that work tile by tile:
//   wgrad_kernel         any dtype / kernel size / stride / g grid: exact-f32 MFMA, operands straight from global memory;
//   wgrad_bf16_kernel    bf16, stride 1, g on the grid of the outputs: x halo and g tile staged in LDS, transposed fragment reads;
//   wgrad_deconv_kernel  the transposed convolution's 8 classes as GEMM columns, four column tiles per workgroup.
// (near copies of tile decode, source selection and epilogue are written out on purpose: wgrad_common.h)
#pragma once
#include "wgrad_common.h"
namespace {
template <typename T> __device__ __forceinline__ float ld1(const char* p, long long idx) {
  return Elem<T>::load(reinterpret_cast<const T*>(p) + idx);
}
// GEMM view: D[ci][co] += A[ci][k] * B[k][co] with k = output position.  Exact-f32 MFMA (v_mfma_f32_32x32x2_f32, k = 2 positions
// per instruction), operands straight from global memory (32 lanes read 32 consecutive channels of one position = one 128-B
// line).  Every wave owns TPW taps of one (ci-tile, co-tile) and a disjoint set of rows (n, d, h); one slab per wave.
template <typename T, int KS, int TPW>
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradArgs a) {
  constexpr int NT = KS * KS * KS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int split = blockIdx.x;
  const int ci_base = blockIdx.y * 32;
  const int co_base = (blockIdx.z / a.tap_groups) * 32;
  const int tap0 = (blockIdx.z % a.tap_groups) * TPW;
  const int ci = ci_base + r;
  const bool first = ci_base < a.c0;
  const char* xs = first ? a.x0 : a.x1;
  const long long ldx = first ? a.ld0 : a.ld1;
  const int cix = first ? ci : ci - a.c0;
  const bool ci_ok = ci < a.c0 + a.c1;
  const int co = co_base + r;
  const bool co_ok = co < a.cg;
  f32x16 acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
  const long long nslots = (long long)a.splits * 4;
  for (long long row = (long long)split * 4 + wave; row < a.rows; row += nslots) {
    const int oh = (int)(row % a.ho);
    const long long t2 = row / a.ho;
    const int od = (int)(t2 % a.do_);
    const int n = (int)(t2 / a.do_);
    const long long grow = (((long long)n * a.gd + (od * a.gs + a.god)) * a.gh + (oh * a.gs + a.goh)) * a.gw;
    long long xrow[TPW];
    int kwv[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int tap = tap0 + t;
      const int kd = tap / (KS * KS), kh = (tap / KS) % KS, kw = tap % KS;
      const int id = od * a.stride + kd - a.pd, ih = oh * a.stride + kh - a.ph;
      const bool ok = tap < NT && id >= 0 && id < a.di && ih >= 0 && ih < a.hi;
      xrow[t] = ok ? (((long long)(n % a.xn) * a.di + id) * a.hi + ih) * a.wi : -1;
      kwv[t] = kw - a.pw;
    }
    for (int ow = h; ow < a.wo + h; ow += 2) {   // both halves iterate the same trip count
      const bool pos_ok = ow < a.wo;
      float b = 0.f;
      if (pos_ok && co_ok) b = ld1<T>(a.g, (grow + (ow * a.gs + a.gow)) * a.ldg + co);
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const int iw = ow * a.stride + kwv[t];
        float av = 0.f;
        if (pos_ok && ci_ok && xrow[t] >= 0 && iw >= 0 && iw < a.wi) av = ld1<T>(xs, (xrow[t] + iw) * ldx + cix);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b, acc[t], 0, 0, 0);
      }
    }
  }
  float* sl = a.slab + ((long long)(split * 4 + wave) * NT) * a.cinp * a.coutp;       // slab[(split*4+wave)][tap][ci][co]
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int tap = tap0 + t;
    if (tap < NT) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = ci_base + acc_row(i, h);
        sl[((long long)tap * a.cinp + row) * a.coutp + co] = acc[t][i];
      }
    }
  }
}

// bf16 stride-1 weight gradient on v_mfma_f32_32x32x16_bf16 (KS = 1, 2, 3).
// D[ci][co] += sum_k A[ci][k] * B[k][co], k = 16 consecutive W positions, fragments by frag_tr (wgrad_common.h).  A workgroup
// stages the x halo and the g tile of one 32x32 (ci, co) block once and its 4 waves share them, each owning 7 (6) of the 27
// taps; the g fragment is reused across a wave's taps.  Accumulators live across all tiles of the workgroup's split.
template <int KS, int TD, int TH, int TW>
__global__ __launch_bounds__(256, 2) void wgrad_bf16_kernel(const WgradArgs a, int tiles_d, int tiles_h,
                                                             int tiles_w, int ntiles) {
  constexpr int NT = KS * KS * KS;
  constexpr int TPWV = (NT + 3) / 4;          // taps per wave
  constexpr int HD = TD + KS - 1, HH = TH + KS - 1, HW = TW + KS - 1;
  constexpr int XROWS = HD * HH * HW, GROWS = TD * TH * TW;
  constexpr int NPX = (XROWS * 4 + 255) / 256, NPG = (GROWS * 4 + 255) / 256;
  constexpr int SEGS = TW / 16;
  static_assert(TW % 16 == 0, "tile width");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* xs = smem;
  char* gsm = smem + XROWS * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int ci_base = blockIdx.y * 32, co_base = blockIdx.z * 32;
  const bool first = ci_base < a.c0;
  const char* xsrc = first ? a.x0 : a.x1;
  const long long ldx = first ? a.ld0 : a.ld1;
  const int cix = first ? ci_base : ci_base - a.c0;
  const int cx_lim = (first ? a.c0 : a.c1) - cix;      // channels of this source left from cix
  // transposed-conv classes folded into the column index: this workgroup's 32 columns are one class
  int gs = 1, gbd = 0, gbh = 0, gbw = 0, gco = co_base;
  if (a.g_cls_cout) {
    const int cls = co_base / a.g_cls_cout;
    gco = co_base - cls * a.g_cls_cout;
    gs = 2; gbd = cls >> 2; gbh = (cls >> 1) & 1; gbw = cls & 1;
  }
  const int cg_lim = (a.g_cls_cout ? a.g_cls_cout : a.cg) - gco;
  constexpr bool WSPLIT = (KS == 1);                    // one tap: the 4 waves split the k-groups instead
  int toff[TPWV];
#pragma unroll
  for (int i = 0; i < TPWV; ++i) {
    const int tap = WSPLIT ? 0 : wave + 4 * i;
    const int kd = tap / (KS * KS), kh = (tap / KS) % KS, kw = tap % KS;
    toff[i] = tap < NT ? ((kd * HH + kh) * HW + kw) * 64 : 0;
  }
  const int gi = lane & 15;
  const int lane_off = (8 * h + (gi >> 2)) * 64 + (16 * ((lane >> 4) & 1) + 4 * (gi & 3)) * 2;
  f32x16 acc[TPWV];
#pragma unroll
  for (int i = 0; i < TPWV; ++i)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int t = tile;
    const int tw_i = t % tiles_w; t /= tiles_w;
    const int th_i = t % tiles_h; t /= tiles_h;
    const int td_i = t % tiles_d;
    const int n = t / tiles_d;
    const int d0 = td_i * TD, h0 = th_i * TH, w0 = tw_i * TW;
    uint4 sx[NPX];
#pragma unroll
    for (int i = 0; i < NPX; ++i) {
      const int p = tid + i * 256;
      const int row = p >> 2, part = p & 3;
      const int hw = row % HW, hh = (row / HW) % HH, hd = row / (HW * HH);
      const int gd = d0 + hd - a.pd, gh = h0 + hh - a.ph, gw = w0 + hw - a.pw;
      const bool ok = p < XROWS * 4 && part * 8 < cx_lim && gd >= 0 && gd < a.di && gh >= 0 && gh < a.hi && gw >= 0 && gw < a.wi;
      sx[i] = ok ? *reinterpret_cast<const uint4*>(xsrc + (((((long long)(n % a.xn) * a.di + gd) * a.hi + gh) * a.wi + gw) * ldx + cix + part * 8) * 2)
                 : make_uint4(0, 0, 0, 0);
    }
    __syncthreads();                      // every wave finished reading the previous tile
#pragma unroll
    for (int i = 0; i < NPX; ++i) {
      const int p = tid + i * 256;
      if (p < XROWS * 4) *reinterpret_cast<uint4*>(xs + p * 16) = sx[i];
    }
#pragma unroll
    for (int i = 0; i < NPG; ++i) {
      const int p = tid + i * 256;
      const int row = p >> 2, part = p & 3;
      const int sw = row % TW, sh = (row / TW) % TH, sd = row / (TW * TH);
      const int gd = d0 + sd, gh = h0 + sh, gw = w0 + sw;
      const bool ok = p < GROWS * 4 && part * 8 < cg_lim && gd < a.do_ && gh < a.ho && gw < a.wo;
      const uint4 v = ok ? *reinterpret_cast<const uint4*>(a.g + (((((long long)n * a.gd + (gd * gs + gbd)) * a.gh + (gh * gs + gbh)) * a.gw + (gw * gs + gbw)) * (long long)a.ldg + gco + part * 8) * 2)
                         : make_uint4(0, 0, 0, 0);
      if (p < GROWS * 4) *reinterpret_cast<uint4*>(gsm + p * 16) = v;
    }
    __syncthreads();
#pragma unroll 2
    for (int kg = WSPLIT ? wave : 0; kg < TD * TH * SEGS; kg += WSPLIT ? 4 : 1) {
      const int seg = kg % SEGS, sh = (kg / SEGS) % TH, sd = kg / (SEGS * TH);
      const char* gp = gsm + ((sd * TH + sh) * TW + seg * 16) * 64 + lane_off;
      const char* xp = xs + ((sd * HH + sh) * HW + seg * 16) * 64 + lane_off;
      const bf16x8 b = frag_tr(gp);
#pragma unroll
      for (int i = 0; i < TPWV; ++i) {
        const bf16x8 af = frag_tr(xp + toff[i]);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, b, acc[i], 0, 0, 0);
      }
    }
  }
  float* sl = a.slab + ((long long)(WSPLIT ? blockIdx.x * 4 + wave : blockIdx.x) * NT) * a.cinp * a.coutp;
  const int co = co_base + r;
#pragma unroll
  for (int i = 0; i < TPWV; ++i) {
    const int tap = WSPLIT ? 0 : wave + 4 * i;
    if (tap < NT) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int row = ci_base + acc_row(j, h);
        st_slab(&sl[((long long)tap * a.cinp + row) * a.coutp + co], acc[i][j]);
      }
    }
  }
}

// Transposed-conv (k2 s2) weight gradient, bf16: D[ci][cls * Cout + co] = sum_v x[v][ci] * g[2v + cls][co], one GEMM
// with 8 * Cout columns.  `wgrad_bf16_kernel<1,..>` staged x once per 32-column tile: for 64->64 at 64^3 that is 16
// re-reads of x and 2 of g (1.06 GB for 0.3 GB of operands, 256 us).  Here a workgroup owns NCO = 4 consecutive
// column tiles: the x tile is staged once, the four g tiles (two parity classes) next to it (80 KB of LDS), each
// wave takes every 4th k-group and feeds one x fragment to four MFMAs.
constexpr int kDeconvNco = 4;
__global__ __launch_bounds__(256, 2) void wgrad_deconv_kernel(const WgradArgs a, int tiles_d, int tiles_h, int tiles_w, int ntiles) {
  constexpr int TD = 2, TH = 4, TW = 32, NCO = kDeconvNco, ROWS = TD * TH * TW, NP = ROWS * 4 / 256, SEGS = TW / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* xs = smem;
  char* gsm = smem + ROWS * 64;                          // NCO tiles of ROWS x 64 B
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int ci_base = blockIdx.y * 32, co_base0 = blockIdx.z * (32 * NCO);
  const int cx_lim = a.c0 - ci_base;
  const int lane_off = frag_tr_lane_off(lane, h);
  f32x16 acc[NCO];
#pragma unroll
  for (int t = 0; t < NCO; ++t)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[t][j] = 0.f;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int q = tile;
    const int tw_i = q % tiles_w; q /= tiles_w;
    const int th_i = q % tiles_h; q /= tiles_h;
    const int td_i = q % tiles_d;
    const int n = q / tiles_d;
    const int d0 = td_i * TD, h0 = th_i * TH, w0 = tw_i * TW;
    uint4 sx[NP], sg[NCO][NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int p = tid + i * 256;
      const int row = p >> 2, part = p & 3;
      const int sw = row % TW, sh = (row / TW) % TH, sd = row / (TW * TH);
      const int gd = d0 + sd, gh = h0 + sh, gw = w0 + sw;
      const bool in = gd < a.do_ && gh < a.ho && gw < a.wo;
      sx[i] = (in && part * 8 < cx_lim)
                  ? *reinterpret_cast<const uint4*>(a.x0 + (((((long long)n * a.di + gd) * a.hi + gh) * a.wi + gw) * (long long)a.ld0 + ci_base + part * 8) * 2)
                  : make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int t = 0; t < NCO; ++t) {
        const int co_base = co_base0 + t * 32;
        const int cls = co_base / a.g_cls_cout, gco = co_base - cls * a.g_cls_cout;
        const int od = cls >> 2, oh = (cls >> 1) & 1, ow = cls & 1;
        sg[t][i] = (in && part * 8 < a.g_cls_cout - gco)
                       ? *reinterpret_cast<const uint4*>(a.g + (((((long long)n * a.gd + (gd * 2 + od)) * a.gh + (gh * 2 + oh)) * a.gw + (gw * 2 + ow)) * (long long)a.ldg + gco + part * 8) * 2)
                       : make_uint4(0, 0, 0, 0);
      }
    }
    __syncthreads();                      // every wave finished reading the previous tile
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int p = tid + i * 256;
      *reinterpret_cast<uint4*>(xs + p * 16) = sx[i];
#pragma unroll
      for (int t = 0; t < NCO; ++t) *reinterpret_cast<uint4*>(gsm + t * (ROWS * 64) + p * 16) = sg[t][i];
    }
    __syncthreads();
#pragma unroll 2
    for (int kg = wave; kg < TD * TH * SEGS; kg += 4) {
      const int off = kg * 16 * 64 + lane_off;            // k-groups are consecutive runs of 16 rows
      const bf16x8 af = frag_tr(xs + off);
#pragma unroll
      for (int t = 0; t < NCO; ++t) {
        const bf16x8 b = frag_tr(gsm + t * (ROWS * 64) + off);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, b, acc[t], 0, 0, 0);
      }
    }
  }
  float* sl = a.slab + (long long)(blockIdx.x * 4 + wave) * a.cinp * a.coutp;
#pragma unroll
  for (int t = 0; t < NCO; ++t) {
    const int co = co_base0 + t * 32 + r;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int row = ci_base + acc_row(j, h);
      st_slab(&sl[(long long)row * a.coutp + co], acc[t][j]);
    }
  }
}
}  // namespace
