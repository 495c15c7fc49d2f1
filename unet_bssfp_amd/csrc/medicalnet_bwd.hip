// Backward of the MedicalNet Perceptual term with respect to the PREDICTION.  The network is frozen and the
// target is a constant: no weight gradients, no gradient of the target.  Gradients between layers are dense bf16 NDHWC, like
// the activations of csrc/medicalnet.hip; f32 accumulation, one rounding at the store.
//   tail_bwd    : one pass over the two layer4 tensors -> d value / d f_pred, times layer4's ReLU mask.  The incoming gradient
//                 is read from DEVICE memory.
//   dgrad       : ONE implicit-GEMM kernel for the data gradient of the 3x3x3 convolutions (stride 1 / 2, dilation 1 / 2 / 4)
//                 and the 1x1x1 downsamples, in gather form: a wave owns 64 INPUT voxels x 64 input channels, K = cout per tap,
//                 fragments straight from global memory; weights packed [tap][cout / 16][cin][16].  For stride 2 the voxels are
//                 ordered by parity class, so a wave holds one class and the "whole wave is padding" test drops the taps that
//                 are dead for it.  Epilogue: + add (the gradient over the residual path), ReLU mask of a saved activation.
//   pool_bwd    : MaxPool3d(k3, s2, p1) backward in gather form, times the stem's ReLU mask.  A first launch records every
//                 window's arg-max tap (first maximum in (d, h, w) scan order, one byte per channel); an input voxel then visits
//                 the up to 2 x 2 x 2 windows that contain it and takes a window's gradient iff it is that window's arg-max.
//   stem_dgrad  : data gradient of Conv3d(1 -> 64, k7, s2, p3) on the matrix pipe.  A 2 x 2 x 2 cell of input voxels (one
//                 voxel per parity class) reads the same 4 x 4 x 4 neighbourhood of dy: M = cells, K = 64 offsets x 64 channels,
//                 N = the 8 parity classes, against a Toeplitz arrangement of the weights (343 of 512 (offset, class) pairs
//                 carry a weight) that sits in LDS, next to the dy patch of a workgroup's 4 x 4 x 16 cells.
//                 v_mfma_f32_16x16x32_bf16; columns 8..15 are zero.  The same launch forms the f64 partial sums of g and g x^
//                 for the normalisation backward.
//   norm_bwd    : dv = (g - sum g / N - x^ sum(g x^) / (N - 1)) / std, the gradient through (v - mean) / std (unbiased).
// No atomics; every reduction has a fixed order, so two calls give identical bits.  No host read.
// Shared with the forward through csrc/medicalnet_common.h, one definition each: the implicit-GEMM loop (dgrad = conv with another
// gather and epilogue), the pool window scan (arg-max = the forward's scan keeping the tap), pass 1 of the tail, the tile decode.
#include "medicalnet_common.h"

namespace {

typedef float f32x4v __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------- tail backward
// grid (chunks, items), as mnet_tail_kernel.  With n = |f|, a = n + 1e-10 and s = 2 g_out / (items * vox):
//   g_u = s (p / a_p - t / a_t),   g_f = g_u / a_p - p (p . g_u) / (n_p a_p^2) = c_p p - c_t t,
//   c_p = s (1 - n_p / a_p + (p . t) / (a_t n_p)) / a_p^2,   c_t = s / (a_t a_p);   n_p == 0: zeros.
__global__ __launch_bounds__(256) void mnet_tail_bwd_kernel(const bf16_t* __restrict__ fp, const bf16_t* __restrict__ ft,
                                                            const float* __restrict__ g_out, int c, int vox, int items,
                                                            bf16_t* __restrict__ gf) {
  __shared__ float red[4][3 * kTailVox];
  __shared__ float coef[2 * kTailVox];
  const int b = blockIdx.y, v0 = blockIdx.x * kTailVox;
  const int nvec = c * (kFeat / 8);
  tail_sums<3>(fp, ft, b, c, vox, v0, red);                               // p . p, t . t and p . t per voxel
  if (threadIdx.x < kTailVox) {
    const int vi = threadIdx.x;
    float tot[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) tot[k] = (red[0][3 * vi + k] + red[1][3 * vi + k]) + (red[2][3 * vi + k] + red[3][3 * vi + k]);
    const float np = sqrtf(tot[0]), nt = sqrtf(tot[1]);
    const float ap = np + 1e-10f, at = nt + 1e-10f;
    const float s = 2.f * g_out[0] / ((float)items * (float)vox);
    float cp = 0.f, ct = 0.f;
    if (np > 0.f) {
      cp = s * ((1.f - np / ap) + tot[2] / (at * np)) / (ap * ap);
      ct = s / (at * ap);
    }
    coef[2 * vi] = cp; coef[2 * vi + 1] = ct;
  }
  __syncthreads();
  for (int ev = threadIdx.x; ev < nvec; ev += 256) {
    const long long base = tail_base(b, c, ev, vox);
#pragma unroll
    for (int vi = 0; vi < kTailVox; ++vi) {
      if (v0 + vi < vox) {
        Vec16<bf16_t> p, t, o;
        p.load(fp + base + (long long)(v0 + vi) * kFeat);
        t.load(ft + base + (long long)(v0 + vi) * kFeat);
        const float cp = coef[2 * vi], ct = coef[2 * vi + 1];
#pragma unroll
        for (int k = 0; k < 8; ++k) o.f[k] = p.f[k] > 0.f ? cp * p.f[k] - ct * t.f[k] : 0.f;
        o.store(gf + base + (long long)(v0 + vi) * kFeat);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- data gradient
// dx[i, ci] = sum_tap sum_co dy[(i + pad - tap dil) / stride, co] w[co, ci, tap]; a tap counts where the division is exact and
// the quotient is in range.  M is ordered class by class: class (pd, ph, pw) holds the input voxels i = step j + p, step = stride.
struct MnetDgradArgs {
  const bf16_t* dy; const bf16_t* wp; const bf16_t* add; const bf16_t* mask; bf16_t* dx;
  int di, hi, wi, do_, ho, wo;                 // extents of dx (the convolution's input) and of dy
  int cin, cout, ks, stride, dil, pad, samples;
  int ncls;                                    // 1 (stride 1) or 8
  int wave0[9];                                // first wave of class c; wave0[ncls] = number of waves
};

// grid (ceil(waves / 4), cin / 64); wave = 64 input voxels of one class x 64 input channels
__global__ __launch_bounds__(256) void mnet_dgrad_kernel(const MnetDgradArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
  if (wid >= a.wave0[a.ncls]) return;                          // wave-uniform; the kernel has no barrier
  int cls = 0;
  for (int k = 1; k < a.ncls; ++k) cls += wid >= a.wave0[k] ? 1 : 0;
  const int step = a.stride;
  const int pd = step == 2 ? (cls >> 2) & 1 : 0, ph = step == 2 ? (cls >> 1) & 1 : 0, pw = step == 2 ? cls & 1 : 0;
  const int nd = class_extent(a.di, pd, step), nh = class_extent(a.hi, ph, step), nw = class_extent(a.wi, pw, step);
  const long long per = (long long)nd * nh * nw, count = per * a.samples;
  const int ci_base = blockIdx.y * 64;
  int s_[2], id_[2], ih_[2], iw_[2], vox[2];                    // vox: linear input voxel of this lane's row, -1 = none
#pragma unroll
  for (int vt = 0; vt < 2; ++vt) {
    const long long m = (long long)(wid - a.wave0[cls]) * 64 + vt * 32 + r;
    const bool ok = m < count;
    const long long mm = ok ? m : 0;
    const int s = (int)(mm / per); const int rem = (int)(mm - s * per);
    const int jd = rem / (nh * nw), r2 = rem - jd * (nh * nw);
    const int jh = r2 / nw, jw = r2 - jh * nw;
    s_[vt] = s; id_[vt] = jd * step + pd; ih_[vt] = jh * step + ph; iw_[vt] = jw * step + pw;
    vox[vt] = ok ? ((s * a.di + id_[vt]) * a.hi + ih_[vt]) * a.wi + iw_[vt] : -1;
  }
  const int sh = step - 1;
  // the source voxel of row 32 vt + r at tap (kd, kh, kw): dy at (i + pad - tap dil) / stride, where that is exact and in range
  const auto gather = [=](int vt, int kd, int kh, int kw, const bf16_t*& p) {
    const int qd = id_[vt] + a.pad - kd * a.dil, qh = ih_[vt] + a.pad - kh * a.dil, qw = iw_[vt] + a.pad - kw * a.dil;
    const int od = qd >> sh, oh = qh >> sh, ow = qw >> sh;
    const bool in = vox[vt] >= 0 && qd >= 0 && qh >= 0 && qw >= 0 && ((qd | qh | qw) & sh) == 0 && od < a.do_ && oh < a.ho && ow < a.wo;
    const long long o = in ? (((long long)s_[vt] * a.do_ + od) * a.ho + oh) * a.wo + ow : 0;     // a dead tap reads voxel 0: in-bounds
    p = a.dy + o * a.cout;
    return in;
  };
  const auto epilogue = [=](const f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int vt = 0; vt < 2; ++vt)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int v = __shfl(vox[vt], acc_row(i, h), 64);       // lane `row` (h = 0) holds the voxel of accumulator row `row`
        if (v >= 0) {
#pragma unroll
          for (int ct = 0; ct < 2; ++ct) {
            const long long off = (long long)v * a.cin + ci_base + ct * 32 + r;
            float g = acc[vt][ct][i];
            if (a.add) g += Elem<bf16_t>::load(a.add + off);
            if (a.mask && !(Elem<bf16_t>::load(a.mask + off) > 0.f)) g = 0.f;
            Elem<bf16_t>::store(a.dx + off, g);
          }
        }
      }
  };
  gemm_wave(a.wp, a.ks, a.cout >> 4, a.cin, ci_base, r, h, gather, epilogue);   // wp: [tap][cout / 16][cin][16]
}

// ---------------------------------------------------------------------------------------------------- max-pool backward
// one thread per (window, 8 channels): the tap kd * 9 + kh * 3 + kw of the window's FIRST maximum in scan order
__global__ __launch_bounds__(256) void mnet_pool_argmax_kernel(const bf16_t* __restrict__ x, uint8_t* __restrict__ arg, long long total,
                                                               int d, int h, int w, int od_, int oh_, int ow_, int c) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  pool_scan<true>(x, i, d, h, w, od_, oh_, ow_, c, [=](long long out, const uint32_t (&idx)[8]) {
    const uint32_t lo = idx[0] | (idx[1] << 8) | (idx[2] << 16) | (idx[3] << 24);
    const uint32_t hi = idx[4] | (idx[5] << 8) | (idx[6] << 16) | (idx[7] << 24);
    *reinterpret_cast<uint2*>(arg + out) = make_uint2(lo, hi);
  });
}

// one thread per (input voxel, 8 channels): dx = [x > 0] sum over the windows whose arg-max this voxel is of dy
__global__ __launch_bounds__(256) void mnet_pool_bwd_kernel(const bf16_t* __restrict__ x, const uint8_t* __restrict__ arg,
                                                            const bf16_t* __restrict__ dy, bf16_t* __restrict__ dx, long long total,
                                                            int d, int h, int w, int od_, int oh_, int ow_, int c) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int groups = c >> 3;
  const int g = (int)(i % groups);
  long long m = i / groups;
  const int iw = (int)(m % w); m /= w;
  const int ih = (int)(m % h); m /= h;
  const int id = (int)(m % d); const long long s = m / d;
  Vec16<bf16_t> xv, o;
  xv.load(x + (i / groups) * c + g * 8);
#pragma unroll
  for (int k = 0; k < 8; ++k) o.f[k] = 0.f;
  for (int kd = 0; kd < 3; ++kd) {                            // window od with 2 od - 1 + kd == id
    const int qd = id + 1 - kd;
    if (qd < 0 || (qd & 1) || (qd >> 1) >= od_) continue;
    for (int kh = 0; kh < 3; ++kh) {
      const int qh = ih + 1 - kh;
      if (qh < 0 || (qh & 1) || (qh >> 1) >= oh_) continue;
      for (int kw = 0; kw < 3; ++kw) {
        const int qw = iw + 1 - kw;
        if (qw < 0 || (qw & 1) || (qw >> 1) >= ow_) continue;
        const long long win = (((s * od_ + (qd >> 1)) * oh_ + (qh >> 1)) * ow_ + (qw >> 1)) * c + g * 8;
        const uint2 av = *reinterpret_cast<const uint2*>(arg + win);
        Vec16<bf16_t> gy;
        gy.load(dy + win);
        const uint32_t tap = kd * 9 + kh * 3 + kw;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const uint32_t ak = ((k < 4 ? av.x : av.y) >> (8 * (k & 3))) & 0xffu;
          if (ak == tap) o.f[k] += gy.f[k];
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) o.f[k] = xv.f[k] > 0.f ? o.f[k] : 0.f;
  o.store(dx + (i / groups) * c + g * 8);
}

// ---------------------------------------------------------------------------------------------------- stem data gradient
// Cell j = (jd, jh, jw) holds the input voxels i = 2 j + p, p in {0, 1}^3 (class 4 pd + 2 ph + pw).  Per axis, offset a = 0..3
// reads dy at o = j - 1 + a through the tap k = p + 5 - 2 a (a weight where 0 <= k <= 6).  wp: bf16 [64 offsets][2][8 classes][32]:
// element (t, half, cls, e) = w[co = 32 half + e][kd][kh][kw] or 0, t = (ad * 4 + ah) * 4 + aw.
struct StemDgradArgs {
  const bf16_t* dy; const char* wp; const float* x; const float* ms; float* g; double* part;
  int d, h, w, do_, ho, wo;                    // do_ = ceil(d / 2): the cells of an axis are the positions of dy
  int tiles_d, tiles_h, tiles_w;
  long long tiles;                             // samples * tiles_d * tiles_h * tiles_w
};

__device__ __forceinline__ void mma32(const uint4 a, const uint4 b, f32x4v& acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}

// Tile of a workgroup: 4 x 4 x 16 cells of one sample; wave = one d-slice, its four 16-row MFMA tiles = the four h-rows, a row
// of a tile = a cell along w.  The tile's dy patch, 7 x 7 x 19 voxels from (od0 - 1, oh0 - 1, ow0 - 1), is staged into LDS one
// half of the channels at a time (padding = 0; 64 bytes per voxel, so the 64 lanes of an A load read 1 KB contiguous): every dy
// voxel is read from memory once per tile instead of once per offset, and the loads of the next stage are issued into
// registers before the current one computes.  Lane (row = lane & 15, q = lane >> 4) holds channels
// 32 half + 8 q .. + 8 of its row's voxel, and D[cell 4 q + i][class lane & 15] in accumulator register i.
constexpr int kSdTD = 4, kSdTH = 4, kSdTW = 16;
constexpr int kSdPD = kSdTD + 3, kSdPH = kSdTH + 3, kSdPW = kSdTW + 3;
constexpr int kSdWeightVecs = 128 * 8 * 4;                                // [t * 2 + half][class][32] bf16 as uint4: 64 KB
constexpr int kSdPatchVecs = kSdPD * kSdPH * kSdPW * 4;                   // [pz][py][px][32] bf16 as uint4: 58.2 KB
constexpr int kSdLdsBytes = (kSdWeightVecs + kSdPatchVecs) * 16;

constexpr int kSdStageVecs = (kSdPatchVecs + 255) / 256;                  // 16-byte vectors per thread and stage

// the loads of one stage (a tile's patch, one half of the channels) into registers: they fly while the previous stage computes
__device__ __forceinline__ void sd_stage_issue(const StemDgradArgs& a, long long tile, int half, uint4 (&v)[kSdStageVecs]) {
  const Tile t = tile_decode(tile, a.tiles_d, a.tiles_h, a.tiles_w);
  const long long s = t.s;
#pragma unroll
  for (int k = 0; k < kSdStageVecs; ++k) {
    const int i = threadIdx.x + k * 256;
    const int vox = (i < kSdPatchVecs ? i : 0) >> 2, ch = i & 3;
    const int pz = vox / (kSdPH * kSdPW), r2 = vox - pz * (kSdPH * kSdPW);
    const int py = r2 / kSdPW, px = r2 - py * kSdPW;
    const int od = t.td * kSdTD - 1 + pz, oh = t.th * kSdTH - 1 + py, ow = t.tw * kSdTW - 1 + px;
    const bool in = (unsigned)od < (unsigned)a.do_ && (unsigned)oh < (unsigned)a.ho && (unsigned)ow < (unsigned)a.wo;
    const long long o = in ? ((s * a.do_ + od) * a.ho + oh) * a.wo + ow : 0;
    const uint4 val = *reinterpret_cast<const uint4*>(a.dy + o * kStemC + half * 32 + ch * 8);       // in-bounds either way
    v[k] = in ? val : make_uint4(0, 0, 0, 0);
  }
}

__global__ __launch_bounds__(256) void mnet_stem_dgrad_kernel(const StemDgradArgs a) {
  extern __shared__ uint4 sd_lds[];
  uint4* wlds = sd_lds;
  uint4* patch = sd_lds + kSdWeightVecs;
  for (int i = threadIdx.x; i < kSdWeightVecs; i += 256) wlds[i] = reinterpret_cast<const uint4*>(a.wp)[i];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = lane & 15, q = lane >> 4;
  const float mean = a.ms[0], std = a.ms[1];
  double sg = 0.0, sgx = 0.0;
  uint4 stage[kSdStageVecs];
  sd_stage_issue(a, blockIdx.x, 0, stage);                                // (the grid never exceeds the number of tiles)
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const Tile tl = tile_decode(tile, a.tiles_d, a.tiles_h, a.tiles_w);
    const long long s = tl.s;
    const int od0 = tl.td * kSdTD, oh0 = tl.th * kSdTH, ow0 = tl.tw * kSdTW;
    f32x4v acc[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4v{0.f, 0.f, 0.f, 0.f};
    for (int half = 0; half < 2; ++half) {
      __syncthreads();                                                    // the previous fragments have been read (first: the weights are in)
#pragma unroll
      for (int k = 0; k < kSdStageVecs; ++k)
        if (threadIdx.x + k * 256 < kSdPatchVecs) patch[threadIdx.x + k * 256] = stage[k];
      __syncthreads();
      if (half == 0) sd_stage_issue(a, tile, 1, stage);
      else if (tile + gridDim.x < a.tiles) sd_stage_issue(a, tile + gridDim.x, 0, stage);
#pragma unroll 8
      for (int t = 0; t < 64; ++t) {
        const int ad = t >> 4, ah = (t >> 2) & 3, aw = t & 3;
        uint4 fb = make_uint4(0, 0, 0, 0);
        if (row < 8) fb = wlds[((t * 2 + half) * 8 + row) * 4 + q];        // columns 8..15 carry no class
        const uint4* pa = patch + ((((wave + ad) * kSdPH + ah) * kSdPW + row + aw) * 4 + q);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) mma32(pa[mt * kSdPW * 4], fb, acc[mt]);
      }
    }
    if (row < 8) {
      const int id = 2 * (od0 + wave) + ((row >> 2) & 1);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int ih = 2 * (oh0 + mt) + ((row >> 1) & 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int iw = 2 * (ow0 + 4 * q + i) + (row & 1);
          if (id < a.d && ih < a.h && iw < a.w) {                         // (implies that the cell exists)
            const long long o = ((s * a.d + id) * a.h + ih) * a.w + iw;
            const float gv = acc[mt][i];
            a.g[o] = gv;
            sg += (double)gv;
            sgx += (double)gv * (double)((a.x[o] - mean) / std);
          }
        }
      }
    }
  }
  __syncthreads();                                                        // the weights are dead: their LDS carries the sums
  double* red = reinterpret_cast<double*>(wlds);
  sg = block_sum_256d(sg, red);
  sgx = block_sum_256d(sgx, red);
  if (threadIdx.x == 0) { a.part[2 * blockIdx.x] = sg; a.part[2 * blockIdx.x + 1] = sgx; }
}

// every workgroup sums the nb partial pairs in the same fixed order, then streams its share of the tensor
__global__ __launch_bounds__(256) void mnet_norm_bwd_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                            const float* __restrict__ ms, const double* __restrict__ part, int nb,
                                                            float* __restrict__ dv, long long n) {
  __shared__ double red[4];
  double s = 0.0, sx = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) { s += part[2 * i]; sx += part[2 * i + 1]; }
  s = block_sum_256d(s, red);
  sx = block_sum_256d(sx, red);
  const float mean = ms[0], std = ms[1];
  const float c0 = (float)(s / (double)n), c1 = (float)(sx / (double)(n - 1));
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float xh = (x[i] - mean) / std;
    dv[i] = (g[i] - c0 - xh * c1) / std;
  }
}

long long stem_dgrad_tiles(int samples, int d, int h, int w) {
  return (long long)samples * ceil_div(out_extent(d, 7, 2, 1), kSdTD) * ceil_div(out_extent(h, 7, 2, 1), kSdTH) *
         ceil_div(out_extent(w, 7, 2, 1), kSdTW);
}
int stem_dgrad_blocks(long long tiles) {
  return (int)(tiles < 1 ? 1 : (tiles > 256 ? 256 : tiles));  // one 122 KB workgroup per CU; the weight copy is amortised over its tiles
}

}  // namespace

extern "C" int mi355_medicalnet_tail_bwd(const void* feat_pred, const void* feat_target, const float* g_out, void* g_feat,
                                         int32_t items, int32_t c, int32_t vox, void* stream) {
  MI355_REQUIRE(feat_pred && feat_target && g_out && g_feat, "medicalnet_tail_bwd: null pointer");
  MI355_REQUIRE(items > 0 && c > 0 && vox > 0, "medicalnet_tail_bwd: bad shape (items=%d c=%d vox=%d)", items, c, vox);
  MI355_REQUIRE(((reinterpret_cast<uintptr_t>(feat_pred) | reinterpret_cast<uintptr_t>(feat_target) |
                  reinterpret_cast<uintptr_t>(g_feat)) & 15) == 0, "medicalnet_tail_bwd: tensors must be 16-byte aligned");
  MNET_SUPPORTED(items <= 65535 && c <= 4096, "medicalnet_tail_bwd: at most 65535 items of at most 4096 channels");
  const int chunks = (vox + kTailVox - 1) / kTailVox;
  mnet_tail_bwd_kernel<<<dim3(chunks, items), 256, 0, (hipStream_t)stream>>>((const bf16_t*)feat_pred, (const bf16_t*)feat_target,
                                                                            g_out, c, vox, items, (bf16_t*)g_feat);
  return mi355_check_launch("medicalnet_tail_bwd");
}

extern "C" int mi355_medicalnet_dgrad(const void* dy, const void* wp, const void* add, const void* mask, void* dx,
                                      int32_t samples, int32_t d, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t ks,
                                      int32_t stride, int32_t dilation, void* stream) {
  MI355_REQUIRE(dy && wp && dx, "medicalnet_dgrad: null pointer");
  const int rc = check_conv_args("medicalnet_dgrad", "dy", dy, wp, samples, d, h, w, cin, cout, ks, stride, dilation);
  if (rc != MI355_OK) return rc;
  MNET_SUPPORTED((long long)samples * d * h * w < (1ll << 31), "medicalnet_dgrad: tensor too large for one launch");
  MnetDgradArgs a;
  a.dy = (const bf16_t*)dy; a.wp = (const bf16_t*)wp; a.add = (const bf16_t*)add; a.mask = (const bf16_t*)mask; a.dx = (bf16_t*)dx;
  a.di = d; a.hi = h; a.wi = w;
  a.do_ = out_extent(d, ks, stride, dilation); a.ho = out_extent(h, ks, stride, dilation); a.wo = out_extent(w, ks, stride, dilation);
  a.cin = cin; a.cout = cout; a.ks = ks; a.stride = stride; a.dil = dilation; a.pad = dilation * (ks / 2); a.samples = samples;
  a.ncls = stride == 2 ? 8 : 1;
  long long waves = 0;
  for (int c = 0; c < 9; ++c) a.wave0[c] = 0;
  for (int c = 0; c < a.ncls; ++c) {
    const int pd = stride == 2 ? (c >> 2) & 1 : 0, ph = stride == 2 ? (c >> 1) & 1 : 0, pw = stride == 2 ? c & 1 : 0;
    const long long count = (long long)samples * class_extent(d, pd, stride) * class_extent(h, ph, stride) * class_extent(w, pw, stride);
    a.wave0[c] = (int)waves;
    waves += (count + 63) / 64;
  }
  for (int c = a.ncls; c < 9; ++c) a.wave0[c] = (int)waves;
  mnet_dgrad_kernel<<<dim3((unsigned)ceil_div(waves, 4), cin / 64), 256, 0, (hipStream_t)stream>>>(a);
  return mi355_check_launch("medicalnet_dgrad");
}

extern "C" int64_t mi355_medicalnet_maxpool_bwd_workspace_bytes(int32_t samples, int32_t d, int32_t h, int32_t w, int32_t c) {
  if (samples <= 0 || d <= 0 || h <= 0 || w <= 0 || c <= 0) return -1;
  return (long long)samples * out_extent(d, 3, 2, 1) * out_extent(h, 3, 2, 1) * out_extent(w, 3, 2, 1) * c;
}

extern "C" int mi355_medicalnet_maxpool_bwd(const void* x, const void* dy, void* workspace, int64_t workspace_bytes, void* dx,
                                            int32_t samples, int32_t d, int32_t h, int32_t w, int32_t c, void* stream) {
  const long long need = mi355_medicalnet_maxpool_bwd_workspace_bytes(samples, d, h, w, c);
  MI355_REQUIRE(need > 0 && c % 8 == 0, "medicalnet_maxpool_bwd: bad shape (samples=%d d=%d h=%d w=%d c=%d)", samples, d, h, w, c);
  MI355_REQUIRE(x && dy && workspace && dx && workspace_bytes >= need, "medicalnet_maxpool_bwd: null pointer or workspace too small");
  MI355_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(workspace) |
                  reinterpret_cast<uintptr_t>(dx)) & 15) == 0, "medicalnet_maxpool_bwd: tensors must be 16-byte aligned");
  const int od = out_extent(d, 3, 2, 1), oh = out_extent(h, 3, 2, 1), ow = out_extent(w, 3, 2, 1);
  const long long wins = need / 8, total = (long long)samples * d * h * w * (c / 8);
  MNET_SUPPORTED(total < (1ll << 39), "medicalnet_maxpool_bwd: tensor too large for one launch");
  hipStream_t st = (hipStream_t)stream;
  mnet_pool_argmax_kernel<<<(unsigned)((wins + 255) / 256), 256, 0, st>>>((const bf16_t*)x, (uint8_t*)workspace, wins, d, h, w, od,
                                                                         oh, ow, c);
  mnet_pool_bwd_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>((const bf16_t*)x, (const uint8_t*)workspace,
                                                                       (const bf16_t*)dy, (bf16_t*)dx, total, d, h, w, od, oh, ow, c);
  return mi355_check_launch("medicalnet_maxpool_bwd");
}

extern "C" int32_t mi355_medicalnet_stem_dgrad_blocks(int32_t samples, int32_t d, int32_t h, int32_t w) {
  if (samples <= 0 || d <= 0 || h <= 0 || w <= 0) return 0;
  return stem_dgrad_blocks(stem_dgrad_tiles(samples, d, h, w));
}

extern "C" int mi355_medicalnet_stem_dgrad(const void* dy, const void* wp, const float* x, const float* mean_std, float* g,
                                           double* part, int32_t samples, int32_t d, int32_t h, int32_t w, void* stream) {
  MI355_REQUIRE(dy && wp && x && mean_std && g && part, "medicalnet_stem_dgrad: null pointer");
  MI355_REQUIRE(samples > 0 && d > 0 && h > 0 && w > 0, "medicalnet_stem_dgrad: bad shape (samples=%d d=%d h=%d w=%d)", samples, d,
                h, w);
  MI355_REQUIRE(((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(wp)) & 15) == 0,
                "medicalnet_stem_dgrad: dy and the packed weights must be 16-byte aligned");
  StemDgradArgs a;
  a.dy = (const bf16_t*)dy; a.wp = (const char*)wp; a.x = x; a.ms = mean_std; a.g = g; a.part = part;
  a.d = d; a.h = h; a.w = w;
  a.do_ = out_extent(d, 7, 2, 1); a.ho = out_extent(h, 7, 2, 1); a.wo = out_extent(w, 7, 2, 1);
  MNET_SUPPORTED((long long)d * h * w < (1ll << 31) && (long long)samples * a.do_ * a.ho * a.wo < (1ll << 40),
                 "medicalnet_stem_dgrad: volume too large (d=%d h=%d w=%d)", d, h, w);
  a.tiles_d = ceil_div(a.do_, kSdTD); a.tiles_h = ceil_div(a.ho, kSdTH); a.tiles_w = ceil_div(a.wo, kSdTW);
  a.tiles = stem_dgrad_tiles(samples, d, h, w);
  const int rc = raise_lds_limit<mnet_stem_dgrad_kernel>("medicalnet_stem_dgrad", kSdLdsBytes);
  if (rc != MI355_OK) return rc;
  mnet_stem_dgrad_kernel<<<stem_dgrad_blocks(a.tiles), 256, kSdLdsBytes, (hipStream_t)stream>>>(a);
  return mi355_check_launch("medicalnet_stem_dgrad");
}

extern "C" int mi355_medicalnet_norm_bwd(const float* g, const float* x, const float* mean_std, const double* part, int32_t nb,
                                         float* dv, int64_t n, void* stream) {
  MI355_REQUIRE(g && x && mean_std && part && dv, "medicalnet_norm_bwd: null pointer");
  MI355_REQUIRE(n >= 2 && nb >= 1, "medicalnet_norm_bwd: bad size (n=%lld nb=%d)", (long long)n, nb);
  const long long b = (n + 256 * 16 - 1) / (256 * 16);
  mnet_norm_bwd_kernel<<<(unsigned)(b > 2048 ? 2048 : b), 256, 0, (hipStream_t)stream>>>(g, x, mean_std, part, nb, dv, n);
  return mi355_check_launch("medicalnet_norm_bwd");
}
