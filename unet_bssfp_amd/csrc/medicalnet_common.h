// What csrc/medicalnet.hip (forward) and csrc/medicalnet_bwd.hip (backward) share: one definition of everything that has to
// stay the same on both sides of the Perceptual term.
//   constants, the reductions, out_extent / is_width, the host check of a residual convolution's arguments;
//   gemm    : the implicit-GEMM loop of mnet_conv_kernel and mnet_dgrad_kernel (a wave's 64 rows x 64 columns, both fragments
//             from global memory).  The kernels differ in how a lane turns (row, tap) into a source voxel and in the epilogue:
//             two functors;
//   pool    : the 27-tap window scan of MaxPool3d(k3, s2, p1), keeping the maximum (forward) or its tap (backward);
//   tail    : pass 1 of the tail kernels, the per-voxel sums over the c * 512 channels;
//   tiles   : tile -> (sample, td, th, tw) of the stem kernels; the positions of a stride-2 parity class along an axis.
// Everything here is inlined into its kernel: sharing is by template and compile-time branch only, never by a run-time mode.
// Two rules keep hipcc's code that of the kernels written out by hand (profiles/medicalnet_refactor_resources.txt):
//  * a register array (the accumulators, a window's maxima) is declared, zeroed and filled in ONE function and handed on
//    read-only to a functor -- zeroed through a reference elsewhere, a second copy of it stays alive across the loop;
//  * the functors capture BY VALUE ([=]): through a captured reference to the kernel's argument struct every use in an unrolled
//    epilogue re-reads the kernel arguments (scalar loads and waits per accumulator row).
#pragma once
#include "common.h"

namespace {

#define MNET_SUPPORTED(cond, ...)                     \
  do {                                                \
    if (!(cond)) {                                    \
      mi355_set_error(__VA_ARGS__);                   \
      return MI355_ERR_UNSUPPORTED;                   \
    }                                                 \
  } while (0)

constexpr int kStemC = 64;                      // output channels of the stem
constexpr int kFeat = 512;                      // channels of layer4
constexpr int kTailVox = 16;                    // voxels per workgroup of the tail pass

template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum over the 256 threads of a workgroup in a fixed order; every thread gets it
__device__ __forceinline__ double block_sum_256d(double v, double* red /* LDS, 4 doubles */) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

int out_extent(int in, int ks, int stride, int dil) { return (in + 2 * (dil * (ks / 2)) - dil * (ks - 1) - 1) / stride + 1; }
bool is_width(int c) { return c == 64 || c == 128 || c == 256 || c == 512; }

// positions i = stride j + p < n of parity class p along an axis of n voxels: the data-gradient kernel decodes its rows with
// it and the launcher counts the waves of a class with it
__host__ __device__ __forceinline__ int class_extent(int n, int p, int stride) { return (n - p + stride - 1) / stride; }

// what mi355_medicalnet_conv and mi355_medicalnet_dgrad accept; `who` is the caller's name and `act` its activation operand
int check_conv_args(const char* who, const char* act, const void* act_ptr, const void* wp, int samples, int d, int h, int w,
                    int cin, int cout, int ks, int stride, int dilation) {
  MI355_REQUIRE(samples > 0 && d > 0 && h > 0 && w > 0, "%s: bad shape (samples=%d d=%d h=%d w=%d)", who, samples, d, h, w);
  MNET_SUPPORTED(is_width(cin) && is_width(cout), "%s: cin and cout must be 64, 128, 256 or 512 (cin=%d cout=%d)", who, cin, cout);
  MNET_SUPPORTED((ks == 3 && (dilation == 1 || dilation == 2 || dilation == 4)) || (ks == 1 && dilation == 1),
                 "%s: ks 3 with dilation 1, 2 or 4, or ks 1 with dilation 1 (ks=%d dilation=%d)", who, ks, dilation);
  MNET_SUPPORTED(stride == 1 || stride == 2, "%s: stride must be 1 or 2 (stride=%d)", who, stride);
  MI355_REQUIRE(((reinterpret_cast<uintptr_t>(act_ptr) | reinterpret_cast<uintptr_t>(wp)) & 15) == 0,
                "%s: %s and the packed weights must be 16-byte aligned", who, act);
  return MI355_OK;
}

// ---------------------------------------------------------------------------------------------------- tiles of the stem kernels
struct Tile { long long s; int td, th, tw; };    // sample and tile coordinates; w runs fastest
__device__ __forceinline__ Tile tile_decode(long long tile, int tiles_d, int tiles_h, int tiles_w) {
  Tile t;
  t.tw = (int)(tile % tiles_w); tile /= tiles_w;
  t.th = (int)(tile % tiles_h); tile /= tiles_h;
  t.td = (int)(tile % tiles_d); t.s = tile / tiles_d;
  return t;
}

// ---------------------------------------------------------------------------------------------------- implicit GEMM
// A wave owns 64 rows (voxels: two 32-row MFMA tiles, lane r = lane & 31 loads row 32 vt + r) x 64 columns (two 32-column
// tiles from col0); lane half h = lane >> 5 owns elements 8 h .. 8 h + 7 of a 16-element K chunk.  wp: [tap][chunk][cols][16],
// ks^3 taps of K = nchunk * 16.  gather(vt, kd, kh, kw, p) says whether the tap reaches row 32 vt + r and sets p to the K
// elements of its source voxel (to those of voxel 0 where it does not: the load stays in bounds and the fragment is zeroed).
// epilogue(acc) stores the wave's tile.  r, h: the kernel's own lane & 31 and lane >> 5, which its functors use as well.
template <typename Gather, typename Epilogue>
__device__ __forceinline__ void gemm_wave(const bf16_t* wp, int ks, int nchunk, int cols, int col0, int r, int h,
                                          const Gather& gather, const Epilogue& epilogue) {
  f32x16 acc[2][2];
#pragma unroll
  for (int vt = 0; vt < 2; ++vt)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[vt][ct][i] = 0.f;
  const int taps = ks * ks * ks;
  const bf16_t* wlane = wp + ((long long)(col0 + r) * 16 + 8 * h);        // this lane's weight rows of chunk 0 / tap 0
  for (int tap = 0; tap < taps; ++tap) {
    const int kd = tap / (ks * ks), kr = tap - kd * ks * ks;
    const int kh = kr / ks, kw = kr - kh * ks;
    const bf16_t* pa[2]; bool in[2];
#pragma unroll
    for (int vt = 0; vt < 2; ++vt) {
      in[vt] = gather(vt, kd, kh, kw, pa[vt]);
      pa[vt] += 8 * h;
    }
    if (!__any(in[0] || in[1])) continue;                     // no row of the wave is reached by this tap
    const bf16_t* pw = wlane + (long long)tap * nchunk * cols * 16;
    for (int kc0 = 0; kc0 < nchunk; kc0 += 4) {               // K is a multiple of 64: four steps' loads go out together
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int kc = kc0 + u;
        Frag<bf16_t> fa[2], fb[2];
#pragma unroll
        for (int vt = 0; vt < 2; ++vt) {
          fa[vt].load(reinterpret_cast<const char*>(pa[vt] + kc * 16));
          if (!in[vt]) fa[vt].zero();
        }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) fb[ct].load(reinterpret_cast<const char*>(pw + ((long long)kc * cols + ct * 32) * 16));
#pragma unroll
        for (int vt = 0; vt < 2; ++vt)
#pragma unroll
          for (int ct = 0; ct < 2; ++ct) mma16(fa[vt], fb[ct], acc[vt][ct]);
      }
    }
  }
  epilogue(acc);
}

// ---------------------------------------------------------------------------------------------------- max-pool k3 s2 p1
// The window scan of thread i = (output voxel, 8 channels), rows of c channels: best = the maximum (padding counts as -inf) and,
// with kArgmax, idx = the tap kd * 9 + kh * 3 + kw of its FIRST occurrence in scan order.  The backward's tie rule is the order
// of this one loop.  store(out, best) or, with kArgmax, store(out, idx): out = the element offset of the thread's 8 channels in
// the output tensor.
template <bool kArgmax, typename Store>
__device__ __forceinline__ void pool_scan(const bf16_t* __restrict__ x, long long i, int d, int h, int w, int od_, int oh_, int ow_,
                                          int c, const Store& store) {
  const int groups = c >> 3;
  const int g = (int)(i % groups);
  long long m = i / groups;
  const int ow = (int)(m % ow_); m /= ow_;
  const int oh = (int)(m % oh_); m /= oh_;
  const int od = (int)(m % od_); const long long s = m / od_;
  float best[8]; [[maybe_unused]] uint32_t idx[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    best[k] = -INFINITY;
    if constexpr (kArgmax) idx[k] = 13;                                 // the centre tap is always in range
  }
  for (int kd = 0; kd < 3; ++kd) {
    const int id = 2 * od - 1 + kd;
    if ((unsigned)id >= (unsigned)d) continue;
    for (int kh = 0; kh < 3; ++kh) {
      const int ih = 2 * oh - 1 + kh;
      if ((unsigned)ih >= (unsigned)h) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int iw = 2 * ow - 1 + kw;
        if ((unsigned)iw >= (unsigned)w) continue;
        Vec16<bf16_t> v;
        v.load(x + ((((s * d + id) * h + ih) * w + iw) * c + g * 8));
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          if constexpr (kArgmax) {
            if (v.f[k] > best[k]) { best[k] = v.f[k]; idx[k] = kd * 9 + kh * 3 + kw; }
          } else {
            best[k] = fmaxf(best[k], v.f[k]);
          }
        }
      }
    }
  }
  const long long out = (i / groups) * c + g * 8;
  if constexpr (kArgmax) store(out, idx); else store(out, best);
}

// ---------------------------------------------------------------------------------------------------- tail
// fp / ft: [items * c][vox][512] bf16; a voxel's feature vector is the c * 512 channels of its c samples.  Element offset of
// 16-byte vector ev (of the c * 64 of a feature vector) of item b at voxel 0
__device__ __forceinline__ long long tail_base(int b, int c, int ev, int vox) {
  return ((long long)(b * c + ev / (kFeat / 8)) * vox) * kFeat + (ev % (kFeat / 8)) * 8;
}

// pass 1 of a tail workgroup (item b, voxels [v0, v0 + 16)): per voxel vi the sums over the channels of p p and t t, and with
// kSums = 3 of p t, in a fixed order.  red[wave][kSums * vi + k] = the wave's share; the sum of the four waves is the caller's,
// after the barrier this ends with.
template <int kSums>
__device__ __forceinline__ void tail_sums(const bf16_t* __restrict__ fp, const bf16_t* __restrict__ ft, int b, int c, int vox, int v0,
                                          float (&red)[4][kSums * kTailVox]) {
  const int nvec = c * (kFeat / 8);                                       // 16-byte vectors per voxel
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float sq[kSums * kTailVox];
#pragma unroll
  for (int i = 0; i < kSums * kTailVox; ++i) sq[i] = 0.f;
  for (int ev = threadIdx.x; ev < nvec; ev += 256) {
    const long long base = tail_base(b, c, ev, vox);
#pragma unroll
    for (int vi = 0; vi < kTailVox; ++vi) {
      if (v0 + vi < vox) {
        Vec16<bf16_t> p, t;
        p.load(fp + base + (long long)(v0 + vi) * kFeat);
        t.load(ft + base + (long long)(v0 + vi) * kFeat);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          sq[kSums * vi] += p.f[k] * p.f[k]; sq[kSums * vi + 1] += t.f[k] * t.f[k];
          if constexpr (kSums == 3) sq[kSums * vi + 2] += p.f[k] * t.f[k];
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kSums * kTailVox; ++i) {
    const float s = wave_sum(sq[i]);
    if (lane == 0) red[wave][i] = s;
  }
  __syncthreads();
}

}  // namespace
