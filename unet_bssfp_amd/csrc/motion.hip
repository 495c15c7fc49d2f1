// tio.RandomMotion (the first stage of the reference's training transform, src/data_module.py:130-139) without an FFT
// and without the moved copies ever existing in HBM.  TorchIO composites the spectra of K + 1 rigidly
// moved copies x_k of the volume in bands along the LAST spatial axis and keeps the real part.  A band mask depends on
// the index along that axis only and the copies are real, so
//     y = real(ifftn(sum_k B_k . fftn(x_k))) = sum_k C_k x_k,     C_k a real N x N circulant applied along W.
// Two kernels:
//   resample_kernel : one rigid transform, trilinear, writes a volume (the resampling primitive on its own).
//   motion_kernel   : the fused stage.  A workgroup of 256 lanes owns 64 lines along W, as axis_apply_kernel<INNER1> of
//                     kspace.hip does.  For each image it fills the XOR-swizzled 32 KB LDS tile with the trilinearly
//                     resampled values of its lines (8 gathers per value; consecutive lanes walk along W of one line, and
//                     neighbouring lines are neighbouring h, so the gathers of a tile stay inside a few source rows), then
//                     adds C_k x_k into the SAME accumulators: each wave owns output rows in chunks of 8, the 8 matrix
//                     entries C_k[i0..i0+8)[j] are wave-uniform and come through the scalar cache (s_load_dwordx4 per
//                     row and 4 values of j, SGPR operands of v_pk_fma_f32; the matrices are read through the constant
//                     address space and their rows are padded to a multiple of 8 with zeros, see motion_kernel).  Sums
//                     run image by image, j in order, one fma per term.  Results return through the LDS tile for
//                     coalesced stores.
// Resampling (sitk.Resample with a linear interpolator, voxel spacing 1, physical point = voxel index): output voxel i reads
// the input at s = M i, three fmas per axis in f32 from the integer index.  Inside iff -0.5 <= s_a < N_a - 0.5 on every
// axis; then trilinear between floor(s) and floor(s) + 1, both clamped into [0, N_a - 1].  Outside: the fill value, which
// is the channel's minimum read from DEVICE memory (the (sum, min) pairs of mi355_channel_sum_min), so no call waits for
// the device.  Every gather index is clamped, so no transform can make a load leave the volume; a NaN coordinate fails the
// inside test.  No atomics, no scratch, no host synchronisation.
#include "common.h"
#include "resample_core.h"

namespace {

constexpr int kMaxN = MI355_AXIS_MAX_N;   // 128
constexpr int kCols = 64;                 // lines per workgroup = lanes per wave
constexpr int kRows = 8;                  // output rows per chunk (one scalar load group per j)
constexpr int kWaves = 4;
constexpr int kChunks = kMaxN / kRows / kWaves;   // chunks per wave at N = 128
constexpr int kThreads = kWaves * 64;
constexpr int kMaxImages = MI355_MOTION_MAX_IMAGES;

typedef __attribute__((address_space(4))) float ConstF;   // a float in the constant address space (scalar loads)

__device__ __forceinline__ int swz(int j, int t) { return j * kCols + (t ^ (j & (kCols - 1))); }

struct ResampleArgs {
  const float* x; float* out; const double* cmin;   // cmin: null, or (sum, min) pairs per channel
  float fill;
  int c, d, h, w, groups;                           // groups of 4 voxels per line
  long long total;                                  // lanes with work
  Rigid q;
};

// one lane owns 4 consecutive voxels of one line along W; VEC: W is a multiple of 4 and out is 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(256) void resample_kernel(const ResampleArgs a) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.total) return;
  const int w0 = (int)(g % a.groups) * 4;
  const long long line = g / a.groups;
  const int ih = (int)(line % a.h), id = (int)(line / a.h % a.d), ch = (int)(line / ((long long)a.h * a.d));
  const float* __restrict__ xc = a.x + (long long)ch * a.d * a.h * a.w;
  const float fill = a.cmin ? (float)a.cmin[2 * ch + 1] : a.fill;
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = w0 + e < a.w ? sample(xc, a.q, a.d, a.h, a.w, id, ih, w0 + e, fill) : 0.f;
  float* __restrict__ o = a.out + line * a.w + w0;
  if constexpr (VEC) {
    *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (w0 + e < a.w) o[e] = v[e];
  }
}

struct MotionArgs {
  const float* x; float* y;
  const float* cmat;            // [nimg][Npad][N] row-major band circulants, Npad = N rounded up to a multiple of 8
  const double* cmin;           // (sum, min) pairs per channel
  int nimg, c, d, h, w;
  long long lines;              // C D H
  Rigid q[kMaxImages];
};

__global__ __launch_bounds__(kThreads) void motion_kernel(const MotionArgs a) {
  __shared__ float xs[kMaxN * kCols];
  __shared__ int line_ch[kCols], line_d[kCols], line_h[kCols];
  __shared__ float line_fill[kCols];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = a.w;
  const long long l0 = (long long)blockIdx.x * kCols;
  const long long base = l0 * n;
  const int valid = a.lines - l0 < kCols ? (int)(a.lines - l0) : kCols;
  const long long vol = (long long)a.d * a.h * a.w;
  if (tid < valid) {                                   // where each line of the tile sits, once per workgroup
    const long long line = l0 + tid;
    const int ch = (int)(line / ((long long)a.h * a.d));
    line_ch[tid] = ch;
    line_d[tid] = (int)(line / a.h % a.d);
    line_h[tid] = (int)(line % a.h);
    line_fill[tid] = (float)a.cmin[2 * ch + 1];
  }
  // element idx = tid + 256 it of the tile is (line t, voxel j) = (idx / n, idx % n): consecutive lanes walk along W
  const int j0 = tid % n, t0 = tid / n, dj = kThreads % n, dt = kThreads / n;

  float acc[kChunks][kRows];
#pragma unroll
  for (int cc = 0; cc < kChunks; ++cc)
#pragma unroll
    for (int r = 0; r < kRows; ++r) acc[cc][r] = 0.f;
  const int nchunks = (n + kRows - 1) / kRows;

  for (int k = 0; k < a.nimg; ++k) {
    __syncthreads();                                   // the line table is written / every wave is done with the last tile
    const Rigid& q = a.q[k];
    for (int j = j0, t = t0; t < valid;) {
      const float* __restrict__ xc = a.x + line_ch[t] * vol;
      xs[swz(j, t)] = sample(xc, q, a.d, a.h, a.w, line_d[t], line_h[t], j, line_fill[t]);
      j += dj;
      t += dt;
      if (j >= n) { j -= n; ++t; }
    }
    __syncthreads();
    // The band matrices are read-only for the whole launch.  Reading them through the constant address space says so to
    // the compiler: behind the loop-carried barriers and LDS stores of the k loop it does not prove a plain global load
    // unclobbered, and would fetch the wave-uniform rows with vector loads instead of s_load.
    const ConstF* mk = (const ConstF*)(a.cmat + (long long)k * nchunks * kRows * n);
#pragma unroll
    for (int cc = 0; cc < kChunks; ++cc) {
      const int chunk = wave + kWaves * cc;
      if (chunk >= nchunks) continue;
      // The offset of the chunk's first row does not depend on k, so the compiler would hoist the row addresses of all
      // four chunks (and of their remainder loops) out of the k loop and keep them in SGPRs across it: 60 spilled SGPRs.
      // The empty statement makes the offset opaque, so that it is recomputed here (one s_mul) and nothing spills.
      int row0 = chunk * kRows * n;
      asm volatile("" : "+s"(row0));
      const ConstF* mrow = mk + row0;
      const ConstF* m0[kRows];
#pragma unroll
      for (int r = 0; r < kRows; ++r) m0[r] = mrow + r * n;   // rows past N are the zero rows of the padding: sums dropped
      for (int j = 0; j < n; ++j) {
        const float xv = xs[swz(j, lane)];
#pragma unroll
        for (int r = 0; r < kRows; ++r) acc[cc][r] = fmaf(m0[r][j], xv, acc[cc][r]);
      }
    }
  }

  __syncthreads();                                     // every wave is done reading the last tile
#pragma unroll
  for (int cc = 0; cc < kChunks; ++cc)
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      const int i = (wave + kWaves * cc) * kRows + r;
      if (i < n) xs[swz(i, lane)] = acc[cc][r];
    }
  __syncthreads();
  for (int idx = tid; idx < valid * n; idx += kThreads) a.y[base + idx] = xs[swz(idx % n, idx / n)];
}

int check_rigid(const char* what, const float* m, int count) {
  for (int i = 0; i < count; ++i) MI355_REQUIRE(m[i] == m[i] && m[i] - m[i] == 0.f, "%s: matrix entry %d is not finite", what, i);
  return MI355_OK;
}

}  // namespace

extern "C" int mi355_rigid_resample(const float* x, float* out, int32_t c, int32_t d, int32_t h, int32_t w, const float* m,
                                    const double* channel_min, float fill, void* stream) {
  MI355_REQUIRE(x && out && m && x != out, "rigid_resample: null pointer or in-place call");
  MI355_REQUIRE(c > 0 && d > 0 && h > 0 && w > 0, "rigid_resample: bad shape");
  if (const int rc = check_rigid("rigid_resample", m, 12)) return rc;
  ResampleArgs a{x, out, channel_min, fill, c, d, h, w, (w + 3) / 4, 0, {}};
  a.total = (long long)c * d * h * a.groups;
  MI355_REQUIRE((a.total + 255) / 256 < (1LL << 31), "rigid_resample: volume too large");
  for (int i = 0; i < 12; ++i) a.q.m[i] = m[i];
  const unsigned grid = (unsigned)((a.total + 255) / 256);
  if (w % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) resample_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
  else resample_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(a);
  return mi355_check_launch("rigid_resample");
}

extern "C" int mi355_aug_motion(const float* x, float* out, int32_t c, int32_t d, int32_t h, int32_t w, int32_t nimg,
                                const float* m, const float* band_matrices, const double* channel_min, void* stream) {
  MI355_REQUIRE(x && out && m && band_matrices && channel_min && x != out, "aug_motion: null pointer or in-place call");
  MI355_REQUIRE(c > 0 && d > 0 && h > 0 && w > 0 && nimg > 0, "aug_motion: bad shape or image count");
  if (nimg > kMaxImages) {
    mi355_set_error("aug_motion: %d images exceed %d", nimg, kMaxImages);
    return MI355_ERR_UNSUPPORTED;
  }
  if (w > kMaxN) {
    mi355_set_error("aug_motion: extent %d along axis 2 exceeds %d (larger extents are not tiled)", w, kMaxN);
    return MI355_ERR_UNSUPPORTED;
  }
  if (const int rc = check_rigid("aug_motion", m, 12 * nimg)) return rc;
  MotionArgs a{x, out, band_matrices, channel_min, nimg, c, d, h, w, (long long)c * d * h, {}};
  const long long tiles = (a.lines + kCols - 1) / kCols;
  MI355_REQUIRE(tiles < (1LL << 31), "aug_motion: volume too large");
  for (int i = 0; i < 12 * nimg; ++i) a.q[i / 12].m[i % 12] = m[i];
  motion_kernel<<<(unsigned)tiles, kThreads, 0, (hipStream_t)stream>>>(a);
  return mi355_check_launch("aug_motion");
}
