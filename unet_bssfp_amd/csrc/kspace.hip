// k-space and blur augmentations of the reference's training transform (src/data_module.py:130-139: tio.RandomGhosting,
// tio.RandomSpike, tio.RandomBlur) without an FFT.  All three reduce to ONE primitive:
//     out[o][i][t] = sum_j M[i][j] * x[o][j][t]
// a small dense N x N matrix applied along one axis of a contiguous f32 (C, D, H, W) tensor, seen as (outer, N, inner):
//   axis D: outer = C,     inner = H W        axis H: outer = C D, inner = W        axis W: outer = C D H, inner = 1
// Ghosting is a circulant along one axis, blur a banded matrix per axis, and the forward 3-D DFT whose maximum RandomSpike
// needs is three passes of a complex DFT matrix (W, H, D), the last of which reduces instead of writing.
//
// One workgroup (256 lanes, 4 waves) owns a tile of 64 lines: it loads x[o][0..N)[t0..t0+64) into LDS once (coalesced along
// t; along W the 64 lines are one contiguous run of 64 N floats), then lane t walks j with ONE conflict-free LDS read per
// 8 FMAs: each wave owns output rows in chunks of 8, and the 8 matrix entries M[i0..i0+8)[j] are wave-uniform, so they
// come through the scalar cache and enter v_fmac as SGPR operands.  Sums run over j in order with one fma per term: the
// error of a real output is bounded by gamma_N sum_j |M_ij x_j|.  Along W the results go back through the LDS tile so that
// the stores are coalesced too.  The LDS column is XOR-swizzled with j, which keeps both the transposing load along W and
// the compute reads free of bank conflicts with a pitch of exactly 64 floats (32 KB per tile, 64 KB at most).
// N <= MI355_AXIS_MAX_N (128); larger extents are rejected, not tiled.  No atomics: reductions finish in a second launch.
#include "common.h"

namespace {

constexpr int kMaxN = MI355_AXIS_MAX_N;   // 128
constexpr int kCols = 64;                 // lines per workgroup = lanes per wave
constexpr int kRows = 8;                  // output rows per chunk (one scalar load group per j)
constexpr int kWaves = 4;
constexpr int kChunks = kMaxN / kRows / kWaves;   // chunks per wave at N = 128
constexpr int kThreads = kWaves * 64;

struct AxisArgs {
  const float* x0; const float* x1;       // input planes (x1: imaginary part or null)
  const float* m0; const float* m1;       // matrix planes, row-major [N][N] (m1: imaginary part or null)
  float* y0; float* y1;                   // output planes
  float* part;                            // REDUCE: [blocks][2] (max Re, |Im| there)
  int n;
  long long outer, inner, tiles;          // tiles per o (inner > 1) or in all (inner == 1)
};

__device__ __forceinline__ int swz(int j, int t) { return j * kCols + (t ^ (j & (kCols - 1))); }

// (re, |im|) ordered lexicographically
__device__ __forceinline__ void lexmax(float& re, float& im, float r2, float i2) {
  if (r2 > re || (r2 == re && i2 > im)) { re = r2; im = i2; }
}

// INNER1: the axis is W.  NIN: input planes.  CPLX: complex matrix and output.  REDUCE: write no output, reduce to the
// lexicographic maximum of (Re, |Im|) per workgroup.
template <bool INNER1, int NIN, bool CPLX, bool REDUCE>
__global__ __launch_bounds__(kThreads) void axis_apply_kernel(const AxisArgs a) {
  constexpr int kTiles = INNER1 && CPLX && !REDUCE ? 2 : NIN;
  __shared__ float xs[kTiles][kMaxN * kCols];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = a.n;
  long long base;      // first element of the tile's line 0, j = 0
  int valid;           // lines of the tile that exist
  if constexpr (INNER1) {
    const long long l0 = (long long)blockIdx.x * kCols;
    base = l0 * n;
    valid = a.outer - l0 < kCols ? (int)(a.outer - l0) : kCols;
  } else {
    const long long o = blockIdx.x / a.tiles, t0 = (blockIdx.x % a.tiles) * kCols;
    base = o * n * a.inner + t0;
    valid = a.inner - t0 < kCols ? (int)(a.inner - t0) : kCols;
  }
#pragma unroll
  for (int p = 0; p < NIN; ++p) {
    const float* __restrict__ x = p ? a.x1 : a.x0;
    if constexpr (INNER1) {
      for (int idx = tid; idx < valid * n; idx += kThreads) xs[p][swz(idx % n, idx / n)] = x[base + idx];
    } else {
      for (int idx = tid; idx < n * kCols; idx += kThreads) {
        const int j = idx >> 6, t = idx & 63;
        if (t < valid) xs[p][swz(j, t)] = x[base + j * a.inner + t];
      }
    }
  }
  __syncthreads();

  const int nchunks = (n + kRows - 1) / kRows;
  float re[kChunks][kRows], im[kChunks][kRows];
#pragma unroll
  for (int cc = 0; cc < kChunks; ++cc) {
#pragma unroll
    for (int r = 0; r < kRows; ++r) re[cc][r] = im[cc][r] = 0.f;
    const int chunk = wave + kWaves * cc;
    if (chunk >= nchunks) continue;
    const float* __restrict__ m0[kRows];
    const float* __restrict__ m1[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {                 // rows past N repeat the last one; their sums are dropped
      const int row = min(chunk * kRows + r, n - 1);
      m0[r] = a.m0 + row * n;
      m1[r] = CPLX ? a.m1 + row * n : nullptr;
    }
    for (int j = 0; j < n; ++j) {
      const float xr = xs[0][swz(j, lane)];
      float xi = 0.f;
      if constexpr (NIN == 2) xi = xs[1][swz(j, lane)];
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        const float mr = m0[r][j];
        re[cc][r] = fmaf(mr, xr, re[cc][r]);
        if constexpr (CPLX) {
          const float mi = m1[r][j];
          im[cc][r] = fmaf(mi, xr, im[cc][r]);
          if constexpr (NIN == 2) {
            re[cc][r] = fmaf(-mi, xi, re[cc][r]);
            im[cc][r] = fmaf(mr, xi, im[cc][r]);
          }
        }
      }
    }
  }

  if constexpr (REDUCE) {
    float br = -INFINITY, bi = 0.f;
    if (lane < valid) {
#pragma unroll
      for (int cc = 0; cc < kChunks; ++cc)
#pragma unroll
        for (int r = 0; r < kRows; ++r)
          if ((wave + kWaves * cc) * kRows + r < n) lexmax(br, bi, re[cc][r], fabsf(im[cc][r]));
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) lexmax(br, bi, __shfl_xor(br, s, 64), __shfl_xor(bi, s, 64));
    __syncthreads();                                   // the input tile is free: its first floats hold the waves' maxima
    float* red = xs[0];
    if (lane == 0) { red[2 * wave] = br; red[2 * wave + 1] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < kWaves; ++w) lexmax(br, bi, red[2 * w], red[2 * w + 1]);
      a.part[2LL * blockIdx.x] = br;
      a.part[2LL * blockIdx.x + 1] = bi;
    }
  } else if constexpr (INNER1) {
    __syncthreads();                                   // every wave is done reading the input tile
#pragma unroll
    for (int cc = 0; cc < kChunks; ++cc)
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        const int i = (wave + kWaves * cc) * kRows + r;
        if (i < n) {
          xs[0][swz(i, lane)] = re[cc][r];
          if constexpr (CPLX) xs[1][swz(i, lane)] = im[cc][r];
        }
      }
    __syncthreads();
    for (int idx = tid; idx < valid * n; idx += kThreads) {
      a.y0[base + idx] = xs[0][swz(idx % n, idx / n)];
      if constexpr (CPLX) a.y1[base + idx] = xs[1][swz(idx % n, idx / n)];
    }
  } else {
    if (lane < valid) {
#pragma unroll
      for (int cc = 0; cc < kChunks; ++cc)
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
          const int i = (wave + kWaves * cc) * kRows + r;
          if (i < n) {
            a.y0[base + i * a.inner + lane] = re[cc][r];
            if constexpr (CPLX) a.y1[base + i * a.inner + lane] = im[cc][r];
          }
        }
    }
  }
}

// per channel: lexicographic maximum of `nparts` (Re, |Im|) pairs -> out[c] = (double Re, double |Im|)
__global__ __launch_bounds__(256) void lexmax_finalize_kernel(const float* __restrict__ part, int nparts, double* __restrict__ out) {
  const int c = blockIdx.x;
  const float* __restrict__ p = part + 2LL * c * nparts;
  float br = -INFINITY, bi = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) lexmax(br, bi, p[2 * i], p[2 * i + 1]);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) lexmax(br, bi, __shfl_xor(br, s, 64), __shfl_xor(bi, s, 64));
  __shared__ float red[4][2];
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = br; red[threadIdx.x >> 6][1] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) lexmax(br, bi, red[w][0], red[w][1]);
    out[2 * c] = br;
    out[2 * c + 1] = bi;
  }
}

constexpr int kSumBlocks = MI355_KSPACE_SUM_BLOCKS;   // partial sums per channel

// per channel (sum, min) in f64: grid (kSumBlocks, C) partials, then one block per channel
__global__ __launch_bounds__(256) void sum_min_kernel(const float* __restrict__ x, long long vol, double* __restrict__ part) {
  const float* __restrict__ xc = x + (long long)blockIdx.y * vol;
  double s = 0.0;
  float mn = INFINITY;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < vol; i += 256LL * kSumBlocks) {
    const float v = xc[i];
    s += (double)v;
    mn = fminf(mn, v);
  }
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) { s += __shfl_xor(s, k, 64); mn = fminf(mn, __shfl_xor(mn, k, 64)); }
  __shared__ double rs[4];
  __shared__ float rm[4];
  if ((threadIdx.x & 63) == 0) { rs[threadIdx.x >> 6] = s; rm[threadIdx.x >> 6] = mn; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = part + 2LL * ((long long)blockIdx.y * kSumBlocks + blockIdx.x);
    o[0] = (rs[0] + rs[1]) + (rs[2] + rs[3]);
    o[1] = (double)fminf(fminf(rm[0], rm[1]), fminf(rm[2], rm[3]));
  }
}

__global__ __launch_bounds__(64) void sum_min_finalize_kernel(const double* __restrict__ part, double* __restrict__ out) {
  const double* p = part + 2LL * blockIdx.x * kSumBlocks;
  double s = 0.0, mn = INFINITY;
  for (int i = threadIdx.x; i < kSumBlocks; i += 64) { s += p[2 * i]; mn = fmin(mn, p[2 * i + 1]); }
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) { s += __shfl_xor(s, k, 64); mn = fmin(mn, __shfl_xor(mn, k, 64)); }
  if (threadIdx.x == 0) { out[2 * blockIdx.x] = s; out[2 * blockIdx.x + 1] = mn; }
}

struct SpikeArgs { int c, d, h, w, f0, f1, f2, dc; float intensity, inv_n; };

// out = x + Re(a e^{+2 pi i (f0 n0 / N0 + f1 n1 / N1 + f2 n2 / N2)}) / (N0 N1 N2), a = M[c] * intensity.  The phase is
// reduced exactly in integers ((f_d n_d) mod N_d, then one common fraction in [0, 1)) before sincospif sees it.
__global__ __launch_bounds__(256) void spike_add_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                        const double* __restrict__ m, const SpikeArgs q) {
  const long long vol = (long long)q.d * q.h * q.w;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= vol) return;
  const int n2 = (int)(i % q.w), n1 = (int)(i / q.w % q.h), n0 = (int)(i / ((long long)q.w * q.h));
  const long long p0 = (long long)q.f0 * n0 % q.d, p1 = (long long)q.f1 * n1 % q.h, p2 = (long long)q.f2 * n2 % q.w;   // f >= 0
  const long long num = (p0 * q.h * q.w + p1 * (long long)q.d * q.w + p2 * (long long)q.d * q.h) % vol;
  const float t = (float)((double)num / (double)vol);
  float sn, cs;
  sincospif(2.f * t, &sn, &cs);
  for (int ch = 0; ch < q.c; ++ch) {
    const float ar = (float)(m[2 * ch] * (double)q.intensity);
    const float ai = q.dc ? 0.f : (float)(m[2 * ch + 1] * (double)q.intensity);
    const float wv = fmaf(ar, cs, -(ai * sn));
    out[ch * vol + i] = fmaf(wv, q.inv_n, x[ch * vol + i]);
  }
}

int axis_dims(const char* what, int c, int d, int h, int w, int axis, int& n, long long& outer, long long& inner) {
  MI355_REQUIRE(c > 0 && d > 0 && h > 0 && w > 0 && axis >= 0 && axis <= 2, "%s: bad shape or axis", what);
  n = axis == 0 ? d : axis == 1 ? h : w;
  outer = axis == 0 ? c : axis == 1 ? (long long)c * d : (long long)c * d * h;
  inner = axis == 0 ? (long long)h * w : axis == 1 ? w : 1;
  if (n > kMaxN) {
    mi355_set_error("%s: extent %d along axis %d exceeds %d (larger extents are not tiled)", what, n, axis, kMaxN);
    return MI355_ERR_UNSUPPORTED;
  }
  MI355_REQUIRE(outer * ((inner + kCols - 1) / kCols) < (1LL << 31), "%s: volume too large", what);
  return MI355_OK;
}

}  // namespace

extern "C" int mi355_axis_apply(const float* x, const float* m, float* out, int32_t c, int32_t d, int32_t h, int32_t w,
                                int32_t axis, void* stream) {
  int n;
  long long outer, inner;
  if (const int rc = axis_dims("axis_apply", c, d, h, w, axis, n, outer, inner)) return rc;
  MI355_REQUIRE(x && m && out && x != out, "axis_apply: null pointer or in-place call");
  AxisArgs a{x, nullptr, m, nullptr, out, nullptr, nullptr, n, outer, inner, 0};
  if (inner == 1) {
    a.tiles = (outer + kCols - 1) / kCols;
    axis_apply_kernel<true, 1, false, false><<<(unsigned)a.tiles, kThreads, 0, (hipStream_t)stream>>>(a);
  } else {
    a.tiles = (inner + kCols - 1) / kCols;
    axis_apply_kernel<false, 1, false, false><<<(unsigned)(a.tiles * outer), kThreads, 0, (hipStream_t)stream>>>(a);
  }
  return mi355_check_launch("axis_apply");
}

extern "C" int mi355_axis_apply_complex(const float* xr, const float* xi, const float* mr, const float* mi, float* outr,
                                        float* outi, int32_t c, int32_t d, int32_t h, int32_t w, int32_t axis, void* stream) {
  int n;
  long long outer, inner;
  if (const int rc = axis_dims("axis_apply_complex", c, d, h, w, axis, n, outer, inner)) return rc;
  MI355_REQUIRE(xr && mr && mi && outr && outi && outr != xr && outr != xi && outi != xr && outi != xi && outr != outi,
                "axis_apply_complex: null pointer or aliased planes");
  AxisArgs a{xr, xi, mr, mi, outr, outi, nullptr, n, outer, inner, 0};
  if (inner == 1 && !xi) {
    a.tiles = (outer + kCols - 1) / kCols;
    axis_apply_kernel<true, 1, true, false><<<(unsigned)a.tiles, kThreads, 0, (hipStream_t)stream>>>(a);
  } else {   // a complex input along W takes the strided form with one line per workgroup: correct, not fast, not on the DFT chain
    a.tiles = (inner + kCols - 1) / kCols;
    const unsigned grid = (unsigned)(a.tiles * outer);
    if (xi) axis_apply_kernel<false, 2, true, false><<<grid, kThreads, 0, (hipStream_t)stream>>>(a);
    else axis_apply_kernel<false, 1, true, false><<<grid, kThreads, 0, (hipStream_t)stream>>>(a);
  }
  return mi355_check_launch("axis_apply_complex");
}

extern "C" int64_t mi355_kspace_workspace_bytes(int32_t c, int32_t d, int32_t h, int32_t w) {
  if (c <= 0 || d <= 0 || h <= 0 || w <= 0) return -1;
  const long long tiles = ((long long)h * w + kCols - 1) / kCols;
  const long long a = (long long)c * tiles * 2 * sizeof(float), b = (long long)c * kSumBlocks * 2 * sizeof(double);
  return a > b ? a : b;
}

extern "C" int mi355_axis_apply_complex_max(const float* xr, const float* xi, const float* mr, const float* mi, int32_t c,
                                            int32_t d, int32_t h, int32_t w, void* workspace, int64_t workspace_bytes,
                                            double* out, void* stream) {
  int n;
  long long outer, inner;
  if (const int rc = axis_dims("axis_apply_complex_max", c, d, h, w, 0, n, outer, inner)) return rc;
  MI355_REQUIRE(xr && mr && mi && workspace && out, "axis_apply_complex_max: null pointer");
  MI355_REQUIRE(workspace_bytes >= mi355_kspace_workspace_bytes(c, d, h, w), "axis_apply_complex_max: workspace too small");
  AxisArgs a{xr, xi, mr, mi, nullptr, nullptr, (float*)workspace, n, outer, inner, (inner + kCols - 1) / kCols};
  const unsigned grid = (unsigned)(a.tiles * outer);
  if (xi) axis_apply_kernel<false, 2, true, true><<<grid, kThreads, 0, (hipStream_t)stream>>>(a);
  else axis_apply_kernel<false, 1, true, true><<<grid, kThreads, 0, (hipStream_t)stream>>>(a);
  lexmax_finalize_kernel<<<c, 256, 0, (hipStream_t)stream>>>((const float*)workspace, (int)a.tiles, out);
  return mi355_check_launch("axis_apply_complex_max");
}

extern "C" int mi355_channel_sum_min(const float* x, int32_t c, int64_t vol, void* workspace, int64_t workspace_bytes,
                                     double* out, void* stream) {
  MI355_REQUIRE(x && workspace && out && c > 0 && c <= 65535 && vol > 0, "channel_sum_min: bad argument");
  MI355_REQUIRE(workspace_bytes >= (int64_t)c * kSumBlocks * 2 * (int64_t)sizeof(double), "channel_sum_min: workspace too small");
  sum_min_kernel<<<dim3(kSumBlocks, c), 256, 0, (hipStream_t)stream>>>(x, vol, (double*)workspace);
  sum_min_finalize_kernel<<<c, 64, 0, (hipStream_t)stream>>>((const double*)workspace, out);
  return mi355_check_launch("channel_sum_min");
}

extern "C" int mi355_aug_spike_add(const float* x, float* out, int32_t c, int32_t d, int32_t h, int32_t w, int32_t f0,
                                   int32_t f1, int32_t f2, const double* m, int32_t dc, float intensity, void* stream) {
  MI355_REQUIRE(x && out && m && c > 0 && d > 0 && h > 0 && w > 0, "aug_spike_add: bad argument");
  const long long vol = (long long)d * h * w;
  // frequencies enter as residues so that every product in the kernel is non-negative
  const SpikeArgs q{c, d, h, w, ((f0 % d) + d) % d, ((f1 % h) + h) % h, ((f2 % w) + w) % w, dc != 0, intensity,
                    (float)(1.0 / (double)vol)};
  spike_add_kernel<<<(unsigned)((vol + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, out, m, q);
  return mi355_check_launch("aug_spike_add");
}
