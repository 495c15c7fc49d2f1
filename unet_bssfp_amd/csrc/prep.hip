// Streaming preprocessing kernels (doc/thesis/03-methods.tex:669-685): dataset ranges, the phase-cycled bSSFP
// rotation and channel assembly, and the masked normalised copy behind the T1w input.  All tensors are channel-first f32
// [c][nvox]; per-voxel arithmetic is f64 (dtifit_core.h) with one rounding at the store.
#include <math.h>
#include "common.h"
#include "dtifit_core.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// ---- mi355_channel_minmax -------------------------------------------------------------------------------------------------
// Min / max of floats through integer atomics on their bits: non-negative floats order like signed integers, negative ones
// in reverse like unsigned integers.  -0 has been mapped to +0, NaN never arrives here.
__device__ __forceinline__ void atomic_min_f32(float* p, float v) {
  if (v >= 0.f) atomicMin(reinterpret_cast<int*>(p), __float_as_int(v));
  else atomicMax(reinterpret_cast<unsigned*>(p), __float_as_uint(v));
}
__device__ __forceinline__ void atomic_max_f32(float* p, float v) {
  if (v >= 0.f) atomicMax(reinterpret_cast<int*>(p), __float_as_int(v));
  else atomicMin(reinterpret_cast<unsigned*>(p), __float_as_uint(v));
}

__device__ __forceinline__ void fold(float x, bool on, float& lo, float& hi) {
  if (on && x == x) {
    x += 0.f;
    lo = fminf(lo, x);
    hi = fmaxf(hi, x);
  }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void channel_minmax_kernel(const float* x, long long nvox, const unsigned char* mask,
                                                                  float* minmax) {
  const float* xc = x + (long long)blockIdx.y * nvox;
  float lo = INFINITY, hi = -INFINITY;
  const long long step = (long long)gridDim.x * kThreads;
  if (VEC) {                               // nvox % 4 == 0, 16-byte aligned channels, 4-byte aligned mask
    const long long n4 = nvox / 4;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n4; i += step) {
      const float4 q = reinterpret_cast<const float4*>(xc)[i];
      uchar4 k = make_uchar4(1, 1, 1, 1);
      if (mask) k = reinterpret_cast<const uchar4*>(mask)[i];
      fold(q.x, k.x != 0, lo, hi); fold(q.y, k.y != 0, lo, hi); fold(q.z, k.z != 0, lo, hi); fold(q.w, k.w != 0, lo, hi);
    }
  } else {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < nvox; i += step)
      fold(xc[i], !mask || mask[i] != 0, lo, hi);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
  }
  __shared__ float slo[kWaves], shi[kWaves];
  if ((threadIdx.x & 63) == 0) { slo[threadIdx.x >> 6] = lo; shi[threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < kWaves; ++i) { lo = fminf(lo, slo[i]); hi = fmaxf(hi, shi[i]); }
    if (lo <= hi) {                        // the block saw at least one value
      atomic_min_f32(minmax + 2 * blockIdx.y, lo);
      atomic_max_f32(minmax + 2 * blockIdx.y + 1, hi);
    }
  }
}

// ---- bSSFP phase sums -----------------------------------------------------------------------------------------------------
// fixed-order sum of one (re, im) pair per thread over the block: tree in LDS, result in thread 0
__device__ __forceinline__ void block_sum2(double& re, double& im, double* sh) {
  sh[2 * threadIdx.x] = re;
  sh[2 * threadIdx.x + 1] = im;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sh[2 * threadIdx.x] += sh[2 * (threadIdx.x + o)];
      sh[2 * threadIdx.x + 1] += sh[2 * (threadIdx.x + o) + 1];
    }
    __syncthreads();
  }
  re = sh[0];
  im = sh[1];
}

__global__ __launch_bounds__(kThreads) void phase_sums_stage1(const float* mag, const float* raw, long long nvox, double* part) {
  __shared__ double sh[2 * kThreads];
  const long long base = (long long)blockIdx.y * nvox;
  double re = 0.0, im = 0.0;
  for (long long v = (long long)blockIdx.x * kThreads + threadIdx.x; v < nvox; v += (long long)gridDim.x * kThreads) {
    const double m = (double)mag[base + v], phi = prep_phase((double)raw[base + v]);
    double sn, cs;
    sincos(phi, &sn, &cs);
    re += m * cs;
    im += m * sn;
  }
  block_sum2(re, im, sh);
  if (threadIdx.x == 0) {
    double* o = part + 2 * ((long long)blockIdx.y * gridDim.x + blockIdx.x);
    o[0] = re;
    o[1] = im;
  }
}

__global__ __launch_bounds__(kThreads) void phase_sums_stage2(const double* part, int nb, double* sums) {
  __shared__ double sh[2 * kThreads];
  const double* p = part + 2 * (long long)blockIdx.x * nb;
  double re = 0.0, im = 0.0;
  for (int b = threadIdx.x; b < nb; b += kThreads) { re += p[2 * b]; im += p[2 * b + 1]; }
  block_sum2(re, im, sh);
  if (threadIdx.x == 0) { sums[2 * blockIdx.x] = re; sums[2 * blockIdx.x + 1] = im; }
}

int phase_sum_blocks(long long nvox) {     // a function of the voxel count alone: the summation order is fixed
  const long long b = (nvox + 8 * kThreads - 1) / (8 * kThreads);
  return (int)(b < 1 ? 1 : b > 512 ? 512 : b);
}

__global__ __launch_bounds__(kThreads) void phase_correct_kernel(const float* mag, const float* raw, long long nvox,
                                                                 const double* sums, float* re, float* im) {
  const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (v >= nvox) return;
  const double theta = atan2(sums[2 * blockIdx.y + 1], sums[2 * blockIdx.y]);     // uniform over the block
  const long long i = (long long)blockIdx.y * nvox + v;
  const double m = (double)mag[i], phi = prep_phase((double)raw[i]) - theta;
  double sn, cs;
  sincos(phi, &sn, &cs);
  re[i] = (float)(m * cs);
  im[i] = (float)(m * sn);
}

// ---- channel assembly -----------------------------------------------------------------------------------------------------
struct AssembleArgs {
  const float* re; const float* im; int p; long long nvox; const unsigned char* mask;
  double mag_lo, mag_hi, pha_lo, pha_hi; int repeat; float* out;
};

__global__ __launch_bounds__(kThreads) void bssfp_assemble_kernel(AssembleArgs a) {
  const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (v >= a.nvox) return;
  const bool on = !a.mask || a.mask[v] != 0;
  float fm = 0.f, fp = 0.f;
  for (int i = 0; i < a.p; ++i) {
    if (on && (a.repeat < 0 || i == 0)) {
      const long long s = (long long)(a.repeat < 0 ? i : a.repeat) * a.nvox + v;
      const double x = (double)a.re[s], y = (double)a.im[s];
      fm = (float)prep_normalize(sqrt(x * x + y * y), a.mag_lo, a.mag_hi);
      fp = (float)prep_normalize(atan2(y, x), a.pha_lo, a.pha_hi);
    }
    a.out[(long long)(2 * i) * a.nvox + v] = fm;
    a.out[(long long)(2 * i + 1) * a.nvox + v] = fp;
  }
}

// ---- masked normalised copy with a source-channel map ---------------------------------------------------------------------
struct NormArgs {
  const float* src; float* dst; long long nvox; const unsigned char* mask; int c_out;
  int map[MI355_PREP_MAX_CHANNELS]; double lo[MI355_PREP_MAX_CHANNELS], hi[MI355_PREP_MAX_CHANNELS];
};

template <bool VEC>
__global__ __launch_bounds__(kThreads) void normalize_channels_kernel(NormArgs a) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (VEC) {                               // nvox % 4 == 0, 16-byte aligned tensors, 4-byte aligned mask
    if (i >= a.nvox / 4) return;
    uchar4 k = make_uchar4(1, 1, 1, 1);
    if (a.mask) k = reinterpret_cast<const uchar4*>(a.mask)[i];
    for (int c = 0; c < a.c_out; ++c) {
      const float4 q = reinterpret_cast<const float4*>(a.src + (long long)a.map[c] * a.nvox)[i];
      float4 o;
      o.x = k.x ? (float)prep_normalize((double)q.x, a.lo[c], a.hi[c]) : 0.f;
      o.y = k.y ? (float)prep_normalize((double)q.y, a.lo[c], a.hi[c]) : 0.f;
      o.z = k.z ? (float)prep_normalize((double)q.z, a.lo[c], a.hi[c]) : 0.f;
      o.w = k.w ? (float)prep_normalize((double)q.w, a.lo[c], a.hi[c]) : 0.f;
      reinterpret_cast<float4*>(a.dst + (long long)c * a.nvox)[i] = o;
    }
  } else {
    if (i >= a.nvox) return;
    const bool on = !a.mask || a.mask[i] != 0;
    for (int c = 0; c < a.c_out; ++c)
      a.dst[(long long)c * a.nvox + i] =
          on ? (float)prep_normalize((double)a.src[(long long)a.map[c] * a.nvox + i], a.lo[c], a.hi[c]) : 0.f;
  }
}

bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }
bool nvox_ok(int64_t nvox) { return nvox >= 0 && nvox < (1ll << 36); }

}  // namespace

extern "C" int mi355_channel_minmax(const float* x, int32_t c, int64_t nvox, const uint8_t* mask, float* minmax, void* stream) {
  MI355_REQUIRE(c >= 1 && c <= 65535, "channel_minmax: bad channel count %d", (int)c);
  MI355_REQUIRE(nvox_ok(nvox), "channel_minmax: bad voxel count %lld", (long long)nvox);
  MI355_REQUIRE(x && minmax, "channel_minmax: null pointer");
  if (nvox == 0) return MI355_OK;
  const bool vec = nvox % 4 == 0 && aligned(x, 16) && (!mask || aligned(mask, 4));
  // about 2048 workgroups in all: each ends in two atomics on its channel's pair, and the atomics of one address serialise
  const long long per = (long long)kThreads * (vec ? 16 : 4), cap = 2048 / c > 1 ? 2048 / c : 1;
  long long bx = (nvox + per - 1) / per;
  bx = bx > cap ? cap : bx;
  const dim3 grid((unsigned)bx, (unsigned)c);
  hipStream_t s = (hipStream_t)stream;
  if (vec) channel_minmax_kernel<true><<<grid, kThreads, 0, s>>>(x, nvox, mask, minmax);
  else channel_minmax_kernel<false><<<grid, kThreads, 0, s>>>(x, nvox, mask, minmax);
  return mi355_check_launch("channel_minmax");
}

extern "C" int64_t mi355_bssfp_workspace_bytes(int32_t p, int64_t nvox) {
  if (p < 1 || p > MI355_BSSFP_MAX_CYCLES || !nvox_ok(nvox)) {
    mi355_set_error("bssfp_workspace_bytes: bad shape (%d cycles, %lld voxels)", (int)p, (long long)nvox);
    return MI355_ERR_ARG;
  }
  return (int64_t)p * phase_sum_blocks(nvox) * 2 * (int64_t)sizeof(double);
}

extern "C" int mi355_bssfp_phase_sums(const float* mag, const float* phase_raw, int32_t p, int64_t nvox, void* workspace,
                                      int64_t workspace_bytes, double* sums, void* stream) {
  MI355_REQUIRE(p >= 1 && p <= MI355_BSSFP_MAX_CYCLES, "bssfp_phase_sums: %d cycles, need 1 .. %d", (int)p, MI355_BSSFP_MAX_CYCLES);
  MI355_REQUIRE(nvox_ok(nvox) && nvox > 0, "bssfp_phase_sums: bad voxel count %lld", (long long)nvox);
  MI355_REQUIRE(mag && phase_raw && workspace && sums, "bssfp_phase_sums: null pointer");
  MI355_REQUIRE(aligned(workspace, 8) && workspace_bytes >= mi355_bssfp_workspace_bytes(p, nvox),
                "bssfp_phase_sums: workspace of %lld bytes is too small or not 8-byte aligned", (long long)workspace_bytes);
  const int nb = phase_sum_blocks(nvox);
  hipStream_t s = (hipStream_t)stream;
  phase_sums_stage1<<<dim3((unsigned)nb, (unsigned)p), kThreads, 0, s>>>(mag, phase_raw, nvox, (double*)workspace);
  phase_sums_stage2<<<(unsigned)p, kThreads, 0, s>>>((const double*)workspace, nb, sums);
  return mi355_check_launch("bssfp_phase_sums");
}

extern "C" int mi355_bssfp_phase_correct(const float* mag, const float* phase_raw, int32_t p, int64_t nvox, const double* sums,
                                         float* re, float* im, void* stream) {
  MI355_REQUIRE(p >= 1 && p <= MI355_BSSFP_MAX_CYCLES, "bssfp_phase_correct: %d cycles, need 1 .. %d", (int)p,
                MI355_BSSFP_MAX_CYCLES);
  MI355_REQUIRE(nvox_ok(nvox), "bssfp_phase_correct: bad voxel count %lld", (long long)nvox);
  MI355_REQUIRE(mag && phase_raw && sums && re && im, "bssfp_phase_correct: null pointer");
  if (nvox == 0) return MI355_OK;
  const dim3 grid((unsigned)((nvox + kThreads - 1) / kThreads), (unsigned)p);
  phase_correct_kernel<<<grid, kThreads, 0, (hipStream_t)stream>>>(mag, phase_raw, nvox, sums, re, im);
  return mi355_check_launch("bssfp_phase_correct");
}

extern "C" int mi355_bssfp_assemble(const float* re, const float* im, int32_t p, int64_t nvox, const uint8_t* mask,
                                    double mag_min, double mag_max, double pha_min, double pha_max, int32_t repeat_cycle,
                                    float* out, void* stream) {
  MI355_REQUIRE(p >= 1 && p <= MI355_BSSFP_MAX_CYCLES, "bssfp_assemble: %d cycles, need 1 .. %d", (int)p, MI355_BSSFP_MAX_CYCLES);
  MI355_REQUIRE(nvox_ok(nvox), "bssfp_assemble: bad voxel count %lld", (long long)nvox);
  MI355_REQUIRE(repeat_cycle >= -1 && repeat_cycle < p, "bssfp_assemble: repeat_cycle %d outside -1 .. %d", (int)repeat_cycle,
                (int)p - 1);
  MI355_REQUIRE(mag_max > mag_min && pha_max > pha_min, "bssfp_assemble: a normalisation range is empty or not finite");
  MI355_REQUIRE(re && im && out, "bssfp_assemble: null pointer");
  if (nvox == 0) return MI355_OK;
  AssembleArgs a{re, im, p, nvox, mask, mag_min, mag_max, pha_min, pha_max, repeat_cycle, out};
  bssfp_assemble_kernel<<<(unsigned)((nvox + kThreads - 1) / kThreads), kThreads, 0, (hipStream_t)stream>>>(a);
  return mi355_check_launch("bssfp_assemble");
}

extern "C" int mi355_normalize_channels(const float* src, int32_t c_src, const int32_t* src_channel, const double* ranges,
                                        int32_t c_out, int64_t nvox, const uint8_t* mask, float* dst, void* stream) {
  MI355_REQUIRE(c_out >= 1 && c_out <= MI355_PREP_MAX_CHANNELS, "normalize_channels: %d output channels, need 1 .. %d", (int)c_out,
                MI355_PREP_MAX_CHANNELS);
  MI355_REQUIRE(c_src >= 1, "normalize_channels: bad source channel count %d", (int)c_src);
  MI355_REQUIRE(nvox_ok(nvox), "normalize_channels: bad voxel count %lld", (long long)nvox);
  MI355_REQUIRE(src && src_channel && ranges && dst, "normalize_channels: null pointer");
  NormArgs a{src, dst, nvox, mask, c_out, {}, {}, {}};
  for (int c = 0; c < c_out; ++c) {
    a.map[c] = src_channel[c];
    a.lo[c] = ranges[2 * c];
    a.hi[c] = ranges[2 * c + 1];
    MI355_REQUIRE(a.map[c] >= 0 && a.map[c] < c_src, "normalize_channels: source channel %d of output %d outside 0 .. %d",
                  a.map[c], c, (int)c_src - 1);
    MI355_REQUIRE(a.hi[c] > a.lo[c], "normalize_channels: range %d is empty or not finite", c);
  }
  const float* src_end = src + (long long)c_src * nvox;
  const float* dst_end = dst + (long long)c_out * nvox;
  MI355_REQUIRE(dst >= src_end || src >= dst_end, "normalize_channels: dst overlaps src (in-place is not supported)");
  if (nvox == 0) return MI355_OK;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = nvox % 4 == 0 && aligned(src, 16) && aligned(dst, 16) && (!mask || aligned(mask, 4));
  if (vec) normalize_channels_kernel<true><<<(unsigned)((nvox / 4 + kThreads - 1) / kThreads), kThreads, 0, s>>>(a);
  else normalize_channels_kernel<false><<<(unsigned)((nvox + kThreads - 1) / kThreads), kThreads, 0, s>>>(a);
  return mi355_check_launch("normalize_channels");
}
