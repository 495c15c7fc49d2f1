// fp8 operand preparation (per-tensor amax, e4m3 cast with delayed scaling, the scale roll) and the two MFMA layout self-tests.
#include "elementwise_common.h"

namespace {

// ------------------------------------------------------------------ fp8 operand preparation
// NaN policy: every amax here (and amax_commit's callers) is a chain of fmaxf, which drops a NaN operand -- the scale stays the
// maximum of the finite values and +-inf -- while the cast keeps the NaN element a NaN byte (common.h: fp8_clamp), so it
// reaches the convolution's output.
__global__ __launch_bounds__(256) void amax_f32_kernel(const float* __restrict__ x, long long n, float* out) {
  float m = 0.f;
  const long long stride = (long long)gridDim.x * 256 * 4;
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 4 <= n) {
      const float4 v = *reinterpret_cast<const float4*>(x + i);
      m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    } else {
      for (long long j = i; j < n; ++j) m = fmaxf(m, fabsf(x[j]));
    }
  }
  amax_commit(m, out);
}
template <typename T>
__global__ __launch_bounds__(256) void amax_act_kernel(const T* __restrict__ x, int ld, int c, long long rows, float* out) {
  constexpr int EPV = Elem<T>::kPer16B;
  const int lpr = c / EPV;
  const long long total = rows * lpr, stride = (long long)gridDim.x * 256;
  float m = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const long long row = i / lpr;
    const int piece = (int)(i - row * lpr);
    Vec16<T> v;
    v.load(x + row * ld + piece * EPV);
#pragma unroll
    for (int j = 0; j < EPV; ++j) m = fmaxf(m, fabsf(v.f[j]));
  }
  amax_commit(m, out);
}
// 16 channels per thread: two 16-B loads of bf16 (four of f32), one 16-B store of e4m3
template <typename T>
__global__ __launch_bounds__(256) void cast_fp8_kernel(const T* __restrict__ x, int ld, int c, long long rows,
                                                        const float* __restrict__ amax, uint8_t* __restrict__ dst, int ld_dst,
                                                        float* __restrict__ next) {
  constexpr int EPV = Elem<T>::kPer16B, NV = 16 / EPV;
  const float sc = fp8_scale_of(amax);
  const int gpr = c / 16;
  const long long total = rows * gpr, stride = (long long)gridDim.x * 256;
  float m = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const long long row = i / gpr;
    const int g = (int)(i - row * gpr);
    float f[16];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      Vec16<T> v;
      v.load(x + row * ld + g * 16 + k * EPV);
#pragma unroll
      for (int j = 0; j < EPV; ++j) {
        m = fmaxf(m, fabsf(v.f[j]));
        f[k * EPV + j] = v.f[j] * sc;
      }
    }
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      w[k] = cvt_pk_fp8(f[4 * k], f[4 * k + 1], 0u, false);
      w[k] = cvt_pk_fp8(f[4 * k + 2], f[4 * k + 3], w[k], true);
    }
    *reinterpret_cast<uint4*>(dst + row * ld_dst + g * 16) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  if (next) amax_commit(m, next);
}
// delayed scaling: the amax gathered during a step becomes the scale of the next one
// sat (optional, int32 per slot): raised when the step that ends here SATURATED in that slot -- a value clamps at +-448 exactly
// when |value| * 224 / amax_in_use > 448, i.e. when the amax gathered during the step exceeds twice the amax in use (every
// kernel that casts an operand also gathers its maximum), so the roll sees it without any counter in the cast kernels
__global__ void fp8_scale_roll_kernel(float* __restrict__ table, int n, int* __restrict__ sat) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float use = table[2 * i], nx = table[2 * i + 1];
  if (sat && use > 0.f && nx > 2.f * use) sat[i] += 1;
  if (nx > 0.f) table[2 * i] = nx;
  table[2 * i + 1] = 0.f;
}
// ------------------------------------------------------------------ MFMA layout probe
__global__ void mfma_selftest_kernel(float* out_f32, float* out_bf16) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 31, h = lane >> 5;
  // A[i][k] = i + 1 (k = 0 only), B[k][j] = 100 * (j + 1) (k = 0 only)  =>  D[i][j] = (i+1)*100*(j+1)
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h == 0 ? (float)(r + 1) : 0.f, h == 0 ? 100.f * (r + 1) : 0.f, acc, 0, 0, 0);
#pragma unroll
  for (int i = 0; i < 16; ++i) out_f32[acc_row(i, h) * 32 + r] = acc[i];
  // bf16: A[i][k] = (i+1) at k == 3, B[k][j] = (j+1) at k == 3 (k = 8h + e -> h = 0, e = 3), plus
  // A[i][k=12] = 1, B[12][j] = 0.5 (h = 1, e = 4)  =>  D[i][j] = (i+1)(j+1) + 0.5
  Frag<bf16_t> fa, fb;
  uint16_t ea[8] = {0, 0, 0, 0, 0, 0, 0, 0}, eb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (h == 0) { ea[3] = f32_to_bf16_bits((float)(r + 1)); eb[3] = f32_to_bf16_bits((float)(r + 1)); }
  else { ea[4] = f32_to_bf16_bits(1.f); eb[4] = f32_to_bf16_bits(0.5f); }
  fa.v = make_uint4(ea[0] | (ea[1] << 16), ea[2] | (ea[3] << 16), ea[4] | (ea[5] << 16), ea[6] | (ea[7] << 16));
  fb.v = make_uint4(eb[0] | (eb[1] << 16), eb[2] | (eb[3] << 16), eb[4] | (eb[5] << 16), eb[6] | (eb[7] << 16));
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  mma16(fa, fb, acc);
#pragma unroll
  for (int i = 0; i < 16; ++i) out_bf16[acc_row(i, h) * 32 + r] = acc[i];
}

// D[i][j] = sum_k A[i][k] B[k][j], 32 x 32 x 64, A[i][k] = ((i + k) % 5) - 2, B[k][j] = ((2 k + j) % 7) - 3 (exact in e4m3)
__global__ void fp8_selftest_kernel(float* out) {
  typedef int i32x8 __attribute__((ext_vector_type(8)));
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  uint32_t wa[8], wb[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    float fa[4], fb[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int k = 32 * h + 4 * w + b;
      fa[b] = (float)(((r + k) % 5) - 2);
      fb[b] = (float)(((2 * k + r) % 7) - 3);
    }
    wa[w] = cvt_pk_fp8(fa[2], fa[3], cvt_pk_fp8(fa[0], fa[1], 0u, false), true);
    wb[w] = cvt_pk_fp8(fb[2], fb[3], cvt_pk_fp8(fb[0], fb[1], 0u, false), true);
  }
  const i32x8 a = {(int)wa[0], (int)wa[1], (int)wa[2], (int)wa[3], (int)wa[4], (int)wa[5], (int)wa[6], (int)wa[7]};
  const i32x8 b = {(int)wb[0], (int)wb[1], (int)wb[2], (int)wb[3], (int)wb[4], (int)wb[5], (int)wb[6], (int)wb[7]};
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
#pragma unroll
  for (int i = 0; i < 16; ++i) out[acc_row(i, h) * 32 + r] = acc[i];
}

}  // namespace

extern "C" {

int mi355_amax_f32(const float* x, int64_t n, float* amax, void* stream) {
  MI355_REQUIRE(x && amax && n > 0, "amax_f32: bad argument");
  if (hipMemsetAsync(amax, 0, 4, (hipStream_t)stream) != hipSuccess) { mi355_set_error("amax: memset failed"); return MI355_ERR_HIP; }
  long long nb = (n + 1023) / 1024;
  if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(amax_f32_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, (long long)n, amax);
  return mi355_check_launch("amax_f32");
}

int mi355_amax_act(const void* x, int32_t ld, int32_t c, int64_t rows, int32_t dtype, float* amax, void* stream) {
  MI355_REQUIRE(x && amax && rows > 0, "amax_act: bad argument");
  int rc = check_rows(c, ld, dtype, "amax_act");
  if (rc) return rc;
  if (hipMemsetAsync(amax, 0, 4, (hipStream_t)stream) != hipSuccess) { mi355_set_error("amax: memset failed"); return MI355_ERR_HIP; }
  const int epv = dtype == MI355_DT_F32 ? 4 : 8;
  long long nb = (rows * (c / epv) + 256 * 8 - 1) / (256 * 8);
  if (nb > 2048) nb = 2048;
  if (nb < 1) nb = 1;
  for_dtype(dtype, [&](auto t) { amax_act_kernel<decltype(t)><<<dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream>>>((const decltype(t)*)x, ld, c, (long long)rows, amax); });
  return mi355_check_launch("amax_act");
}

int mi355_cast_fp8(const void* src, int32_t ld_src, int32_t c, int64_t rows, int32_t src_dtype, const float* amax,
                   void* dst, int32_t ld_dst, void* stream) {
  return mi355_cast_fp8_delayed(src, ld_src, c, rows, src_dtype, amax, nullptr, dst, ld_dst, stream);
}

int mi355_fp8_scale_roll(float* table, int32_t n, int32_t* sat, void* stream) {
  MI355_REQUIRE(table && n > 0, "fp8_scale_roll: bad argument");
  hipLaunchKernelGGL(fp8_scale_roll_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, table, (int)n, (int*)sat);
  return mi355_check_launch("fp8_scale_roll");
}

int mi355_cast_fp8_delayed(const void* src, int32_t ld_src, int32_t c, int64_t rows, int32_t src_dtype, const float* amax,
                           float* amax_next, void* dst, int32_t ld_dst, void* stream) {
  MI355_REQUIRE(src && dst && amax && rows > 0 && ld_dst >= c && ld_dst % 16 == 0, "cast_fp8: bad argument");
  int rc = check_rows(c, ld_src, src_dtype, "cast_fp8");
  if (rc) return rc;
  long long nb = (rows * (c / 16) + 256 * 4 - 1) / (256 * 4);
  if (nb > 2048) nb = 2048;
  if (nb < 1) nb = 1;
  for_dtype(src_dtype, [&](auto t) {
    cast_fp8_kernel<decltype(t)><<<dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream>>>((const decltype(t)*)src, ld_src, c, (long long)rows, amax, (uint8_t*)dst, ld_dst, amax_next);
  });
  return mi355_check_launch("cast_fp8");
}

int mi355_mfma_selftest(float* out_f32_1024, float* out_bf16_1024, void* stream) {
  MI355_REQUIRE(out_f32_1024 && out_bf16_1024, "selftest: null pointer");
  hipLaunchKernelGGL(mfma_selftest_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out_f32_1024, out_bf16_1024);
  return mi355_check_launch("selftest");
}

int mi355_fp8_selftest(float* out_1024, void* stream) {
  MI355_REQUIRE(out_1024, "fp8_selftest: null pointer");
  hipLaunchKernelGGL(fp8_selftest_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out_1024);
  return mi355_check_launch("fp8_selftest");
}

}  // extern "C"
