// Per-voxel math of the intensity augmentations (tio.RandomBiasField, tio.RandomNoise, tio.RandomGamma), shared by
// augment.hip (one pass per transform) and patch_queue.hip (every stage fused into the patch gather).  hipcc contracts
// a*b + c into one fma, and in a fused kernel it could do so across a stage boundary (the bias product followed by the
// noise add), which changes the rounding.  The two operations that meet at that boundary are therefore compiled with
// `#pragma clang fp contract(off)`, which hipcc honours.  `__fmul_rn` / `__fadd_rn` are no barrier: without
// OCML_BASIC_ROUNDED_OPERATIONS the HIP headers define them as plain `*` / `+`.  The noise stage's own fma is an
// explicit fmaf.  The fused value then equals the chained one bit for bit whatever the surrounding control flow;
// tests/test_patch_queue.py compiles a probe that puts both operations in one basic block and checks its ISA.
#pragma once

#include <hip/hip_runtime.h>

#define MI355_AUG_MAX_COEF 35   // order <= 4: (4+1)(4+2)(4+3)/6 coefficients

// TorchIO: np.arange(-n/2, n/2) + 0.5 per axis, divided by its maximum n/2 - 0.5 (when positive)
__device__ __forceinline__ float aug_bias_coord(int idx, int n) {
  const float half = 0.5f * (float)n, v = (float)idx - half + 0.5f, mx = half - 0.5f;
  return mx > 0.f ? v / mx : v;
}

// log of the field at voxel (a, b, c) of a (d, h, w) volume: sum_i coef_i * u0^xo * u1^yo * u2^zo over
// xo + yo + zo <= order, loops in TorchIO's order (x outer, then y, then z)
__device__ __forceinline__ float aug_bias_log_field(int a, int b, int c, int d, int h, int w, int order, const float* coef) {
  const float u0 = aug_bias_coord(a, d), u1 = aug_bias_coord(b, h), u2 = aug_bias_coord(c, w);
  float p0[5], p1[5], p2[5];
  p0[0] = p1[0] = p2[0] = 1.f;
#pragma unroll
  for (int k = 1; k < 5; ++k) { p0[k] = p0[k - 1] * u0; p1[k] = p1[k - 1] * u1; p2[k] = p2[k - 1] * u2; }
  float f = 0.f;
  int n = 0;
  for (int xo = 0; xo <= order; ++xo)
    for (int yo = 0; yo <= order - xo; ++yo)
      for (int zo = 0; zo <= order - xo - yo; ++zo) f += coef[n++] * p0[xo] * p1[yo] * p2[zo];
  return f;
}

// out = x * exp(field); g = expf(aug_bias_log_field(...)).  The product is rounded on its own (never contracted).
__device__ __forceinline__ float aug_bias_apply(float x, float g) {
#pragma clang fp contract(off)
  return x * g;
}

// N(0, 1) of element i (flat index of the whole volume): counter-based hash + Box-Muller, no RNG state
__device__ __forceinline__ float aug_noise_normal(long long i, unsigned long long seed) {
  unsigned long long h = ((unsigned long long)i + 1ull) * 0x9E3779B97F4A7C15ull + seed;
  h ^= h >> 32; h *= 0xD6E8FEB86659FD93ull; h ^= h >> 32; h *= 0xD6E8FEB86659FD93ull; h ^= h >> 32;
  const float u1 = ((float)(unsigned)(h >> 40) + 0.5f) * (1.f / 16777216.f);      // (0, 1)
  const float u2 = ((float)(unsigned)((h >> 16) & 0xffffffu) + 0.5f) * (1.f / 16777216.f);
  return sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

// x + mean, rounded on its own: never contracted with a product that produced x (the bias stage)
__device__ __forceinline__ float aug_noise_shift(float x, float mean) {
#pragma clang fp contract(off)
  return x + mean;
}

// out = x + mean + std * z, evaluated as fma(std, z, x + mean)
__device__ __forceinline__ float aug_noise_apply(float x, long long i, float mean, float std, unsigned long long seed) {
  return fmaf(std, aug_noise_normal(i, seed), aug_noise_shift(x, mean));
}

// TorchIO keeps the sign of negative intensities
__device__ __forceinline__ float aug_gamma_apply(float x, float gamma) { return copysignf(powf(fabsf(x), gamma), x); }
