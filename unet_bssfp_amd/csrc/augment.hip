// GPU-side versions of the cheap intensity augmentations of the reference's training transform
// (src/data_module.py:130-139: tio.RandomBiasField, tio.RandomNoise, tio.RandomGamma), f32 NCDHW / (C, D, H, W)
// tensors, one pass each (read + write: HBM-bound).  The random PARAMETERS are drawn on the host like TorchIO
// does; the per-voxel noise comes from a counter-based hash (no RNG state, hipGraph-safe).  The per-voxel math lives in
// augment_core.h, which the fused patch-queue gather (patch_queue.hip) shares.
#include "common.h"
#include "augment_core.h"

namespace {

struct BiasArgs { int c, d, h, w, order, ncoef; float coef[MI355_AUG_MAX_COEF]; };

// field(a, b, c): augment_core.h; out = x * exp(field)
__global__ __launch_bounds__(256) void bias_field_kernel(const float* __restrict__ x, float* __restrict__ out, BiasArgs q) {
  const long long vol = (long long)q.d * q.h * q.w;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= vol) return;
  const int c0 = (int)(i % q.w), b0 = (int)(i / q.w % q.h), a0 = (int)(i / ((long long)q.w * q.h));
  const float g = expf(aug_bias_log_field(a0, b0, c0, q.d, q.h, q.w, q.order, q.coef));
  for (int ch = 0; ch < q.c; ++ch) out[ch * vol + i] = aug_bias_apply(x[ch * vol + i], g);
}

__global__ __launch_bounds__(256) void gamma_kernel(const float* __restrict__ x, float* __restrict__ out, long long n, float gamma) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i] = aug_gamma_apply(x[i], gamma);
}

__global__ __launch_bounds__(256) void noise_kernel(const float* __restrict__ x, float* __restrict__ out, long long n, float mean,
                                                    float std, unsigned long long seed) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i] = aug_noise_apply(x[i], i, mean, std, seed);
}

}  // namespace

extern "C" int mi355_aug_bias_field(const float* x, float* out, int32_t c, int32_t d, int32_t h, int32_t w,
                                    const float* coefficients, int32_t order, void* stream) {
  MI355_REQUIRE(x && out && coefficients && c > 0 && d > 0 && h > 0 && w > 0, "aug_bias_field: bad argument");
  MI355_REQUIRE(order >= 0 && order <= 4, "aug_bias_field: order must be 0..4");
  BiasArgs q{c, d, h, w, order, (order + 1) * (order + 2) * (order + 3) / 6, {}};
  for (int i = 0; i < q.ncoef; ++i) q.coef[i] = coefficients[i];
  const long long vol = (long long)d * h * w;
  bias_field_kernel<<<(unsigned)((vol + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, out, q);
  return mi355_check_launch("aug_bias_field");
}

extern "C" int mi355_aug_gamma(const float* x, float* out, int64_t count, float gamma, void* stream) {
  MI355_REQUIRE(x && out && count > 0, "aug_gamma: bad argument");
  gamma_kernel<<<(unsigned)((count + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, out, count, gamma);
  return mi355_check_launch("aug_gamma");
}

extern "C" int mi355_aug_noise(const float* x, float* out, int64_t count, float mean, float std, uint64_t seed, void* stream) {
  MI355_REQUIRE(x && out && count > 0 && std >= 0.f, "aug_noise: bad argument");
  noise_kernel<<<(unsigned)((count + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, out, count, mean, std, seed);
  return mi355_check_launch("aug_noise");
}
