// Pieces of the separable Gaussian-window SSIM shared by the metric (metrics.hip) and the loss term (ssim_loss.hip):
// the window, the fixed-order block reduction, and the W and H passes over the five moment fields (x, y, xx, yy, xy).
#pragma once
#include "common.h"

namespace {

constexpr int kMaxWin = 15;
struct Gauss { int n; float g[kMaxWin]; };

__device__ __forceinline__ double block_sum_256(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void sum_partials_kernel(const double* __restrict__ part, int nparts, int width,
                                                           double* __restrict__ out, double scale) {
  __shared__ double red[4];
  for (int j = 0; j < width; ++j) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) s += part[((long long)blockIdx.x * nparts + i) * width + j];
    const double t = block_sum_256(s, red);
    if (threadIdx.x == 0) out[(long long)blockIdx.x * width + j] = t * scale;
  }
}

// The window length is a template parameter (WIN = 11 for MONAI's default, 0 = runtime): with a compile-time trip
// count the tap loops unroll and their loads go out together (the runtime loops had one load in flight per lane).
// pass W: rows = items*C*D*H rows of W floats -> 5 fields of Wo = W - n + 1
template <int WIN>
__global__ __launch_bounds__(256) void ssim_pass_w_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                          float* __restrict__ out, long long rows, int w, int wo, Gauss G) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * wo) return;
  const long long row = i / wo; const int o = (int)(i - row * wo);
  const float* px = x + row * w + o; const float* py = y + row * w + o;
  float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
  const int n = WIN ? WIN : G.n;
#pragma unroll
  for (int k = 0; k < n; ++k) {
    const float a = px[k], b = py[k], g = G.g[k];
    sx += g * a; sy += g * b; sxx += g * (a * a); syy += g * (b * b); sxy += g * (a * b);
  }
  const long long fs = rows * wo;
  out[i] = sx; out[fs + i] = sy; out[2 * fs + i] = sxx; out[3 * fs + i] = syy; out[4 * fs + i] = sxy;
}

// pass H: planes = 5*items*C*D planes of [h][wo] -> [ho][wo]
template <int WIN>
__global__ __launch_bounds__(256) void ssim_pass_h_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                          long long planes, int h, int ho, int wo, Gauss G) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long per = (long long)ho * wo;
  if (i >= planes * per) return;
  const long long pl = i / per; const long long r = i - pl * per;
  const int oh = (int)(r / wo), ow = (int)(r - (long long)oh * wo);
  const float* p = in + (pl * h + oh) * wo + ow;
  float s = 0.f;
  const int n = WIN ? WIN : G.n;
#pragma unroll
  for (int k = 0; k < n; ++k) s += G.g[k] * p[(long long)k * wo];
  out[i] = s;
}

int blocks_for(long long n) { long long b = (n + 256 * 16 - 1) / (256 * 16); return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b)); }

}  // namespace
