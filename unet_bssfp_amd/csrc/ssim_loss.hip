// 1 - SSIM as a differentiable reconstruction-loss term (reference objective: L1 + (1 - SSIM) + Perceptual, thesis 03-methods;
// src/model.py:209 averages the terms of the recon slot).  f32 NCDHW, Gaussian window, "valid" windows, as metrics.hip's ssim3d.
//   fwd : the metric's W and H passes over the five moment fields (ssim_common.h); the D pass filters, applies the SSIM formula,
//         reduces S per block in f64 and ALSO writes the three local derivatives of S at every valid position:
//           P1 = dS/d(G*x), P2 = dS/d(G*xx), P3 = dS/d(G*xy)          ([3][items*C][dd][ho][wo] f32)
//   bwd : d ssim_b / d x(q) = [ Gt(P1)(q) + 2 x(q) Gt(P2)(q) + y(q) Gt(P3)(q) ] / (C dd ho wo), Gt = the transposed separable
//         filter (zero outside the valid box) back to D x H x W: three gather passes D, H, W -- output q sums the taps k with
//         0 <= q - k < valid extent, so nothing is scattered and no atomics are needed; the W pass also combines with x and y and
//         applies grad[item] / (C dd ho wo), grad read from DEVICE memory (no host read: the call records into a hipGraph).
// Gradient with respect to x (the first argument) only.  Deterministic.  The window need not be symmetric.
#include "ssim_common.h"

namespace {

// pass D + SSIM formula + local derivatives + per-block sum.  grid (blocks, items*C); in: [5][items*C][d][ho][wo]
template <int WIN>
__global__ __launch_bounds__(256) void ssim_loss_pass_d_kernel(const float* __restrict__ in, double* __restrict__ part,
                                                               float* __restrict__ pout, long long nvol, int d, int dd, int ho,
                                                               int wo, float c1, float c2, Gauss G) {
  __shared__ double red[4];
  const long long plane = (long long)ho * wo, per = (long long)dd * plane;
  const long long fs = nvol * d * plane;                       // field stride of the moment fields
  const long long ps = nvol * per;                             // field stride of the derivative fields
  const float* base = in + (long long)blockIdx.y * d * plane;
  float* pb = pout + (long long)blockIdx.y * per;
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long long)gridDim.x * 256) {
    const float* p = base + i;                                 // (od, oh, ow) flattened == offset of the first tap
    float m[5];
    const int n = WIN ? WIN : G.n;
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < n; ++k) s += G.g[k] * p[f * fs + (long long)k * plane];
      m[f] = s;
    }
    // the value exactly as the metric computes it
    const float sx = m[2] - m[0] * m[0], sy = m[3] - m[1] * m[1], sxy = m[4] - m[0] * m[1];
    const float b2 = sx + sy + c2, b1 = m[0] * m[0] + m[1] * m[1] + c1;
    const float cs = (2.f * sxy + c2) / b2;
    const float l = (2.f * m[0] * m[1] + c1) / b1;
    acc += (double)(l * cs);
    // P1 = (2 m2 / B1 - 2 m1 A1 / B1^2) cs + L (-2 m2 / B2 + 2 m1 A2 / B2^2), with A1 / B1 = L and A2 / B2 = cs
    const float r1 = 2.f / b1, r2 = 2.f / b2;
    pb[i] = r1 * (m[1] - m[0] * l) * cs + l * r2 * (m[0] * cs - m[1]);
    pb[ps + i] = -(l * cs) / b2;
    pb[2 * ps + i] = l * r2;
  }
  const double t = block_sum_256(acc, red);
  if (threadIdx.x == 0) part[(long long)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

// One output of a transposed 1-D pass: sum_k g[k] * p[(q - k) * stride] over the taps with 0 <= q - k < ext.  Every load is
// issued (at a clamped, in-bounds index) and the out-of-range taps are dropped after it, so the unrolled loads go out together.
template <int WIN>
__device__ __forceinline__ float gather_taps(const float* __restrict__ p, int q, int ext, long long stride, const Gauss& G) {
  float s = 0.f;
  const int n = WIN ? WIN : G.n;
#pragma unroll
  for (int k = 0; k < n; ++k) {
    const int j = q - k;
    const bool ok = j >= 0 && j < ext;
    const float v = p[(long long)(ok ? j : 0) * stride];
    s += ok ? G.g[k] * v : 0.f;
  }
  return s;
}

// transposed pass D: [3*items*C][dd][plane] -> [3*items*C][d][plane], plane = ho*wo
template <int WIN>
__global__ __launch_bounds__(256) void ssim_bwd_d_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                         long long vols, int d, int dd, long long plane, Gauss G) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long per = (long long)d * plane;
  if (i >= vols * per) return;
  const long long v = i / per, r = i - v * per;
  const int q = (int)(r / plane);
  const long long pos = r - (long long)q * plane;
  out[i] = gather_taps<WIN>(in + v * dd * plane + pos, q, dd, plane, G);
}

// transposed pass H: planes = 3*items*C*d planes of [ho][wo] -> [h][wo]
template <int WIN>
__global__ __launch_bounds__(256) void ssim_bwd_h_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                         long long planes, int h, int ho, int wo, Gauss G) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long per = (long long)h * wo;
  if (i >= planes * per) return;
  const long long pl = i / per, r = i - pl * per;
  const int q = (int)(r / wo), ow = (int)(r - (long long)q * wo);
  out[i] = gather_taps<WIN>(in + pl * ho * wo + ow, q, ho, wo, G);
}

// transposed pass W + combine: in = 3 fields of rows = items*C*d*h rows of wo floats -> dx rows of w floats
template <int WIN>
__global__ __launch_bounds__(256) void ssim_bwd_w_kernel(const float* __restrict__ in, const float* __restrict__ x,
                                                         const float* __restrict__ y, const float* __restrict__ grad,
                                                         float* __restrict__ dx, long long rows, long long rows_per_item, int w,
                                                         int wo, float inv_count, Gauss G) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * w) return;
  const long long row = i / w; const int q = (int)(i - row * w);
  const long long fs = rows * wo;
  const float* p = in + row * wo;
  const float t1 = gather_taps<WIN>(p, q, wo, 1, G);
  const float t2 = gather_taps<WIN>(p + fs, q, wo, 1, G);
  const float t3 = gather_taps<WIN>(p + 2 * fs, q, wo, 1, G);
  const float scale = grad[row / rows_per_item] * inv_count;
  dx[i] = scale * (t1 + 2.f * x[i] * t2 + y[i] * t3);
}

// grid of a one-thread-per-element launch; 0 = more blocks than a launch takes
unsigned grid_256(long long n) { const long long b = (n + 255) / 256; return b > 0x7fffffffLL ? 0u : (unsigned)b; }

}  // namespace

extern "C" int64_t mi355_ssim3d_loss_workspace_bytes(int32_t items, int32_t c, int32_t d, int32_t h, int32_t w, int32_t win) {
  if (items <= 0 || c <= 0 || win < 1 || win > kMaxWin || d < win || h < win || w < win) return -1;
  const long long nvol = (long long)items * c, wo = w - win + 1, ho = h - win + 1, dd = d - win + 1;
  // fwd: the five moment fields after W and after H; bwd: the three derivative fields after D and after H (smaller)
  const long long f1 = 5 * nvol * d * h * wo, f2 = 5 * nvol * d * ho * wo;
  const long long parts = nvol * blocks_for(dd * ho * wo);
  return (f1 + f2) * 4 + parts * 8 + 256;
}

extern "C" int mi355_ssim3d_loss_fwd(const float* x, const float* y, int32_t items, int32_t c, int32_t d, int32_t h, int32_t w,
                                     int32_t win, const float* window, float c1, float c2, void* workspace,
                                     int64_t workspace_bytes, double* ssim, float* p, void* stream) {
  const long long need = mi355_ssim3d_loss_workspace_bytes(items, c, d, h, w, win);
  MI355_REQUIRE(need > 0, "ssim3d_loss_fwd: bad shape (items=%d c=%d d=%d h=%d w=%d win=%d)", items, c, d, h, w, win);
  MI355_REQUIRE(x && y && window && workspace && ssim && p && workspace_bytes >= need,
                "ssim3d_loss_fwd: null pointer or workspace too small");
  MI355_REQUIRE((long long)items * c <= 65535, "ssim3d_loss_fwd: too many channel volumes");
  Gauss G; G.n = win;
  for (int i = 0; i < kMaxWin; ++i) G.g[i] = i < win ? window[i] : 0.f;
  const long long nvol = (long long)items * c, wo = w - win + 1, ho = h - win + 1, dd = d - win + 1;
  const long long rows = nvol * d * h;
  const long long planes = 5 * nvol * d;
  const unsigned gw = grid_256(rows * wo), gh = grid_256(planes * ho * wo);
  MI355_REQUIRE(gw && gh, "ssim3d_loss_fwd: tensor too large for one launch");
  float* f1 = (float*)workspace;
  float* f2 = f1 + 5 * nvol * d * h * wo;
  double* part = (double*)(((uintptr_t)(f2 + 5 * nvol * d * ho * wo) + 255) & ~(uintptr_t)255);
  hipStream_t st = (hipStream_t)stream;
  const int nb = blocks_for(dd * ho * wo);
  if (win == 11) {
    ssim_pass_w_kernel<11><<<gw, 256, 0, st>>>(x, y, f1, rows, w, (int)wo, G);
    ssim_pass_h_kernel<11><<<gh, 256, 0, st>>>(f1, f2, planes, h, (int)ho, (int)wo, G);
    ssim_loss_pass_d_kernel<11><<<dim3(nb, (unsigned)nvol), 256, 0, st>>>(f2, part, p, nvol, d, (int)dd, (int)ho, (int)wo, c1, c2, G);
  } else {
    ssim_pass_w_kernel<0><<<gw, 256, 0, st>>>(x, y, f1, rows, w, (int)wo, G);
    ssim_pass_h_kernel<0><<<gh, 256, 0, st>>>(f1, f2, planes, h, (int)ho, (int)wo, G);
    ssim_loss_pass_d_kernel<0><<<dim3(nb, (unsigned)nvol), 256, 0, st>>>(f2, part, p, nvol, d, (int)dd, (int)ho, (int)wo, c1, c2, G);
  }
  sum_partials_kernel<<<items, 256, 0, st>>>(part, c * nb, 1, ssim, 1.0 / ((double)c * dd * ho * wo));
  return mi355_check_launch("ssim3d_loss_fwd");
}

extern "C" int mi355_ssim3d_loss_bwd(const float* x, const float* y, const float* p, const float* grad, int32_t items,
                                     int32_t c, int32_t d, int32_t h, int32_t w, int32_t win, const float* window,
                                     void* workspace, int64_t workspace_bytes, float* dx, void* stream) {
  const long long need = mi355_ssim3d_loss_workspace_bytes(items, c, d, h, w, win);
  MI355_REQUIRE(need > 0, "ssim3d_loss_bwd: bad shape (items=%d c=%d d=%d h=%d w=%d win=%d)", items, c, d, h, w, win);
  MI355_REQUIRE(x && y && p && grad && window && workspace && dx && workspace_bytes >= need,
                "ssim3d_loss_bwd: null pointer or workspace too small");
  Gauss G; G.n = win;
  for (int i = 0; i < kMaxWin; ++i) G.g[i] = i < win ? window[i] : 0.f;
  const long long nvol = (long long)items * c, wo = w - win + 1, ho = h - win + 1, dd = d - win + 1;
  const long long plane = ho * wo, rows = nvol * d * h;
  const unsigned gd = grid_256(3 * nvol * d * plane), gh = grid_256(3 * nvol * d * h * wo), gw = grid_256(rows * w);
  MI355_REQUIRE(gd && gh && gw, "ssim3d_loss_bwd: tensor too large for one launch");
  float* t1 = (float*)workspace;                               // [3][nvol][d][ho][wo]
  float* t2 = t1 + 3 * nvol * d * plane;                       // [3][nvol][d][h][wo]
  hipStream_t st = (hipStream_t)stream;
  const float inv_count = (float)(1.0 / ((double)c * dd * ho * wo));
  if (win == 11) {
    ssim_bwd_d_kernel<11><<<gd, 256, 0, st>>>(p, t1, 3 * nvol, d, (int)dd, plane, G);
    ssim_bwd_h_kernel<11><<<gh, 256, 0, st>>>(t1, t2, 3 * nvol * d, h, (int)ho, (int)wo, G);
    ssim_bwd_w_kernel<11><<<gw, 256, 0, st>>>(t2, x, y, grad, dx, rows, (long long)c * d * h, w, (int)wo, inv_count, G);
  } else {
    ssim_bwd_d_kernel<0><<<gd, 256, 0, st>>>(p, t1, 3 * nvol, d, (int)dd, plane, G);
    ssim_bwd_h_kernel<0><<<gh, 256, 0, st>>>(t1, t2, 3 * nvol * d, h, (int)ho, (int)wo, G);
    ssim_bwd_w_kernel<0><<<gw, 256, 0, st>>>(t2, x, y, grad, dx, rows, (long long)c * d * h, w, (int)wo, inv_count, G);
  }
  return mi355_check_launch("ssim3d_loss_bwd");
}
