// MaxPool3d(2) on NDHWC rows, forward (optionally recording the window positions) and backward (optionally adding the
// skip connection's gradient).
#include "elementwise_common.h"

namespace {

// ------------------------------------------------------------------ max-pool 2x2x2
template <typename T>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* __restrict__ x, int ldx, T* __restrict__ y,
                                                           int ldy, int c, int d, int h, int w, long long total,
                                                           uint8_t* __restrict__ widx) {
  constexpr int EPV = Elem<T>::kPer16B;
  const int lpr = c / EPV;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int piece = (int)(idx % lpr);
  long long o = idx / lpr;
  const int od_ = d / 2, oh_ = h / 2, ow_ = w / 2;
  const int ow = (int)(o % ow_); long long t = o / ow_;
  const int oh = (int)(t % oh_); t /= oh_;
  const int od = (int)(t % od_); const int n = (int)(t / od_);
  Vec16<T> m;
  bool firstv = true;
  // window position (kd, kh, kw as 3 bits) of the element the BACKWARD kernel routes the gradient to: the first one in scan
  // order that equals the maximum or is NaN (maxpool_bwd_kernel's `hit`), i.e. the first NaN if the window holds one, else the
  // first occurrence of the maximum
  unsigned long long where = 0;
  unsigned nan_seen = 0;
#pragma unroll
  for (int kd = 0; kd < 2; ++kd)
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int kw = 0; kw < 2; ++kw) {
        const long long vox = (((long long)n * d + 2 * od + kd) * h + 2 * oh + kh) * w + 2 * ow + kw;
        const unsigned long long kk = (unsigned long long)(kd * 4 + kh * 2 + kw);
        Vec16<T> v;
        v.load(x + vox * ldx + piece * EPV);
        if (firstv) {
          m = v; firstv = false;
#pragma unroll
          for (int j = 0; j < EPV; ++j) nan_seen |= (v.f[j] != v.f[j] ? 1u : 0u) << j;
        } else {
#pragma unroll
          for (int j = 0; j < EPV; ++j) {
            const bool isnan_ = v.f[j] != v.f[j];
            const bool take = v.f[j] > m.f[j] || isnan_;
            m.f[j] = take ? v.f[j] : m.f[j];
            const bool mark = ((nan_seen >> j) & 1u) ? false : take;          // after the first NaN the position stays
            where = mark ? ((where & ~(0xffull << (8 * j))) | (kk << (8 * j))) : where;
            nan_seen |= (isnan_ ? 1u : 0u) << j;
          }
        }
      }
  m.store(y + o * ldy + piece * EPV);
  if (widx) {
    if constexpr (EPV == 8) *reinterpret_cast<unsigned long long*>(widx + o * c + piece * EPV) = where;
    else *reinterpret_cast<unsigned*>(widx + o * c + piece * EPV) = (unsigned)where;
  }
}

// ODD: some extent is odd -- MaxPool3d(2) floors, the last plane / row / column belongs to no window: its gradient is zero
// (+ add); the thread of the last window along such an axis writes it.
template <typename T, bool ODD>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ y,
                                                           int ldy, const T* __restrict__ dy, int lddy,
                                                           T* __restrict__ dx, int lddx, int c, int d, int h, int w,
                                                           long long total, const T* __restrict__ add, int ldadd) {
  constexpr int EPV = Elem<T>::kPer16B;
  const int lpr = c / EPV;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int piece = (int)(idx % lpr);
  long long o = idx / lpr;
  const int od_ = d / 2, oh_ = h / 2, ow_ = w / 2;
  const int ow = (int)(o % ow_); long long t = o / ow_;
  const int oh = (int)(t % oh_); t /= oh_;
  const int od = (int)(t % od_); const int n = (int)(t / od_);
  Vec16<T> m, g;
  m.load(y + o * ldy + piece * EPV);
  g.load(dy + o * lddy + piece * EPV);
  bool taken[EPV];
#pragma unroll
  for (int j = 0; j < EPV; ++j) taken[j] = false;
  constexpr int KN = ODD ? 3 : 2;
  const bool xd = ODD && od == od_ - 1 && (d & 1), xh = ODD && oh == oh_ - 1 && (h & 1), xw = ODD && ow == ow_ - 1 && (w & 1);
#pragma unroll
  for (int kd = 0; kd < KN; ++kd)
#pragma unroll
    for (int kh = 0; kh < KN; ++kh)
#pragma unroll
      for (int kw = 0; kw < KN; ++kw) {
        const bool inwin = kd < 2 && kh < 2 && kw < 2;
        if (!inwin && ((kd == 2 && !xd) || (kh == 2 && !xh) || (kw == 2 && !xw))) continue;
        const long long vox = (((long long)n * d + 2 * od + kd) * h + 2 * oh + kh) * w + 2 * ow + kw;
        Vec16<T> v, outv;
        if (inwin) v.load(x + vox * ldx + piece * EPV);
#pragma unroll
        for (int j = 0; j < EPV; ++j) {
          const bool hit = inwin && !taken[j] && (v.f[j] == m.f[j] || v.f[j] != v.f[j]);
          outv.f[j] = hit ? g.f[j] : 0.f;
          taken[j] = taken[j] || hit;
        }
        if (add) {            // second gradient of the pooled tensor (its skip-connection use): summed here in f32
          Vec16<T> s2;
          s2.load(add + vox * ldadd + piece * EPV);
#pragma unroll
          for (int j = 0; j < EPV; ++j) outv.f[j] += s2.f[j];
        }
        outv.store(dx + vox * lddx + piece * EPV);
      }
}

}  // namespace

extern "C" {

int mi355_maxpool2_fwd(const void* x, int32_t ldx, void* y, int32_t ldy, int32_t n, int32_t c, int32_t d, int32_t h,
                       int32_t w, int32_t dtype, void* stream) {
  return mi355_maxpool2_fwd_idx(x, ldx, y, ldy, nullptr, n, c, d, h, w, dtype, stream);
}

int mi355_maxpool2_fwd_idx(const void* x, int32_t ldx, void* y, int32_t ldy, uint8_t* idx, int32_t n, int32_t c, int32_t d,
                           int32_t h, int32_t w, int32_t dtype, void* stream) {
  MI355_REQUIRE(x && y && n > 0, "maxpool_fwd: bad argument");
  MI355_REQUIRE(d >= 2 && h >= 2 && w >= 2, "maxpool: extents must be >= 2 (%d,%d,%d)", d, h, w);   // odd: floor, as MaxPool3d(2)
  int rc = check_rows(c, ldx, dtype, "maxpool_fwd");
  if (rc) return rc;
  rc = check_rows(c, ldy, dtype, "maxpool_fwd");
  if (rc) return rc;
  const int epv = dtype == MI355_DT_F32 ? 4 : 8;
  const long long total = (long long)n * (d / 2) * (h / 2) * (w / 2) * (c / epv);
  dim3 grid((unsigned)((total + 255) / 256));
  for_dtype(dtype, [&](auto t) { maxpool_fwd_kernel<decltype(t)><<<grid, dim3(256), 0, (hipStream_t)stream>>>((const decltype(t)*)x, ldx, (decltype(t)*)y, ldy, c, d, h, w, total, idx); });
  return mi355_check_launch("maxpool_fwd");
}

static int maxpool_bwd_impl(const void* x, int32_t ldx, const void* y, int32_t ldy, const void* dy, int32_t lddy, void* dx,
                            int32_t lddx, const void* add, int32_t ldadd, int32_t n, int32_t c, int32_t d, int32_t h,
                            int32_t w, int32_t dtype, void* stream) {
  MI355_REQUIRE(x && y && dy && dx && n > 0, "maxpool_bwd: bad argument");
  MI355_REQUIRE(d >= 2 && h >= 2 && w >= 2, "maxpool: extents must be >= 2 (%d,%d,%d)", d, h, w);
  const bool odd = (d | h | w) & 1;
  int rc = check_rows(c, ldx, dtype, "maxpool_bwd");
  if (rc) return rc;
  if ((rc = check_rows(c, ldy, dtype, "maxpool_bwd"))) return rc;
  if ((rc = check_rows(c, lddy, dtype, "maxpool_bwd"))) return rc;
  if ((rc = check_rows(c, lddx, dtype, "maxpool_bwd"))) return rc;
  if (add && (rc = check_rows(c, ldadd, dtype, "maxpool_bwd"))) return rc;
  const int epv = dtype == MI355_DT_F32 ? 4 : 8;
  const long long total = (long long)n * (d / 2) * (h / 2) * (w / 2) * (c / epv);
  dim3 grid((unsigned)((total + 255) / 256));
#define MP_BWD(T, O) hipLaunchKernelGGL((maxpool_bwd_kernel<T, O>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx, (const T*)y, ldy, (const T*)dy, lddy, (T*)dx, lddx, c, d, h, w, total, (const T*)add, ldadd)
  if (dtype == MI355_DT_F32) { if (odd) MP_BWD(float, true); else MP_BWD(float, false); }
  else { if (odd) MP_BWD(bf16_t, true); else MP_BWD(bf16_t, false); }
#undef MP_BWD
  return mi355_check_launch("maxpool_bwd");
}

int mi355_maxpool2_bwd(const void* x, int32_t ldx, const void* y, int32_t ldy, const void* dy, int32_t lddy, void* dx,
                       int32_t lddx, int32_t n, int32_t c, int32_t d, int32_t h, int32_t w, int32_t dtype, void* stream) {
  return maxpool_bwd_impl(x, ldx, y, ldy, dy, lddy, dx, lddx, nullptr, 0, n, c, d, h, w, dtype, stream);
}

int mi355_maxpool2_bwd_add(const void* x, int32_t ldx, const void* y, int32_t ldy, const void* dy, int32_t lddy, void* dx,
                           int32_t lddx, const void* add, int32_t ldadd, int32_t n, int32_t c, int32_t d, int32_t h,
                           int32_t w, int32_t dtype, void* stream) {
  MI355_REQUIRE(add, "maxpool_bwd_add: null pointer");
  return maxpool_bwd_impl(x, ldx, y, ldy, dy, lddy, dx, lddx, add, ldadd, n, c, d, h, w, dtype, stream);
}

}  // extern "C"
