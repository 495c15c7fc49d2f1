// Tail of a ResNet input head (nn.ResidualUnit): y = ReLU(Norm(z)) + residual(x) in ONE pass -- reads the last convolution's output
// z and the block's input x, writes the sum; the residual is x itself or a 1x1x1 convolution of x evaluated per row on the VALU.
// HBM-bound: thread = (row, 16-byte piece of the output channels), as the streaming kernels of normact.hip.
#include <type_traits>
#include "elementwise_common.h"

namespace {

constexpr int kResMaxC = 64;      // output channels (padded) of the launch
constexpr int kResMaxCx = 32;     // real input channels of the projection (LDS table kResMaxCx x kResMaxC floats = 8 KB)

struct ResTailArgs {
  const char* z; int ldz; const char* x; int ldx; char* y; int ldy;
  int c, n_real, cx; long long rows_per_group;
  const float* mean; const float* rstd; const float* gamma; const float* beta;
  const float* rw; const float* rb;
};

// the weight the arithmetic uses: the f32 master value, in bf16 mode rounded to bf16 (mi355_normact_desc's rule for fy / gw)
template <typename T> __device__ __forceinline__ float res_weight(float w) {
  if constexpr (sizeof(T) == 2) return bf16_bits_to_f32(f32_to_bf16_bits(w));
  else return w;
}

// PROJ false: identity residual (cx == n_real).  PROJ true: projection of cx <= kResMaxCx input channels, the weights as a
// [ci][ch] f32 table in LDS, filled once per workgroup (a lane reads the 32 or 16 bytes of its own channels per ci: the 16 rows of a
// wave broadcast, the pieces of a row fall on different banks).
template <typename T, bool PROJ>
__global__ __launch_bounds__(256) void restail_fwd_kernel(const ResTailArgs q) {
  constexpr int EPV = Elem<T>::kPer16B;
  __shared__ __attribute__((aligned(16))) float wl[PROJ ? kResMaxCx * kResMaxC : 4];
  if constexpr (PROJ) {
    for (int i = threadIdx.x; i < q.cx * q.c; i += 256) {
      const int ci = i / q.c, ch = i % q.c;
      wl[i] = ch < q.n_real ? res_weight<T>(q.rw[ch * q.cx + ci]) : 0.f;
    }
    __syncthreads();
  }
  const int g = blockIdx.y;
  const int lpr = q.c / EPV, rpp = 256 / lpr;
  const int piece = threadIdx.x % lpr, rsub = threadIdx.x / lpr;
  if (rsub >= rpp) return;
  const int ch0 = piece * EPV;
  // t = z * sc + sh, as normact_fwd_kernel evaluates the norm
  float sc[EPV], sh[EPV], rbv[EPV];
#pragma unroll
  for (int j = 0; j < EPV; ++j) {
    const int ch = ch0 + j;
    const bool real = ch < q.n_real;
    const float ga = q.gamma ? (real ? q.gamma[ch] : 0.f) : 1.f, be = (q.beta && real) ? q.beta[ch] : 0.f;
    const float rs = q.rstd[(long long)g * q.c + ch], mu = q.mean[(long long)g * q.c + ch];
    sc[j] = ga * rs;
    sh[j] = be - mu * ga * rs;
    rbv[j] = (PROJ && q.rb && real) ? q.rb[ch] : 0.f;
  }
  const T* zb = reinterpret_cast<const T*>(q.z) + (long long)g * q.rows_per_group * q.ldz;
  const T* xb = reinterpret_cast<const T*>(q.x) + (long long)g * q.rows_per_group * q.ldx;
  T* yb = reinterpret_cast<T*>(q.y) + (long long)g * q.rows_per_group * q.ldy;
  const long long stride = (long long)gridDim.x * rpp;
  for (long long row = (long long)blockIdx.x * rpp + rsub; row < q.rows_per_group; row += stride) {
    Vec16<T> v;
    v.load_nt(zb + row * q.ldz + ch0);          // z and x are read for the last time in the forward pass
    float r[EPV];
    if constexpr (!PROJ) {
      Vec16<T> xv;
      xv.load_nt(xb + row * q.ldx + ch0);
#pragma unroll
      for (int j = 0; j < EPV; ++j) r[j] = xv.f[j];
    } else {
#pragma unroll
      for (int j = 0; j < EPV; ++j) r[j] = rbv[j];
      for (int p = 0; p * EPV < q.cx; ++p) {    // (the lanes of a row read the same 16 bytes: one request)
        Vec16<T> xv;
        xv.load_nt(xb + row * q.ldx + p * EPV);
#pragma unroll
        for (int k = 0; k < EPV; ++k) {
          const int ci = p * EPV + k;
          if (ci < q.cx) {
            const float* wr = wl + ci * q.c + ch0;
#pragma unroll
            for (int j = 0; j < EPV; ++j) r[j] = fmaf(xv.f[k], wr[j], r[j]);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < EPV; ++j) {
      const float t = v.f[j] * sc[j] + sh[j];
      v.f[j] = (ch0 + j) < q.n_real ? (t > 0.f ? t : 0.f) + r[j] : 0.f;
    }
    v.store(yb + row * q.ldy + ch0);
  }
}

static bool aligned16(const void* p) { return ((unsigned long long)p & 15ull) == 0; }

}  // namespace

int mi355_restail_fwd(const mi355_restail_desc* d, void* stream) {
  const char* who = "restail_fwd";
  MI355_REQUIRE(d && d->z && d->x && d->y && d->mean && d->rstd, "%s: null pointer", who);
  if (d->layout != 0) {
    mi355_set_error("%s: only plain NDHWC rows are implemented (layout=%d)", who, d->layout);
    return MI355_ERR_UNSUPPORTED;
  }
  int rc = check_rows(d->c, d->ldz, d->dtype, who);
  if (rc) return rc;
  rc = check_rows(d->c, d->ldy, d->dtype, who);
  if (rc) return rc;
  const int epv = d->dtype == MI355_DT_F32 ? 4 : 8;
  MI355_REQUIRE(d->rows_per_group > 0 && d->groups > 0 && d->groups <= 65535, "%s: empty, or more than 65535 groups", who);
  MI355_REQUIRE(d->n_real > 0 && d->n_real <= d->c && d->cx > 0, "%s: bad channel counts (n_real=%d, c=%d, cx=%d)", who, d->n_real, d->c, d->cx);
  MI355_REQUIRE(aligned16(d->z) && aligned16(d->x) && aligned16(d->y), "%s: rows must start on 16-byte boundaries", who);
  MI355_REQUIRE(d->ldx % epv == 0, "%s: ldx=%d must keep rows 16-byte aligned", who, d->ldx);
  if (d->c > kResMaxC) {
    mi355_set_error("%s: at most %d (padded) output channels (c=%d)", who, kResMaxC, d->c);
    return MI355_ERR_UNSUPPORTED;
  }
  ResTailArgs q;
  q.z = (const char*)d->z; q.ldz = d->ldz; q.x = (const char*)d->x; q.ldx = d->ldx; q.y = (char*)d->y; q.ldy = d->ldy;
  q.c = d->c; q.n_real = d->n_real; q.cx = d->cx; q.rows_per_group = d->rows_per_group;
  q.mean = d->mean; q.rstd = d->rstd; q.gamma = d->gamma; q.beta = d->beta; q.rw = d->rw; q.rb = d->rb;
  const bool proj = d->rw != nullptr;
  if (!proj) {
    MI355_REQUIRE(d->cx == d->n_real && !d->rb, "%s: the identity residual needs cx == n_real and no bias (cx=%d, n_real=%d)", who, d->cx, d->n_real);
    MI355_REQUIRE(d->ldx >= d->c, "%s: the identity residual reads rows of c channels (ldx=%d, c=%d)", who, d->ldx, d->c);
  } else {
    if (d->cx > kResMaxCx) {
      mi355_set_error("%s: the projection takes at most %d input channels (cx=%d)", who, kResMaxCx, d->cx);
      return MI355_ERR_UNSUPPORTED;
    }
    // every 16-byte piece that holds a real input channel is read whole
    MI355_REQUIRE(d->ldx >= (d->cx + epv - 1) / epv * epv, "%s: ldx=%d is shorter than the padded input row (cx=%d)", who, d->ldx, d->cx);
  }
  // workgroups as the streaming norm kernels (normact.hip: stream_blocks): 8 passes each, at most 1024 per group
  const int rpp = 256 / (d->c / epv);
  long long b = (d->rows_per_group + (long long)rpp * 8 - 1) / ((long long)rpp * 8);
  if (b < 1) b = 1;
  if (b > 1024) b = 1024;
  const dim3 grid((unsigned)b, (unsigned)d->groups);
  for_dtype(d->dtype, [&](auto t) {
    using T = decltype(t);
    if (!proj) restail_fwd_kernel<T, false><<<grid, dim3(256), 0, (hipStream_t)stream>>>(q);
    else restail_fwd_kernel<T, true><<<grid, dim3(256), 0, (hipStream_t)stream>>>(q);
  });
  return mi355_check_launch(who);
}
