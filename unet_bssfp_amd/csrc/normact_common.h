// Arguments of the fused norm + dropout + LeakyReLU / PReLU kernels and their validation, shared by the streaming kernels (normact.hip) and
// the one-workgroup-per-channel-piece kernels of small tensors (normact_small.hip), with the per-element backward both use.
#pragma once
#include "elementwise_common.h"

namespace {

struct NormActArgs {
  const char* z; int ldz; char* a; int lda;
  int c; long long rows_per_group; int groups;
  const float* mean; const float* rstd; const float* gamma; const float* beta;
  float slope; float drop_scale; unsigned thr16; unsigned long long seed; const unsigned long long* seed_ptr;
  const char* da; int ldda; char* dz; int lddz;
  float* part; int blocks_per_group; const float* sums; int batch_stats;
  int n_affine;   // entries of gamma / beta
  S2D s2d_a;      // forward: write `a` in space-to-depth layout
  S2D s2d_da;     // backward: read `da` from a space-to-depth tensor
  uint8_t* q8; int ld8; const float* q_use; float* q_next;   // e4m3 copy of a (fwd) / dz (bwd_apply), bf16 with c == 32 only
  // backward, optional: da is NOT materialised -- it is the data gradient of the 1x1x1 convolution that consumed a:
  // da[row][ch] = bf16(sum_k gz[row][k] * gw[k][ch]), k < gk <= 8 (bf16 only)
  const char* gz; int ldgz; const float* gw; int gw_ld; int gk;
  // forward, optional: the 1x1x1 convolution that consumes a, evaluated per row on the rounded bf16 values:
  // fy[row][k] = bf16(sum_ch a[row][ch] * bf16(gw[k][ch]) + fbias[k]), k < gk <= 8, channels gk .. fcp - 1 zero; skip_a: a itself is not stored
  char* fy; int ldfy; int fcp; const float* fbias; int skip_a;
  // backward, optional: da is NOT materialised -- a was consumed by MaxPool3d(2) (and, optionally, a skip connection whose gradient
  // is `da`): da[v][ch] = (pool_idx[o(v)][ch] == k(v) ? pool_dy[o(v)][ch] : 0) (+ da[v][ch]), rounded to T like the stored tensor
  const uint8_t* pool_idx; const char* pool_dy; int ldpdy; int pd, ph, pw;
  // forward, optional: MaxPool3d(2) of a in the pass that writes it: pool_y[o][ch] = max over the window, pool_widx = the window
  // positions (as mi355_maxpool2_fwd_idx), extents pd x ph x pw (even)
  char* pool_y; int ldpy; uint8_t* pool_widx;
  // PReLU: the trained slope in device memory (null: `slope`), read once per kernel by act_slope(); backward, the reducing kernels'
  // PRELU instantiations: scratch for the partial sums of the slope gradient (streaming: f32 [groups * blocks][c], small: f64 [groups][c])
  const float* alpha; void* dalpha_part;
};

constexpr int kImplicitMaxC = 64;     // channels of the implicit 1x1x1 data gradient's LDS weight table (normact.hip: fill_implicit_w)

// per-thread channel constants of the backward kernels
template <int EPV> struct BwdConst { float mu[EPV], rs[EPV], ga[EPV], be[EPV]; };
template <int EPV>
__device__ __forceinline__ void load_bwd_const(const NormActArgs& q, int g, int ch0, BwdConst<EPV>& k) {
#pragma unroll
  for (int j = 0; j < EPV; ++j) {
    const int ch = ch0 + j;
    k.mu[j] = q.mean ? q.mean[(long long)g * q.c + ch] : 0.f;
    k.rs[j] = q.mean ? q.rstd[(long long)g * q.c + ch] : 1.f;
    k.ga[j] = q.gamma ? (ch < q.n_affine ? q.gamma[ch] : 0.f) : 1.f;
    k.be[j] = (q.beta && ch < q.n_affine) ? q.beta[ch] : 0.f;
  }
}
// the negative slope of this launch: uniform and loop-invariant, read before the row loop
__device__ __forceinline__ float act_slope(const NormActArgs& q) { return q.alpha ? q.alpha[0] : q.slope; }
// g = da * dropout * lrelu'(pre);  xhat = (z - mean) * rstd  (xhat = z when there is no norm);
// aterm = this element's share of the slope gradient: [u <= 0] da u with u = Dropout(pre) (dead code where it is not summed)
template <bool DROP>
__device__ __forceinline__ void bwd_elem(const NormActArgs& q, float slope, bool keep, float mu, float rs, float ga,
                                         float be, float zv, float dav, float& gout, float& xhat, float& aterm) {
  xhat = (zv - mu) * rs;
  float pre = xhat * ga + be;
  float gv = dav;
  if constexpr (DROP) {
    pre = keep ? pre : 0.f;
    gv = keep ? gv * q.drop_scale : 0.f;
  }
  gout = pre > 0.f ? gv : gv * slope;
  aterm = pre > 0.f ? 0.f : gv * pre;
}
template <bool DROP>
__device__ __forceinline__ void bwd_elem(const NormActArgs& q, float slope, bool keep, float mu, float rs, float ga,
                                         float be, float zv, float dav, float& gout, float& xhat) {
  float aterm;
  bwd_elem<DROP>(q, slope, keep, mu, rs, ga, be, zv, dav, gout, xhat, aterm);
}

// The slope gradient's last step (PReLU nodes only): n f64 partial sums -> one f32 scalar, written or accumulated.  ONE workgroup;
// thread t adds src[t], src[t + 256], ... and the 256 totals are folded in a fixed tree: the same bits in every run.
__global__ __launch_bounds__(256) void slope_grad_sum_kernel(const double* __restrict__ src, int n, float* __restrict__ out,
                                                             int accumulate) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += src[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = accumulate ? out[0] + (float)red[0] : (float)red[0];
}

static int fill_normact(const mi355_normact_desc* d, NormActArgs* q, const char* who) {
  MI355_REQUIRE(d && d->z, "%s: null pointer", who);
  int rc = check_rows(d->c, d->ldz, d->dtype, who);
  if (rc) return rc;
  MI355_REQUIRE(d->rows_per_group > 0 && d->groups > 0, "%s: empty", who);
  MI355_REQUIRE(!d->mean || d->rstd, "%s: mean without rstd", who);
  MI355_REQUIRE(d->drop_p >= 0.f && d->drop_p < 1.f, "%s: dropout p out of range", who);
  q->z = (const char*)d->z; q->ldz = d->ldz; q->a = (char*)d->a; q->lda = d->lda;
  q->c = d->c; q->rows_per_group = d->rows_per_group; q->groups = d->groups;
  q->mean = d->mean; q->rstd = d->rstd; q->gamma = d->gamma; q->beta = d->beta;
  q->slope = d->slope;
  q->alpha = d->alpha; q->dalpha_part = d->dalpha_part;
  MI355_REQUIRE(!d->dalpha || (d->alpha && d->dalpha_part && d->mean), "%s: the slope gradient needs alpha, dalpha_part and a norm", who);
  q->thr16 = d->drop_p > 0.f ? (unsigned)(d->drop_p * 65536.f + 0.5f) : 0u;
  q->drop_scale = d->drop_p > 0.f ? 1.f / (1.f - d->drop_p) : 1.f;
  q->seed = d->seed;
  q->seed_ptr = (const unsigned long long*)d->seed_ptr;
  q->n_affine = d->n_affine > 0 ? d->n_affine : d->c;
  q->da = (const char*)d->da; q->ldda = d->ldda; q->dz = (char*)d->dz; q->lddz = d->lddz;
  q->part = d->part; q->blocks_per_group = d->blocks_per_group; q->sums = d->sums; q->batch_stats = d->batch_stats;
  q->s2d_a = S2D{0, 0, 0, 0};
  q->s2d_da = S2D{0, 0, 0, 0};
  MI355_REQUIRE(!d->q8 || (d->dtype == MI355_DT_BF16 && d->c == 32 && d->ld8 >= d->c && d->ld8 % 8 == 0 && d->q_use && d->q_next &&
                           !d->s2d_a && !d->s2d_da),
                "%s: the e4m3 copy is written for plain bf16 tensors of 32 channels (q8, q_use, q_next)", who);
  q->q8 = (uint8_t*)d->q8; q->ld8 = d->ld8; q->q_use = d->q_use; q->q_next = d->q_next;
  MI355_REQUIRE(!d->gz || (d->dtype == MI355_DT_BF16 && !d->da && !d->s2d_da && d->gw && d->gk > 0 && d->gk <= 8 && d->ldgz >= 8 &&
                           d->ldgz % 8 == 0 && d->gw_ld > 0 && d->c <= kImplicitMaxC),
                "%s: the implicit 1x1x1 data gradient needs bf16, gz rows of >= 8 channels, gk <= 8 and no da", who);
  q->gz = (const char*)d->gz; q->ldgz = d->ldgz; q->gw = d->gw; q->gw_ld = d->gw_ld; q->gk = d->gk;
  MI355_REQUIRE(!d->fy || (d->dtype == MI355_DT_BF16 && d->gw && d->gk > 0 && d->gk <= 8 && d->gw_ld > 0 && d->c == 32 &&
                           d->fcp >= 8 && d->fcp % 8 == 0 && d->fcp <= d->c && d->ldfy >= d->fcp && d->ldfy % 8 == 0 && !d->s2d_a &&
                           !d->q8 && d->ldz % 8 == 0 && (d->skip_a || d->lda % 8 == 0)),
                "%s: the fused 1x1x1 convolution needs bf16, 32 channels, gk <= 8 outputs in rows of fcp (8 .. 32) channels", who);
  MI355_REQUIRE(!d->skip_a || d->fy, "%s: skip_a without the fused convolution", who);
  q->fy = (char*)d->fy; q->ldfy = d->ldfy; q->fcp = d->fcp; q->fbias = d->fbias; q->skip_a = d->skip_a;
  MI355_REQUIRE(!d->pool_idx || (d->pool_dy && !d->gz && !d->s2d_da && !d->s2d_a && d->sd >= 2 && d->sh >= 2 && d->sw >= 2 &&
                                 !((d->sd | d->sh | d->sw) & 1) && d->ldpdy >= d->c && d->ldpdy % (d->dtype == MI355_DT_F32 ? 4 : 8) == 0 &&
                                 ((long long)d->rows_per_group * d->groups) % ((long long)d->sd * d->sh * d->sw) == 0 &&
                                 (long long)d->rows_per_group * d->groups < (1ll << 31) && (!d->da || d->ldda >= d->c)),
                "%s: the implicit max-pool gradient needs pool_dy, even extents sd/sh/sw that divide the row count, and plain layouts", who);
  q->pool_idx = (const uint8_t*)d->pool_idx; q->pool_dy = (const char*)d->pool_dy; q->ldpdy = d->ldpdy;
  q->pd = d->sd; q->ph = d->sh; q->pw = d->sw;
  MI355_REQUIRE(!d->pool_y || (d->pool_widx && !d->pool_idx && !d->s2d_a && !d->s2d_da && !d->q8 && !d->fy && d->a && d->sd >= 2 &&
                               d->sh >= 2 && d->sw >= 2 && !((d->sd | d->sh | d->sw) & 1) && d->ldpy >= d->c &&
                               d->ldpy % (d->dtype == MI355_DT_F32 ? 4 : 8) == 0 &&
                               d->rows_per_group % ((long long)d->sd * d->sh * d->sw) == 0),
                "%s: the fused max-pool needs pool_widx, even extents sd/sh/sw that divide the row count, and plain layouts", who);
  q->pool_y = (char*)d->pool_y; q->ldpy = d->ldpy; q->pool_widx = (uint8_t*)d->pool_widx;
  if (d->s2d_a || d->s2d_da) {
    MI355_REQUIRE((long long)d->sd * d->sh * d->sw * (d->groups == 1 ? 1 : 1) > 0 &&
                  ((long long)d->rows_per_group * d->groups) % ((long long)d->sd * d->sh * d->sw) == 0,
                  "%s: space-to-depth extents do not match the row count", who);
    if (d->s2d_a) { int rc2 = check_s2d(d->sd, d->sh, d->sw, d->c, d->lda, who); if (rc2) return rc2; q->s2d_a = S2D{d->sd, d->sh, d->sw, d->c}; }
    if (d->s2d_da) { int rc2 = check_s2d(d->sd, d->sh, d->sw, d->c, d->ldda, who); if (rc2) return rc2; q->s2d_da = S2D{d->sd, d->sh, d->sw, d->c}; }
  }
  return MI355_OK;
}

}  // namespace
