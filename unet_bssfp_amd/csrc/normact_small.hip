// Fused norm + dropout + LeakyReLU of SMALL tensors (the low U-Net levels, the last PatchGAN blocks): statistics and apply in one
// launch each way, a workgroup per 16-byte channel piece.
#include "normact_common.h"

namespace {

// ------------------------------------------------------------------ norm + act of SMALL tensors, one kernel each way
// The low levels of the U-Net (16^3 x 256, 8^3 x 512 channels) and the last PatchGAN blocks (16^3 x 128 ... 4^3 x 512) hold
// 64 KB - 2 MB per tensor: statistics-from-the-conv-epilogue + norm_finalize + normact_fwd (forward) and reduce + finalize +
// apply (backward) are three launches of 4 - 13 us each on data that fits in L2 -- latency, not bandwidth.  Here ONE
// workgroup owns EPV channels (one 16-byte piece of every row) of ALL rows and groups: mean, then variance about that mean
// (two-pass: no sum-of-squares cancellation), then the apply pass, re-reading its L2-resident column; the groups are walked
// in order, so BatchNorm's running statistics and the affine gradients need no cross-workgroup reduction (deterministic).
struct NormSmallArgs {
  NormActArgs q;
  float eps, momentum;
  float* mean_out; float* rstd_out;                       // forward: [groups][c], saved for the backward pass
  float* running_mean; float* running_var; long long* batches_tracked; int n_real;
  float* dgamma; float* dbeta; int accumulate;            // backward: [n_affine]
};

constexpr int kSmallThreads = 512, kSmallWaves = kSmallThreads / 64;      // (1024 would cap the kernel at 128 registers: it spilled 500)
// per-thread f32 partial sums (a few rows each) -> block totals, combined in f64 in a fixed order (the three-launch path
// combines its per-block partials in f64 too: gradient sums with heavy cancellation keep their sign)
template <int EPV>
__device__ __forceinline__ void block_sum_vec(const float (&v)[EPV], double (&t)[EPV], double* red /* [kSmallWaves][EPV] */) {
#pragma unroll
  for (int j = 0; j < EPV; ++j) {
    double d = (double)v[j];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) d += __shfl_xor(d, o, 64);
    t[j] = d;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();                                        // red may still be read from the previous reduction
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < EPV; ++j) red[wave * EPV + j] = t[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < EPV; ++j) {
    double a = 0.0;
#pragma unroll
    for (int w = 0; w < kSmallWaves; ++w) a += red[w * EPV + j];
    t[j] = a;
  }
}

template <typename T, bool DROP>
__global__ __launch_bounds__(kSmallThreads) void normact_small_fwd_kernel(const NormSmallArgs p) {
  constexpr int EPV = Elem<T>::kPer16B;
  __shared__ double red[kSmallWaves * EPV];
  const NormActArgs& q = p.q;
  const int ch0 = blockIdx.x * EPV;
  const unsigned long long seed = DROP ? eff_seed(q.seed, q.seed_ptr) : 0ull;
  const float slope = act_slope(q);
  float ga[EPV], be[EPV];
#pragma unroll
  for (int j = 0; j < EPV; ++j) {
    const int ch = ch0 + j;
    ga[j] = q.gamma ? (ch < q.n_affine ? q.gamma[ch] : 0.f) : 1.f;
    be[j] = (q.beta && ch < q.n_affine) ? q.beta[ch] : 0.f;
  }
  if (p.batches_tracked && blockIdx.x == 0 && threadIdx.x == 0) p.batches_tracked[0] += q.groups;
  const double inv = 1.0 / (double)q.rows_per_group;
  for (int g = 0; g < q.groups; ++g) {
    const T* zb = reinterpret_cast<const T*>(q.z) + (long long)g * q.rows_per_group * q.ldz + ch0;
    float s[EPV], mu[EPV], rs[EPV];
    double t[EPV];
#pragma unroll
    for (int j = 0; j < EPV; ++j) s[j] = 0.f;
    // (512 threads x U rows in flight: the column is L2-resident and a pass is one latency -- with 256 threads walking it one
    //  dependent load per iteration the kernel took 24 us, longer than the three launches it replaces)
    constexpr int U = 8;
    for (long long row0 = threadIdx.x; row0 < q.rows_per_group; row0 += kSmallThreads * U) {
      uint4 raw[U];                                        // (packed while in flight: 4 registers per row, not EPV)
#pragma unroll
      for (int u = 0; u < U; ++u) if (row0 + u * kSmallThreads < q.rows_per_group) raw[u] = *reinterpret_cast<const uint4*>(zb + (row0 + u * kSmallThreads) * q.ldz);
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (row0 + u * kSmallThreads < q.rows_per_group) {
          Vec16<T> v; v.from_bits(raw[u]);
#pragma unroll
          for (int j = 0; j < EPV; ++j) s[j] += v.f[j];
        }
    }
    block_sum_vec<EPV>(s, t, red);
#pragma unroll
    for (int j = 0; j < EPV; ++j) { mu[j] = (float)(t[j] * inv); s[j] = 0.f; }
    for (long long row0 = threadIdx.x; row0 < q.rows_per_group; row0 += kSmallThreads * U) {
      uint4 raw[U];
#pragma unroll
      for (int u = 0; u < U; ++u) if (row0 + u * kSmallThreads < q.rows_per_group) raw[u] = *reinterpret_cast<const uint4*>(zb + (row0 + u * kSmallThreads) * q.ldz);
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (row0 + u * kSmallThreads < q.rows_per_group) {
          Vec16<T> v; v.from_bits(raw[u]);
#pragma unroll
          for (int j = 0; j < EPV; ++j) { const float d = v.f[j] - mu[j]; s[j] += d * d; }
        }
    }
    block_sum_vec<EPV>(s, t, red);
#pragma unroll
    for (int j = 0; j < EPV; ++j) rs[j] = (float)(1.0 / sqrt(t[j] * inv + (double)p.eps));
    if (threadIdx.x == 0) {
#pragma unroll
      for (int j = 0; j < EPV; ++j) {
        const int ch = ch0 + j;
        p.mean_out[(long long)g * q.c + ch] = mu[j];
        p.rstd_out[(long long)g * q.c + ch] = rs[j];
        if (p.running_mean && ch < p.n_real) {
          const double var = t[j] * inv;
          const double unb = q.rows_per_group > 1 ? var * (double)q.rows_per_group / (double)(q.rows_per_group - 1) : var;
          p.running_mean[ch] = (float)((1.0 - p.momentum) * p.running_mean[ch] + p.momentum * (double)mu[j]);
          p.running_var[ch] = (float)((1.0 - p.momentum) * p.running_var[ch] + p.momentum * unb);
        }
      }
    }
    float sc[EPV], sh[EPV];
#pragma unroll
    for (int j = 0; j < EPV; ++j) { sc[j] = ga[j] * rs[j]; sh[j] = be[j] - mu[j] * ga[j] * rs[j]; }
    T* ab = reinterpret_cast<T*>(q.a) + (long long)g * q.rows_per_group * q.lda + ch0;
    for (long long row0 = threadIdx.x; row0 < q.rows_per_group; row0 += kSmallThreads * U) {
      uint4 raw[U];
#pragma unroll
      for (int u = 0; u < U; ++u) if (row0 + u * kSmallThreads < q.rows_per_group) raw[u] = *reinterpret_cast<const uint4*>(zb + (row0 + u * kSmallThreads) * q.ldz);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long row = row0 + u * kSmallThreads;
        if (row >= q.rows_per_group) continue;
        Vec16<T> v; v.from_bits(raw[u]);
        unsigned keep = 0;
        if constexpr (DROP) keep = drop_keep_mask<EPV>(seed, ((unsigned long long)g * q.rows_per_group + row) * q.c + ch0, q.thr16);
#pragma unroll
        for (int j = 0; j < EPV; ++j) {
          float t2 = v.f[j] * sc[j] + sh[j];
          if constexpr (DROP) t2 = (keep >> j) & 1u ? t2 * q.drop_scale : 0.f;
          v.f[j] = t2 > 0.f ? t2 : t2 * slope;
        }
        if (q.s2d_a.d) {
          long long srow; int blk, border;
          s2d_cell(q.s2d_a, (long long)g * q.rows_per_group + row, srow, blk, border);
          v.store(reinterpret_cast<T*>(q.a) + srow * q.lda + (long long)blk * q.s2d_a.cblk + ch0);
          s2d_zero_siblings<T>(reinterpret_cast<T*>(q.a), q.s2d_a, srow, blk, border, q.lda, ch0);
        } else v.store(ab + row * q.lda);
      }
    }
  }
}

// PRELU: a third sum, the slope gradient's share, per group and channel into q.dalpha_part ([groups][c] doubles); the host's
// slope_grad_sum_kernel launch adds them
template <typename T, bool DROP, bool PRELU = false>
__global__ __launch_bounds__(kSmallThreads) void normact_small_bwd_kernel(const NormSmallArgs p) {
  constexpr int EPV = Elem<T>::kPer16B;
  __shared__ double red[kSmallWaves * EPV];
  const NormActArgs& q = p.q;
  const int ch0 = blockIdx.x * EPV;
  const unsigned long long seed = DROP ? eff_seed(q.seed, q.seed_ptr) : 0ull;
  const float slope = act_slope(q);
  const double inv = 1.0 / (double)q.rows_per_group;
  double tg[EPV], tb[EPV];
#pragma unroll
  for (int j = 0; j < EPV; ++j) { tg[j] = 0.0; tb[j] = 0.0; }
  for (int g = 0; g < q.groups; ++g) {
    BwdConst<EPV> k;
    load_bwd_const<EPV>(q, g, ch0, k);
    const T* zb = reinterpret_cast<const T*>(q.z) + (long long)g * q.rows_per_group * q.ldz + ch0;
    const T* db = reinterpret_cast<const T*>(q.da) + (long long)g * q.rows_per_group * q.ldda + ch0;
    auto load_da = [&](long long row) {
      if (q.s2d_da.d) return *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(q.da) + s2d_offset(q.s2d_da, (long long)g * q.rows_per_group + row, q.ldda) + ch0);
      return *reinterpret_cast<const uint4*>(db + row * q.ldda);
    };
    float s0[EPV], s1[EPV], s2[EPV];
#pragma unroll
    for (int j = 0; j < EPV; ++j) { s0[j] = 0.f; s1[j] = 0.f; s2[j] = 0.f; }
    constexpr int U = 2;                                 // (z and da rows in flight per thread: see the forward kernel)
    for (long long row0 = threadIdx.x; row0 < q.rows_per_group; row0 += kSmallThreads * U) {
      uint4 zr[U], dr[U];                                  // (packed while in flight)
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (row0 + u * kSmallThreads < q.rows_per_group) { zr[u] = *reinterpret_cast<const uint4*>(zb + (row0 + u * kSmallThreads) * q.ldz); dr[u] = load_da(row0 + u * kSmallThreads); }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long row = row0 + u * kSmallThreads;
        if (row >= q.rows_per_group) continue;
        Vec16<T> zv, dv; zv.from_bits(zr[u]); dv.from_bits(dr[u]);
        unsigned keep = 0;
        if constexpr (DROP) keep = drop_keep_mask<EPV>(seed, ((unsigned long long)g * q.rows_per_group + row) * q.c + ch0, q.thr16);
#pragma unroll
        for (int j = 0; j < EPV; ++j) {
          float gv, xh, at;
          bwd_elem<DROP>(q, slope, (keep >> j) & 1u, k.mu[j], k.rs[j], k.ga[j], k.be[j], zv.f[j], dv.f[j], gv, xh, at);
          s0[j] += gv;
          s1[j] += gv * xh;
          if constexpr (PRELU) s2[j] += at;
        }
      }
    }
    if constexpr (PRELU) {                 // (first, and written at once: its totals are live next to nothing else)
      double t2[EPV];
      block_sum_vec<EPV>(s2, t2, red);
      if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < EPV; ++j)      // (padded channels: u = 0, but their da is whatever the producer left)
          reinterpret_cast<double*>(q.dalpha_part)[(long long)g * q.c + ch0 + j] = ch0 + j < q.n_affine ? t2[j] : 0.0;
      }
    }
    double t0[EPV], t1[EPV];
    block_sum_vec<EPV>(s0, t0, red);
    block_sum_vec<EPV>(s1, t1, red);
    float kk[EPV], m0[EPV], m1[EPV];
    const bool sub = q.mean && q.batch_stats;
#pragma unroll
    for (int j = 0; j < EPV; ++j) {
      tb[j] += t0[j]; tg[j] += t1[j];
      kk[j] = k.ga[j] * k.rs[j];
      m0[j] = sub ? (float)(t0[j] * inv) : 0.f;
      m1[j] = sub ? (float)(t1[j] * inv) : 0.f;
    }
    T* ob = reinterpret_cast<T*>(q.dz) + (long long)g * q.rows_per_group * q.lddz + ch0;
    for (long long row0 = threadIdx.x; row0 < q.rows_per_group; row0 += kSmallThreads * U) {
      uint4 zr[U], dr[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (row0 + u * kSmallThreads < q.rows_per_group) { zr[u] = *reinterpret_cast<const uint4*>(zb + (row0 + u * kSmallThreads) * q.ldz); dr[u] = load_da(row0 + u * kSmallThreads); }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long row = row0 + u * kSmallThreads;
        if (row >= q.rows_per_group) continue;
        Vec16<T> zv, dv; zv.from_bits(zr[u]); dv.from_bits(dr[u]);
        unsigned keep = 0;
        if constexpr (DROP) keep = drop_keep_mask<EPV>(seed, ((unsigned long long)g * q.rows_per_group + row) * q.c + ch0, q.thr16);
#pragma unroll
        for (int j = 0; j < EPV; ++j) {
          float gv, xh;
          bwd_elem<DROP>(q, slope, (keep >> j) & 1u, k.mu[j], k.rs[j], k.ga[j], k.be[j], zv.f[j], dv.f[j], gv, xh);
          zv.f[j] = kk[j] * (gv - m0[j] - xh * m1[j]);
        }
        zv.store(ob + row * q.lddz);
      }
    }
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < EPV; ++j) {
      const int ch = ch0 + j;
      if (ch < q.n_affine) {
        if (p.dgamma) p.dgamma[ch] = p.accumulate ? p.dgamma[ch] + (float)tg[j] : (float)tg[j];
        if (p.dbeta) p.dbeta[ch] = p.accumulate ? p.dbeta[ch] + (float)tb[j] : (float)tb[j];
      }
    }
  }
}

// Register-resident forms (round 4, third session).  The kernels above are chains of dependent L2 round trips: the forward
// kernel reads its column three times (mean, variance, apply), the backward kernel twice in four dependent iterations, and
// the statistic groups of a stacked PatchGAN pair are walked one after the other -- 14 - 31 us for 64 KB per workgroup.
// Every eligible tensor is at most 16 rows per thread (<= 512 K elements of >= 64 channels over 512 threads), so the rows
// of GC groups x S slots stay in registers as the packed 16-byte pieces: ONE load latency per launch for GC groups, the
// passes after it are arithmetic.  Row -> thread assignment, accumulation order and the f64 block sums are those of the
// kernels above (bit-identical results); the host picks S = 1 (<= 512 rows per group) or 8 (<= 4096) and GC = 2 for an even
// number of groups.
constexpr int kSmallResMaxGroups = 16;
// Block sums of NV per-thread f32 partials, combined in f64 in a fixed order, through an LDS transpose: block_sum_vec's 6-step
// f64 butterfly per value is 12 ds_bpermute + 8 ds_read_b64 per value and THREAD -- 320 LDS instructions per wave for 16
// values, and the LDS pipe of one CU serves all 8 waves: that, not the loads, was most of these kernels' time (two groups per
// chunk cost 8 us more than one).  Here every thread writes its partials ([value][thread]: conflict-free), TPV threads per
// value add 512 / TPV of them each (strided by TPV: conflict-free) and finish with a log2(TPV)-step butterfly on ONE value;
// ~4 LDS instructions per value and thread.  CH values at a time (part: CH x 512 floats of LDS).
template <int NV, int CH>
__device__ __forceinline__ void block_sum_lds(const float (&v)[NV], double (&t)[NV], float* part /* [CH][kSmallThreads] */,
                                              double* total /* [CH] */) {
  static_assert(NV % CH == 0, "chunk");
  constexpr int TPV = (kSmallThreads / CH) < 64 ? (kSmallThreads / CH) : 64, CNT = kSmallThreads / TPV;
  const int tid = threadIdx.x;
#pragma unroll
  for (int c0 = 0; c0 < NV; c0 += CH) {
    __syncthreads();                                       // part / total may still be read from the previous round
#pragma unroll
    for (int i = 0; i < CH; ++i) part[i * kSmallThreads + tid] = v[c0 + i];
    __syncthreads();
    if (tid < CH * TPV) {
      const int val = tid / TPV, sg = tid % TPV;
      double a = 0.0;
#pragma unroll
      for (int i = 0; i < CNT; ++i) a += (double)part[val * kSmallThreads + i * TPV + sg];
#pragma unroll
      for (int o = 1; o < TPV; o <<= 1) a += __shfl_xor(a, o, 64);
      if (sg == 0) total[val] = a;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < CH; ++i) t[c0 + i] = total[i];
  }
}
template <typename T, bool DROP, int S, int GC>
__global__ __launch_bounds__(kSmallThreads) void normact_small_res_fwd_kernel(const NormSmallArgs p) {
  constexpr int EPV = Elem<T>::kPer16B, NV = GC * EPV;
  constexpr int CH = NV < 16 ? NV : 16;
  __shared__ float part[CH * kSmallThreads];
  __shared__ double total[CH];
  const NormActArgs& q = p.q;
  const int ch0 = blockIdx.x * EPV;
  const unsigned long long seed = DROP ? eff_seed(q.seed, q.seed_ptr) : 0ull;
  const float slope = act_slope(q);
  float ga[EPV], be[EPV];
#pragma unroll
  for (int j = 0; j < EPV; ++j) {
    const int ch = ch0 + j;
    ga[j] = q.gamma ? (ch < q.n_affine ? q.gamma[ch] : 0.f) : 1.f;
    be[j] = (q.beta && ch < q.n_affine) ? q.beta[ch] : 0.f;
  }
  if (p.batches_tracked && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) p.batches_tracked[0] += q.groups;
  const double inv = 1.0 / (double)q.rows_per_group;
  const int rows = (int)q.rows_per_group;
  // blockIdx.y = a chunk of groups when they are independent (no running statistics: the host sets gridDim.y = groups / GC)
  for (int g0 = blockIdx.y * GC; g0 < q.groups; g0 += gridDim.y * GC) {
    uint4 raw[GC][S];
#pragma unroll
    for (int c = 0; c < GC; ++c) {
      const T* zb = reinterpret_cast<const T*>(q.z) + (long long)(g0 + c) * q.rows_per_group * q.ldz + ch0;
#pragma unroll
      for (int u = 0; u < S; ++u) {
        const int row = threadIdx.x + u * kSmallThreads;
        raw[c][u] = row < rows ? *reinterpret_cast<const uint4*>(zb + (long long)row * q.ldz) : make_uint4(0, 0, 0, 0);
      }
    }
    float s[NV], mu[NV], rs[NV];
    double t[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) s[i] = 0.f;
#pragma unroll
    for (int c = 0; c < GC; ++c)
#pragma unroll
      for (int u = 0; u < S; ++u)
        if ((int)threadIdx.x + u * kSmallThreads < rows) {
          Vec16<T> v; v.from_bits(raw[c][u]);
#pragma unroll
          for (int j = 0; j < EPV; ++j) s[c * EPV + j] += v.f[j];
        }
    block_sum_lds<NV, CH>(s, t, part, total);
#pragma unroll
    for (int i = 0; i < NV; ++i) { mu[i] = (float)(t[i] * inv); s[i] = 0.f; }
#pragma unroll
    for (int c = 0; c < GC; ++c)
#pragma unroll
      for (int u = 0; u < S; ++u)
        if ((int)threadIdx.x + u * kSmallThreads < rows) {
          Vec16<T> v; v.from_bits(raw[c][u]);
#pragma unroll
          for (int j = 0; j < EPV; ++j) { const float d = v.f[j] - mu[c * EPV + j]; s[c * EPV + j] += d * d; }
        }
    block_sum_lds<NV, CH>(s, t, part, total);
#pragma unroll
    for (int i = 0; i < NV; ++i) rs[i] = (float)(1.0 / sqrt(t[i] * inv + (double)p.eps));
    if (threadIdx.x == 0) {
#pragma unroll
      for (int c = 0; c < GC; ++c) {                       // (groups in order: the running statistics are a recurrence)
        const int g = g0 + c;
#pragma unroll
        for (int j = 0; j < EPV; ++j) {
          const int ch = ch0 + j;
          p.mean_out[(long long)g * q.c + ch] = mu[c * EPV + j];
          p.rstd_out[(long long)g * q.c + ch] = rs[c * EPV + j];
          if (p.running_mean && ch < p.n_real) {
            const double var = t[c * EPV + j] * inv;
            const double unb = q.rows_per_group > 1 ? var * (double)q.rows_per_group / (double)(q.rows_per_group - 1) : var;
            p.running_mean[ch] = (float)((1.0 - p.momentum) * p.running_mean[ch] + p.momentum * (double)mu[c * EPV + j]);
            p.running_var[ch] = (float)((1.0 - p.momentum) * p.running_var[ch] + p.momentum * unb);
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < GC; ++c) {
      const int g = g0 + c;
      float sc[EPV], sh[EPV];
#pragma unroll
      for (int j = 0; j < EPV; ++j) { sc[j] = ga[j] * rs[c * EPV + j]; sh[j] = be[j] - mu[c * EPV + j] * ga[j] * rs[c * EPV + j]; }
      T* ab = reinterpret_cast<T*>(q.a) + (long long)g * q.rows_per_group * q.lda + ch0;
#pragma unroll
      for (int u = 0; u < S; ++u) {
        const long long row = threadIdx.x + u * kSmallThreads;
        if (row >= q.rows_per_group) continue;
        Vec16<T> v; v.from_bits(raw[c][u]);
        unsigned keep = 0;
        if constexpr (DROP) keep = drop_keep_mask<EPV>(seed, ((unsigned long long)g * q.rows_per_group + row) * q.c + ch0, q.thr16);
#pragma unroll
        for (int j = 0; j < EPV; ++j) {
          float t2 = v.f[j] * sc[j] + sh[j];
          if constexpr (DROP) t2 = (keep >> j) & 1u ? t2 * q.drop_scale : 0.f;
          v.f[j] = t2 > 0.f ? t2 : t2 * slope;
        }
        if (q.s2d_a.d) {
          long long srow; int blk, border;
          s2d_cell(q.s2d_a, (long long)g * q.rows_per_group + row, srow, blk, border);
          v.store(reinterpret_cast<T*>(q.a) + srow * q.lda + (long long)blk * q.s2d_a.cblk + ch0);
          s2d_zero_siblings<T>(reinterpret_cast<T*>(q.a), q.s2d_a, srow, blk, border, q.lda, ch0);
        } else v.store(ab + row * q.lda);
      }
    }
  }
}

template <typename T, bool DROP, int S, int GC>
__global__ __launch_bounds__(kSmallThreads) void normact_small_res_bwd_kernel(const NormSmallArgs p) {
  constexpr int EPV = Elem<T>::kPer16B, NV = 2 * GC * EPV;     // sum g | sum g * xhat, per group of the chunk
  constexpr int CH = NV < 16 ? NV : 16;
  __shared__ float part[CH * kSmallThreads];
  __shared__ double total[CH];
  const NormActArgs& q = p.q;
  const int ch0 = blockIdx.x * EPV;
  const unsigned long long seed = DROP ? eff_seed(q.seed, q.seed_ptr) : 0ull;
  const double inv = 1.0 / (double)q.rows_per_group;
  const int rows = (int)q.rows_per_group;
  const float slope = act_slope(q);
  constexpr int NST = S > 1 ? 3 : 0;                      // S = 8: the last 3 da rows wait in LDS between the passes (each thread its
  __shared__ uint4 stash[NST ? NST * kSmallThreads : 1];   //  own 16-byte slots, conflict-free; as registers next to z they spilled 13 - 70)
  __shared__ double tot[kSmallResMaxGroups * 2 * EPV];     // per group (sum g | sum g * xhat), written by thread 0: the sums over the
                                                           //  groups are formed at the end (as 32 registers of every thread they spilled)
  // blockIdx.y = a chunk of groups when the host gave scratch for the per-group sums (q.part: [groups][2][c] doubles); the affine
  // gradients are then summed over the groups, in the same order and in f64, by normact_small_affine_kernel
  double* const gpart = reinterpret_cast<double*>(q.part);
  for (int g0 = blockIdx.y * GC; g0 < q.groups; g0 += gridDim.y * GC) {
    BwdConst<EPV> k[GC];
    uint4 zr[GC][S], dr[GC][S];
#pragma unroll
    for (int c = 0; c < GC; ++c) {
      const int g = g0 + c;
      load_bwd_const<EPV>(q, g, ch0, k[c]);
      const T* zb = reinterpret_cast<const T*>(q.z) + (long long)g * q.rows_per_group * q.ldz + ch0;
      const T* db = reinterpret_cast<const T*>(q.da) + (long long)g * q.rows_per_group * q.ldda + ch0;
#pragma unroll
      for (int u = 0; u < S; ++u) {
        const int row = threadIdx.x + u * kSmallThreads;
        zr[c][u] = dr[c][u] = make_uint4(0, 0, 0, 0);
        if (row < rows) {
          zr[c][u] = *reinterpret_cast<const uint4*>(zb + (long long)row * q.ldz);
          dr[c][u] = q.s2d_da.d ? *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(q.da) + s2d_offset(q.s2d_da, (long long)g * q.rows_per_group + row, q.ldda) + ch0)
                                : *reinterpret_cast<const uint4*>(db + (long long)row * q.ldda);
        }
      }
    }
    float s[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) s[i] = 0.f;
#pragma unroll
    for (int c = 0; c < GC; ++c)
#pragma unroll
      for (int u = 0; u < S; ++u) {
        const long long row = threadIdx.x + u * kSmallThreads;
        if (row >= q.rows_per_group) continue;
        Vec16<T> zv, dv; zv.from_bits(zr[c][u]); dv.from_bits(dr[c][u]);
        unsigned keep = 0;
        if constexpr (DROP) keep = drop_keep_mask<EPV>(seed, ((unsigned long long)(g0 + c) * q.rows_per_group + row) * q.c + ch0, q.thr16);
#pragma unroll
        for (int j = 0; j < EPV; ++j) {
          float gv, xh;
          bwd_elem<DROP>(q, slope, (keep >> j) & 1u, k[c].mu[j], k[c].rs[j], k[c].ga[j], k[c].be[j], zv.f[j], dv.f[j], gv, xh);
          s[(2 * c) * EPV + j] += gv;
          s[(2 * c + 1) * EPV + j] += gv * xh;
        }
        if (u >= S - NST) stash[(u - (S - NST)) * kSmallThreads + threadIdx.x] = dr[c][u];
      }
    double t[NV];
    block_sum_lds<NV, CH>(s, t, part, total);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        if (gpart) gpart[((long long)g0 * 2 + i / EPV) * q.c + ch0 + i % EPV] = t[i];
        else tot[g0 * 2 * EPV + i] = t[i];
      }
    }
    const bool sub = q.mean && q.batch_stats;
#pragma unroll
    for (int c = 0; c < GC; ++c) {
      const int g = g0 + c;
      float kk[EPV], m0[EPV], m1[EPV];
#pragma unroll
      for (int j = 0; j < EPV; ++j) {
        const double t0 = t[(2 * c) * EPV + j], t1 = t[(2 * c + 1) * EPV + j];
        kk[j] = k[c].ga[j] * k[c].rs[j];
        m0[j] = sub ? (float)(t0 * inv) : 0.f;
        m1[j] = sub ? (float)(t1 * inv) : 0.f;
      }
      T* ob = reinterpret_cast<T*>(q.dz) + (long long)g * q.rows_per_group * q.lddz + ch0;
#pragma unroll
      for (int u = 0; u < S; ++u) {
        const long long row = threadIdx.x + u * kSmallThreads;
        if (row >= q.rows_per_group) continue;
        Vec16<T> zv, dv; zv.from_bits(zr[c][u]);
        if (u >= S - NST) dv.from_bits(stash[(u - (S - NST)) * kSmallThreads + threadIdx.x]); else dv.from_bits(dr[c][u]);
        unsigned keep = 0;
        if constexpr (DROP) keep = drop_keep_mask<EPV>(seed, ((unsigned long long)g * q.rows_per_group + row) * q.c + ch0, q.thr16);
#pragma unroll
        for (int j = 0; j < EPV; ++j) {
          float gv, xh;
          bwd_elem<DROP>(q, slope, (keep >> j) & 1u, k[c].mu[j], k[c].rs[j], k[c].ga[j], k[c].be[j], zv.f[j], dv.f[j], gv, xh);
          zv.f[j] = kk[j] * (gv - m0[j] - xh * m1[j]);
        }
        zv.store(ob + row * q.lddz);
      }
    }
  }
  if (threadIdx.x == 0 && !gpart) {
#pragma unroll
    for (int j = 0; j < EPV; ++j) {
      const int ch = ch0 + j;
      if (ch < q.n_affine) {
        double tb = 0.0, tg = 0.0;
        for (int g = 0; g < q.groups; ++g) { tb += tot[(2 * g) * EPV + j]; tg += tot[(2 * g + 1) * EPV + j]; }
        if (p.dgamma) p.dgamma[ch] = p.accumulate ? p.dgamma[ch] + (float)tg : (float)tg;
        if (p.dbeta) p.dbeta[ch] = p.accumulate ? p.dbeta[ch] + (float)tb : (float)tb;
      }
    }
  }
}

// the affine gradients of the form above with blockIdx.y = chunk of groups: sum over the groups in order, in f64 (what thread 0 of
// the single-workgroup form does from its LDS totals: bit-identical)
__global__ __launch_bounds__(256) void normact_small_affine_kernel(const double* __restrict__ gpart, int groups, int c, int n_affine,
                                                                   float* dgamma, float* dbeta, int accumulate) {
  const int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= n_affine) return;
  double tb = 0.0, tg = 0.0;
  for (int g = 0; g < groups; ++g) { tb += gpart[((long long)g * 2 + 0) * c + ch]; tg += gpart[((long long)g * 2 + 1) * c + ch]; }
  if (dgamma) dgamma[ch] = accumulate ? dgamma[ch] + (float)tg : (float)tg;
  if (dbeta) dbeta[ch] = accumulate ? dbeta[ch] + (float)tb : (float)tb;
}

// S = 1 / 8 row slots per thread and group (s_slots), GC = 1 / 2 groups per chunk (chunk; two groups of 8 slots spilled 100 - 900 registers)
#define MI355_SMALL_RES_LAUNCH(KERNEL, T, DROP, GC8)                                                                \
  do {                                                                                                              \
    if (s_slots == 1) {                                                                                             \
      if (chunk == 2) KERNEL<T, DROP, 1, 2><<<grid, dim3(kSmallThreads), 0, (hipStream_t)stream>>>(p);              \
      else KERNEL<T, DROP, 1, 1><<<grid, dim3(kSmallThreads), 0, (hipStream_t)stream>>>(p);                         \
    } else {                                                                                                        \
      if (chunk == 2) KERNEL<T, DROP, 8, GC8><<<grid, dim3(kSmallThreads), 0, (hipStream_t)stream>>>(p);            \
      else KERNEL<T, DROP, 8, 1><<<grid, dim3(kSmallThreads), 0, (hipStream_t)stream>>>(p);                         \
    }                                                                                                               \
  } while (0)

}  // namespace

extern "C" {

int mi355_normact_small_fwd(const mi355_normact_small_desc* d, void* stream) {
  NormSmallArgs p;
  MI355_REQUIRE(d, "normact_small_fwd: null pointer");
  int rc = fill_normact(&d->base, &p.q, "normact_small_fwd");
  if (rc) return rc;
  MI355_REQUIRE(d->base.a && d->base.lda >= d->base.c && d->mean_out && d->rstd_out, "normact_small_fwd: bad output");
  MI355_REQUIRE(!d->running_mean || d->running_var, "normact_small_fwd: running_mean without running_var");
  p.eps = d->eps; p.momentum = d->momentum; p.mean_out = d->mean_out; p.rstd_out = d->rstd_out;
  p.running_mean = d->running_mean; p.running_var = d->running_var; p.batches_tracked = (long long*)d->batches_tracked;
  p.n_real = d->n_real > 0 ? d->n_real : d->base.c;
  p.dgamma = p.dbeta = nullptr; p.accumulate = 0;
  const int epv = d->base.dtype == MI355_DT_F32 ? 4 : 8;
  dim3 grid(d->base.c / epv);
  if (p.q.rows_per_group <= 8ll * kSmallThreads && p.q.groups <= kSmallResMaxGroups) {       // register-resident form: one load latency per chunk of groups
    const int s_slots = p.q.rows_per_group <= kSmallThreads ? 1 : 8, chunk = p.q.groups % 2 == 0 ? 2 : 1;
    // InstanceNorm (no running statistics, which are a recurrence over the groups): the chunks of groups are independent workgroups --
    // the reference's batch of 8 patches is 8 groups of 64 - 512 rows, walked 4 chunks deep by c / 8 = 16 - 32 workgroups otherwise
    if (!p.running_mean) grid.y = (unsigned)(p.q.groups / chunk);
    for_dtype_drop(d->base.dtype, p.q.thr16, [&](auto t, auto drop) { MI355_SMALL_RES_LAUNCH(normact_small_res_fwd_kernel, decltype(t), drop, 2); });
    return mi355_check_launch("normact_small_fwd");
  }
  for_dtype_drop(d->base.dtype, p.q.thr16, [&](auto t, auto drop) { normact_small_fwd_kernel<decltype(t), drop><<<grid, dim3(kSmallThreads), 0, (hipStream_t)stream>>>(p); });
  return mi355_check_launch("normact_small_fwd");
}

int mi355_normact_small_bwd(const mi355_normact_small_desc* d, void* stream) {
  NormSmallArgs p;
  MI355_REQUIRE(d, "normact_small_bwd: null pointer");
  int rc = fill_normact(&d->base, &p.q, "normact_small_bwd");
  if (rc) return rc;
  MI355_REQUIRE(d->base.da && d->base.dz && d->base.mean, "normact_small_bwd: null pointer");
  p.eps = d->eps; p.momentum = 0.f; p.mean_out = p.rstd_out = nullptr;
  p.running_mean = p.running_var = nullptr; p.batches_tracked = nullptr; p.n_real = 0;
  p.dgamma = d->dgamma; p.dbeta = d->dbeta; p.accumulate = d->accumulate;
  const int epv = d->base.dtype == MI355_DT_F32 ? 4 : 8;
  dim3 grid(d->base.c / epv);
  if (d->base.dalpha) {
    // PReLU with a slope gradient to form: the plain kernel with a third sum (the register-resident forms below sit at their register
    // limit -- see the notes on NST and GC8 -- and were not given one more value per channel and group), then the sum over groups and channels
    for_dtype_drop(d->base.dtype, p.q.thr16, [&](auto t, auto drop) { normact_small_bwd_kernel<decltype(t), drop, true><<<grid, dim3(kSmallThreads), 0, (hipStream_t)stream>>>(p); });
    slope_grad_sum_kernel<<<dim3(1), dim3(256), 0, (hipStream_t)stream>>>(reinterpret_cast<const double*>(d->base.dalpha_part),
                                                                          p.q.groups * p.q.c, d->base.dalpha, d->accumulate);
    return mi355_check_launch("normact_small_bwd");
  }
  if (p.q.rows_per_group <= 8ll * kSmallThreads && p.q.groups <= kSmallResMaxGroups) {       // register-resident form: one load latency per chunk of groups
    const int s_slots = p.q.rows_per_group <= kSmallThreads ? 1 : 8, chunk = p.q.groups % 2 == 0 ? 2 : 1;
    // scratch for the per-group sums given (base.part: groups x 2 x c doubles): the chunks of groups are independent workgroups and the
    // affine gradients are summed over the groups by a second, tiny launch
    const bool split = d->base.part != nullptr && p.q.groups / chunk > 1;
    if (split) grid.y = (unsigned)(p.q.groups / chunk); else p.q.part = nullptr;
    for_dtype_drop(d->base.dtype, p.q.thr16, [&](auto t, auto drop) { MI355_SMALL_RES_LAUNCH(normact_small_res_bwd_kernel, decltype(t), drop, 1); });
    if (split && (p.dgamma || p.dbeta) && p.q.n_affine > 0)
      normact_small_affine_kernel<<<dim3((p.q.n_affine + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(
          reinterpret_cast<const double*>(d->base.part), p.q.groups, p.q.c, p.q.n_affine, p.dgamma, p.dbeta, p.accumulate);
    return mi355_check_launch("normact_small_bwd");
  }
  for_dtype_drop(d->base.dtype, p.q.thr16, [&](auto t, auto drop) { normact_small_bwd_kernel<decltype(t), drop><<<grid, dim3(kSmallThreads), 0, (hipStream_t)stream>>>(p); });
  return mi355_check_launch("normact_small_bwd");
}

}  // extern "C"
