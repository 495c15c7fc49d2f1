// Channel statistics and the fused norm + dropout + LeakyReLU of the large tensors, forward (plain, with the MaxPool3d(2) that
// consumes it, with the final 1x1x1 convolution) and backward (reduce / finalize / apply; da a tensor, an implicit 1x1x1 data
// gradient or an implicit max-pool backward).  HBM-bound: thread = (row, 16-byte piece of its channels).
#include "normact_common.h"

namespace {

constexpr int kRowsPerStatBlock = 2048;

// ------------------------------------------------------------------ channel statistics
// One block = up to kRowsPerStatBlock rows of one group.  Thread = (row-in-pass, 16-B piece).
// f(row values) is supplied by the functor; sums of two quantities per channel are produced -- or of three (out2: the PReLU slope
// gradient's share, which the functor adds into s2).
template <typename T, bool THIRD = false, typename F>
__device__ __forceinline__ void block_channel_sums(int c, long long row_begin, long long row_end, F f,
                                                   float* out0, float* out1, float* out2 = nullptr) {
  constexpr int EPV = Elem<T>::kPer16B;
  constexpr int W = THIRD ? 24 : 16;       // floats of LDS per thread
  __shared__ float red[256 * W];
  const int lpr = c / EPV;                 // 16-B pieces per row (<= 128)
  const int rpp = 256 / lpr;               // rows per pass
  const int piece = threadIdx.x % lpr, rsub = threadIdx.x / lpr;
  float s0[EPV], s1[EPV], s2[EPV];
#pragma unroll
  for (int j = 0; j < EPV; ++j) { s0[j] = 0.f; s1[j] = 0.f; s2[j] = 0.f; }
  if (rsub < rpp)
    for (long long row = row_begin + rsub; row < row_end; row += rpp) {
      if constexpr (THIRD) f(row, piece * EPV, s0, s1, s2);
      else f(row, piece * EPV, s0, s1);
    }
#pragma unroll
  for (int j = 0; j < EPV; ++j) {
    red[threadIdx.x * W + j] = s0[j];
    red[threadIdx.x * W + 8 + j] = s1[j];
    if constexpr (THIRD) red[threadIdx.x * W + 16 + j] = s2[j];
  }
  __syncthreads();
  for (int ch = threadIdx.x; ch < c; ch += 256) {
    const int p = ch / EPV, j = ch % EPV;
    float t0 = 0.f, t1 = 0.f, t2 = 0.f;
    for (int q = 0; q < rpp; ++q) {
      t0 += red[(q * lpr + p) * W + j];
      t1 += red[(q * lpr + p) * W + 8 + j];
      if constexpr (THIRD) t2 += red[(q * lpr + p) * W + 16 + j];
    }
    out0[ch] = t0;
    out1[ch] = t1;
    if constexpr (THIRD) out2[ch] = t2;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void channel_stats_kernel(const T* __restrict__ x, int ld, int c,
                                                             long long rows_per_group, float* __restrict__ part,
                                                             int blocks_per_group) {
  const int g = blockIdx.y, b = blockIdx.x;
  const long long rb = (rows_per_group + blocks_per_group - 1) / blocks_per_group;
  const long long r0 = (long long)b * rb;
  long long r1 = r0 + rb;
  if (r1 > rows_per_group) r1 = rows_per_group;
  const T* base = x + (long long)g * rows_per_group * ld;
  float* out = part + ((long long)g * blocks_per_group + b) * 2 * c;
  block_channel_sums<T>(c, r0, r1,
      [&](long long row, int ch0, float* s0, float* s1) {
        Vec16<T> v;
        v.load(base + row * ld + ch0);
#pragma unroll
        for (int j = 0; j < Vec16<T>::N; ++j) { s0[j] += v.f[j]; s1[j] += v.f[j] * v.f[j]; }
      },
      out, out + c);
}

// Sum of per-block/per-tile partials part[k][2][c] over k for 8 channels per workgroup:
// 1024 threads = 8 channels x 128 partial lanes, f64 accumulate, fixed-order shuffle + LDS combine (deterministic).
// The totals of channel ch0 + (tid & 7) are returned to the threads with tid < 8.
__device__ __forceinline__ void block_sum_parts(const float* __restrict__ part, int nparts, int c, int ch0,
                                                double& t0, double& t1) {
  __shared__ double red[16][8][2];
  const int cl = threadIdx.x & 7, pl = threadIdx.x >> 3;
  const int ch = ch0 + cl;
  double s0 = 0.0, s1 = 0.0;
  if (ch < c) {
    int k = pl;
    for (; k + 384 < nparts; k += 512) {
      const float a0 = part[(long long)k * 2 * c + ch], b0 = part[(long long)k * 2 * c + c + ch];
      const float a1 = part[(long long)(k + 128) * 2 * c + ch], b1 = part[(long long)(k + 128) * 2 * c + c + ch];
      const float a2 = part[(long long)(k + 256) * 2 * c + ch], b2 = part[(long long)(k + 256) * 2 * c + c + ch];
      const float a3 = part[(long long)(k + 384) * 2 * c + ch], b3 = part[(long long)(k + 384) * 2 * c + c + ch];
      s0 += ((double)a0 + (double)a1) + ((double)a2 + (double)a3);
      s1 += ((double)b0 + (double)b1) + ((double)b2 + (double)b3);
    }
    for (; k < nparts; k += 128) {
      s0 += (double)part[(long long)k * 2 * c + ch];
      s1 += (double)part[(long long)k * 2 * c + c + ch];
    }
  }
  // the 8 partial lanes of a wave (lane bits 3..5) by shuffles, then the 16 waves through LDS in a fixed order:
  // two barriers instead of a 7-level LDS tree (these kernels are pure latency: ~90 launches per step)
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) {
    s0 += __shfl_xor(s0, o, 64);
    s1 += __shfl_xor(s1, o, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) < 8) { red[wave][cl][0] = s0; red[wave][cl][1] = s1; }
  __syncthreads();
  double a0 = 0.0, a1 = 0.0;
#pragma unroll
  for (int w = 0; w < 16; ++w) { a0 += red[w][cl][0]; a1 += red[w][cl][1]; }
  t0 = a0;
  t1 = a1;
  __syncthreads();      // red is reused by the caller's next call
}

__global__ __launch_bounds__(1024) void norm_finalize_kernel(const float* __restrict__ part, int ppg, int c,
                                                             long long count, const float* __restrict__ shift,
                                                             int n_real, float eps, float* __restrict__ mean,
                                                             float* __restrict__ rstd, float* running_mean,
                                                             float* running_var, float momentum,
                                                             long long* batches_tracked, int groups_here) {
  // groups_here == 1: this workgroup's group is blockIdx.y.  groups_here > 1 (BatchNorm over several statistic groups in
  // one call -- the discriminator's fake and real batch stacked, src/model.py:185-186): the groups are walked IN ORDER by one
  // workgroup per channel block, so that the running statistics receive the momentum updates of two consecutive forward calls.
  const int ch0 = blockIdx.x * 8;
  if (batches_tracked && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) batches_tracked[0] += groups_here;   // BatchNorm's counter
  for (int gi = 0; gi < groups_here; ++gi) {
    const int g = groups_here > 1 ? gi : blockIdx.y;
    double s1, s2;
    block_sum_parts(part + (long long)g * ppg * 2 * c, ppg, c, ch0, s1, s2);
    const int ch = ch0 + (int)threadIdx.x;
    if (threadIdx.x >= 8 || ch >= c) continue;
    const double m = s1 / (double)count;
    double var = s2 / (double)count - m * m;
    if (var < 0.0) var = 0.0;
    const double mu = m + ((shift && ch < n_real) ? (double)shift[ch] : 0.0);
    mean[(long long)g * c + ch] = (float)mu;
    rstd[(long long)g * c + ch] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean && ch < n_real) {
      const double unb = count > 1 ? var * (double)count / (double)(count - 1) : var;
      running_mean[ch] = (float)((1.0 - momentum) * running_mean[ch] + momentum * mu);
      running_var[ch] = (float)((1.0 - momentum) * running_var[ch] + momentum * unb);
    }
  }
}

// out[j] (+)= column sum of channel offset + j, j < n_out
__global__ __launch_bounds__(1024) void colsum_finalize_kernel(const float* __restrict__ part, int parts, int c, int offset,
                                                               float* __restrict__ out, int n_out, int accumulate) {
  const int ch0 = offset + blockIdx.x * 8;
  double s0, s1;
  block_sum_parts(part, parts, c, ch0, s0, s1);
  const int j = blockIdx.x * 8 + (int)threadIdx.x;
  if (threadIdx.x < 8 && j < n_out) out[j] = accumulate ? out[j] + (float)s0 : (float)s0;
}

// ------------------------------------------------------------------ norm + dropout + LeakyReLU
template <typename T, bool DROP>
__global__ __launch_bounds__(256) void normact_fwd_kernel(const NormActArgs q) {
  constexpr int EPV = Elem<T>::kPer16B;
  const int g = blockIdx.y;
  const int lpr = q.c / EPV, rpp = 256 / lpr;
  const int piece = threadIdx.x % lpr, rsub = threadIdx.x / lpr;
  if (rsub >= rpp) return;
  const int ch0 = piece * EPV;
  const unsigned long long seed = DROP ? eff_seed(q.seed, q.seed_ptr) : 0ull;
  float sc[EPV], sh[EPV];
#pragma unroll
  for (int j = 0; j < EPV; ++j) {
    const int ch = ch0 + j;
    const float ga = q.gamma ? (ch < q.n_affine ? q.gamma[ch] : 0.f) : 1.f, be = (q.beta && ch < q.n_affine) ? q.beta[ch] : 0.f;
    if (q.mean) {
      const float rs = q.rstd[(long long)g * q.c + ch], mu = q.mean[(long long)g * q.c + ch];
      sc[j] = ga * rs;
      sh[j] = be - mu * ga * rs;
    } else { sc[j] = ga; sh[j] = be; }
  }
  const T* zb = reinterpret_cast<const T*>(q.z) + (long long)g * q.rows_per_group * q.ldz;
  T* ab = reinterpret_cast<T*>(q.a) + (long long)g * q.rows_per_group * q.lda;
  const long long stride = (long long)gridDim.x * rpp;
  const float sc8 = q.q8 ? fp8_scale_of(q.q_use) : 1.f;
  const float slope = act_slope(q);
  float m8 = 0.f;
  for (long long row = (long long)blockIdx.x * rpp + rsub; row < q.rows_per_group; row += stride) {
    Vec16<T> v;
#ifdef NORM_NT_FWD
    v.load_nt(zb + row * q.ldz + ch0);
#else
    v.load(zb + row * q.ldz + ch0);
#endif
    const unsigned long long e0 = ((unsigned long long)g * q.rows_per_group + row) * q.c + ch0;
    unsigned keep = 0;
    if constexpr (DROP) keep = drop_keep_mask<EPV>(seed, e0, q.thr16);
#pragma unroll
    for (int j = 0; j < EPV; ++j) {
      float t = v.f[j] * sc[j] + sh[j];
      if constexpr (DROP) t = (keep >> j) & 1u ? t * q.drop_scale : 0.f;
      v.f[j] = t > 0.f ? t : t * slope;
    }
    if (q.s2d_a.d) {
      long long srow; int blk, border;
      s2d_cell(q.s2d_a, (long long)g * q.rows_per_group + row, srow, blk, border);
      v.store(reinterpret_cast<T*>(q.a) + srow * q.lda + (long long)blk * q.s2d_a.cblk + ch0);
      s2d_zero_siblings<T>(reinterpret_cast<T*>(q.a), q.s2d_a, srow, blk, border, q.lda, ch0);
    }
#ifdef FP8_NT_A     // (fp8 mode: the next convolution reads the e4m3 copy; the bf16 tensor's next reader is the weight gradient, a backward pass away)
    else if (q.q8) store16_nt(v, ab + row * q.lda + ch0);
#endif
    else v.store(ab + row * q.lda + ch0);
    if constexpr (sizeof(T) == 2) {
      if (q.q8) m8 = fmaxf(m8, e4m3_piece(v.f, sc8, q.q8 + ((long long)g * q.rows_per_group + row) * q.ld8 + ch0));
    }
  }
  if constexpr (sizeof(T) == 2) {
    if (q.q8) amax_commit(m8, q.q_next);      // (c == 32: every lane of the wave is here)
  }
}

// Norm + act TOGETHER WITH the MaxPool3d(2) that consumes the result (an encoder level of the U-Net: the activation goes to the
// skip connection and to the pool, src/model.py:22-28 via MONAI's Down): thread = (pooled voxel, 16-byte piece) walks the eight
// voxels of its window -- reads z, writes a, keeps the running maximum of the ROUNDED values (what maxpool_fwd_kernel would
// read back) and its window position.  Saves the pool launch's read of a (134 MB at 128^3 x 32), in both generator forwards
// of a training step.  blockIdx.y = sample.
template <typename T, bool DROP>
__global__ __launch_bounds__(256) void normact_pool_fwd_kernel(const NormActArgs q) {
  constexpr int EPV = Elem<T>::kPer16B;
  const int lpr = q.c / EPV, vpp = 256 / lpr;                     // pooled voxels per pass of the workgroup
  const int piece = threadIdx.x % lpr, vsub = threadIdx.x / lpr;
  if (vsub >= vpp) return;
  const int ch0 = piece * EPV;
  const int n_ = blockIdx.y;
  const long long dhw = (long long)q.pd * q.ph * q.pw;
  const int g = (int)(((long long)n_ * dhw) / q.rows_per_group);
  const unsigned long long seed = DROP ? eff_seed(q.seed, q.seed_ptr) : 0ull;
  float sc[EPV], sh[EPV];
#pragma unroll
  for (int j = 0; j < EPV; ++j) {
    const int ch = ch0 + j;
    const float ga = q.gamma ? (ch < q.n_affine ? q.gamma[ch] : 0.f) : 1.f, be = (q.beta && ch < q.n_affine) ? q.beta[ch] : 0.f;
    if (q.mean) {
      const float rs = q.rstd[(long long)g * q.c + ch], mu = q.mean[(long long)g * q.c + ch];
      sc[j] = ga * rs;
      sh[j] = be - mu * ga * rs;
    } else { sc[j] = ga; sh[j] = be; }
  }
  const int od_ = q.pd / 2, oh_ = q.ph / 2, ow_ = q.pw / 2;
  const int pooled = od_ * oh_ * ow_;
  const T* zb = reinterpret_cast<const T*>(q.z);
  T* ab = reinterpret_cast<T*>(q.a);
  const float slope = act_slope(q);
  for (int o = blockIdx.x * vpp + vsub; o < pooled; o += gridDim.x * vpp) {
    const int ow = o % ow_, t = o / ow_, oh = t % oh_, od = t / oh_;
    Vec16<T> m;
    unsigned long long where = 0;
    unsigned nan_seen = 0;
#pragma unroll
    for (int kd = 0; kd < 2; ++kd)
#pragma unroll
      for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int kw = 0; kw < 2; ++kw) {
          const long long vox = (((long long)n_ * q.pd + 2 * od + kd) * q.ph + 2 * oh + kh) * q.pw + 2 * ow + kw;
          const unsigned long long kk = (unsigned long long)(kd * 4 + kh * 2 + kw);
          Vec16<T> v;
#ifdef NORM_NT_FWD
          v.load_nt(zb + vox * q.ldz + ch0);
#else
          v.load(zb + vox * q.ldz + ch0);
#endif
          unsigned keep = 0;
          if constexpr (DROP) keep = drop_keep_mask<EPV>(seed, (unsigned long long)vox * q.c + ch0, q.thr16);
#pragma unroll
          for (int j = 0; j < EPV; ++j) {
            float t2 = v.f[j] * sc[j] + sh[j];
            if constexpr (DROP) t2 = (keep >> j) & 1u ? t2 * q.drop_scale : 0.f;
            t2 = t2 > 0.f ? t2 : t2 * slope;
            if constexpr (sizeof(T) == 2) t2 = bf16_bits_to_f32(f32_to_bf16_bits(t2));      // the stored value
            v.f[j] = t2;
          }
          v.store(ab + vox * q.lda + ch0);
          if (kk == 0) {
            m = v;
#pragma unroll
            for (int j = 0; j < EPV; ++j) nan_seen |= (v.f[j] != v.f[j] ? 1u : 0u) << j;
          } else {
#pragma unroll
            for (int j = 0; j < EPV; ++j) {                       // (as maxpool_fwd_kernel)
              const bool isnan_ = v.f[j] != v.f[j];
              const bool take = v.f[j] > m.f[j] || isnan_;
              m.f[j] = take ? v.f[j] : m.f[j];
              const bool mark = ((nan_seen >> j) & 1u) ? false : take;
              where = mark ? ((where & ~(0xffull << (8 * j))) | (kk << (8 * j))) : where;
              nan_seen |= (isnan_ ? 1u : 0u) << j;
            }
          }
        }
    const long long orow = (long long)n_ * pooled + o;
    m.store(reinterpret_cast<T*>(q.pool_y) + orow * q.ldpy + ch0);
    if constexpr (EPV == 8) *reinterpret_cast<unsigned long long*>(q.pool_widx + orow * q.c + ch0) = where;
    else *reinterpret_cast<unsigned*>(q.pool_widx + orow * q.c + ch0) = (unsigned)where;
  }
}

// Norm + act of a 32-channel bf16 tensor TOGETHER WITH the 1x1x1 convolution that consumes it (NormActArgs::fy: the U-Net's last block
// and its final convolution), the convolution on the MATRIX pipe.  Forms tried at 128^3 (plain kernel 57 us + the convolution launch it
// replaces 57 us): thread = 8 channels with v_dot2c_f32_bf16, weights in LDS, 16 cross-lane adds per row: 98 us; lane = 16 channels of a
// row + two v_mfma_f32_32x32x16_bf16 per 32 rows (96 registers + 16 accumulators: 4 waves per SIMD): 65 - 73 us.  This one keeps the plain
// kernel's work per thread: a wave owns 16 consecutive rows, lane (n, p) = row n, channel piece p (8 channels, one 16-byte load), and the
// rounded bf16 words it stores ARE the B operand of ONE v_mfma_f32_16x16x32_bf16 (k = 8 p + e; A = the weights, rows = outputs): lane
// (n, p) ends up with outputs 4 p .. 4 p + 3 of row n -- outputs 8..15 are the zero padding of the 16-channel output row, so every lane
// stores 8 bytes and the row is complete.
typedef float f32x4v __attribute__((ext_vector_type(4)));
template <bool DROP>
__global__ __launch_bounds__(256) void normact_fwd_final32_kernel(const NormActArgs q) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, p = lane >> 4;
  const int g = blockIdx.y, ch0 = 8 * p;
  const unsigned long long seed = DROP ? eff_seed(q.seed, q.seed_ptr) : 0ull;
  float sc[8], sh[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ch = ch0 + j;
    const float ga = q.gamma ? (ch < q.n_affine ? q.gamma[ch] : 0.f) : 1.f, be = (q.beta && ch < q.n_affine) ? q.beta[ch] : 0.f;
    if (q.mean) {
      const float rs = q.rstd[(long long)g * 32 + ch], mu = q.mean[(long long)g * 32 + ch];
      sc[j] = ga * rs;
      sh[j] = be - mu * ga * rs;
    } else { sc[j] = ga; sh[j] = be; }
  }
  // A fragment: row m = n (an output channel, < gk), k = 8 p + e (input channel)
  uint4 wf;
  {
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ch = ch0 + 2 * i;
      const float lo = (n < q.gk && ch < q.gw_ld) ? q.gw[(long long)n * q.gw_ld + ch] : 0.f;
      const float hi = (n < q.gk && ch + 1 < q.gw_ld) ? q.gw[(long long)n * q.gw_ld + ch + 1] : 0.f;
      w[i] = (unsigned)f32_to_bf16_bits(lo) | ((unsigned)f32_to_bf16_bits(hi) << 16);
    }
    wf = make_uint4(w[0], w[1], w[2], w[3]);
  }
  float fb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) fb[j] = (q.fbias && 4 * p + j < q.gk) ? q.fbias[4 * p + j] : 0.f;
  const bf16_t* zb = reinterpret_cast<const bf16_t*>(q.z) + (long long)g * q.rows_per_group * q.ldz;
  bf16_t* ab = reinterpret_cast<bf16_t*>(q.a) + (long long)g * q.rows_per_group * q.lda;
  bf16_t* yb = reinterpret_cast<bf16_t*>(q.fy) + (long long)g * q.rows_per_group * q.ldfy;
  const long long stride = (long long)gridDim.x * 64;
  const float slope = act_slope(q);
  // (the next block's piece is loaded before this block's is processed: load -> math -> MFMA -> store is one dependent chain per wave)
  const long long first = (long long)blockIdx.x * 64 + wave * 16;
  uint4 zn = make_uint4(0u, 0u, 0u, 0u);
  if (first < q.rows_per_group) {
    const long long rc = first + n < q.rows_per_group ? first + n : q.rows_per_group - 1;
    zn = *reinterpret_cast<const uint4*>(zb + rc * q.ldz + ch0);
  }
  for (long long row0 = first; row0 < q.rows_per_group; row0 += stride) {      // wave-uniform
    const long long row = row0 + n;
    const bool ok = row < q.rows_per_group;
    const long long rowc = ok ? row : q.rows_per_group - 1;
    const uint4 zc = zn;
    if (row0 + stride < q.rows_per_group) {
      const long long rc = row + stride < q.rows_per_group ? row + stride : q.rows_per_group - 1;
      zn = *reinterpret_cast<const uint4*>(zb + rc * q.ldz + ch0);
    }
    Vec16<bf16_t> v;
    v.from_bits(zc);
    unsigned keep = 0;
    if constexpr (DROP) keep = drop_keep_mask<8>(seed, ((unsigned long long)g * q.rows_per_group + rowc) * 32 + ch0, q.thr16);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float x = v.f[j] * sc[j] + sh[j];
      if constexpr (DROP) x = (keep >> j) & 1u ? x * q.drop_scale : 0.f;
      v.f[j] = x > 0.f ? x : x * slope;
    }
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (unsigned)f32_to_bf16_bits(v.f[2 * i]) | ((unsigned)f32_to_bf16_bits(v.f[2 * i + 1]) << 16);
    const uint4 aw = make_uint4(w[0], w[1], w[2], w[3]);
    if (ok && !q.skip_a) *reinterpret_cast<uint4*>(ab + row * q.lda + ch0) = aw;
    f32x4v acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf), __builtin_bit_cast(bf16x8, aw), acc, 0, 0, 0);
    if (ok && 4 * p < q.fcp) {
      // outputs 4 p .. 4 p + 3 of this lane's row (p >= 2: the padding channels, whose weight rows are zero)
      const uint2 yv = make_uint2((uint32_t)f32_to_bf16_bits(acc[0] + fb[0]) | ((uint32_t)f32_to_bf16_bits(acc[1] + fb[1]) << 16),
                                  (uint32_t)f32_to_bf16_bits(acc[2] + fb[2]) | ((uint32_t)f32_to_bf16_bits(acc[3] + fb[3]) << 16));
      *reinterpret_cast<uint2*>(yb + row * q.ldfy + 4 * p) = yv;
    }
  }
}

// implicit da (NormActArgs::gz): the 1x1x1 weights as bf16 PAIRS (k even | k odd), one uint4 per channel in LDS (512 B for 32
// channels: as registers -- 64 f32 or 32 packed -- they took the streaming kernels from 5 waves per SIMD to 3-4 and made them
// slower than reading the materialised gradient), and one row's EPV gradients by v_dot2c_f32_bf16 on the row's raw bf16 pairs.
// The weights are rounded to bf16 like the packed weights of the launch this replaces.
__device__ __forceinline__ void fill_implicit_w(const NormActArgs& q, uint4* wtab) {
  const int ch = threadIdx.x;
  if (ch < q.c && ch < kImplicitMaxC) {
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool okc = ch < q.gw_ld;
      const float lo = (okc && 2 * i < q.gk) ? q.gw[(long long)(2 * i) * q.gw_ld + ch] : 0.f;
      const float hi = (okc && 2 * i + 1 < q.gk) ? q.gw[(long long)(2 * i + 1) * q.gw_ld + ch] : 0.f;
      w[i] = (unsigned)f32_to_bf16_bits(lo) | ((unsigned)f32_to_bf16_bits(hi) << 16);
    }
    wtab[ch] = make_uint4(w[0], w[1], w[2], w[3]);
  }
  __syncthreads();
}
template <typename T, int EPV>
__device__ __forceinline__ void implicit_da(const NormActArgs& q, long long grow, const uint4* wtab, int ch0, Vec16<T>& dv) {
  if constexpr (sizeof(T) == 2) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const uint4 gv = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(q.gz) + grow * q.ldgz);   // channels 0..7 (gk <= 8)
    asm volatile("" : "+v"(ch0));      // opaque per row: otherwise the table reads are hoisted out of the row loop into 32 registers
#pragma unroll
    for (int j = 0; j < EPV; ++j) {
      const uint4 wv = wtab[ch0 + j];
      float t = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, gv.x), __builtin_bit_cast(bf16x2, wv.x), 0.f, false);
      t = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, gv.y), __builtin_bit_cast(bf16x2, wv.y), t, false);
      t = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, gv.z), __builtin_bit_cast(bf16x2, wv.z), t, false);
      t = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, gv.w), __builtin_bit_cast(bf16x2, wv.w), t, false);
      dv.f[j] = bf16_bits_to_f32(f32_to_bf16_bits(t));                   // what a stored bf16 gradient would hold
    }
  }
}
// implicit da (NormActArgs::pool_idx): the gradient MaxPool3d(2)'s backward would have written for global row `grow` (voxel
// (n, d, h, w) of the full-resolution grid): the pooled gradient where this voxel was its window's (first) maximum -- the window
// position recorded by maxpool_fwd_kernel -- plus the skip connection's gradient, rounded to T as maxpool_bwd_kernel stores it.
template <typename T, int EPV>
__device__ __forceinline__ void pooled_da(const NormActArgs& q, long long grow, int ch0, Vec16<T>& dv) {
  const unsigned v = (unsigned)grow, W = (unsigned)q.pw, H = (unsigned)q.ph, D = (unsigned)q.pd;
  const unsigned w_ = v % W, t1 = v / W, h_ = t1 % H, t2 = t1 / H, d_ = t2 % D, n_ = t2 / D;
  const long long o = (((long long)n_ * (D >> 1) + (d_ >> 1)) * (H >> 1) + (h_ >> 1)) * (W >> 1) + (w_ >> 1);
  const unsigned k = ((d_ & 1u) << 2) | ((h_ & 1u) << 1) | (w_ & 1u);
  Vec16<T> gy;
  gy.load(reinterpret_cast<const T*>(q.pool_dy) + o * q.ldpdy + ch0);
  unsigned long long ib;
  if constexpr (EPV == 8) ib = *reinterpret_cast<const unsigned long long*>(q.pool_idx + o * q.c + ch0);
  else ib = *reinterpret_cast<const unsigned*>(q.pool_idx + o * q.c + ch0);
  if (q.da) dv.load(reinterpret_cast<const T*>(q.da) + grow * q.ldda + ch0);
#pragma unroll
  for (int j = 0; j < EPV; ++j) {
    float t = ((unsigned)(ib >> (8 * j)) & 0xffu) == k ? gy.f[j] : 0.f;
    if (q.da) t += dv.f[j];
    if constexpr (sizeof(T) == 2) t = bf16_bits_to_f32(f32_to_bf16_bits(t));
    dv.f[j] = t;
  }
}
// IMPL: 0 = da is a tensor, 1 = implicit 1x1x1 data gradient (gz), 2 = implicit max-pool backward (pool_idx)
// PRELU: a third sum per channel, the slope gradient's share, into q.dalpha_part[group * blocks + block][c]
template <typename T, bool DROP, int IMPL = 0, bool PRELU = false>
__global__ __launch_bounds__(256) void normact_bwd_reduce_kernel(const NormActArgs q) {
  constexpr int EPV = Elem<T>::kPer16B;
  const int g = blockIdx.y, b = blockIdx.x;
  const long long rb = (q.rows_per_group + q.blocks_per_group - 1) / q.blocks_per_group;
  const long long r0 = (long long)b * rb;
  long long r1 = r0 + rb;
  if (r1 > q.rows_per_group) r1 = q.rows_per_group;
  const T* zb = reinterpret_cast<const T*>(q.z) + (long long)g * q.rows_per_group * q.ldz;
  const T* db = reinterpret_cast<const T*>(q.da) + (long long)g * q.rows_per_group * q.ldda;
  float* out = q.part + ((long long)g * q.blocks_per_group + b) * 2 * q.c;
  BwdConst<EPV> k;
  load_bwd_const<EPV>(q, g, (int)(threadIdx.x % (q.c / EPV)) * EPV, k);
  const unsigned long long seed = DROP ? eff_seed(q.seed, q.seed_ptr) : 0ull;
  __shared__ uint4 wtab[IMPL == 1 ? kImplicitMaxC : 1];
  if constexpr (IMPL == 1) fill_implicit_w(q, wtab);
  const float slope = act_slope(q);
  float* aout = PRELU ? reinterpret_cast<float*>(q.dalpha_part) + ((long long)g * q.blocks_per_group + b) * q.c : nullptr;
  block_channel_sums<T, PRELU>(q.c, r0, r1,
      [&](long long row, int ch0, float* s0, float* s1, float* s2 = nullptr) {
        Vec16<T> zv, dv;
        zv.load(zb + row * q.ldz + ch0);
        if constexpr (IMPL == 1) implicit_da<T, EPV>(q, (long long)g * q.rows_per_group + row, wtab, ch0, dv);
        else if constexpr (IMPL == 2) pooled_da<T, EPV>(q, (long long)g * q.rows_per_group + row, ch0, dv);
        else if (q.s2d_da.d) dv.load(reinterpret_cast<const T*>(q.da) + s2d_offset(q.s2d_da, (long long)g * q.rows_per_group + row, q.ldda) + ch0);
        else dv.load(db + row * q.ldda + ch0);
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
      },
      out, out + q.c, aout);
}

// block_sum_parts for ONE quantity per partial, part[k][c] (the slope-gradient partials): same lanes, same order, f64
__device__ __forceinline__ double block_sum_parts1(const float* __restrict__ part, int nparts, int c, int ch0) {
  __shared__ double red[16][8];
  const int cl = threadIdx.x & 7, pl = threadIdx.x >> 3;
  const int ch = ch0 + cl;
  double s = 0.0;
  if (ch < c)
    for (int k = pl; k < nparts; k += 128) s += (double)part[(long long)k * c + ch];
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) < 8) red[wave][cl] = s;
  __syncthreads();
  double a = 0.0;
#pragma unroll
  for (int w = 0; w < 16; ++w) a += red[w][cl];
  __syncthreads();
  return a;
}

// PRELU: also alpha_ch[ch] = this channel's slope-gradient total over all groups (slope_grad_sum_kernel adds the channels)
template <bool PRELU>
__global__ __launch_bounds__(1024) void normact_bwd_finalize_kernel(const float* __restrict__ part, int bpg,
                                                                    int groups, int c, float* __restrict__ sums,
                                                                    float* dgamma, float* dbeta, int n_affine, int accumulate,
                                                                    const float* __restrict__ apart, double* __restrict__ alpha_ch) {
  const int ch0 = blockIdx.x * 8;
  const int ch = ch0 + (int)threadIdx.x;
  const bool owner = threadIdx.x < 8 && ch < c;
  double tg = 0.0, tb = 0.0, ta = 0.0;
  for (int g = 0; g < groups; ++g) {
    double s0, s1;
    block_sum_parts(part + (long long)g * bpg * 2 * c, bpg, c, ch0, s0, s1);
    if (owner) {
      sums[((long long)g * 2 + 0) * c + ch] = (float)s0;
      sums[((long long)g * 2 + 1) * c + ch] = (float)s1;
      tb += s0;
      tg += s1;
    }
    if constexpr (PRELU) ta += block_sum_parts1(apart + (long long)g * bpg * c, bpg, c, ch0);
  }
  if constexpr (PRELU) {
    if (owner) alpha_ch[ch] = ch < n_affine ? ta : 0.0;      // (padded channels: u = 0, but their da is whatever the producer left)
  }
  if (owner && ch < n_affine) {
    if (dgamma) dgamma[ch] = accumulate ? dgamma[ch] + (float)tg : (float)tg;
    if (dbeta) dbeta[ch] = accumulate ? dbeta[ch] + (float)tb : (float)tb;
  }
}

template <typename T, bool DROP, int IMPL = 0>
__global__ __launch_bounds__(256, IMPL == 1 ? 5 : 1) void normact_bwd_apply_kernel(const NormActArgs q) {   // (IMPL 1: 97 registers without the bound: 4 waves)
  constexpr int EPV = Elem<T>::kPer16B;
  __shared__ uint4 wtab[IMPL == 1 ? kImplicitMaxC : 1];
  if constexpr (IMPL == 1) fill_implicit_w(q, wtab);     // (before the early return below: it ends with a barrier)
  const int g = blockIdx.y;
  const int lpr = q.c / EPV, rpp = 256 / lpr;
  const int piece = threadIdx.x % lpr, rsub = threadIdx.x / lpr;
  if (rsub >= rpp) return;
  const int ch0 = piece * EPV;
  const float inv = 1.f / (float)q.rows_per_group;
  BwdConst<EPV> k;
  load_bwd_const<EPV>(q, g, ch0, k);
  const unsigned long long seed = DROP ? eff_seed(q.seed, q.seed_ptr) : 0ull;
  float kk[EPV], m0[EPV], m1[EPV];
#pragma unroll
  for (int j = 0; j < EPV; ++j) {
    const int ch = ch0 + j;
    kk[j] = k.ga[j] * k.rs[j];
    const bool sub = q.mean && q.batch_stats;
    m0[j] = sub ? q.sums[((long long)g * 2 + 0) * q.c + ch] * inv : 0.f;
    m1[j] = sub ? q.sums[((long long)g * 2 + 1) * q.c + ch] * inv : 0.f;
  }
  const T* zb = reinterpret_cast<const T*>(q.z) + (long long)g * q.rows_per_group * q.ldz;
  const T* db = reinterpret_cast<const T*>(q.da) + (long long)g * q.rows_per_group * q.ldda;
  T* ob = reinterpret_cast<T*>(q.dz) + (long long)g * q.rows_per_group * q.lddz;
  const long long stride = (long long)gridDim.x * rpp;
  const float sc8 = q.q8 ? fp8_scale_of(q.q_use) : 1.f;
  const float slope = act_slope(q);
  float m8 = 0.f;
  for (long long row = (long long)blockIdx.x * rpp + rsub; row < q.rows_per_group; row += stride) {
    Vec16<T> zv, dv;
#ifdef NORM_NT_APPLY
    zv.load_nt(zb + row * q.ldz + ch0);
#else
    zv.load(zb + row * q.ldz + ch0);
#endif
    if constexpr (IMPL == 1) implicit_da<T, EPV>(q, (long long)g * q.rows_per_group + row, wtab, ch0, dv);
    else if constexpr (IMPL == 2) pooled_da<T, EPV>(q, (long long)g * q.rows_per_group + row, ch0, dv);
    else if (q.s2d_da.d) dv.load(reinterpret_cast<const T*>(q.da) + s2d_offset(q.s2d_da, (long long)g * q.rows_per_group + row, q.ldda) + ch0);
#ifdef NORM_NT_APPLY
    else dv.load_nt(db + row * q.ldda + ch0);
#else
    else dv.load(db + row * q.ldda + ch0);
#endif
    unsigned keep = 0;
    if constexpr (DROP) keep = drop_keep_mask<EPV>(seed, ((unsigned long long)g * q.rows_per_group + row) * q.c + ch0, q.thr16);
#pragma unroll
    for (int j = 0; j < EPV; ++j) {
      float gv, xh;
      bwd_elem<DROP>(q, slope, (keep >> j) & 1u, k.mu[j], k.rs[j], k.ga[j], k.be[j], zv.f[j], dv.f[j], gv, xh);
      zv.f[j] = kk[j] * (gv - m0[j] - xh * m1[j]);
    }
    zv.store(ob + row * q.lddz + ch0);
    if constexpr (sizeof(T) == 2) {
      if (q.q8) m8 = fmaxf(m8, e4m3_piece(zv.f, sc8, q.q8 + ((long long)g * q.rows_per_group + row) * q.ld8 + ch0));
    }
  }
  if constexpr (sizeof(T) == 2) {
    if (q.q8) amax_commit(m8, q.q_next);
  }
}

}  // namespace

extern "C" {

int32_t mi355_channel_stats_blocks(int64_t rows_per_group) {
  // >= 128 rows per block, ~1024 blocks for the big tensors (2048 rows each at 128^3)
  long long b = rows_per_group / 128;
  if (b > 1024) b = (rows_per_group + kRowsPerStatBlock - 1) / kRowsPerStatBlock;
  if (b < 1024 && rows_per_group / 128 > 1024) b = 1024;
  // small tensors (16^3: 4 096 rows) got 32 workgroups -- 17 us for a 2 MB reduction in the replay trace: at least
  // min(256, rows / 16) of them
  const long long fine = rows_per_group / 16 < 256 ? rows_per_group / 16 : 256;
  if (b < fine) b = fine;
  if (b < 1) b = 1;
  if (b > 2048) b = 2048;
  return (int32_t)b;
}

int mi355_channel_stats(const void* x, int32_t ld, int32_t c, int64_t rows_per_group, int32_t groups, float* part,
                        int32_t blocks_per_group, int32_t dtype, void* stream) {
  MI355_REQUIRE(x && part && rows_per_group > 0 && groups > 0 && blocks_per_group > 0, "channel_stats: bad argument");
  int rc = check_rows(c, ld, dtype, "channel_stats");
  if (rc) return rc;
  dim3 grid(blocks_per_group, groups);
  for_dtype(dtype, [&](auto t) { channel_stats_kernel<decltype(t)><<<grid, dim3(256), 0, (hipStream_t)stream>>>((const decltype(t)*)x, ld, c, (long long)rows_per_group, part, blocks_per_group); });
  return mi355_check_launch("channel_stats");
}

int mi355_norm_finalize(const float* part, int32_t parts_per_group, int32_t groups, int32_t c, int64_t count_per_group,
                        const float* shift, int32_t n_real, float eps, float* mean, float* rstd, float* running_mean,
                        float* running_var, float momentum, int64_t* batches_tracked, void* stream) {
  MI355_REQUIRE(part && mean && rstd && parts_per_group > 0 && groups > 0 && c > 0 && count_per_group > 0, "norm_finalize: bad argument");
  MI355_REQUIRE(!running_mean || running_var, "norm_finalize: running_mean without running_var");
  const bool serial = running_mean && groups > 1;         // running statistics: the groups' momentum updates in order
  hipLaunchKernelGGL(norm_finalize_kernel, dim3((c + 7) / 8, serial ? 1 : groups), dim3(1024), 0, (hipStream_t)stream, part,
                     parts_per_group, c, (long long)count_per_group, shift, n_real > 0 ? n_real : c, eps, mean, rstd, running_mean, running_var, momentum,
                     (long long*)batches_tracked, serial ? groups : 1);
  return mi355_check_launch("norm_finalize");
}

int mi355_colsum_finalize(const float* part, int32_t parts, int32_t c, float* out, void* stream) {
  return mi355_colsum_finalize_into(part, parts, c, out, c, 0, stream);
}

int mi355_colsum_finalize_into(const float* part, int32_t parts, int32_t c, float* out, int32_t n_out, int32_t accumulate,
                               void* stream) {
  return mi355_colsum_finalize_from(part, parts, c, 0, out, n_out, accumulate, stream);
}

int mi355_colsum_finalize_from(const float* part, int32_t parts, int32_t c, int32_t offset, float* out, int32_t n_out,
                               int32_t accumulate, void* stream) {
  MI355_REQUIRE(part && out && parts > 0 && c > 0 && n_out > 0 && offset >= 0 && offset + n_out <= c, "colsum_finalize: bad argument");
  hipLaunchKernelGGL(colsum_finalize_kernel, dim3((n_out + 7) / 8), dim3(1024), 0, (hipStream_t)stream, part, parts, c, offset, out, n_out,
                     accumulate);
  return mi355_check_launch("colsum_finalize");
}

static unsigned stream_blocks(long long rows, int c, int dtype) {
  const int epv = dtype == MI355_DT_F32 ? 4 : 8;
  const int rpp = 256 / (c / epv);
  long long b = (rows + (long long)rpp * 8 - 1) / ((long long)rpp * 8);
  if (b < 1) b = 1;
  // 4 workgroups per CU, each streaming a long row range: measured against 256 ... 16384 in the full step
  // (interleaved A/B): 1024 and 768 best, 4096 +0.12 ms, 256 +0.75 ms
  if (b > 1024) b = 1024;
  return (unsigned)b;
}

int mi355_normact_fwd(const mi355_normact_desc* d, void* stream) {
  NormActArgs q;
  int rc = fill_normact(d, &q, "normact_fwd");
  if (rc) return rc;
  MI355_REQUIRE((d->a && d->lda >= d->c) || d->skip_a, "normact_fwd: bad output");
  dim3 grid(stream_blocks(d->rows_per_group, d->c, d->dtype), d->groups);
  if (q.pool_y) {
    const long long dhw = (long long)d->sd * d->sh * d->sw, samples = (long long)d->rows_per_group * d->groups / dhw;
    const int epv = d->dtype == MI355_DT_F32 ? 4 : 8, vpp = 256 / (d->c / epv);
    long long b = (dhw / 8 + vpp - 1) / vpp;                      // one window per thread and pass; up to ~2048 workgroups in all
    const long long cap = std::max(1ll, 2048 / samples);
    if (b > cap) b = cap;
    const dim3 gridp((unsigned)b, (unsigned)samples);
    for_dtype_drop(d->dtype, q.thr16, [&](auto t, auto drop) { normact_pool_fwd_kernel<decltype(t), drop><<<gridp, dim3(256), 0, (hipStream_t)stream>>>(q); });
    return mi355_check_launch("normact_pool_fwd");
  }
  if (q.fy) {
    // (bf16 only: fill_normact.  The convolution on the matrix pipe; 64 rows per workgroup and pass)
    MI355_REQUIRE(d->fcp == 16, "normact_fwd: the fused convolution writes 16-channel rows");
    long long b = (d->rows_per_group + 64 * 8 - 1) / (64 * 8);
    const dim3 grid32((unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b)), d->groups);
    if (q.thr16) normact_fwd_final32_kernel<true><<<grid32, dim3(256), 0, (hipStream_t)stream>>>(q);
    else normact_fwd_final32_kernel<false><<<grid32, dim3(256), 0, (hipStream_t)stream>>>(q);
  } else {
    for_dtype_drop(d->dtype, q.thr16, [&](auto t, auto drop) { normact_fwd_kernel<decltype(t), drop><<<grid, dim3(256), 0, (hipStream_t)stream>>>(q); });
  }
  return mi355_check_launch("normact_fwd");
}

int mi355_normact_bwd_reduce(const mi355_normact_desc* d, void* stream) {
  NormActArgs q;
  int rc = fill_normact(d, &q, "normact_bwd_reduce");
  if (rc) return rc;
  MI355_REQUIRE((d->gz || d->pool_idx || (d->da && d->ldda >= d->c)) && d->part && d->blocks_per_group > 0, "normact_bwd_reduce: bad argument");
  dim3 grid(d->blocks_per_group, d->groups);
  if (d->dalpha) {            // PReLU with a slope gradient to form: the same launch, a third sum per channel
    if (q.gz) {
      if (q.thr16) normact_bwd_reduce_kernel<bf16_t, true, 1, true><<<grid, dim3(256), 0, (hipStream_t)stream>>>(q);
      else normact_bwd_reduce_kernel<bf16_t, false, 1, true><<<grid, dim3(256), 0, (hipStream_t)stream>>>(q);
    } else {
      for_dtype_drop(d->dtype, q.thr16, [&](auto t, auto drop) {
        if (q.pool_idx) normact_bwd_reduce_kernel<decltype(t), drop, 2, true><<<grid, dim3(256), 0, (hipStream_t)stream>>>(q);
        else normact_bwd_reduce_kernel<decltype(t), drop, 0, true><<<grid, dim3(256), 0, (hipStream_t)stream>>>(q);
      });
    }
  } else if (q.gz) {          // (bf16 only, and never together with pool_idx: fill_normact)
    if (q.thr16) normact_bwd_reduce_kernel<bf16_t, true, 1><<<grid, dim3(256), 0, (hipStream_t)stream>>>(q);
    else normact_bwd_reduce_kernel<bf16_t, false, 1><<<grid, dim3(256), 0, (hipStream_t)stream>>>(q);
  } else {
    for_dtype_drop(d->dtype, q.thr16, [&](auto t, auto drop) {
      if (q.pool_idx) normact_bwd_reduce_kernel<decltype(t), drop, 2><<<grid, dim3(256), 0, (hipStream_t)stream>>>(q);
      else normact_bwd_reduce_kernel<decltype(t), drop, 0><<<grid, dim3(256), 0, (hipStream_t)stream>>>(q);
    });
  }
  return mi355_check_launch("normact_bwd_reduce");
}

int mi355_normact_bwd_finalize(const float* part, int32_t blocks_per_group, int32_t groups, int32_t c, float* sums,
                               float* dgamma, float* dbeta, void* stream) {
  return mi355_normact_bwd_finalize_into(part, blocks_per_group, groups, c, sums, dgamma, dbeta, c, 0, stream);
}

int mi355_normact_bwd_finalize_into(const float* part, int32_t blocks_per_group, int32_t groups, int32_t c, float* sums,
                                    float* dgamma, float* dbeta, int32_t n_affine, int32_t accumulate, void* stream) {
  MI355_REQUIRE(part && sums && blocks_per_group > 0 && groups > 0 && c > 0 && n_affine > 0 && n_affine <= c,
                "normact_bwd_finalize: bad argument");
  hipLaunchKernelGGL(normact_bwd_finalize_kernel<false>, dim3((c + 7) / 8), dim3(1024), 0, (hipStream_t)stream, part,
                     blocks_per_group, groups, c, sums, dgamma, dbeta, n_affine, accumulate, (const float*)nullptr, (double*)nullptr);
  return mi355_check_launch("normact_bwd_finalize");
}

int mi355_normact_bwd_finalize_prelu(const float* part, const float* apart, int32_t blocks_per_group, int32_t groups, int32_t c,
                                     float* sums, float* dgamma, float* dbeta, int32_t n_affine, int32_t accumulate,
                                     double* alpha_ch, float* dalpha, void* stream) {
  MI355_REQUIRE(part && apart && sums && alpha_ch && dalpha && blocks_per_group > 0 && groups > 0 && c > 0 && n_affine > 0 &&
                n_affine <= c, "normact_bwd_finalize_prelu: bad argument");
  hipLaunchKernelGGL(normact_bwd_finalize_kernel<true>, dim3((c + 7) / 8), dim3(1024), 0, (hipStream_t)stream, part,
                     blocks_per_group, groups, c, sums, dgamma, dbeta, n_affine, accumulate, apart, alpha_ch);
  hipLaunchKernelGGL(slope_grad_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)alpha_ch, c, dalpha, accumulate);
  return mi355_check_launch("normact_bwd_finalize_prelu");
}

int mi355_normact_bwd_apply(const mi355_normact_desc* d, void* stream) {
  NormActArgs q;
  int rc = fill_normact(d, &q, "normact_bwd_apply");
  if (rc) return rc;
  MI355_REQUIRE((d->gz || d->pool_idx || (d->da && d->ldda >= d->c)) && d->dz && d->lddz >= d->c, "normact_bwd_apply: bad argument");
  MI355_REQUIRE(!(d->mean && d->batch_stats) || d->sums, "normact_bwd_apply: sums required");
  dim3 grid(stream_blocks(d->rows_per_group, d->c, d->dtype), d->groups);
  if (q.gz) {                 // (bf16 only, and never together with pool_idx: fill_normact)
    if (q.thr16) normact_bwd_apply_kernel<bf16_t, true, 1><<<grid, dim3(256), 0, (hipStream_t)stream>>>(q);
    else normact_bwd_apply_kernel<bf16_t, false, 1><<<grid, dim3(256), 0, (hipStream_t)stream>>>(q);
  } else {
    for_dtype_drop(d->dtype, q.thr16, [&](auto t, auto drop) {
      if (q.pool_idx) normact_bwd_apply_kernel<decltype(t), drop, 2><<<grid, dim3(256), 0, (hipStream_t)stream>>>(q);
      else normact_bwd_apply_kernel<decltype(t), drop, 0><<<grid, dim3(256), 0, (hipStream_t)stream>>>(q);
    });
  }
  return mi355_check_launch("normact_bwd_apply");
}

}  // extern "C"
