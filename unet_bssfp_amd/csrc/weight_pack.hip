// Weight packing: f32 parameters -> the [chunk][tap][co][16] operand order of the convolution kernels (f32 / bf16 / e4m3), one
// tensor per launch (gather) or a list per launch (gather, dense 3x3x3 and space-to-depth k4 through LDS transposes).
#include "common.h"

namespace {

// ------------------------------------------------------------------ weight pack
struct WpackArgs {
  const float* src; void* dst;
  int cout, cin, coutp, cinp, ks;
  long long s_co, s_ci, s_k0, s_k1, s_k2;
  int tb0, tb1, tb2, ts0, ts1, ts2;
  int s2d_mode, s2d_cp;   // 1: the GEMM cin index is (block, channel) of a space-to-depth tensor; 2: the cout index is
  const float* q_amax;    // fp8 packings: per-tensor max |w| (device), values are stored as w * 224 / amax
};
template <typename T>
__global__ __launch_bounds__(256) void wpack_kernel(const WpackArgs a) {
  const int ntaps = a.ks * a.ks * a.ks;
  const long long total = (long long)(a.cinp / 16) * ntaps * a.coutp * 16;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int e = (int)(idx % 16);
  const int co = (int)((idx / 16) % a.coutp);
  const int tap = (int)((idx / (16ll * a.coutp)) % ntaps);
  const int chunk = (int)(idx / (16ll * a.coutp * ntaps));
  int ci = chunk * 16 + e;
  int cor = co, blk = 0;
  if (a.s2d_mode == 1) { blk = ci / a.s2d_cp; ci = ci % a.s2d_cp; }
  if (a.s2d_mode == 2) { blk = cor / a.s2d_cp; cor = cor % a.s2d_cp; }
  float v = 0.f;
  if (cor < a.cout && ci < a.cin && blk < 8) {
    const int td = tap / (a.ks * a.ks), th = (tap / a.ks) % a.ks, tw = tap % a.ks;
    v = a.src[cor * a.s_co + ci * a.s_ci + (a.tb0 + a.ts0 * td + (blk >> 2)) * a.s_k0 +
              (a.tb1 + a.ts1 * th + ((blk >> 1) & 1)) * a.s_k1 + (a.tb2 + a.ts2 * tw + (blk & 1)) * a.s_k2];
  }
  if constexpr (sizeof(T) == 1) v *= fp8_scale_of(a.q_amax);
  Elem<T>::store(reinterpret_cast<T*>(a.dst) + idx, v);
}

constexpr int kWpackChunk = 16;
struct WpackMulti { WpackArgs a[kWpackChunk]; };
template <typename T>
__global__ __launch_bounds__(256) void wpack_multi_kernel(const WpackMulti m) {
  const WpackArgs& a = m.a[blockIdx.y];
  const int ntaps = a.ks * a.ks * a.ks;
  const long long total = (long long)(a.cinp / 16) * ntaps * a.coutp * 16;
  const long long stride = (long long)gridDim.x * 256;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) {
    const int e = (int)(idx % 16);
    const int co = (int)((idx / 16) % a.coutp);
    const int tap = (int)((idx / (16ll * a.coutp)) % ntaps);
    const int chunk = (int)(idx / (16ll * a.coutp * ntaps));
    int ci = chunk * 16 + e;
    int cor = co, blk = 0;
    if (a.s2d_mode == 1) { blk = ci / a.s2d_cp; ci = ci % a.s2d_cp; }
    if (a.s2d_mode == 2) { blk = cor / a.s2d_cp; cor = cor % a.s2d_cp; }
    float v = 0.f;
    if (cor < a.cout && ci < a.cin && blk < 8) {
      const int td = tap / (a.ks * a.ks), th = (tap / a.ks) % a.ks, tw = tap % a.ks;
      v = a.src[cor * a.s_co + ci * a.s_ci + (a.tb0 + a.ts0 * td + (blk >> 2)) * a.s_k0 +
                (a.tb1 + a.ts1 * th + ((blk >> 1) & 1)) * a.s_k1 + (a.tb2 + a.ts2 * tw + (blk & 1)) * a.s_k2];
    }
    if constexpr (sizeof(T) == 1) v *= fp8_scale_of(a.q_amax);
    Elem<T>::store(reinterpret_cast<T*>(a.dst) + idx, v);
  }
}

// Dense 3x3x3 weights W[R][C][27] (forward: R = cout, C = cin; data gradient: roles swapped, taps flipped): the
// kernels above gather 4-byte elements 27 floats (or C*27 floats) apart -- 16x read amplification on 34 M
// parameters after every optimiser step.  Here a block loads a 16 (R) x 16 (C) x 27 patch as 16 contiguous runs of
// 432 floats, keeps it in LDS and writes the packed [chunk][tap][co][16] order 512 contiguous bytes per tap.
template <typename T>
__global__ __launch_bounds__(256) void wpack_dense3_multi_kernel(const WpackMulti m) {
  const WpackArgs& a = m.a[blockIdx.y];
  constexpr int NT = 27, ROW = 16 * NT + 1;
  __shared__ float tile[16 * ROW];
  const int nchunk = a.cinp / 16, ncob = a.coutp / 16;
  if ((int)blockIdx.x >= nchunk * ncob) return;
  const int chunk = blockIdx.x / ncob, cob = blockIdx.x % ncob;
  const bool co_is_row = a.s_co > a.s_ci;                       // forward packing
  const int r0 = (co_is_row ? cob : chunk) * 16, c0 = (co_is_row ? chunk : cob) * 16;
  const int nr = co_is_row ? a.cout : a.cin, nc = co_is_row ? a.cin : a.cout;      // extents of W's two channel axes
  const long long rstride = co_is_row ? a.s_co : a.s_ci;
  const int cvalid = min(16, nc - c0);                          // may be <= 0: the patch is padding only
  for (int rl = 0; rl < 16; ++rl) {
    const float* src = a.src + (long long)(r0 + rl) * rstride + (long long)c0 * NT;
    const bool rok = r0 + rl < nr;
    for (int j = threadIdx.x; j < 16 * NT; j += 256) tile[rl * ROW + j] = (rok && j < cvalid * NT) ? src[j] : 0.f;
  }
  __syncthreads();
  // 16-byte stores: a thread packs EPT consecutive channels of one (tap, output channel) row of the chunk (2-byte stores, one
  // element per thread, left the launch at a third of the HBM rate: 120 us per generator update)
  constexpr int EPT = 16 / (int)sizeof(T), PPR = 16 / EPT;      // elements per 16-byte piece, pieces per 16-channel row
  const float qs = sizeof(T) == 1 ? fp8_scale_of(a.q_amax) : 1.f;
  T* dst0 = reinterpret_cast<T*>(a.dst) + ((long long)chunk * NT * a.coutp + (long long)cob * 16) * 16;
  for (int idx = threadIdx.x; idx < NT * 16 * PPR; idx += 256) {
    const int tap = idx / (16 * PPR), within = idx - tap * (16 * PPR);
    const int col = within / PPR, e0 = (within - col * PPR) * EPT;
    const int td = tap / 9, th = (tap / 3) % 3, tw = tap % 3;
    const int ts = (a.tb0 + a.ts0 * td) * 9 + (a.tb1 + a.ts1 * th) * 3 + (a.tb2 + a.ts2 * tw);
    alignas(16) T out[EPT];
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
      const int e = e0 + j;
      const int rl = co_is_row ? col : e, cl = co_is_row ? e : col;
      Elem<T>::store(out + j, tile[rl * ROW + cl * NT + ts] * qs);
    }
    *reinterpret_cast<uint4*>(dst0 + (long long)tap * a.coutp * 16 + col * 16 + e0) = *reinterpret_cast<const uint4*>(out);
  }
}

// The PatchGAN k4 s2 weights W[co][c][4][4][4] packed for the space-to-depth formulation (8 dense taps j x 8 parity
// blocks blk; s2d_mode 1: the GEMM input-channel index is blk * cp + c (forward), 2: the GEMM output-channel index is
// (data gradient)).  For one (co, c) the 64 (j, blk) values are the contiguous 4x4x4 taps, so a block loads a
// [rows][cols][64] patch as contiguous runs and writes every (j, blk) slice as 128 contiguous packed elements
// (the gather kernel reads 4 bytes per 256-byte stride: 150 us per step for 11 M discriminator weights).
template <typename T>
__global__ __launch_bounds__(256) void wpack_s2d_multi_kernel(const WpackMulti m) {
  const WpackArgs& a = m.a[blockIdx.y];
  __shared__ float tile[128 * 65];
  const bool fwd = a.s2d_mode == 1;
  const int R = fwd ? 8 : 16, Ccols = fwd ? 16 : 8;                 // rows = W's first axis, cols = channels c
  const int nrb = (fwd ? a.coutp : a.cinp) / R, ncb = a.s2d_cp / Ccols;
  if ((int)blockIdx.x >= nrb * ncb) return;
  const int rb = blockIdx.x / ncb, cb = blockIdx.x % ncb;
  const int r0 = rb * R, c0 = cb * Ccols;
  const int nrow = fwd ? a.cout : a.cin, ncol = fwd ? a.cin : a.cout;   // real extents of W's two channel axes
  const long long rstride = fwd ? a.s_co : a.s_ci;                      // 64 * (channels of the second axis)
  for (int i = threadIdx.x; i < R * Ccols * 64; i += 256) {
    const int rl = i / (Ccols * 64), rest = i - rl * (Ccols * 64);      // rest = cl * 64 + tap: contiguous in W
    const int cl = rest >> 6;
    const bool ok = r0 + rl < nrow && c0 + cl < ncol;
    tile[(rl * Ccols + cl) * 65 + (rest & 63)] = ok ? a.src[(long long)(r0 + rl) * rstride + (long long)c0 * 64 + rest] : 0.f;
  }
  __syncthreads();
  // 64 (j, blk) slices of 128 packed elements each; 256 threads write two slices per pass
  const int half = threadIdx.x >> 7, q = threadIdx.x & 127;
  const int x8 = q >> 4, e = q & 15;                                   // fwd: (co_l, e = c_l); dgrad: (c_l, e = row_l)
  const int rl = fwd ? x8 : e, cl = fwd ? e : x8;
  for (int sidx = half; sidx < 64; sidx += 2) {
    const int j = sidx >> 3, blk = sidx & 7;
    const int jd = j >> 2, jh = (j >> 1) & 1, jw = j & 1;
    const int tap = (a.tb0 + a.ts0 * jd + (blk >> 2)) * 16 + (a.tb1 + a.ts1 * jh + ((blk >> 1) & 1)) * 4 + (a.tb2 + a.ts2 * jw + (blk & 1));
    const float v = tile[(rl * Ccols + cl) * 65 + tap];
    long long dst;
    if (fwd) {   // dest [chunk = (blk*cp + c0)/16][j][co][e]
      const int chunk = (blk * a.s2d_cp + c0) >> 4;
      dst = (((long long)chunk * 8 + j) * a.coutp + r0 + x8) * 16 + e;
    } else {     // dest [chunk = r0/16][j][co' = blk*cp + c0 + c_l][e]
      dst = (((long long)(r0 >> 4) * 8 + j) * a.coutp + (long long)blk * a.s2d_cp + c0 + x8) * 16 + e;
    }
    Elem<T>::store(reinterpret_cast<T*>(a.dst) + dst, v);
  }
}

static bool wpack_is_s2d_dense(const mi355_wpack_desc* d) {
  if (d->ks != 2 || (d->s2d_mode != 1 && d->s2d_mode != 2) || d->s2d_cp % 16 || d->s_k[2] != 1 || d->s_k[1] != 4 || d->s_k[0] != 16) return false;
  for (int k = 0; k < 3; ++k) {
    const int lo = d->tbase[k] < d->tbase[k] + d->tstep[k] ? d->tbase[k] : d->tbase[k] + d->tstep[k];
    const int hi = d->tbase[k] + d->tstep[k] + 1 > d->tbase[k] + 1 ? d->tbase[k] + d->tstep[k] + 1 : d->tbase[k] + 1;
    if (lo < 0 || hi > 3) return false;                              // taps tb + ts*j + b, j and b in {0, 1}, stay in 0..3
  }
  if (d->s2d_mode == 1) return d->s_ci == 64 && d->s_co == 64ll * d->cin && d->cinp == 8 * d->s2d_cp && d->coutp % 8 == 0 && d->cin <= d->s2d_cp;
  return d->s_co == 64 && d->s_ci == 64ll * d->cout && d->coutp == 8 * d->s2d_cp && d->cinp % 16 == 0 && d->cout <= d->s2d_cp;
}

static bool wpack_is_dense3(const mi355_wpack_desc* d) {
  if (d->ks != 3 || d->s2d_mode != 0 || d->s_k[2] != 1 || d->s_k[1] != 3 || d->s_k[0] != 9) return false;
  const long long lo = d->s_co < d->s_ci ? d->s_co : d->s_ci, hi = d->s_co < d->s_ci ? d->s_ci : d->s_co;
  const long long inner = d->s_co > d->s_ci ? d->cin : d->cout;              // channels along W's second axis
  for (int k = 0; k < 3; ++k) {
    const int first = d->tbase[k], last = d->tbase[k] + 2 * d->tstep[k];
    if (first < 0 || first > 2 || last < 0 || last > 2) return false;
  }
  return lo == 27 && hi == 27 * inner;
}

static int fill_wpack(const mi355_wpack_desc* d, WpackArgs* a) {
  MI355_REQUIRE(d && d->src && d->dst, "weight_pack: null pointer");
  MI355_REQUIRE(d->coutp % 32 == 0 && d->cinp % 16 == 0 && d->cout <= d->coutp && d->cin <= d->cinp && d->ks >= 1 && d->ks <= 4,
                "weight_pack: bad extents");
  MI355_REQUIRE(d->s2d_mode >= 0 && d->s2d_mode <= 2 && (d->s2d_mode == 0 || (d->s2d_cp > 0 && d->s2d_cp % 8 == 0)),
                "weight_pack: bad space-to-depth mode");
  a->src = d->src; a->dst = d->dst; a->cout = d->cout; a->cin = d->cin; a->coutp = d->coutp; a->cinp = d->cinp; a->ks = d->ks;
  a->s_co = d->s_co; a->s_ci = d->s_ci; a->s_k0 = d->s_k[0]; a->s_k1 = d->s_k[1]; a->s_k2 = d->s_k[2];
  a->tb0 = d->tbase[0]; a->tb1 = d->tbase[1]; a->tb2 = d->tbase[2];
  a->ts0 = d->tstep[0]; a->ts1 = d->tstep[1]; a->ts2 = d->tstep[2];
  a->s2d_mode = d->s2d_mode; a->s2d_cp = d->s2d_cp;
  a->q_amax = d->q_amax;
  return MI355_OK;
}

}  // namespace

extern "C" {

int mi355_weight_pack(const mi355_wpack_desc* d, void* stream) {
  WpackArgs a;
  int rc = fill_wpack(d, &a);
  if (rc) return rc;
  MI355_REQUIRE(d->dtype == MI355_DT_F32 || d->dtype == MI355_DT_BF16 || d->dtype == MI355_DT_FP8, "weight_pack: bad dtype");
  MI355_REQUIRE(d->dtype != MI355_DT_FP8 || d->q_amax, "weight_pack: fp8 packing needs q_amax");
  const long long total = (long long)d->cinp * d->ks * d->ks * d->ks * d->coutp;
  dim3 grid((unsigned)((total + 255) / 256));
  if (d->dtype == MI355_DT_F32) hipLaunchKernelGGL(wpack_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else if (d->dtype == MI355_DT_FP8) hipLaunchKernelGGL(wpack_kernel<fp8_t>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(wpack_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, a);
  return mi355_check_launch("weight_pack");
}

int mi355_weight_pack_multi(const mi355_wpack_desc* descs, int32_t n, void* stream) {
  MI355_REQUIRE(descs && n > 0, "weight_pack_multi: bad argument");
  const int dtype = descs[0].dtype;
  MI355_REQUIRE(dtype == MI355_DT_F32 || dtype == MI355_DT_BF16 || dtype == MI355_DT_FP8, "weight_pack_multi: bad dtype");
  // three passes over the list: dense 3x3x3 packings and the space-to-depth k4 packings go through their
  // LDS-transposing kernels, the rest through the gather
  for (int pass = 0; pass < 3; ++pass) {
    const bool want_dense = pass == 0, want_s2d = pass == 1;
    int i0 = 0;
    while (i0 < n) {
      WpackMulti m;
      int cnt = 0;
      long long mx = 0, patches = 0;
      for (; i0 < n && cnt < kWpackChunk; ++i0) {
        const mi355_wpack_desc* d = &descs[i0];
        MI355_REQUIRE(d->dtype == dtype, "weight_pack_multi: mixed dtypes");
        const int klass = wpack_is_dense3(d) ? 0 : (wpack_is_s2d_dense(d) ? 1 : 2);
        if (klass != pass) continue;
        int rc = fill_wpack(d, &m.a[cnt]);
        if (rc) return rc;
        const long long total = (long long)d->cinp * d->ks * d->ks * d->ks * d->coutp;
        const long long np = want_s2d ? (d->s2d_mode == 1 ? (long long)(d->coutp / 8) * (d->s2d_cp / 16) : (long long)(d->cinp / 16) * (d->s2d_cp / 8))
                                      : (long long)(d->cinp / 16) * (d->coutp / 16);
        if (total > mx) mx = total;
        if (np > patches) patches = np;
        ++cnt;
      }
      if (cnt == 0) break;
      for (int i = cnt; i < kWpackChunk; ++i) m.a[i] = m.a[0];       // unused slots: never indexed (grid.y = cnt)
      if (want_dense) {
        MI355_REQUIRE(patches < (1ll << 31), "weight_pack_multi: too many patches");
        dim3 grid((unsigned)patches, cnt);
        if (dtype == MI355_DT_F32) wpack_dense3_multi_kernel<float><<<grid, dim3(256), 0, (hipStream_t)stream>>>(m);
        else if (dtype == MI355_DT_FP8) wpack_dense3_multi_kernel<fp8_t><<<grid, dim3(256), 0, (hipStream_t)stream>>>(m);
        else wpack_dense3_multi_kernel<bf16_t><<<grid, dim3(256), 0, (hipStream_t)stream>>>(m);
      } else if (want_s2d) {
        MI355_REQUIRE(patches < (1ll << 31), "weight_pack_multi: too many patches");
        dim3 grid((unsigned)patches, cnt);
        MI355_REQUIRE(dtype != MI355_DT_FP8, "weight_pack_multi: no fp8 space-to-depth packing");
        if (dtype == MI355_DT_F32) wpack_s2d_multi_kernel<float><<<grid, dim3(256), 0, (hipStream_t)stream>>>(m);
        else wpack_s2d_multi_kernel<bf16_t><<<grid, dim3(256), 0, (hipStream_t)stream>>>(m);
      } else {
        long long nb = (mx + 256 * 8 - 1) / (256 * 8);
        if (nb > 512) nb = 512;
        dim3 grid((unsigned)nb, cnt);
        if (dtype == MI355_DT_F32) hipLaunchKernelGGL(wpack_multi_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, m);
        else if (dtype == MI355_DT_FP8) hipLaunchKernelGGL(wpack_multi_kernel<fp8_t>, grid, dim3(256), 0, (hipStream_t)stream, m);
        else hipLaunchKernelGGL(wpack_multi_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, m);
      }
    }
  }
  return mi355_check_launch("weight_pack_multi");
}

}  // extern "C"
