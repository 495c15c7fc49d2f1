// Weight packing: f32 parameters -> the [chunk][tap][co][16] operand order of the convolution kernels (f32 / bf16 / e4m3), one
// tensor per launch (gather) or a list per launch (gather, dense 3x3x3 and space-to-depth k4 through LDS transposes; the forward
// and the data-gradient packing of one tensor from one read of it).
#include "common.h"

#include <vector>

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

// One packing of a forward / data-gradient pair: what differs between the two packings of one tensor.
struct WpackHalf {
  void* dst; const float* q_amax;
  int coutp, cinp;
  int tb0, tb1, tb2, ts0, ts1, ts2;
};
// Both packings of W[nr][nc][taps] (f: forward, rows are its cout; g: data gradient, rows are its cin): one read of W serves both.
struct WpackPair {
  const float* src;
  int nr, nc, cp;          // real extents of W's two channel axes; cp: s2d_cp of a space-to-depth pair
  WpackHalf f, g;
};
struct WpackPairs { WpackPair p[kWpackChunk]; };
__device__ __forceinline__ WpackHalf wpack_half_of(const WpackArgs& a) {
  return WpackHalf{a.dst, a.q_amax, a.coutp, a.cinp, a.tb0, a.tb1, a.tb2, a.ts0, a.ts1, a.ts2};
}

// Dense 3x3x3 weights W[R][C][27] (forward: R = cout, C = cin; data gradient: roles swapped, taps flipped): the
// kernels above gather 4-byte elements 27 floats (or C*27 floats) apart -- 16x read amplification on 34 M
// parameters after every optimiser step.  Here a block loads a 16 (R) x 16 (C) x 27 patch as 16 contiguous runs of
// 432 floats, keeps it in LDS and writes the packed [chunk][tap][co][16] order 512 contiguous bytes per tap.
constexpr int kDense3Taps = 27, kDense3Row = 16 * kDense3Taps + 1;      // LDS tile: [16 rows][kDense3Row]

// rows r0.. of W, columns c0.. (x 27 taps) -> tile, zeros outside W[nr][nc]; 4-byte loads
__device__ __forceinline__ void dense3_load(float* tile, const float* w, int r0, int c0, int nr, int nc, long long rstride) {
  constexpr int NT = kDense3Taps, ROW = kDense3Row;
  const int cvalid = min(16, nc - c0);                          // may be <= 0: the patch is padding only
  for (int rl = 0; rl < 16; ++rl) {
    const float* src = w + (long long)(r0 + rl) * rstride + (long long)c0 * NT;
    const bool rok = r0 + rl < nr;
    for (int j = threadIdx.x; j < 16 * NT; j += 256) tile[rl * ROW + j] = (rok && j < cvalid * NT) ? src[j] : 0.f;
  }
}

// the same with 16-byte loads: needs w and rstride * 4 to be multiples of 16 bytes (the patch offset c0 * 27 * 4 always is)
__device__ __forceinline__ void dense3_load_vec(float* tile, const float* w, int r0, int c0, int nr, int nc, long long rstride) {
  constexpr int NT = kDense3Taps, ROW = kDense3Row, VPR = 16 * NT / 4, NV = 16 * VPR, PASSES = (NV + 255) / 256;
  const int run = max(0, min(16, nc - c0)) * NT;                // valid floats of a row's run
  float4 v[PASSES];
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {                            // every load of the patch is in flight before the first LDS write
    const int i = threadIdx.x + p * 256, rl = i / VPR, j0 = (i - rl * VPR) * 4;
    v[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < NV && r0 + rl < nr && j0 < run) {
      const float* src = w + (long long)(r0 + rl) * rstride + (long long)c0 * NT + j0;
      if (j0 + 4 <= run) {
        v[p] = *reinterpret_cast<const float4*>(src);
      } else {                                                  // the run ends inside this piece (run is a multiple of 27, not of 4)
        v[p].x = src[0];
        if (j0 + 1 < run) v[p].y = src[1];
        if (j0 + 2 < run) v[p].z = src[2];
      }
    }
  }
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    const int i = threadIdx.x + p * 256, rl = i / VPR, j0 = (i - rl * VPR) * 4;
    if (i < NV) {
      float* t = tile + rl * ROW + j0;
      t[0] = v[p].x; t[1] = v[p].y; t[2] = v[p].z; t[3] = v[p].w;
    }
  }
}

// tile -> the packed (chunk, 16 output channels from cob * 16) block of one packing
template <typename T>
__device__ __forceinline__ void dense3_emit(const float* tile, const WpackHalf& a, int chunk, int cob, bool co_is_row) {
  constexpr int NT = kDense3Taps, ROW = kDense3Row;
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

template <typename T>
__global__ __launch_bounds__(256) void wpack_dense3_multi_kernel(const WpackMulti m) {
  const WpackArgs& a = m.a[blockIdx.y];
  __shared__ float tile[16 * kDense3Row];
  const int nchunk = a.cinp / 16, ncob = a.coutp / 16;
  if ((int)blockIdx.x >= nchunk * ncob) return;
  const int chunk = blockIdx.x / ncob, cob = blockIdx.x % ncob;
  const bool co_is_row = a.s_co > a.s_ci;                       // forward packing
  const int r0 = (co_is_row ? cob : chunk) * 16, c0 = (co_is_row ? chunk : cob) * 16;
  const int nr = co_is_row ? a.cout : a.cin, nc = co_is_row ? a.cin : a.cout;      // extents of W's two channel axes
  dense3_load(tile, a.src, r0, c0, nr, nc, co_is_row ? a.s_co : a.s_ci);
  __syncthreads();
  dense3_emit<T>(tile, wpack_half_of(a), chunk, cob, co_is_row);
}

// Forward and data-gradient packing of one tensor from ONE read of it (after an optimiser step both are stale, and the f32
// weights, just written past the caches, are the larger half of the traffic).  The two packings pad W differently (forward:
// rows to coutp, columns to cinp; data gradient: rows to its cinp, columns to its coutp), so the grid covers the union of the
// two patch grids and a block writes each packing only where that packing has the patch -- zeros in the padding, as above.
template <typename T>
__global__ __launch_bounds__(256) void wpack_dense3_pair_kernel(const WpackPairs m) {
  const WpackPair& p = m.p[blockIdx.y];
  __shared__ float tile[16 * kDense3Row];
  const int nrb = max(p.f.coutp, p.g.cinp) / 16, ncb = max(p.f.cinp, p.g.coutp) / 16;
  if ((int)blockIdx.x >= nrb * ncb) return;
  const int rb = blockIdx.x / ncb, cb = blockIdx.x % ncb;
  const bool in_f = rb * 16 < p.f.coutp && cb * 16 < p.f.cinp, in_g = rb * 16 < p.g.cinp && cb * 16 < p.g.coutp;
  if (!in_f && !in_g) return;                                   // a corner of the bounding grid that neither packing has
  const long long rstride = (long long)p.nc * kDense3Taps;
  if ((reinterpret_cast<uintptr_t>(p.src) & 15) == 0 && (p.nc & 3) == 0) dense3_load_vec(tile, p.src, rb * 16, cb * 16, p.nr, p.nc, rstride);
  else dense3_load(tile, p.src, rb * 16, cb * 16, p.nr, p.nc, rstride);
  __syncthreads();
  if (in_f) dense3_emit<T>(tile, p.f, cb, rb, true);
  if (in_g) dense3_emit<T>(tile, p.g, rb, cb, false);
}

// The PatchGAN k4 s2 weights W[co][c][4][4][4] packed for the space-to-depth formulation (8 dense taps j x 8 parity
// blocks blk; s2d_mode 1: the GEMM input-channel index is blk * cp + c (forward), 2: the GEMM output-channel index is
// (data gradient)).  For one (co, c) the 64 (j, blk) values are the contiguous 4x4x4 taps, so a block loads a
// [rows][cols][64] patch as contiguous runs and writes every (j, blk) slice as contiguous packed elements
// (the gather kernel reads 4 bytes per 256-byte stride: 150 us per step for 11 M discriminator weights).
// LDS tile [rows * cols][64]: the 64 taps of pair n = row * cols + col are rotated by n + n / 8, so that the 16-byte store
// pieces below, whose lanes read pairs 8 (bf16) apart, spread over the banks (a pitch of 65 would put them on 4 of 32).
__device__ __forceinline__ int s2d_tile_at(int n, int tap) { return n * 64 + ((tap + n + (n >> 3)) & 63); }

// rows r0.. (R of them) of W, channels c0.. (CC of them) x 64 taps -> tile, zeros outside W[nrow][ncol]; rstride = 64 * ncol
template <int R, int CC>
__device__ __forceinline__ void s2d_load(float* tile, const float* w, int r0, int c0, int nrow, int ncol, long long rstride) {
  if ((reinterpret_cast<uintptr_t>(w) & 15) == 0) {             // 16-byte loads: every (row, channel) run of 64 floats is aligned
    constexpr int PASSES = R * CC * 16 / 256;
    float4 v[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {                          // every load of the patch is in flight before the first LDS write
      const int i = threadIdx.x + p * 256, rl = i / (CC * 16), rest = i - rl * (CC * 16);   // rest * 4 = cl * 64 + tap: contiguous in W
      const int cl = rest >> 4;
      v[p] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r0 + rl < nrow && c0 + cl < ncol) v[p] = *reinterpret_cast<const float4*>(w + (long long)(r0 + rl) * rstride + (long long)c0 * 64 + rest * 4);
    }
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int i = threadIdx.x + p * 256, n = i >> 4, t0 = (i & 15) * 4;      // n = rl * CC + cl
      tile[s2d_tile_at(n, t0)] = v[p].x; tile[s2d_tile_at(n, t0 + 1)] = v[p].y;
      tile[s2d_tile_at(n, t0 + 2)] = v[p].z; tile[s2d_tile_at(n, t0 + 3)] = v[p].w;
    }
  } else {
    for (int i = threadIdx.x; i < R * CC * 64; i += 256) {
      const int rl = i / (CC * 64), rest = i - rl * (CC * 64);
      const int cl = rest >> 6;
      const bool ok = r0 + rl < nrow && c0 + cl < ncol;
      tile[s2d_tile_at(rl * CC + cl, rest & 63)] = ok ? w[(long long)(r0 + rl) * rstride + (long long)c0 * 64 + rest] : 0.f;
    }
  }
}

// tile -> the 64 (j, blk) slices of one packing, in 16-byte pieces: EPT consecutive e of one (j, co) row.
// fwd: a slice is R output channels x 16 e (e = channel c_l, CC == 16); data gradient: CC output channels x 16 e (e = row, R == 16)
template <typename T>
__device__ __forceinline__ void s2d_emit(const float* tile, const WpackHalf& a, bool fwd, int R, int CC, int cp, int r0, int c0) {
  constexpr int EPT = 16 / (int)sizeof(T), PPR = 16 / EPT;
  const int pps = (fwd ? R : CC) * PPR;                         // pieces per slice
  for (int idx = threadIdx.x; idx < 64 * pps; idx += 256) {
    const int sidx = idx / pps, within = idx - sidx * pps;
    const int x = within / PPR, e0 = (within - x * PPR) * EPT;  // fwd: x = co_l; dgrad: x = c_l
    const int j = sidx >> 3, blk = sidx & 7;
    const int jd = j >> 2, jh = (j >> 1) & 1, jw = j & 1;
    const int tap = (a.tb0 + a.ts0 * jd + (blk >> 2)) * 16 + (a.tb1 + a.ts1 * jh + ((blk >> 1) & 1)) * 4 + (a.tb2 + a.ts2 * jw + (blk & 1));
    alignas(16) T out[EPT];
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      const int e = e0 + k;
      const int rl = fwd ? x : e, cl = fwd ? e : x;
      Elem<T>::store(out + k, tile[s2d_tile_at(rl * CC + cl, tap)]);
    }
    long long dst;
    if (fwd) {   // dest [chunk = (blk*cp + c0)/16][j][co][e]
      const int chunk = (blk * cp + c0) >> 4;
      dst = (((long long)chunk * 8 + j) * a.coutp + r0 + x) * 16 + e0;
    } else {     // dest [chunk = r0/16][j][co' = blk*cp + c0 + c_l][e]
      dst = (((long long)(r0 >> 4) * 8 + j) * a.coutp + (long long)blk * cp + c0 + x) * 16 + e0;
    }
    *reinterpret_cast<uint4*>(reinterpret_cast<T*>(a.dst) + dst) = *reinterpret_cast<const uint4*>(out);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void wpack_s2d_multi_kernel(const WpackMulti m) {
  const WpackArgs& a = m.a[blockIdx.y];
  __shared__ float tile[128 * 64];
  const bool fwd = a.s2d_mode == 1;
  const int R = fwd ? 8 : 16, Ccols = fwd ? 16 : 8;                 // rows = W's first axis, cols = channels c
  const int nrb = (fwd ? a.coutp : a.cinp) / R, ncb = a.s2d_cp / Ccols;
  if ((int)blockIdx.x >= nrb * ncb) return;
  const int rb = blockIdx.x / ncb, cb = blockIdx.x % ncb;
  const int r0 = rb * R, c0 = cb * Ccols;
  const int nrow = fwd ? a.cout : a.cin, ncol = fwd ? a.cin : a.cout;   // real extents of W's two channel axes
  if (fwd) s2d_load<8, 16>(tile, a.src, r0, c0, nrow, ncol, a.s_co);    // row stride: 64 * (channels of the second axis)
  else s2d_load<16, 8>(tile, a.src, r0, c0, nrow, ncol, a.s_ci);
  __syncthreads();
  s2d_emit<T>(tile, wpack_half_of(a), fwd, R, Ccols, a.s2d_cp, r0, c0);
}

// Both space-to-depth packings of one tensor from one 16 x 16 x 64 patch (64 KB of LDS): the union of the two grids differs
// in the rows only (forward pads them to coutp, the data gradient to its cinp; both pad the channels to cp).
template <typename T>
__global__ __launch_bounds__(256) void wpack_s2d_pair_kernel(const WpackPairs m) {
  const WpackPair& p = m.p[blockIdx.y];
  __shared__ float tile[256 * 64];
  const int nrb = max(p.f.coutp, p.g.cinp) / 16, ncb = p.cp / 16;
  if ((int)blockIdx.x >= nrb * ncb) return;
  const int r0 = (blockIdx.x / ncb) * 16, c0 = (blockIdx.x % ncb) * 16;
  s2d_load<16, 16>(tile, p.src, r0, c0, p.nr, p.nc, 64ll * p.nc);
  __syncthreads();
  if (r0 < p.f.coutp) s2d_emit<T>(tile, p.f, true, 16, 16, p.cp, r0, c0);
  if (r0 < p.g.cinp) s2d_emit<T>(tile, p.g, false, 16, 16, p.cp, r0, c0);
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

static WpackHalf wpack_half(const mi355_wpack_desc* d) {
  return WpackHalf{d->dst, d->q_amax, d->coutp, d->cinp, d->tbase[0], d->tbase[1], d->tbase[2], d->tstep[0], d->tstep[1], d->tstep[2]};
}

enum { kWpackDense = 0, kWpackS2d = 1, kWpackGather = 2 };
static int wpack_class(const mi355_wpack_desc* d) { return wpack_is_dense3(d) ? kWpackDense : (wpack_is_s2d_dense(d) ? kWpackS2d : kWpackGather); }

// f is the forward packing of a tensor and g the data-gradient packing of the same tensor: same source, same real extents
// with the roles swapped (the dense predicates then pin both to the same W[f.cout][f.cin][taps])
static bool wpack_is_pair(const mi355_wpack_desc* f, int klass_f, const mi355_wpack_desc* g, int klass_g) {
  if (klass_f != klass_g || klass_f == kWpackGather || f->src != g->src || f->dtype != g->dtype || f->cout != g->cin || f->cin != g->cout) return false;
  if (klass_f == kWpackDense) return f->s_co > f->s_ci && g->s_co < g->s_ci;
  return f->s2d_mode == 1 && g->s2d_mode == 2 && f->s2d_cp == g->s2d_cp;
}

// Validates the list and finds the forward / data-gradient pairs in it, wherever their members stand: partner[i] is the index
// of i's partner or -1, klass[i] the kernel family of i.  Host only.  Returns the number of pairs, or an error code.
static int wpack_plan(const mi355_wpack_desc* descs, int n, std::vector<int>* klass, std::vector<int>* partner) {
  klass->assign(n, kWpackGather);
  partner->assign(n, -1);
  for (int i = 0; i < n; ++i) {
    WpackArgs a;
    int rc = fill_wpack(&descs[i], &a);
    if (rc) return rc;
    (*klass)[i] = wpack_class(&descs[i]);
  }
  int pairs = 0;
  for (int i = 0; i < n; ++i) {
    if ((*partner)[i] >= 0 || (*klass)[i] == kWpackGather) continue;
    for (int j = 0; j < n; ++j) {
      if (j == i || (*partner)[j] >= 0 || !wpack_is_pair(&descs[i], (*klass)[i], &descs[j], (*klass)[j])) continue;
      (*partner)[i] = j;
      (*partner)[j] = i;
      ++pairs;
      break;
    }
  }
  return pairs;
}

template <typename T>
static void launch_wpack_group(int klass, bool paired, dim3 grid, hipStream_t stream, const WpackMulti& m, const WpackPairs& mp) {
  if (klass == kWpackDense && paired) wpack_dense3_pair_kernel<T><<<grid, dim3(256), 0, stream>>>(mp);
  else if (klass == kWpackDense) wpack_dense3_multi_kernel<T><<<grid, dim3(256), 0, stream>>>(m);
  else if (klass == kWpackGather) wpack_multi_kernel<T><<<grid, dim3(256), 0, stream>>>(m);
  if constexpr (sizeof(T) != 1) {                               // no fp8 space-to-depth packing
    if (klass == kWpackS2d && paired) wpack_s2d_pair_kernel<T><<<grid, dim3(256), 0, stream>>>(mp);
    else if (klass == kWpackS2d) wpack_s2d_multi_kernel<T><<<grid, dim3(256), 0, stream>>>(m);
  }
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
  for (int i = 0; i < n; ++i) MI355_REQUIRE(descs[i].dtype == dtype, "weight_pack_multi: mixed dtypes");
  std::vector<int> klass, partner;
  const int pairs = wpack_plan(descs, n, &klass, &partner);
  if (pairs < 0) return pairs;
  for (int i = 0; i < n; ++i) MI355_REQUIRE(dtype != MI355_DT_FP8 || klass[i] != kWpackS2d, "weight_pack_multi: no fp8 space-to-depth packing");
  // five groups, each launched kWpackChunk members at a time: dense 3x3x3 pairs and single packings and the space-to-depth k4
  // pairs and single packings go through their LDS-transposing kernels, the rest through the gather
  for (int group = 0; group < 5; ++group) {
    const int want = group < 2 ? kWpackDense : (group < 4 ? kWpackS2d : kWpackGather);
    const bool paired = group == 0 || group == 2;
    int i0 = 0;
    while (i0 < n) {
      WpackMulti m;
      WpackPairs mp;
      int cnt = 0;
      long long mx = 0, patches = 0;
      for (; i0 < n && cnt < kWpackChunk; ++i0) {
        const mi355_wpack_desc* d = &descs[i0];
        if (klass[i0] != want || (partner[i0] >= 0) != paired) continue;
        long long np;
        if (paired) {
          const bool d_is_fwd = want == kWpackDense ? d->s_co > d->s_ci : d->s2d_mode == 1;
          if (!d_is_fwd) continue;                                   // a pair is launched where its forward member stands
          const mi355_wpack_desc* g = &descs[partner[i0]];
          mp.p[cnt] = WpackPair{d->src, d->cout, d->cin, d->s2d_cp, wpack_half(d), wpack_half(g)};
          const long long nrb = (d->coutp > g->cinp ? d->coutp : g->cinp) / 16;
          np = nrb * (want == kWpackDense ? (d->cinp > g->coutp ? d->cinp : g->coutp) / 16 : d->s2d_cp / 16);
        } else {
          fill_wpack(d, &m.a[cnt]);
          np = want == kWpackS2d ? (d->s2d_mode == 1 ? (long long)(d->coutp / 8) * (d->s2d_cp / 16) : (long long)(d->cinp / 16) * (d->s2d_cp / 8))
                                 : (long long)(d->cinp / 16) * (d->coutp / 16);
        }
        const long long total = (long long)d->cinp * d->ks * d->ks * d->ks * d->coutp;
        if (total > mx) mx = total;
        if (np > patches) patches = np;
        ++cnt;
      }
      if (cnt == 0) break;
      for (int i = cnt; i < kWpackChunk; ++i) {                     // unused slots: never indexed (grid.y = cnt)
        if (paired) mp.p[i] = mp.p[0];
        else m.a[i] = m.a[0];
      }
      dim3 grid((unsigned)patches, cnt);
      if (want == kWpackGather) {
        long long nb = (mx + 256 * 8 - 1) / (256 * 8);
        grid.x = (unsigned)(nb > 512 ? 512 : nb);
      } else {
        MI355_REQUIRE(patches < (1ll << 31), "weight_pack_multi: too many patches");
      }
      if (dtype == MI355_DT_F32) launch_wpack_group<float>(want, paired, grid, (hipStream_t)stream, m, mp);
      else if (dtype == MI355_DT_FP8) launch_wpack_group<fp8_t>(want, paired, grid, (hipStream_t)stream, m, mp);
      else launch_wpack_group<bf16_t>(want, paired, grid, (hipStream_t)stream, m, mp);
    }
  }
  return mi355_check_launch("weight_pack_multi");
}

int32_t mi355_weight_pack_multi_pairs(const mi355_wpack_desc* descs, int32_t n) {
  MI355_REQUIRE(descs && n > 0, "weight_pack_multi_pairs: bad argument");
  std::vector<int> klass, partner;
  return wpack_plan(descs, n, &klass, &partner);
}

}  // extern "C"
