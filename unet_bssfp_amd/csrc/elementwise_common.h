// Pieces shared by the HBM-bound row kernels (layout_pack, normact, normact_small, pool, fp8_prep): space-to-depth
// addressing, the dropout keep-mask, the e4m3 copy and its amax, non-temporal 16-byte stores, row validation, and the host-side
// dispatch from a runtime (dtype, dropout) pair to kernel template arguments.  NDHWC rows are read and written as 16-byte
// vectors per lane (coalesced along channels).  Not part of common.h: the convolution sources do not see these.
#pragma once
#include <type_traits>
#include "common.h"

namespace {

// ------------------------------------------------------------------ space-to-depth addressing
// S(a)[n, jd, jh, jw, blk*C + c] = a[n, 2jd+bd-1, 2jh+bh-1, 2jw+bw-1, c], blk = bd*4 + bh*2 + bw, extents
// (D/2+1, H/2+1, W/2+1): a k4 s2 p1 convolution of `a` is a dense k2 s1 p0 convolution of S(a).
struct S2D { int d, h, w, cblk; };   // extents of the plain tensor (per sample); d == 0: off
// (cell row, block) of plain voxel `row`; `border`: bit set per axis (4 d, 2 h, 1 w) on which the voxel is the first or
// last one -- the same cell's block with that parity bit flipped would read a[-1] / a[D]: it must hold zeros, and the
// writer of the border voxel stores them (every slot of S(a) is then written by exactly one thread: the output
// tensor needs no prior zero-fill).
__device__ __forceinline__ void s2d_cell(const S2D& q, long long row /* n*D*H*W + ... */, long long& srow, int& blk, int& border) {
  const int w = (int)(row % q.w); long long t = row / q.w;
  const int h = (int)(t % q.h); t /= q.h;
  const int d = (int)(t % q.d); const long long n = t / q.d;
  srow = ((n * (q.d / 2 + 1) + ((d + 1) >> 1)) * (q.h / 2 + 1) + ((h + 1) >> 1)) * (q.w / 2 + 1) + ((w + 1) >> 1);
  blk = ((d + 1) & 1) * 4 + ((h + 1) & 1) * 2 + ((w + 1) & 1);
  border = ((d == 0 || d == q.d - 1) ? 4 : 0) | ((h == 0 || h == q.h - 1) ? 2 : 0) | ((w == 0 || w == q.w - 1) ? 1 : 0);
}
__device__ __forceinline__ long long s2d_offset(const S2D& q, long long row, int ld) {
  long long srow; int blk, border;
  s2d_cell(q, row, srow, blk, border);
  return srow * ld + (long long)blk * q.cblk;
}
// zeros into [e0, e0 + 16 B) of the border voxel's sibling blocks (all non-empty subsets of the border axes)
template <typename T>
__device__ __forceinline__ void s2d_zero_siblings(T* base, const S2D& q, long long srow, int blk, int border, int ld, int e0) {
  if (!border) return;
  Vec16<T> z;
#pragma unroll
  for (int j = 0; j < Vec16<T>::N; ++j) z.f[j] = 0.f;
  for (int sub = 1; sub < 8; ++sub)
    if ((sub & ~border) == 0) z.store(base + srow * ld + (long long)(blk ^ sub) * q.cblk + e0);
}

static int check_s2d(int d, int h, int w, int cblk, int ld, const char* who) {
  MI355_REQUIRE(d > 0 && h > 0 && w > 0 && d % 2 == 0 && h % 2 == 0 && w % 2 == 0, "%s: space-to-depth needs even extents", who);
  MI355_REQUIRE(cblk > 0 && cblk % 8 == 0 && ld >= 8 * cblk, "%s: space-to-depth row must hold 8 channel blocks (of a multiple of 8 channels)", who);
  return MI355_OK;
}

static int check_rows(int c, int ld, int dtype, const char* who) {
  const int epv = dtype == MI355_DT_F32 ? 4 : 8;
  MI355_REQUIRE(dtype == MI355_DT_F32 || dtype == MI355_DT_BF16, "%s: bad dtype", who);
  MI355_REQUIRE(c > 0 && c % 16 == 0 && c <= 1024, "%s: channels must be a multiple of 16 and <= 1024 (c=%d)", who, c);
  MI355_REQUIRE(ld >= c && ld % epv == 0, "%s: ld=%d must be >= c and keep rows 16-byte aligned", who, ld);
  MI355_REQUIRE(c / epv <= 256, "%s: too many channels", who);
  return MI355_OK;
}

// ------------------------------------------------------------------ dropout keep-mask
// effective seed: a per-call salt, optionally combined with a step counter kept in device memory (so
// that a launch captured in a hipGraph draws a new mask on every replay)
__device__ __forceinline__ unsigned long long eff_seed(unsigned long long salt, const unsigned long long* p) {
  return p ? p[0] * 0x9E3779B97F4A7C15ull + salt * 0xD1B54A32D192ED03ull + 1ull : salt;
}
// keep-mask of element `idx` (logical index, independent of ld): 16 bits per element, one 64-bit mix per
// aligned group of 4 elements (the compiler shares it across the 4 / 8 elements of a 16-byte piece)
__device__ __forceinline__ unsigned long long drop_group_bits(unsigned long long seed, unsigned long long group) {
  unsigned long long x = group * 0x9E3779B97F4A7C15ull + seed;
  x ^= x >> 32; x *= 0xD6E8FEB86659FD93ull; x ^= x >> 32;
  return x;
}
// keep-masks of the EPV (4 or 8) elements of one 16-byte piece starting at logical index e0 (a multiple of 4:
// channel counts are multiples of 16).  The mixes are computed explicitly once per group of 4 -- hipcc cannot
// prove the alignment of e0 and would otherwise mix once per element.
template <int EPV>
__device__ __forceinline__ unsigned drop_keep_mask(unsigned long long seed, unsigned long long e0, unsigned thr16) {
  unsigned m = 0;
#pragma unroll
  for (int g4 = 0; g4 < EPV / 4; ++g4) {
    const unsigned long long x = drop_group_bits(seed, (e0 >> 2) + g4);
#pragma unroll
    for (int k = 0; k < 4; ++k) m |= ((((unsigned)(x >> (16 * k))) & 0xffffu) >= thr16 ? 1u : 0u) << (4 * g4 + k);
  }
  return m;
}

// ---- e4m3 copies written by the PRODUCER of an fp8 convolution's operand (delayed per-tensor scaling) ----
// block maximum -> at most one atomic per workgroup, and none when the tensor-wide maximum is already there (m >= 0: bit
// order = value order).  Every thread of a 256-thread workgroup calls it.  One atomic per WAVE was measured to double
// the kernels: all waves finish together and ~6 ns per same-address atomic serialise behind each other.
__device__ __forceinline__ void amax_commit(float m, float* out) {
  __shared__ float red[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const unsigned cur = __hip_atomic_load(reinterpret_cast<unsigned int*>(out), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__float_as_uint(m) > cur) atomicMax(reinterpret_cast<unsigned int*>(out), __float_as_uint(m));
  }
}
// 8 results that are about to be stored as bf16 -> the 8 e4m3 bytes mi355_cast_fp8 would make of the stored tensor
// (rounded through bf16 first, then * 224 / amax); returns max |bf16 value| for the next step's scale
__device__ __forceinline__ float e4m3_piece(const float (&f)[8], float sc, uint8_t* dst) {
  float m = 0.f, r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float b = __uint_as_float((uint32_t)f32_to_bf16_bits(f[j]) << 16);
    m = fmaxf(m, fabsf(b));
    r[j] = b * sc;
  }
  uint32_t w0 = cvt_pk_fp8(r[0], r[1], 0u, false), w1 = cvt_pk_fp8(r[4], r[5], 0u, false);
  w0 = cvt_pk_fp8(r[2], r[3], w0, true);
  w1 = cvt_pk_fp8(r[6], r[7], w1, true);
  *reinterpret_cast<uint2*>(dst) = make_uint2(w0, w1);
  return m;
}

// fp8 mode: the next convolution reads the e4m3 copy this launch writes, the bf16 tensor's next reader is the weight gradient a
// backward pass away -- stored non-temporally.  1x24x160^3, three interleaved rounds: fp8 18.48 against 18.65 ms per step (bf16: 18.53).
#ifndef MI355_DIAG_NO_NT
#define FP8_NT_A 1
#endif
// Vec16<T>::store with the non-temporal policy (a tensor whose next reader is far away)
__device__ __forceinline__ void st_nt_b128(void* p, const uint4 v) {
  typedef unsigned u4 __attribute__((ext_vector_type(4)));
  const u4 x = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(x, reinterpret_cast<u4*>(p));
}
__device__ __forceinline__ void store16_nt(const Vec16<float>& v, void* p) {
  st_nt_b128(p, make_uint4(__float_as_uint(v.f[0]), __float_as_uint(v.f[1]), __float_as_uint(v.f[2]), __float_as_uint(v.f[3])));
}
__device__ __forceinline__ void store16_nt(const Vec16<bf16_t>& v, void* p) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = (uint32_t)f32_to_bf16_bits(v.f[2 * i]) | ((uint32_t)f32_to_bf16_bits(v.f[2 * i + 1]) << 16);
  st_nt_b128(p, make_uint4(w[0], w[1], w[2], w[3]));
}

// ------------------------------------------------------------------ host: runtime (dtype, dropout) -> template arguments
// f is a generic lambda, `[&](auto t, auto drop) { kernel<decltype(t), drop><<<...>>>(...); }`: t is a value of the element type
// (float or bf16_t), drop a std::bool_constant.  Every kernel f names is instantiated for all the pairs, so a family that is
// no full product (bf16 only, no dropout template) is selected with an `if` around the call instead.  The caller has validated
// dtype (check_rows or its own MI355_REQUIRE): whatever is not f32 is taken as bf16.
template <typename F> static void for_dtype(int dtype, F&& f) { if (dtype == MI355_DT_F32) f(float()); else f(bf16_t()); }
template <typename F> static void for_dtype_drop(int dtype, bool drop, F&& f) {
  for_dtype(dtype, [&](auto t) { if (drop) f(t, std::true_type()); else f(t, std::false_type()); });
}

}  // namespace
