// What the slab-writing weight-gradient kernels share (wgrad_tile.h, wgrad_march.h, wgrad_pw.h): argument blocks, the transposed
// LDS fragment read with its lane offset, the slab store.  Every further device helper tried (x source selection, tile decode, slab-tile
// epilogue, marching prologue) changed its callers' instructions; all 29 kernels equal the parent's (profiles/wgrad_refactor_resources.txt).
#pragma once
#include "common.h"
namespace {
struct WgradArgs {
  const char* x0; const char* x1;
  int c0, c1, ld0, ld1;
  int n, di, hi, wi;
  const char* g; int cg, ldg;
  int do_, ho, wo;
  int gd, gh, gw, gs, god, goh, gow;
  int stride, pd, ph, pw;
  float* slab;
  int cinp, coutp;       // slab extents (multiples of 32)
  int splits;
  int tap_groups;
  long long rows;        // n*do*ho
  int g_cls_cout;        // tile kernels, KS=1: GEMM column blk*g_cls_cout + co reads g at 2p + bits(blk)
  int xn;                // samples held by x: grid sample n reads x sample n % xn
};
struct WMarchArgs { int seg_len, nseg, tiles_h, tiles_w, nslabs, ci_tiles, co_tiles; };     // the marching kernels

// Both MFMA operands are k-strided in LDS ([position][channel] rows of 64 B), so the bf16 fragments are fetched with the gfx950
// transposed read ds_read_b64_tr_b16 (4 positions x 16 channels per 16-lane group, two reads per fragment of 16 positions);
// 4 consecutive positions x 32 channels = 256 contiguous bytes per 32-lane half => conflict-free.
typedef short s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ s16x4 lds_tr16(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
}
__device__ __forceinline__ bf16x8 frag_tr(const char* p) {
  const s16x4 lo = lds_tr16(p), hi = lds_tr16(p + 4 * 64);
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
// this lane's byte offset inside the 16 rows frag_tr(p) reads
__device__ __forceinline__ int frag_tr_lane_off(const int lane, const int h) {      // h = lane >> 5, which every caller holds
  const int gi = lane & 15;
  return (8 * h + (gi >> 2)) * 64 + (16 * ((lane >> 4) & 1) + 4 * (gi & 3)) * 2;
}

// slab stores: written once, read once by a reduction that (round 4) runs at the end of the backward pass
__device__ __forceinline__ void st_slab(float* p, float v) {
#ifdef WGRAD_NT_SLABS
  __builtin_nontemporal_store(v, p);
#else
  *p = v;
#endif
}
}  // namespace
