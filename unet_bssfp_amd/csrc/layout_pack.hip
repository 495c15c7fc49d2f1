// Layout passes between NCDHW f32 tensors and the NDHWC (optionally space-to-depth) activations of the path: pack / unpack,
// the plain -> space-to-depth repack, and the gradient seam between the PatchGAN and the generator.
#include "elementwise_common.h"

namespace {

// ------------------------------------------------------------------ pack / unpack
// Optional second source: channels [c, c + c1) of the window come from src1 (torch.cat([x, y], 1) of the
// discriminator as ONE pass that writes whole rows; two single-source passes wrote 48 and 16 of every 64 bytes).
// Thread = (voxel, 16-byte piece of its channel window): the P pieces of a voxel row sit in P consecutive lanes, so a wave
// writes whole rows -- 64 / P voxels x P x 16 contiguous bytes -- instead of one 16-byte piece of 64 different rows per
// store instruction (the one-voxel-per-thread form ran the 251 MB -> 137 MB discriminator pack at 2.2 TB/s: 174 us);
// the loads of a piece are EPV channel-strided dwords, lanes of equal piece reading consecutive voxels (64-byte runs).
template <typename T>
__global__ __launch_bounds__(256) void pack_kernel(const float* __restrict__ src, T* __restrict__ dst, int c,
                                                    long long v, int ld, int coff, int zero_to, S2D q,
                                                    const float* __restrict__ src1, int c1, int pieces) {
  constexpr int EPV = Elem<T>::kPer16B;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long vox = idx / pieces;
  const int piece = (int)(idx - vox * pieces);
  const int n = blockIdx.y;
  if (vox >= v) return;
  const float* s = src + (long long)n * c * v + vox;
  const float* s1 = src1 ? src1 + (long long)n * c1 * v + vox : nullptr;
  long long srow = 0; int blk = 0, border = 0;
  if (q.d) s2d_cell(q, (long long)n * v + vox, srow, blk, border);
  T* drow = q.d ? dst + srow * ld + (long long)blk * q.cblk : dst + ((long long)n * v + vox) * ld;
  const int e0 = coff + piece * EPV;
  Vec16<T> o;
#pragma unroll
  for (int j = 0; j < EPV; ++j) {
    const int ch = e0 + j - coff;
    o.f[j] = ch < c ? s[(long long)ch * v] : ((s1 && ch < c + c1) ? s1[(long long)(ch - c) * v] : 0.f);
  }
  o.store(drow + e0);
  if (q.d) s2d_zero_siblings<T>(dst, q, srow, blk, border, ld, e0);
}

// The same pack through an LDS tile, for channel windows of up to 64 elements (every activation of the path): a block owns
// 256 consecutive voxels; per source channel its threads read 256 consecutive floats (whole 128-byte lines: the
// piece-per-lane form above reads 64-byte runs of 4 channels per instruction and ran at 3 TB/s), the tile is turned in
// LDS (row stride odd in dwords: conflict-free 2- / 4-byte writes), and every voxel row leaves as contiguous 16-byte pieces.
template <typename T>
__global__ __launch_bounds__(256) void pack_tile_kernel(const float* __restrict__ src, T* __restrict__ dst, int c,
                                                         long long v, int ld, int coff, int zero_to, S2D q,
                                                         const float* __restrict__ src1, int c1) {
  constexpr int EPV = Elem<T>::kPer16B, ES = 16 / EPV;
  extern __shared__ __attribute__((aligned(16))) char tile[];
  const int wch = zero_to - coff;                         // window channels (multiple of EPV)
  const int rowb = wch * ES + 4;                          // LDS row bytes: +1 dword -> odd dword stride for 32 / 64-byte rows
  const long long v0 = (long long)blockIdx.x * 256;
  const int n = blockIdx.y, t = threadIdx.x;
  const long long vox = v0 + t;
  const bool in = vox < v;
  const float* s = src + (long long)n * c * v + vox;
  const float* s1 = src1 ? src1 + (long long)n * c1 * v + vox : nullptr;
  char* my = tile + t * rowb;
  for (int cb = 0; cb < wch; cb += 8) {                    // 8 loads in flight per thread (window channels are a multiple of 4 or 8)
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ch = cb + j;
      f[j] = 0.f;
      if (in && ch < wch) f[j] = ch < c ? s[(long long)ch * v] : ((s1 && ch < c + c1) ? s1[(long long)(ch - c) * v] : 0.f);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (cb + j < wch) Elem<T>::store(reinterpret_cast<T*>(my + (cb + j) * ES), f[j]);
  }
  __syncthreads();
  const int pieces = wch / EPV;
  for (int idx = t; idx < 256 * pieces; idx += 256) {
    const int lv = idx / pieces, piece = idx - lv * pieces;
    const long long gv = v0 + lv;
    if (gv >= v) continue;
    const uint32_t* r = reinterpret_cast<const uint32_t*>(tile + lv * rowb + piece * 16);
    const uint4 val = make_uint4(r[0], r[1], r[2], r[3]);
    const int e0 = coff + piece * EPV;
    if (q.d) {
      long long srow; int blk, border;
      s2d_cell(q, (long long)n * v + gv, srow, blk, border);
      *reinterpret_cast<uint4*>(dst + srow * ld + (long long)blk * q.cblk + e0) = val;
      s2d_zero_siblings<T>(dst, q, srow, blk, border, ld, e0);
    } else {
      *reinterpret_cast<uint4*>(dst + ((long long)n * v + gv) * ld + e0) = val;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void unpack_kernel(const T* __restrict__ src, float* __restrict__ dst, int c,
                                                      long long v, int ld, int coff, S2D q) {
  const long long vox = (long long)blockIdx.x * 256 + threadIdx.x;
  const int n = blockIdx.y;
  if (vox >= v) return;
  const T* srow = (q.d ? src + s2d_offset(q, (long long)n * v + vox, ld) : src + ((long long)n * v + vox) * ld) + coff;
  float* d = dst + (long long)n * c * v + vox;
  for (int ch = 0; ch < c; ++ch) d[(long long)ch * v] = Elem<T>::load(srow + ch);
}

// plain NDHWC activation -> its space-to-depth tensor S(a) (same element type): thread = (voxel, 16-byte piece)
template <typename T>
__global__ __launch_bounds__(256) void s2d_repack_kernel(const T* __restrict__ src, int lds_, T* __restrict__ dst, int ldd, long long v, int pieces, S2D q) {
  constexpr int EPV = Elem<T>::kPer16B;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long vox = idx / pieces;
  const int piece = (int)(idx - vox * pieces);
  const int n = blockIdx.y;
  if (vox >= v) return;
  const long long row = (long long)n * v + vox;
  long long srow; int blk, border;
  s2d_cell(q, row, srow, blk, border);
  const uint4 val = *reinterpret_cast<const uint4*>(src + row * lds_ + piece * EPV);
  *reinterpret_cast<uint4*>(dst + srow * ldd + (long long)blk * q.cblk + piece * EPV) = val;
  s2d_zero_siblings<T>(dst, q, srow, blk, border, ldd, piece * EPV);
}

// Gradient seam between the PatchGAN and the generator (src/model.py:172, 268: the generator phase back-propagates through D into
// G): dz[v][ch] = g_ncdhw[ch][v] (the loss head's gradient of the NCDHW output, or absent) + unS(g_s)[v][ch] (the PatchGAN's
// gradient of S(y_hat), or absent), as the NDHWC activation gradient the final convolution's backward reads.  One pass instead of
// unpack (S -> NCDHW f32) + add + pack (NCDHW f32 -> NDHWC).  thread = (voxel, 16-byte piece of the output row)
template <typename T>
__global__ __launch_bounds__(256) void seam_grad_kernel(const float* __restrict__ gy, const T* __restrict__ gs, int ld_s, T* __restrict__ dz, int ld_dz,
                                                        int pieces, int c, long long v, S2D q) {
  constexpr int EPV = Elem<T>::kPer16B;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long vox = idx / pieces;
  const int piece = (int)(idx - vox * pieces), n = blockIdx.y;
  if (vox >= v) return;
  Vec16<T> o;
#pragma unroll
  for (int j = 0; j < EPV; ++j) {
    const int ch = piece * EPV + j;
    o.f[j] = (gy && ch < c) ? gy[((long long)n * c + ch) * v + vox] : 0.f;
  }
  if (gs && piece * EPV < q.cblk) {
    Vec16<T> sv;
    sv.load(gs + s2d_offset(q, (long long)n * v + vox, ld_s) + piece * EPV);
#pragma unroll
    for (int j = 0; j < EPV; ++j) o.f[j] += sv.f[j];
  }
  o.store(dz + ((long long)n * v + vox) * ld_dz + piece * EPV);
}

}  // namespace

extern "C" {

static int pack_impl(const float* src, void* dst, int32_t n, int32_t c, int64_t v, int32_t ld, int32_t coff,
                     int32_t zero_to, int32_t dtype, S2D q, void* stream, const float* src1 = nullptr, int32_t c1 = 0) {
  MI355_REQUIRE(src && dst && n > 0 && c > 0 && v > 0 && c1 >= 0 && (c1 == 0 || src1), "pack: bad argument");
  const int epv = dtype == MI355_DT_F32 ? 4 : 8;
  MI355_REQUIRE(dtype == MI355_DT_F32 || dtype == MI355_DT_BF16, "pack: bad dtype");
  MI355_REQUIRE(coff % epv == 0 && zero_to <= ld && (zero_to - coff) % epv == 0 && zero_to - coff >= c + c1 && ld % epv == 0,
                "pack: channel window [%d,%d) of ld %d must be 16-byte aligned and hold c=%d", coff, zero_to, ld, c);
  const int pieces = (zero_to - coff) / epv;
  const int es = dtype == MI355_DT_F32 ? 4 : 2;
  const size_t lds = (size_t)256 * ((zero_to - coff) * es + 4);
  // LDS-tiled form: whole-line reads, whole-row writes.  Its tile must fit the 64 KB a launch gets without a raised limit
  // (common.h: raise_lds_limit): an f32 window of 64 channels (66 560 bytes; no caller has one) takes the piece-per-lane form.
  if (zero_to - coff <= 64 && v >= 4096 && lds <= 64 * 1024) {
    dim3 grid((unsigned)((v + 255) / 256), n);
    for_dtype(dtype, [&](auto t) { pack_tile_kernel<decltype(t)><<<grid, dim3(256), lds, (hipStream_t)stream>>>(src, (decltype(t)*)dst, c, (long long)v, ld, coff, zero_to, q, src1, c1); });
    return mi355_check_launch("pack");
  }
  MI355_REQUIRE(((long long)v * pieces + 255) / 256 < (1ll << 31), "pack: too many voxels for one launch");
  dim3 grid((unsigned)(((long long)v * pieces + 255) / 256), n);
  for_dtype(dtype, [&](auto t) { pack_kernel<decltype(t)><<<grid, dim3(256), 0, (hipStream_t)stream>>>(src, (decltype(t)*)dst, c, (long long)v, ld, coff, zero_to, q, src1, c1, pieces); });
  return mi355_check_launch("pack");
}

static int unpack_impl(const void* src, float* dst, int32_t n, int32_t c, int64_t v, int32_t ld, int32_t coff,
                       int32_t dtype, S2D q, void* stream) {
  MI355_REQUIRE(src && dst && n > 0 && c > 0 && v > 0 && coff >= 0 && coff + c <= ld, "unpack: bad argument");
  MI355_REQUIRE(dtype == MI355_DT_F32 || dtype == MI355_DT_BF16, "unpack: bad dtype");
  dim3 grid((unsigned)((v + 255) / 256), n);
  for_dtype(dtype, [&](auto t) { unpack_kernel<decltype(t)><<<grid, dim3(256), 0, (hipStream_t)stream>>>((const decltype(t)*)src, dst, c, (long long)v, ld, coff, q); });
  return mi355_check_launch("unpack");
}

int mi355_pack_ncdhw(const float* src, void* dst, int32_t n, int32_t c, int64_t v, int32_t ld, int32_t coff,
                     int32_t zero_to, int32_t dtype, void* stream) {
  return pack_impl(src, dst, n, c, v, ld, coff, zero_to, dtype, S2D{0, 0, 0, 0}, stream);
}

int mi355_unpack_ncdhw(const void* src, float* dst, int32_t n, int32_t c, int64_t v, int32_t ld, int32_t coff,
                       int32_t dtype, void* stream) {
  return unpack_impl(src, dst, n, c, v, ld, coff, dtype, S2D{0, 0, 0, 0}, stream);
}

int mi355_pack_ncdhw_s2d(const float* src, void* dst, int32_t n, int32_t c, int32_t d, int32_t h, int32_t w,
                         int32_t cblk, int32_t ld, int32_t coff, int32_t zero_to, int32_t dtype, void* stream) {
  int rc = check_s2d(d, h, w, cblk, ld, "pack_s2d");
  if (rc) return rc;
  MI355_REQUIRE(zero_to <= cblk, "pack_s2d: channel window exceeds the block");
  return pack_impl(src, dst, n, c, (int64_t)d * h * w, ld, coff, zero_to, dtype, S2D{d, h, w, cblk}, stream);
}

int mi355_pack2_ncdhw(const float* src0, int32_t c0, const float* src1, int32_t c1, void* dst, int32_t n, int64_t v,
                      int32_t ld, int32_t coff, int32_t zero_to, int32_t dtype, void* stream) {
  MI355_REQUIRE(src1 && c1 > 0, "pack2: second source missing");
  return pack_impl(src0, dst, n, c0, v, ld, coff, zero_to, dtype, S2D{0, 0, 0, 0}, stream, src1, c1);
}

int mi355_pack2_ncdhw_s2d(const float* src0, int32_t c0, const float* src1, int32_t c1, void* dst, int32_t n, int32_t d,
                          int32_t h, int32_t w, int32_t cblk, int32_t ld, int32_t coff, int32_t zero_to, int32_t dtype,
                          void* stream) {
  int rc = check_s2d(d, h, w, cblk, ld, "pack2_s2d");
  if (rc) return rc;
  MI355_REQUIRE(src1 && c1 > 0 && zero_to <= cblk, "pack2_s2d: bad argument");
  return pack_impl(src0, dst, n, c0, (int64_t)d * h * w, ld, coff, zero_to, dtype, S2D{d, h, w, cblk}, stream, src1, c1);
}

int mi355_unpack_ncdhw_s2d(const void* src, float* dst, int32_t n, int32_t c, int32_t d, int32_t h, int32_t w,
                           int32_t cblk, int32_t ld, int32_t coff, int32_t dtype, void* stream) {
  int rc = check_s2d(d, h, w, cblk, ld, "unpack_s2d");
  if (rc) return rc;
  MI355_REQUIRE(coff + c <= cblk, "unpack_s2d: channel window exceeds the block");
  return unpack_impl(src, dst, n, c, (int64_t)d * h * w, ld, coff, dtype, S2D{d, h, w, cblk}, stream);
}

int mi355_s2d_repack(const void* src, int32_t ld_src, void* dst, int32_t ld_dst, int32_t n, int32_t d, int32_t h, int32_t w,
                     int32_t c, int32_t dtype, void* stream) {
  int rc = check_s2d(d, h, w, c, ld_dst, "s2d_repack");
  if (rc) return rc;
  MI355_REQUIRE(src && dst && n > 0 && ld_src >= c, "s2d_repack: bad argument");
  MI355_REQUIRE(dtype == MI355_DT_F32 || dtype == MI355_DT_BF16, "s2d_repack: bad dtype");
  const int epv = dtype == MI355_DT_F32 ? 4 : 8, pieces = c / epv;
  MI355_REQUIRE(ld_src % epv == 0 && ld_dst % epv == 0, "s2d_repack: rows must be 16-byte aligned");
  const long long v = (long long)d * h * w;
  const dim3 grid((unsigned)((v * pieces + 255) / 256), (unsigned)n);
  const S2D q{d, h, w, c};
  for_dtype(dtype, [&](auto t) { s2d_repack_kernel<decltype(t)><<<grid, dim3(256), 0, (hipStream_t)stream>>>((const decltype(t)*)src, ld_src, (decltype(t)*)dst, ld_dst, v, pieces, q); });
  return mi355_check_launch("s2d_repack");
}

int mi355_seam_grad(const float* g_ncdhw, const void* g_s2d, int32_t ld_s, int32_t cblk, void* dz, int32_t ld_dz, int32_t cpad,
                    int32_t n, int32_t c, int32_t d, int32_t h, int32_t w, int32_t dtype, void* stream) {
  MI355_REQUIRE(dz && (g_ncdhw || g_s2d) && n > 0 && c > 0, "seam_grad: bad argument");
  MI355_REQUIRE(dtype == MI355_DT_F32 || dtype == MI355_DT_BF16, "seam_grad: bad dtype");
  const int epv = dtype == MI355_DT_F32 ? 4 : 8;
  MI355_REQUIRE(cpad % epv == 0 && cpad >= c && ld_dz >= cpad && ld_dz % epv == 0, "seam_grad: bad output row");
  if (g_s2d) {
    int rc = check_s2d(d, h, w, cblk, ld_s, "seam_grad");
    if (rc) return rc;
    MI355_REQUIRE(cblk % epv == 0 && cblk <= cpad && ld_s % epv == 0, "seam_grad: bad space-to-depth block");
  }
  const long long v = (long long)d * h * w;
  const int pieces = cpad / epv;
  const dim3 grid((unsigned)((v * pieces + 255) / 256), (unsigned)n);
  const S2D q{d, h, w, g_s2d ? cblk : 0};
  for_dtype(dtype, [&](auto t) { seam_grad_kernel<decltype(t)><<<grid, dim3(256), 0, (hipStream_t)stream>>>(g_ncdhw, (const decltype(t)*)g_s2d, ld_s, (decltype(t)*)dz, ld_dz, pieces, c, v, q); });
  return mi355_check_launch("seam_grad");
}

}  // extern "C"
