// The two marching weight-gradient kernels: wgrad_march_kernel (3x3x3, padding 1) and wgrad_march2_kernel (dense 2x2x2, padding 0)
// on wide tensors (W >= 32).  A workgroup owns one 32 x 32 (ci, co) tile pair and an 8 (h) x 32 (w) footprint of output positions
// and walks a segment of output planes along d; x and g planes arrive by LDS-DMA in rings, two planes ahead of their use, with one
// barrier and one counted wait per plane; ONE slab per workgroup.
// Both are hand-scheduled and kept instruction for instruction (profiles/wgrad_refactor_resources.txt).  Their prologues are near
// copies ON PURPOSE: shared helpers for them made hipcc emit another sequence (wgrad_common.h).  Merge them when re-tuning one.
#pragma once
#include <type_traits>
#include "wgrad_common.h"
namespace {
// wgrad_march_kernel: the 3x3x3 stride-1 weight gradient of the wide levels (W >= 32), marching along d.
// wgrad_bf16_kernel<3, 2, 4, 32> stages a 4 x 6 x 34 halo for 2 x 4 x 32 output positions (3.2x the tile's own
// voxels) through registers, with a barrier on either side of the copy: 124 us for 32 -> 32 at 128^3, where the
// MFMA work is 35 us and reading both operands once is 34 us.  Here a workgroup owns an 8 (h) x 32 (w) footprint
// of one (ci-tile, co-tile) pair and walks a segment of output planes:
//   * x planes (10 x 34 halo voxels x 32 channels) and g planes (8 x 32 x 32 channels) arrive by LDS-DMA
//     (buffer_load_dwordx4 ... lds, 1 KB per instruction) TWO steps ahead of their use (one step of MFMAs, 1.6 us, is
//     shorter than the loaded memory latency: with one step of look-ahead the kernel ran at 3.4 us per plane): a ring
//     of 5 x planes -- output plane p pairs with x planes p - 1, p, p + 1 (kd = 0, 1, 2) while p + 2 and p + 3 are in
//     flight -- and 3 g planes, 158 of the 160 KB; every x plane is read from memory once per workgroup (halo 1.33x in
//     (h, w), (L + 2) / L along d), one barrier per plane, which waits for the OLDER of the two copies in flight only;
//   * the 4 waves are (w-segment of 16 positions) x (half of the 9 (kd, kw) tap columns: 4 whole columns each and the
//     footprint's upper / lower rows of the ninth, 108 MFMAs per plane for every wave).  A wave keeps the 8 g
//     fragments of its segment (one per footprint row) in registers for the whole plane, and an x fragment of halo row y
//     feeds the three taps kh = 0, 1, 2 (output rows y, y - 1, y - 2): ~1 ds_read_b64_tr_b16 per MFMA instead of 2.3;
//   * the accumulators (15 taps x 16 registers) stay resident for the whole segment; at the end the waves that hold
//     parts of a tap are added through LDS in a fixed order and ONE slab per workgroup is written (28 MB per layer
//     instead of 57 MB); wgrad_reduce.h sums the slabs in order as before: bit-identical reruns.
constexpr int kWmFH = 8, kWmFW = 32, kWmHR = kWmFH + 2, kWmHC = kWmFW + 2;
constexpr int kWmXV = kWmHR * kWmHC;                  // 340 halo voxels per x plane
constexpr int kWmXI = 24;                             // 1-KB DMA instructions per x plane, 6 per wave: 22 carry data, the last
                                                      // two (out-of-range source: zeros) go to a 2-KB dump area
constexpr int kWmXS = 22 * 1024;                      // bytes per x ring slot
constexpr int kWmGI = 16, kWmGS = kWmGI * 1024;       // g plane: 256 voxels x 64 B
constexpr int kWmXR = 5, kWmGR = 3;                   // ring depths
constexpr int kWmLds = kWmXR * kWmXS + kWmGR * kWmGS + 2048;   // 160 KB
constexpr int kWmPerStep = kWmXI / 4 + kWmGI / 4;     // DMA instructions per wave and step

// Tap columns of a wave: HALF 0 owns (kd, kw) columns 0..3, HALF 1 columns 5..8 (local index 0..3), and both own
// column 4 (local index 4) for half of the footprint rows each -- 4.5 columns = 108 MFMAs per plane for every wave.
constexpr int wm_unit(int half, int i) { return i == 4 ? 4 : (half ? 5 + i : i); }
constexpr bool wm_valid(int half, int i, int y, int kh) {            // does halo row y feed tap kh of local column i?
  const int sh = y - kh, lo = (i == 4 && half == 1) ? kWmFH / 2 : 0, hi = (i == 4 && half == 0) ? kWmFH / 2 : kWmFH;
  return sh >= lo && sh < hi;
}
constexpr bool wm_need(int half, int i, int y) { return y < kWmHR && (wm_valid(half, i, y, 0) || wm_valid(half, i, y, 1) || wm_valid(half, i, y, 2)); }
constexpr int wm_row_mfmas(int half, int y) {
  int n = 0;
  for (int i = 0; i < 5; ++i) for (int kh = 0; kh < 3; ++kh) n += wm_valid(half, i, y, kh) ? 1 : 0;
  return n;
}
constexpr int wm_row_reads(int half, int y) {
  int n = 0;
  for (int i = 0; i < 5; ++i) n += wm_need(half, i, y) ? 2 : 0;
  return n;
}

// one plane of one wave.  between(y): called behind halo row y's MFMAs, fenced (nothing is scheduled across it): the
// step's copy tickets, one per row -- issued together at the top of the step, the 10 copies cost the wave their whole issue
// time with the matrix pipe idle; behind a row, a copy's issue runs under the MFMA in flight (conv_march.h).
template <int HALF, typename Between>
__device__ __forceinline__ void wm_plane(f32x16 (&acc)[5][3], const char* xs, const char* gp, const int p, const int seg_lane_off,
                                         Between between) {
  bf16x8 gf[kWmFH];
#pragma unroll
  for (int sh = 0; sh < kWmFH; ++sh) gf[sh] = frag_tr(gp + sh * (kWmFW * 64));
  const char* xb[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int u = wm_unit(HALF, i), kd = u / 3, kw = u - kd * 3;
    xb[i] = xs + ((unsigned)(p + kd) % kWmXR) * kWmXS + kw * 64 + seg_lane_off;      // x plane q sits in ring slot (q + 1) % 5
  }
  bf16x8 xf[2][5];
#pragma unroll
  for (int i = 0; i < 5; ++i)
    if (wm_need(HALF, i, 0)) xf[0][i] = frag_tr(xb[i]);
  // order: the g fragments and halo row 0, then per halo row its MFMAs with the next row's reads spread between them
  // (one wave per SIMD: nothing else hides the LDS latency, and hipcc would sink every read next to its first use)
  __builtin_amdgcn_sched_group_barrier(0x100, 2 * kWmFH + wm_row_reads(HALF, 0), 0);
#pragma unroll
  for (int y = 0; y < kWmHR; ++y) {
#pragma unroll
    for (int i = 0; i < 5; ++i)
      if (wm_need(HALF, i, y + 1)) xf[(y + 1) & 1][i] = frag_tr(xb[i] + (y + 1) * (kWmHC * 64));
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
        if (wm_valid(HALF, i, y, kh))
          acc[i][kh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xf[y & 1][i], gf[y - kh], acc[i][kh], 0, 0, 0);
    const int M = wm_row_mfmas(HALF, y), R = wm_row_reads(HALF, y + 1);
#pragma unroll
    for (int k = 0; k < M; ++k) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      const int nr = R * (k + 1) / M - R * k / M;
      if (nr == 1) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      else if (nr == 2) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      else if (nr == 3) __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    between(y);
    __builtin_amdgcn_sched_barrier(0);
  }
}

__global__ __launch_bounds__(256, 1) void wgrad_march_kernel(const WgradArgs a, const WMarchArgs m) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const xs = smem;
  char* const gsm = smem + kWmXR * kWmXS;
  char* const dump = gsm + kWmGR * kWmGS;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int seg = wave & 1, half = wave >> 1;
  // workgroup -> (slab, ci tile, co tile): the tile pairs of one slab (same g planes / same x voxels) are neighbours in
  // dispatch order ON THE SAME XCD (workgroup ids go round-robin over the 8 XCDs), so that what they share is read from
  // memory once and from that XCD's L2 afterwards (96 -> 32: three ci tiles re-read the same g)
  const int tpairs = m.ci_tiles * m.co_tiles;
  const int xcd = blockIdx.x & 7, kq = blockIdx.x >> 3;
  const int slab = (kq / tpairs) * 8 + xcd, pair = kq % tpairs;
  if (slab >= m.nslabs) return;                                       // (whole workgroup; grid rounded up to 8 slabs)
  const int ci_base = (pair % m.ci_tiles) * 32, co_base = (pair / m.ci_tiles) * 32;
  const bool first = ci_base < a.c0;
  const char* xsrc = first ? a.x0 : a.x1;
  const int ldx = first ? a.ld0 : a.ld1;
  const int cix = first ? ci_base : ci_base - a.c0;
  const int csrc = first ? a.c0 : a.c1;
  const int cx_lim = csrc - cix, cg_lim = a.cg - co_base;

  const int per_seg = m.tiles_h * m.tiles_w, per_sample = per_seg * m.nseg;
  int t = slab;
  const int tn = t / per_sample;
  t -= tn * per_sample;
  const int sg = t / per_seg;
  t -= sg * per_seg;
  const int th_i = t / m.tiles_w, tw_i = t - th_i * m.tiles_w;
  const int d0 = sg * m.seg_len, d1 = min(a.do_, d0 + m.seg_len);
  const int h0 = th_i * kWmFH, w0 = tw_i * kWmFW;

  // ---- DMA source offsets: instruction j = i * 4 + wave covers 16 voxels, lane = (voxel, 16-byte piece of 8 channels);
  //      voxels outside the volume, channels past the source's width: out-of-range offset -> the DMA writes zeros
  const int piece = lane & 3;
  int xoff[kWmXI / 4], goff[kWmGI / 4];
#pragma unroll
  for (int i = 0; i < kWmXI / 4; ++i) {
    const int v = (i * 4 + wave) * 16 + (lane >> 2);
    const int y = v / kWmHC, col = v - y * kWmHC;
    const int gh = h0 - 1 + y, gw = w0 - 1 + col;
    const bool ok = v < kWmXV && gh >= 0 && gh < a.hi && gw >= 0 && gw < a.wi && piece * 8 < cx_lim;
    xoff[i] = ok ? ((gh * a.wi + gw) * ldx + cix + piece * 8) * 2 : (int)0x80000000;
  }
#pragma unroll
  for (int i = 0; i < kWmGI / 4; ++i) {
    const int v = (i * 4 + wave) * 16 + (lane >> 2);
    const int sh = v >> 5, sw = v & 31;
    const int gh = h0 + sh, gw = w0 + sw;
    const bool ok = gh < a.ho && gw < a.wo && piece * 8 < cg_lim;
    goff[i] = ok ? ((gh * a.gw + gw) * a.ldg + co_base + piece * 8) * 2 : (int)0x80000000;
  }
  const long long nvx = (long long)a.n * a.di * a.hi * a.wi, nvg = (long long)a.n * a.gd * a.gh * a.gw;
  const dma_rsrc_t rsx = dma_rsrc(xsrc, ((nvx - 1) * ldx + csrc) * 2), rsg = dma_rsrc(a.g, ((nvg - 1) * a.ldg + a.cg) * 2);
  const int xplane = a.hi * a.wi * ldx * 2, gplane = a.gh * a.gw * a.ldg * 2;
  auto load_x = [&](int q) __attribute__((always_inline)) {           // x plane q into ring slot (q + 1) % 5 (outside [0, D): zeros)
    const bool pin = q >= 0 && q < a.di;
    const int soff = pin ? (tn * a.di + q) * xplane : 0;
    const int kill = pin ? 0 : (int)0x80000000;
    char* dst = xs + ((unsigned)(q + 1) % kWmXR) * kWmXS + wave * 1024;
#pragma unroll
    for (int i = 0; i < kWmXI / 4; ++i)
      dma_lds_b128(rsx, (i == 5 && wave >= 2) ? dump + (wave - 2) * 1024 : dst + i * 4096, xoff[i] | kill, soff);
  };
  auto load_g = [&](int p) __attribute__((always_inline)) {           // g plane p into slot p % 3 (outside the segment: zeros, never read)
    const bool pin = p < d1;
    const int soff = pin ? (tn * a.gd + p) * gplane : 0;
    const int kill = pin ? 0 : (int)0x80000000;
    char* dst = gsm + ((unsigned)p % kWmGR) * kWmGS + wave * 1024;
#pragma unroll
    for (int i = 0; i < kWmGI / 4; ++i) dma_lds_b128(rsg, dst + i * 4096, goff[i] | kill, soff);
  };
  load_x(d0 - 1);
  load_x(d0);
  load_x(d0 + 1);
  load_x(d0 + 2);
  load_g(d0);
  load_g(d0 + 1);

  f32x16 acc[5][3];
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[i][k][j] = 0.f;
  const int seg_lane_off = seg * 16 * 64 + frag_tr_lane_off(lane, h);
  dma_wait_all();
  __syncthreads();                                                    // the first planes have landed
  // two whole marches (a wave's role never changes; a join of the two plane bodies inside the loop would make hipcc
  // shuffle the 240 accumulator registers); every wave passes the same number of barriers
  auto march = [&](auto halfc) __attribute__((always_inline)) {
    for (int p = d0; p < d1; ++p) {
      // every step issues the same number of copies (past the segment: zeros into free slots), so that "all but the newest
      // kWmPerStep" is the wait for the copies of the step before; ticket y goes behind halo row y: x plane p + 3 (rows
      // 0 .. 5), g plane p + 2 (rows 6 .. 9)
      const int qx = p + 3, pg = p + 2;
      const bool pinx = qx >= 0 && qx < a.di, ping = pg < d1;
      const int soffx = pinx ? (tn * a.di + qx) * xplane : 0, soffg = ping ? (tn * a.gd + pg) * gplane : 0;
      const int killx = pinx ? 0 : (int)0x80000000, killg = ping ? 0 : (int)0x80000000;
      char* const dstx = xs + ((unsigned)(qx + 1) % kWmXR) * kWmXS + wave * 1024;
      char* const dstg = gsm + ((unsigned)pg % kWmGR) * kWmGS + wave * 1024;
      auto ticket = [&](const int y) __attribute__((always_inline)) {
#ifndef WM_DIAG_NO_DMA
        static_assert(kWmXI / 4 + kWmGI / 4 == kWmHR, "one copy ticket per halo row");
        if (y < kWmXI / 4) dma_lds_b128(rsx, (y == 5 && wave >= 2) ? dump + (wave - 2) * 1024 : dstx + y * 4096, xoff[y] | killx, soffx);
        else dma_lds_b128(rsg, dstg + (y - kWmXI / 4) * 4096, goff[y - kWmXI / 4] | killg, soffg);
#endif
      };
      const char* gp = gsm + ((unsigned)p % kWmGR) * kWmGS + seg_lane_off;
#ifndef WM_DIAG_NO_MMA
      wm_plane<decltype(halfc)::value>(acc, xs, gp, p, seg_lane_off, ticket);
#else
#pragma unroll
      for (int y = 0; y < kWmHR; ++y) ticket(y);
#endif
#ifndef WM_DIAG_NO_WAIT
      asm volatile("s_waitcnt vmcnt(%0)" :: "n"(kWmPerStep) : "memory");   // x plane p + 2, g plane p + 1 have landed (this wave's share) ...
#endif
#ifndef WM_DIAG_NO_BARRIER
      __syncthreads();            // ... everybody's; and every wave is done with this plane's slots
#endif
    }
  };
  if (half == 0) march(std::integral_constant<int, 0>{});
  else march(std::integral_constant<int, 1>{});
  dma_wait_all();                 // the zero copies of the last steps must not land in the parking area
  __syncthreads();
  // ---- partial sums of a tap live in two waves (the two w-segments), those of the shared column 4 in all four: everybody
  //      but the writer parks them in LDS, the writer adds them in a fixed order (bit-identical reruns) and writes the slab
  float* const parkA = reinterpret_cast<float*>(smem) + lane;         // [half][i (5)][kh][j][lane]: the segment-1 waves
  float* const parkB = parkA + 2 * 5 * 48 * 64;                       // [kh][j][lane]: column 4 of (segment 0, half 1)
  if (seg == 1) {
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 16; ++j) parkA[(((half * 5 + i) * 3 + k) * 16 + j) * 64] = acc[i][k][j];
  } else if (half == 1) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < 16; ++j) parkB[(k * 16 + j) * 64] = acc[4][k][j];
  }
  __syncthreads();
  if (seg == 0) {
    float* sl = a.slab + (long long)slab * 27 * a.cinp * a.coutp;
    const int co = co_base + r;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      if (i == 4 && half == 1) break;                                 // column 4 is written by (segment 0, half 0)
      const int u = i == 4 ? 4 : (half ? 5 + i : i), kd = u / 3, kw = u - kd * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int tap = (kd * 3 + k) * 3 + kw;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          float v = acc[i][k][j] + parkA[(((half * 5 + i) * 3 + k) * 16 + j) * 64];
          if (i == 4) v = (v + parkB[(k * 16 + j) * 64]) + parkA[(((1 * 5 + 4) * 3 + k) * 16 + j) * 64];
          st_slab(&sl[((long long)tap * a.cinp + ci_base + acc_row(j, h)) * a.coutp + co], v);
        }
      }
    }
  }
}

// wgrad_march2_kernel: weight gradient of the dense 2x2x2 stride-1 convolutions on wide tensors -- the PatchGAN's strided blocks on
// space-to-depth operands (src/model.py:72-82) and the composite kernel of UpCat's fused up-branch (upcat.hip) --
// marching along d like wgrad_march_kernel.  wgrad_bf16_kernel<2, 2, 4, 32> staged a 3 x 5 x 33 halo per 2 x 4 x 32 outputs through
// registers with two barriers per tile: 0.15 of the MFMA peak on d1, whose operands alone need 1/4 of its time.
//   * workgroup = (32 x 32 (ci, co) tile pair, 8 (h) x 32 (w) footprint, segment of output planes); x planes (9 x 33 halo voxels) and
//     g planes arrive by LDS-DMA two planes ahead: ring of 4 x planes (output plane p pairs with x planes p, p + 1; p + 2 and
//     p + 3 in flight) and 3 g planes, 128 KB; one barrier per plane with a counted wait for the older copy;
//   * waves = (w-segment of 16 positions) x (kd): four taps (kh, kw) each -- 32 MFMAs per plane and wave; the 8 g fragments of the
//     segment stay in registers for the plane, an x fragment of halo row y feeds kh = 0 (output row y) and kh = 1 (row y - 1);
//   * at the end the two w-segments of a tap are added through LDS in a fixed order: ONE slab per workgroup, reduced in slab
//     order by wgrad_reduce.h: bit-identical reruns.
constexpr int kW2FH = 8, kW2FW = 32, kW2HR = kW2FH + 1, kW2HC = kW2FW + 1;
constexpr int kW2XI = 20, kW2XS = kW2XI * 1024;       // x plane: 297 halo voxels x 64 B = 18.6 KB -> 20 DMA instructions, 5 per wave
constexpr int kW2GI = 16, kW2GS = kW2GI * 1024;       // g plane: 256 voxels x 64 B
constexpr int kW2XR = 4, kW2GR = 3;
constexpr int kW2Lds = kW2XR * kW2XS + kW2GR * kW2GS;  // 128 KB
constexpr int kW2PerStep = kW2XI / 4 + kW2GI / 4;     // 9 copies per wave and step

__global__ __launch_bounds__(256, 1) void wgrad_march2_kernel(const WgradArgs a, const WMarchArgs m) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const xs = smem;
  char* const gsm = smem + kW2XR * kW2XS;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int seg = wave & 1, kd = wave >> 1;
  const int tpairs = m.ci_tiles * m.co_tiles;
  const int xcd = blockIdx.x & 7, kq = blockIdx.x >> 3;
  const int slab = (kq / tpairs) * 8 + xcd, pair = kq % tpairs;       // (the tile pairs of a slab are neighbours on one XCD: wgrad_march_kernel)
  if (slab >= m.nslabs) return;
  const int ci_base = (pair % m.ci_tiles) * 32, co_base = (pair / m.ci_tiles) * 32;
  const int cx_lim = a.c0 - ci_base, cg_lim = a.cg - co_base;
  const int per_seg = m.tiles_h * m.tiles_w, per_sample = per_seg * m.nseg;
  int t = slab;
  const int tn = t / per_sample;
  t -= tn * per_sample;
  const int sg = t / per_seg;
  t -= sg * per_seg;
  const int th_i = t / m.tiles_w, tw_i = t - th_i * m.tiles_w;
  const int d0 = sg * m.seg_len, d1 = min(a.do_, d0 + m.seg_len);
  const int h0 = th_i * kW2FH, w0 = tw_i * kW2FW;

  const int piece = lane & 3;
  int xoff[kW2XI / 4], goff[kW2GI / 4];
#pragma unroll
  for (int i = 0; i < kW2XI / 4; ++i) {
    const int v = (i * 4 + wave) * 16 + (lane >> 2);
    const int y = v / kW2HC, col = v - y * kW2HC;
    const int gh = h0 + y, gw = w0 + col;
    const bool ok = v < kW2HR * kW2HC && gh < a.hi && gw < a.wi && piece * 8 < cx_lim;
    xoff[i] = ok ? ((gh * a.wi + gw) * a.ld0 + ci_base + piece * 8) * 2 : (int)0x80000000;
  }
#pragma unroll
  for (int i = 0; i < kW2GI / 4; ++i) {
    const int v = (i * 4 + wave) * 16 + (lane >> 2);
    const int sh = v >> 5, sw = v & 31;
    const int gh = h0 + sh, gw = w0 + sw;
    const bool ok = gh < a.ho && gw < a.wo && piece * 8 < cg_lim;
    goff[i] = ok ? ((gh * a.gw + gw) * a.ldg + co_base + piece * 8) * 2 : (int)0x80000000;
  }
  const long long nvx = (long long)a.n * a.di * a.hi * a.wi, nvg = (long long)a.n * a.gd * a.gh * a.gw;
  const dma_rsrc_t rsx = dma_rsrc(a.x0, ((nvx - 1) * a.ld0 + a.c0) * 2), rsg = dma_rsrc(a.g, ((nvg - 1) * a.ldg + a.cg) * 2);
  const int xplane = a.hi * a.wi * a.ld0 * 2, gplane = a.gh * a.gw * a.ldg * 2;
  auto load_x = [&](int q) __attribute__((always_inline)) {           // x plane q -> ring slot q % 4 (beyond the tensor: zeros)
    const bool pin = q < a.di;
    const int soff = pin ? (tn * a.di + q) * xplane : 0, kill = pin ? 0 : (int)0x80000000;
    char* dst = xs + ((unsigned)q % kW2XR) * kW2XS + wave * 1024;
#pragma unroll
    for (int i = 0; i < kW2XI / 4; ++i) dma_lds_b128(rsx, dst + i * 4096, xoff[i] | kill, soff);
  };
  auto load_g = [&](int p) __attribute__((always_inline)) {
    const bool pin = p < d1;
    const int soff = pin ? (tn * a.gd + p) * gplane : 0, kill = pin ? 0 : (int)0x80000000;
    char* dst = gsm + ((unsigned)p % kW2GR) * kW2GS + wave * 1024;
#pragma unroll
    for (int i = 0; i < kW2GI / 4; ++i) dma_lds_b128(rsg, dst + i * 4096, goff[i] | kill, soff);
  };
  load_x(d0);
  load_x(d0 + 1);
  load_x(d0 + 2);
  load_g(d0);
  load_g(d0 + 1);

  f32x16 acc[2][2];                                                    // [kh][kw]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[i][k][j] = 0.f;
  const int gi = lane & 15;                                            // frag_tr_lane_off written out (it swaps two instructions here)
  const int lane_off = (8 * h + (gi >> 2)) * 64 + (16 * ((lane >> 4) & 1) + 4 * (gi & 3)) * 2;
  const int seg_lane_off = seg * 16 * 64 + lane_off;
  dma_wait_all();
  __syncthreads();
  for (int p = d0; p < d1; ++p) {
    // this step's copies: x plane p + 3 (tickets 0 .. 4), g plane p + 2 (tickets 5 .. 8), one behind each halo row's MFMAs
    const int qx = p + 3, pg = p + 2;
    const bool pinx = qx < a.di, ping = pg < d1;
    const int soffx = pinx ? (tn * a.di + qx) * xplane : 0, soffg = ping ? (tn * a.gd + pg) * gplane : 0;
    const int killx = pinx ? 0 : (int)0x80000000, killg = ping ? 0 : (int)0x80000000;
    char* const dstx = xs + ((unsigned)qx % kW2XR) * kW2XS + wave * 1024;
    char* const dstg = gsm + ((unsigned)pg % kW2GR) * kW2GS + wave * 1024;
    const char* gp = gsm + ((unsigned)p % kW2GR) * kW2GS + seg_lane_off;
    const char* xp = xs + ((unsigned)(p + kd) % kW2XR) * kW2XS + seg_lane_off;
    bf16x8 gf[kW2FH];
#pragma unroll
    for (int sh = 0; sh < kW2FH; ++sh) gf[sh] = frag_tr(gp + sh * (kW2FW * 64));
    bf16x8 xf[2][2];
#pragma unroll
    for (int kw = 0; kw < 2; ++kw) xf[0][kw] = frag_tr(xp + kw * 64);
    __builtin_amdgcn_sched_group_barrier(0x100, 2 * kW2FH + 4, 0);
#pragma unroll
    for (int y = 0; y < kW2HR; ++y) {
      if (y + 1 < kW2HR) {
#pragma unroll
        for (int kw = 0; kw < 2; ++kw) xf[(y + 1) & 1][kw] = frag_tr(xp + (y + 1) * (kW2HC * 64) + kw * 64);
      }
      int nm = 0;
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        const int row = y - kh;
        if (row >= 0 && row < kW2FH) {
#pragma unroll
          for (int kw = 0; kw < 2; ++kw) acc[kh][kw] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xf[y & 1][kw], gf[row], acc[kh][kw], 0, 0, 0);
          nm += 2;
        }
      }
      // the row's MFMAs with the next row's four transposed reads spread between them
      const int nrd = y + 1 < kW2HR ? 4 : 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < nm) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        const int nr = nm ? (nrd * (k + 1) / nm - nrd * k / nm) : 0;
        if (k < nm && nr == 1) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        else if (k < nm && nr == 2) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      static_assert(kW2PerStep == kW2HR, "one copy ticket per halo row");
      if (y < kW2XI / 4) dma_lds_b128(rsx, dstx + y * 4096, xoff[y] | killx, soffx);
      else dma_lds_b128(rsg, dstg + (y - kW2XI / 4) * 4096, goff[y - kW2XI / 4] | killg, soffg);
      __builtin_amdgcn_sched_barrier(0);
    }
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(kW2PerStep) : "memory");   // x plane p + 2, g plane p + 1 have landed (this wave's share) ...
    __syncthreads();                                                    // ... everybody's; every wave is done with this plane's slots
  }
  dma_wait_all();
  __syncthreads();
  // ---- the two w-segments of a tap: segment 1 parks, segment 0 adds (fixed order) and writes the workgroup's slab
  float* const park = reinterpret_cast<float*>(smem) + lane;           // [kd][kh][kw][j][lane]
  if (seg == 1) {
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int kw = 0; kw < 2; ++kw)
#pragma unroll
        for (int j = 0; j < 16; ++j) park[((((kd * 2 + kh) * 2 + kw) * 16) + j) * 64] = acc[kh][kw][j];
  }
  __syncthreads();
  if (seg == 0) {
    float* sl = a.slab + (long long)slab * 8 * a.cinp * a.coutp;
    const int co = co_base + r;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int kw = 0; kw < 2; ++kw) {
        const int tap = (kd * 2 + kh) * 2 + kw;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float v = acc[kh][kw][j] + park[((((kd * 2 + kh) * 2 + kw) * 16) + j) * 64];
          st_slab(&sl[((long long)tap * a.cinp + ci_base + acc_row(j, h)) * a.coutp + co], v);
        }
      }
  }
}
}  // namespace
