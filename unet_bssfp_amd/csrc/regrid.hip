// Regridding between two different voxel grids: nearest, trilinear and cubic B-spline interpolation through
// a 3 x 4 f64 index matrix, and the separable prefilter that turns samples into cubic B-spline coefficients (regrid_core.h).
//
// Prefilter: one lane owns one line.  Along W a block stages a tile of rows through LDS with coalesced loads and stores and
// runs the recursion on the LDS image (row pitch an odd number of doubles: the 32 lanes of a half-wave hit distinct banks
// with 8-byte accesses); along H and D the lanes sit on adjacent w and march with a stride of a row or a plane, which is
// coalesced as it stands.  Three launches for all channels: W (f32 in, f64 out), then H and D in place on the f64 output.
// Regrid: one output voxel per lane, lanes adjacent along W; coordinates, taps and weights once per voxel, reused over the
// channels; f64 sums in a fixed order, one rounding at the store.
#include "common.h"
#include "regrid_core.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileBytes = 64 * 1024;           // LDS of one W-pass block
constexpr int kTileRowsMax = 64;

// rows [r0, r0 + rows_per_block) of the [rows][w] image: load, recursion along W in LDS, store
__global__ __launch_bounds__(kThreads) void prefilter_w_kernel(const float* __restrict__ x, double* __restrict__ out,
                                                               long long rows, int w, int pitch, int rows_per_block) {
  extern __shared__ double tile[];
  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const int nr = (int)min((long long)rows_per_block, rows - r0);
  const int count = nr * w;                     // <= 64 * 512
  const float* __restrict__ xs = x + r0 * w;
  double* __restrict__ os = out + r0 * w;
  for (int e = threadIdx.x; e < count; e += kThreads) {
    const int r = e / w;
    tile[r * pitch + (e - r * w)] = (double)xs[e];
  }
  __syncthreads();
  if ((int)threadIdx.x < nr) regrid_prefilter_line(tile + threadIdx.x * pitch, 1, w);
  __syncthreads();
  for (int e = threadIdx.x; e < count; e += kThreads) {
    const int r = e / w;
    os[e] = tile[r * pitch + (e - r * w)];
  }
}

// line L of an [outer][n][inner] image, in place: lanes adjacent along inner
__global__ __launch_bounds__(kThreads) void prefilter_strided_kernel(double* __restrict__ c, long long lines, long long inner,
                                                                     int n) {
  const long long line = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (line >= lines) return;
  const long long o = line / inner;
  regrid_prefilter_line(c + o * n * inner + (line - o * inner), inner, n);
}

struct RegridArgs {
  const void* src; float* out;
  int c, sd, sh, sw, od, oh, ow;
  float fill;
  double m[12];
};

template <int ORDER, typename TS>
__global__ __launch_bounds__(kThreads) void regrid_kernel(RegridArgs a) {
  constexpr int T = ORDER == MI355_REGRID_CUBIC ? 4 : ORDER == MI355_REGRID_LINEAR ? 2 : 1;
  const long long ovox = (long long)a.od * a.oh * a.ow;
  const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (v >= ovox) return;
  const long long row = v / a.ow;
  const int iw = (int)(v - row * a.ow), ih = (int)(row % a.oh), id = (int)(row / a.oh);
  const double s0 = regrid_coord(a.m, id, ih, iw), s1 = regrid_coord(a.m + 4, id, ih, iw), s2 = regrid_coord(a.m + 8, id, ih, iw);
  float* __restrict__ out = a.out + v;
  if (!(regrid_inside(s0, a.sd) && regrid_inside(s1, a.sh) && regrid_inside(s2, a.sw))) {
    for (int ch = 0; ch < a.c; ++ch) out[ch * ovox] = a.fill;
    return;
  }
  int idx[3][4];
  double wt[3][4];
  if (ORDER == MI355_REGRID_CUBIC) {
    regrid_taps_cubic(s0, a.sd, idx[0], wt[0]); regrid_taps_cubic(s1, a.sh, idx[1], wt[1]); regrid_taps_cubic(s2, a.sw, idx[2], wt[2]);
  } else if (ORDER == MI355_REGRID_LINEAR) {
    regrid_taps_linear(s0, a.sd, idx[0], wt[0]); regrid_taps_linear(s1, a.sh, idx[1], wt[1]); regrid_taps_linear(s2, a.sw, idx[2], wt[2]);
  } else {
    regrid_taps_nearest(s0, a.sd, idx[0], wt[0]); regrid_taps_nearest(s1, a.sh, idx[1], wt[1]); regrid_taps_nearest(s2, a.sw, idx[2], wt[2]);
  }
  const long long svox = (long long)a.sd * a.sh * a.sw;
  const TS* __restrict__ src = reinterpret_cast<const TS*>(a.src);
  for (int ch = 0; ch < a.c; ++ch) out[ch * ovox] = (float)regrid_gather<T, TS>(src + ch * svox, a.sh, a.sw, idx, wt);
}

template <int ORDER, typename TS>
int launch_regrid(const RegridArgs& a, hipStream_t s) {
  const long long ovox = (long long)a.od * a.oh * a.ow;
  regrid_kernel<ORDER, TS><<<(unsigned)((ovox + kThreads - 1) / kThreads), kThreads, 0, s>>>(a);
  return mi355_check_launch("regrid");
}

}  // namespace

extern "C" int mi355_bspline_prefilter(const float* x, double* coef, int32_t c, int32_t d, int32_t h, int32_t w, void* stream) {
  MI355_REQUIRE(x && coef, "bspline_prefilter: null pointer");
  MI355_REQUIRE(c >= 1 && c <= 65536, "bspline_prefilter: %d channels, need 1 .. 65536", (int)c);
  MI355_REQUIRE(d >= 1 && h >= 1 && w >= 1, "bspline_prefilter: extents (%d, %d, %d) must be positive", (int)d, (int)h, (int)w);
  if (d > MI355_REGRID_MAX_N || h > MI355_REGRID_MAX_N || w > MI355_REGRID_MAX_N) {
    mi355_set_error("bspline_prefilter: extents (%d, %d, %d) exceed %d (a line is not tiled)", (int)d, (int)h, (int)w,
                    MI355_REGRID_MAX_N);
    return MI355_ERR_UNSUPPORTED;
  }
  const long long rows = (long long)c * d * h, vox = rows * w;
  MI355_REQUIRE(rows <= 0x7fffffffll, "bspline_prefilter: %lld rows of W exceed 2^31 - 1 (split the channels)", rows);
  {
    const uintptr_t xa = (uintptr_t)x, ca = (uintptr_t)coef;
    MI355_REQUIRE(xa + (uintptr_t)vox * 4 <= ca || ca + (uintptr_t)vox * 8 <= xa, "bspline_prefilter: coef overlaps x");
  }
  hipStream_t s = (hipStream_t)stream;
  const int pitch = w | 1;                                                       // odd, >= w
  const int rpb = min(kTileRowsMax, kTileBytes / (pitch * (int)sizeof(double))); // >= 15
  prefilter_w_kernel<<<(unsigned)((rows + rpb - 1) / rpb), kThreads, (size_t)rpb * pitch * sizeof(double), s>>>(x, coef, rows, w,
                                                                                                              pitch, rpb);
  int rc = mi355_check_launch("bspline_prefilter (W)");
  if (rc != MI355_OK) return rc;
  if (h > 1) {
    const long long lines = (long long)c * d * w;
    prefilter_strided_kernel<<<(unsigned)((lines + kThreads - 1) / kThreads), kThreads, 0, s>>>(coef, lines, w, h);
    rc = mi355_check_launch("bspline_prefilter (H)");
    if (rc != MI355_OK) return rc;
  }
  if (d > 1) {
    const long long lines = (long long)c * h * w;
    prefilter_strided_kernel<<<(unsigned)((lines + kThreads - 1) / kThreads), kThreads, 0, s>>>(coef, lines, (long long)h * w, d);
    rc = mi355_check_launch("bspline_prefilter (D)");
  }
  return rc;
}

extern "C" int mi355_regrid(const void* src, float* out, int32_t c, int32_t sd, int32_t sh, int32_t sw, int32_t od, int32_t oh,
                            int32_t ow, const double* m, int32_t order, float fill, void* stream) {
  MI355_REQUIRE(src && out && m, "regrid: null pointer");
  MI355_REQUIRE(order == MI355_REGRID_NEAREST || order == MI355_REGRID_LINEAR || order == MI355_REGRID_CUBIC,
                "regrid: unknown order %d (0 nearest, 1 linear, 3 cubic B-spline)", (int)order);
  MI355_REQUIRE(c >= 1 && c <= 65536, "regrid: %d channels, need 1 .. 65536", (int)c);
  constexpr int kMaxExtent = 1 << 12;
  MI355_REQUIRE(sd >= 1 && sh >= 1 && sw >= 1 && sd <= kMaxExtent && sh <= kMaxExtent && sw <= kMaxExtent,
                "regrid: source extents (%d, %d, %d) outside 1 .. %d", (int)sd, (int)sh, (int)sw, kMaxExtent);
  MI355_REQUIRE(od >= 1 && oh >= 1 && ow >= 1 && od <= kMaxExtent && oh <= kMaxExtent && ow <= kMaxExtent,
                "regrid: output extents (%d, %d, %d) outside 1 .. %d", (int)od, (int)oh, (int)ow, kMaxExtent);
  RegridArgs a{src, out, c, sd, sh, sw, od, oh, ow, fill, {}};
  for (int i = 0; i < 12; ++i) {
    MI355_REQUIRE(isfinite(m[i]), "regrid: matrix entry %d is not finite", i);
    a.m[i] = m[i];
  }
  {
    const uintptr_t sa = (uintptr_t)src, oa = (uintptr_t)out;
    const uintptr_t sbytes = (uintptr_t)c * sd * sh * sw * (order == MI355_REGRID_CUBIC ? 8 : 4), obytes = (uintptr_t)c * od * oh * ow * 4;
    MI355_REQUIRE(sa + sbytes <= oa || oa + obytes <= sa, "regrid: out overlaps src");
  }
  hipStream_t s = (hipStream_t)stream;
  if (order == MI355_REGRID_CUBIC) return launch_regrid<MI355_REGRID_CUBIC, double>(a, s);
  if (order == MI355_REGRID_LINEAR) return launch_regrid<MI355_REGRID_LINEAR, float>(a, s);
  return launch_regrid<MI355_REGRID_NEAREST, float>(a, s);
}
