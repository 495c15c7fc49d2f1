// Regridding between two voxel grids: coordinates, boundary rules, interpolation weights and the cubic
// B-spline prefilter, shared by the HIP kernels of regrid.hip and by the host-compiled check in tests/ (plain C++: g++ sees
// the qualifiers as empty).  Everything is f64.
//
// Output voxel i = (i_D, i_H, i_W) reads the source at s_a = m[4a] i_D + m[4a+1] i_H + m[4a+2] i_W + m[4a+3], three fused
// multiply-adds per axis.  Inside iff -0.5 <= s_a < N_a - 0.5 on every axis (the rule of resample_core.h); an outside voxel
// is filled.
//   order 0: the tap floor(s + 0.5), clamped into [0, N - 1];
//   order 1: the taps floor(s) and floor(s) + 1, both clamped (resample_core.h; scipy's mode='nearest');
//   order 3: the taps floor(s) - 1 .. floor(s) + 2, MIRRORED about the centres of the edge voxels (period 2 (N - 1), scipy's
//            mode='mirror'), read from prefiltered coefficients, not from samples.
// Why the boundary rule differs by order: the prefilter is a recursion whose start value is a sum over the infinite extension
// of the line.  Under the mirror extension that sum folds onto the line itself and has the closed form below, so the
// coefficients interpolate the samples EXACTLY; under the clamp extension no such closed form exists (scipy solves a
// different, approximate start there).  Orders 0 and 1 need no prefilter and keep the project's clamp.
#pragma once
#include <math.h>
#ifndef MI355_HD
#ifndef __HIPCC__
#define MI355_HD
#else
#define MI355_HD __host__ __device__ __forceinline__
#endif
#endif

#define REGRID_POLE (-0.2679491924311228)      // sqrt(3.0) - 2.0 in f64, the pole of the cubic B-spline
#define REGRID_GAIN 6.0                         // (1 - z)(1 - 1/z)

// s_a of one axis: row = m + 4 a
MI355_HD double regrid_coord(const double* row, int id, int ih, int iw) {
  return fma(row[2], (double)iw, fma(row[1], (double)ih, fma(row[0], (double)id, row[3])));
}
MI355_HD bool regrid_inside(double s, int n) { return s >= -0.5 && s < (double)n - 0.5; }   // a NaN is outside

MI355_HD int regrid_clamp(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }
// reflection about the centres of the edge voxels: ... 2 1 | 0 1 2 .. n-1 | n-2 n-3 ...; an axis of extent 1 reads index 0
MI355_HD int regrid_mirror(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}

// taps and weights of one axis for an INSIDE coordinate s (-0.5 <= s < n - 0.5); T = 1, 2, 4 taps for order 0, 1, 3
MI355_HD void regrid_taps_nearest(double s, int n, int* idx, double* wt) {
  idx[0] = regrid_clamp((int)floor(s + 0.5), n);
  wt[0] = 1.0;
}
MI355_HD void regrid_taps_linear(double s, int n, int* idx, double* wt) {
  const double f = floor(s), t = s - f;
  const int a = (int)f;                         // -1 .. n - 1
  idx[0] = regrid_clamp(a, n);
  idx[1] = regrid_clamp(a + 1, n);
  wt[0] = 1.0 - t;
  wt[1] = t;
}
MI355_HD void regrid_taps_cubic(double s, int n, int* idx, double* wt) {
  const double f = floor(s), t = s - f;
  const int a = (int)f;
#pragma unroll
  for (int k = 0; k < 4; ++k) idx[k] = regrid_mirror(a - 1 + k, n);
  const double u = 1.0 - t, t2 = t * t, t3 = t2 * t;
  wt[0] = u * u * u / 6.0;
  wt[1] = (3.0 * t3 - 6.0 * t2 + 4.0) / 6.0;
  wt[2] = (-3.0 * t3 + 3.0 * t2 + 3.0 * t + 1.0) / 6.0;
  wt[3] = t3 / 6.0;
}

// sum_a wD[a] (sum_b wH[b] (sum_c wW[c] v[a][b][c])): axis D outermost, taps ascending, every partial sum starts at 0
template <int T, typename TS>
MI355_HD double regrid_gather(const TS* src, long long sh, long long sw, const int (*idx)[4], const double (*wt)[4]) {
  double acc0 = 0.0;
#pragma unroll
  for (int a = 0; a < T; ++a) {
    double acc1 = 0.0;
#pragma unroll
    for (int b = 0; b < T; ++b) {
      const TS* row = src + ((long long)idx[0][a] * sh + idx[1][b]) * sw;
      double acc2 = 0.0;
#pragma unroll
      for (int c = 0; c < T; ++c) acc2 += wt[2][c] * (double)row[idx[2][c]];
      acc1 += wt[1][b] * acc2;
    }
    acc0 += wt[0][a] * acc1;
  }
  return acc0;
}

// z^e by squaring (e >= 0): the same products on the host and on the device
MI355_HD double regrid_powi(double z, int e) {
  double r = 1.0, b = z;
  while (e) {
    if (e & 1) r *= b;
    b *= b;
    e >>= 1;
  }
  return r;
}

// Cubic B-spline prefilter of one line c[0], c[stride], .., c[(n - 1) stride], in place: on return the line holds the
// coefficients whose mirror-extended spline interpolates the samples.  Every sample enters multiplied by the gain 6.
//   start   c0 = (x0 + z^(n-1) x(n-1) + sum_{i=1..n-2} z^i (x(i) + z^(n-1) x(n-1-i))) / (1 - z^(2n-2))      (exact under mirror)
//   causal  c(i) = x(i) + z c(i-1)
//   start   c(n-1) = (z c(n-2) + c(n-1)) z / (z^2 - 1)
//   anti    c(i) = z (c(i+1) - c(i))
// A line of extent 1 is left as it is.
MI355_HD void regrid_prefilter_line(double* c, long long stride, int n) {
  if (n < 2) return;
  const double z = REGRID_POLE;
  const double zn1 = regrid_powi(z, n - 1);
  double zi = z;
  double c0 = REGRID_GAIN * c[0] + zn1 * (REGRID_GAIN * c[(long long)(n - 1) * stride]);
  for (int i = 1; i < n - 1; ++i) {
    c0 += zi * (REGRID_GAIN * c[(long long)i * stride] + zn1 * (REGRID_GAIN * c[(long long)(n - 1 - i) * stride]));
    zi *= z;
  }
  c0 /= 1.0 - zn1 * zn1;
  double prev = c0, before = c0;
  c[0] = c0;
  for (int i = 1; i < n; ++i) {
    before = prev;
    prev = REGRID_GAIN * c[(long long)i * stride] + z * prev;
    c[(long long)i * stride] = prev;
  }
  prev = (z * before + prev) * z / (z * z - 1.0);
  c[(long long)(n - 1) * stride] = prev;
  for (int i = n - 2; i >= 0; --i) {
    prev = z * (prev - c[(long long)i * stride]);
    c[(long long)i * stride] = prev;
  }
}
