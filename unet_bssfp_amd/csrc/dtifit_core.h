// Per-voxel arithmetic of the preprocessing kernels: the streaming log-linear tensor fit of dtifit.hip and
// the scalar maps of prep.hip, shared by the HIP kernels and by the host-compiled check in tests/ (plain C++: g++ sees the
// qualifiers as empty).  Everything is f64.  Arrays are indexed by constants once the loops are unrolled, so a voxel's state
// stays in registers on the device.
#pragma once
#include <math.h>
#ifndef MI355_HD
#ifndef __HIPCC__
#define MI355_HD
#else
#define MI355_HD __host__ __device__ __forceinline__
#endif
#endif

#define DTIFIT_NP 7                     // unknowns: Dxx, Dxy, Dxz, Dyy, Dyz, Dzz, ln S0
#define DTIFIT_NT 28                    // upper triangle of the 7 x 7 normal matrix

// element (i, j), j >= i, of a packed upper triangle
MI355_HD constexpr int dtifit_tri(int i, int j) { return i * DTIFIT_NP - i * (i - 1) / 2 + (j - i); }

// y_i of the model: ln S where S > 0, else 0 (NaN compares false: 0)
MI355_HD double dtifit_logsig(double s) { return s > 0.0 ? log(s) : 0.0; }

// ---- OLS: beta = pinv y, one measurement at a time; prow = the 7 entries of pinv's column for this measurement ----
MI355_HD void dtifit_ols_init(double* beta) {
#pragma unroll
  for (int j = 0; j < DTIFIT_NP; ++j) beta[j] = 0.0;
}
MI355_HD void dtifit_ols_step(double* beta, const double* prow, double y) {
#pragma unroll
  for (int j = 0; j < DTIFIT_NP; ++j) beta[j] += prow[j] * y;
}

// ---- WLS: weights w = S^2 from the measured signal; M = A^T W A (packed upper triangle), r = A^T W y ----
struct DtiFitWls {
  double m[DTIFIT_NT];
  double r[DTIFIT_NP];
  int npos;                             // measurements with a positive signal (weight > 0)
};
MI355_HD void dtifit_wls_init(DtiFitWls& a) {
#pragma unroll
  for (int k = 0; k < DTIFIT_NT; ++k) a.m[k] = 0.0;
#pragma unroll
  for (int j = 0; j < DTIFIT_NP; ++j) a.r[j] = 0.0;
  a.npos = 0;
}
// arow = the design row of this measurement, s = the measured signal, y = dtifit_logsig(s)
MI355_HD void dtifit_wls_step(DtiFitWls& a, const double* arow, double s, double y) {
  const bool pos = s > 0.0;
  const double w = pos ? s * s : 0.0;
  a.npos += pos ? 1 : 0;
#pragma unroll
  for (int i = 0; i < DTIFIT_NP; ++i) {
    const double wa = w * arow[i];
    a.r[i] += wa * y;
#pragma unroll
    for (int j = i; j < DTIFIT_NP; ++j) a.m[dtifit_tri(i, j)] += wa * arow[j];
  }
}
// Cholesky M = U^T U, then U^T z = r and U beta = z.  false (beta untouched) when fewer than 7 measurements carry weight or a
// pivot is not > 0 (NaN included): the caller takes the OLS solution.
MI355_HD bool dtifit_wls_solve(const DtiFitWls& a, double* beta) {
  if (a.npos < DTIFIT_NP) return false;
  double u[DTIFIT_NT], inv[DTIFIT_NP], z[DTIFIT_NP];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < DTIFIT_NP; ++i) {
#pragma unroll
    for (int j = i; j < DTIFIT_NP; ++j) {
      double s = a.m[dtifit_tri(i, j)];
#pragma unroll
      for (int k = 0; k < i; ++k) s -= u[dtifit_tri(k, i)] * u[dtifit_tri(k, j)];
      if (j == i) {
        ok = ok && (s > 0.0);
        const double d = sqrt(s);
        u[dtifit_tri(i, i)] = d;
        inv[i] = 1.0 / d;
      } else {
        u[dtifit_tri(i, j)] = s * inv[i];
      }
    }
  }
  if (!ok) return false;
#pragma unroll
  for (int i = 0; i < DTIFIT_NP; ++i) {
    double s = a.r[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= u[dtifit_tri(k, i)] * z[k];
    z[i] = s * inv[i];
  }
#pragma unroll
  for (int i = DTIFIT_NP - 1; i >= 0; --i) {
    double s = z[i];
#pragma unroll
    for (int k = i + 1; k < DTIFIT_NP; ++k) s -= u[dtifit_tri(i, k)] * beta[k];
    beta[i] = s * inv[i];
  }
  return true;
}

// min-max normalisation (v - min) / (max - min): a subtraction and an IEEE division, nothing to contract
MI355_HD double prep_normalize(double v, double lo, double hi) { return (v - lo) / (hi - lo); }

// scanner phase [0, 4095] -> [-pi, pi]: raw / 4095 * 2 pi - pi as three separately rounded operations (a fused multiply-add
// would change the last bit against the numpy restatement)
MI355_HD double prep_phase(double raw) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double t = raw / 4095.0;
  const double u = t * 6.283185307179586476925;
  return u - 3.141592653589793238463;
}
