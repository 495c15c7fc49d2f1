// Per-voxel arithmetic of the DTI relative-error table (reference: src/eval.py:154-166 `do_calc_diff_maps`,
// :240-257 `do_calc_error_avg`, :285-287 the probseg preparation of `calc_error_table`), shared by the HIP
// kernel (dti_errors.hip) and by the host-compiled check in tests/ (plain C++: g++ sees the qualifiers as empty).
//
// Columns, in calc_error_table's order: dxx dxy dxz dyy dyz dzz md fa ad rd azimuth inclination.
//   tensor components : |p - t| / t of the tensors AS PASSED (the reference's "normalized" tensor errors)
//   md, fa, ad, rd    : the same of the scalar maps of the de-normalised tensors (dti_voxel_maps, f64 angles)
//   azimuth, incl.    : r = (p - t) mod 360 (Python/numpy float remainder), then min(r, 360 - r)
// Post-processing: |diff|, 0 outside the mask, +inf -> 0; NaN STAYS NaN (a 0/0 inside the mask poisons its
// column in every ROI, since probseg * NaN = NaN also where probseg is 0 -- as in the reference).
// The principal eigenvector keeps dti_voxel_maps' z >= 0 sign, so the angle columns equal the reference's
// wherever LAPACK's principal eigenvector also has z > 0 (its sign is otherwise arbitrary).
#pragma once
#include "dti_core.h"

#define DTI_ERR_COLS 12
#define DTI_ERR_MAX_ROI 4

// Python's float `x % 360.0`, then the shorter way round the circle
MI355_HD double dti_angle_diff(double p, double t) {
  double m = fmod(p - t, 360.0);
  if (m < 0.0) m += 360.0;
  return m < 180.0 ? m : 360.0 - m;
}

MI355_HD double dti_rel_diff(double p, double t) { return fabs(p - t) / t; }

// |diff|, +inf -> 0 (the mask is applied by the caller: every column is 0 outside it)
MI355_HD double dti_err_post(double v) {
  v = fabs(v);
  return v == INFINITY ? 0.0 : v;
}

// p, t: the 6 components as passed; scale/offset: the de-normalisation x * scale + offset in front of the maps.
// out: the 12 post-processed columns of a voxel inside the mask.
MI355_HD void dti_error_voxel(const double* p, const double* t, double scale, double offset, double* out) {
  double dp[6], dt[6], mp[9], mt[9];
  for (int i = 0; i < 6; ++i) {
    out[i] = dti_err_post(dti_rel_diff(p[i], t[i]));
    dp[i] = p[i] * scale + offset;
    dt[i] = t[i] * scale + offset;
  }
  dti_voxel_maps(dp, false, mp);
  dti_voxel_maps(dt, false, mt);
  out[6] = dti_err_post(dti_rel_diff(mp[1], mt[1]));    // md
  out[7] = dti_err_post(dti_rel_diff(mp[0], mt[0]));    // fa
  out[8] = dti_err_post(dti_rel_diff(mp[2], mt[2]));    // ad
  out[9] = dti_err_post(dti_rel_diff(mp[3], mt[3]));    // rd
  out[10] = dti_err_post(dti_angle_diff(mp[4], mt[4]));
  out[11] = dti_err_post(dti_angle_diff(mp[5], mt[5]));
}

// tissue weight of a voxel: probseg where the mask is > 0 and probseg > 1e-5, else 0
MI355_HD double dti_roi_weight(bool in_mask, double ps) { return in_mask && ps > 1e-5 ? ps : 0.0; }
