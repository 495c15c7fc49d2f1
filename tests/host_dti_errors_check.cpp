// Host build of the error-table kernel's per-voxel arithmetic (csrc/dti_errors_core.h) for the CPU test-suite.
// usage: hdec <in.bin> <out.bin> <n> <nroi> <scale> <offset>
//   in : pred[n][6], target[n][6], probseg[n][nroi] (f64), mask[n] (u8)
//   out: maps[n][12], then table[nroi][12] (weighted means, voxel-order f64 sums).  Test harness only.
#include <stdio.h>
#include <stdlib.h>
#include "../unet_bssfp_amd/csrc/dti_errors_core.h"
int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const long n = atol(argv[3]); const int R = atoi(argv[4]);
  const double scale = atof(argv[5]), offset = atof(argv[6]);
  if (R < 1 || R > DTI_ERR_MAX_ROI) return 2;
  double* p = (double*)malloc(sizeof(double) * 6 * n); double* t = (double*)malloc(sizeof(double) * 6 * n);
  double* ps = (double*)malloc(sizeof(double) * R * n); unsigned char* m = (unsigned char*)malloc(n + 1);
  double* maps = (double*)malloc(sizeof(double) * 12 * n);
  FILE* fi = fopen(argv[1], "rb");
  if (!fi || fread(p, sizeof(double) * 6, n, fi) != (size_t)n || fread(t, sizeof(double) * 6, n, fi) != (size_t)n ||
      fread(ps, sizeof(double) * R, n, fi) != (size_t)n || fread(m, 1, n, fi) != (size_t)n) return 3;
  fclose(fi);
  double s[DTI_ERR_MAX_ROI][DTI_ERR_COLS + 1] = {};
  for (long v = 0; v < n; ++v) {
    double* col = maps + 12 * v;
    const bool in = m[v] != 0;
    if (in) dti_error_voxel(p + 6 * v, t + 6 * v, scale, offset, col);
    else for (int c = 0; c < DTI_ERR_COLS; ++c) col[c] = 0.0;
    for (int r = 0; r < R; ++r) {
      const double w = dti_roi_weight(in, ps[v * R + r]);
      s[r][0] += w;
      for (int c = 0; c < DTI_ERR_COLS; ++c) s[r][1 + c] += w * col[c];
    }
  }
  double table[DTI_ERR_MAX_ROI * DTI_ERR_COLS];
  for (int r = 0; r < R; ++r)
    for (int c = 0; c < DTI_ERR_COLS; ++c) table[r * DTI_ERR_COLS + c] = s[r][1 + c] / s[r][0];
  FILE* fo = fopen(argv[2], "wb");
  if (!fo || fwrite(maps, sizeof(double) * 12, n, fo) != (size_t)n || fwrite(table, sizeof(double) * 12, R, fo) != (size_t)R) return 4;
  fclose(fo);
  return 0;
}
