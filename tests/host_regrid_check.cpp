// Host build of the regridding arithmetic (csrc/regrid_core.h) for the CPU test-suite.
// in : c, sd, sh, sw, od, oh, ow, order, fill, m[12], samples [c][sd][sh][sw]                 (doubles)
// out: coefficients [c][sd][sh][sw] (the samples themselves for orders 0 and 1), values [c][od][oh][ow]   (doubles, unrounded)
// The loops are the kernels': the prefilter along W, H and D line by line, then one output voxel at a time with its
// coordinates, taps and weights computed once and reused over the channels.  Test harness only.
#include <stdio.h>
#include <stdlib.h>
#include "../unet_bssfp_amd/csrc/regrid_core.h"

template <int T>
static void interpolate(const double* src, double* out, int c, const int* sn, const int* on, const double* m, int order, double fill) {
  const long long svox = (long long)sn[0] * sn[1] * sn[2], ovox = (long long)on[0] * on[1] * on[2];
  for (int id = 0; id < on[0]; ++id)
    for (int ih = 0; ih < on[1]; ++ih)
      for (int iw = 0; iw < on[2]; ++iw) {
        const long long v = ((long long)id * on[1] + ih) * on[2] + iw;
        double s[3];
        bool in = true;
        for (int a = 0; a < 3; ++a) {
          s[a] = regrid_coord(m + 4 * a, id, ih, iw);
          in = in && regrid_inside(s[a], sn[a]);
        }
        if (!in) {
          for (int ch = 0; ch < c; ++ch) out[ch * ovox + v] = fill;
          continue;
        }
        int idx[3][4];
        double wt[3][4];
        for (int a = 0; a < 3; ++a) {
          if (order == 3) regrid_taps_cubic(s[a], sn[a], idx[a], wt[a]);
          else if (order == 1) regrid_taps_linear(s[a], sn[a], idx[a], wt[a]);
          else regrid_taps_nearest(s[a], sn[a], idx[a], wt[a]);
        }
        for (int ch = 0; ch < c; ++ch) out[ch * ovox + v] = regrid_gather<T, double>(src + ch * svox, sn[1], sn[2], idx, wt);
      }
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  double head[21];
  if (!fi || fread(head, sizeof(double), 21, fi) != 21) return 3;
  const int c = (int)head[0], order = (int)head[7];
  const int sn[3] = {(int)head[1], (int)head[2], (int)head[3]}, on[3] = {(int)head[4], (int)head[5], (int)head[6]};
  if (c < 1 || c > 16 || (order != 0 && order != 1 && order != 3)) return 2;
  for (int a = 0; a < 3; ++a)
    if (sn[a] < 1 || sn[a] > 512 || on[a] < 1 || on[a] > 512) return 2;
  const size_t svox = (size_t)sn[0] * sn[1] * sn[2], ovox = (size_t)on[0] * on[1] * on[2];
  double* coef = (double*)malloc(sizeof(double) * c * svox);
  double* out = (double*)malloc(sizeof(double) * c * ovox);
  if (!coef || !out) return 5;
  if (fread(coef, sizeof(double), c * svox, fi) != c * svox) return 3;
  fclose(fi);
  if (order == 3) {
    const long long d = sn[0], h = sn[1], w = sn[2];
    for (long long r = 0; r < c * d * h; ++r) regrid_prefilter_line(coef + r * w, 1, (int)w);
    for (long long o = 0; o < c * d; ++o)
      for (long long i = 0; i < w; ++i) regrid_prefilter_line(coef + o * h * w + i, w, (int)h);
    for (long long o = 0; o < c; ++o)
      for (long long i = 0; i < h * w; ++i) regrid_prefilter_line(coef + o * d * h * w + i, h * w, (int)d);
  }
  if (order == 3) interpolate<4>(coef, out, c, sn, on, head + 9, order, head[8]);
  else if (order == 1) interpolate<2>(coef, out, c, sn, on, head + 9, order, head[8]);
  else interpolate<1>(coef, out, c, sn, on, head + 9, order, head[8]);
  FILE* fo = fopen(argv[2], "wb");
  if (!fo || fwrite(coef, sizeof(double), c * svox, fo) != c * svox || fwrite(out, sizeof(double), c * ovox, fo) != c * ovox) return 4;
  fclose(fo);
  free(coef); free(out);
  return 0;
}
