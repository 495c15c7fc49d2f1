// Host build of the preprocessing kernels' per-voxel arithmetic (csrc/dtifit_core.h) for the CPU test-suite.
// in : design [n][7], pinv [7][n], signals [nvox][n], raw phases [nphase]            (doubles)
// out: OLS beta [nvox][7], WLS beta [nvox][7], WLS fell back [nvox], phases [nphase]  (doubles)
// The loop is the kernel's: one pass over the measurements, 7 (+ 28 + 7) sums per voxel.  Test harness only.
#include <stdio.h>
#include <stdlib.h>
#include "../unet_bssfp_amd/csrc/dtifit_core.h"
int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const long nvox = atol(argv[3]), n = atol(argv[4]), nphase = atol(argv[5]);
  if (nvox < 1 || n < 7 || n > 512 || nphase < 0) return 2;
  const size_t nin = (size_t)(14 * n + nvox * n + nphase), nout = (size_t)(15 * nvox + nphase);
  double* in = (double*)malloc(sizeof(double) * nin);
  double* out = (double*)malloc(sizeof(double) * nout);
  if (!in || !out) return 5;
  FILE* fi = fopen(argv[1], "rb"); if (!fi || fread(in, sizeof(double), nin, fi) != nin) return 3; fclose(fi);
  const double *design = in, *pinv = in + 7 * n, *sig = in + 14 * n, *raw = sig + nvox * n;
  double *ols = out, *wls = out + 7 * nvox, *fell = out + 14 * nvox, *ph = out + 15 * nvox;
  for (long v = 0; v < nvox; ++v) {
    double beta[DTIFIT_NP];
    DtiFitWls w;
    dtifit_ols_init(beta);
    dtifit_wls_init(w);
    for (long m = 0; m < n; ++m) {
      double prow[DTIFIT_NP];
      for (int j = 0; j < DTIFIT_NP; ++j) prow[j] = pinv[j * n + m];
      const double s = sig[v * n + m], y = dtifit_logsig(s);
      dtifit_ols_step(beta, prow, y);
      dtifit_wls_step(w, design + 7 * m, s, y);
    }
    for (int j = 0; j < DTIFIT_NP; ++j) ols[7 * v + j] = beta[j];
    fell[v] = dtifit_wls_solve(w, beta) ? 0.0 : 1.0;
    for (int j = 0; j < DTIFIT_NP; ++j) wls[7 * v + j] = beta[j];
  }
  for (long i = 0; i < nphase; ++i) ph[i] = prep_phase(raw[i]);
  FILE* fo = fopen(argv[2], "wb"); if (!fo || fwrite(out, sizeof(double), nout, fo) != nout) return 4; fclose(fo);
  free(in); free(out);
  return 0;
}
