// Log-linear diffusion tensor fit per voxel (FSL DTIFIT's model; the thesis's DWI preprocessing, doc/thesis/03-methods.tex:661-668):
// ln S_i = ln S0 - b_i g_i^T D g_i, ordinary or signal-weighted least squares (dtifit_core.h).  A lane owns one voxel, or four
// adjacent ones when the series can be read 16 bytes at a time; it streams over the measurements with the pseudo-inverse (and,
// for WLS, the design matrix) in LDS, read as broadcasts.  State per voxel: 7 sums (OLS) or 28 + 7 + 7 (WLS), all f64, whatever
// the number of measurements.  HBM traffic: 4 N bytes in, 4 or 8 bytes per written output.
#include "common.h"
#include "dtifit_core.h"

namespace {

struct FitArgs {
  const float* dwi; long long nvox, ms, vs; int nmeas;
  const double* design; const double* pinv; const unsigned char* mask;
  void* tensor; long long ocs, ovs; void* s0;
  int has_norm; double lo[6], hi[6];
};

constexpr int kFitThreads = 256;

template <typename TO, int METHOD, int VPL>
__global__ __launch_bounds__(kFitThreads) void dtifit_kernel(FitArgs a) {
  extern __shared__ double fit_lds[];
  const int n = a.nmeas;
  double* lp = fit_lds;                    // [n][7]: row m = column m of pinv
  double* la = fit_lds + n * DTIFIT_NP;    // [n][7]: the design matrix (WLS only)
  for (int i = threadIdx.x; i < n * DTIFIT_NP; i += kFitThreads) {
    const int m = i / DTIFIT_NP, j = i - m * DTIFIT_NP;
    lp[i] = a.pinv[(long long)j * n + m];
    if (METHOD == MI355_DTIFIT_WLS) la[i] = a.design[i];
  }
  __syncthreads();
  const long long v0 = ((long long)blockIdx.x * kFitThreads + threadIdx.x) * VPL;
  if (v0 >= a.nvox) return;
  const bool full = v0 + VPL <= a.nvox;
  bool live[VPL];
  bool any = false;
#pragma unroll
  for (int k = 0; k < VPL; ++k) {
    live[k] = v0 + k < a.nvox && (!a.mask || a.mask[v0 + k] != 0);
    any = any || live[k];
  }
  double beta[VPL][DTIFIT_NP];
  DtiFitWls w[METHOD == MI355_DTIFIT_WLS ? VPL : 1];
#pragma unroll
  for (int k = 0; k < VPL; ++k) {
    dtifit_ols_init(beta[k]);
    if (METHOD == MI355_DTIFIT_WLS) dtifit_wls_init(w[k]);
  }
  if (any) {
    const float* src = a.dwi + v0 * a.vs;
    for (int m = 0; m < n; ++m) {
      float s[VPL];
      const float* p = src + (long long)m * a.ms;
      if (VPL == 4 && full) {              // vs == 1 and 16-byte aligned rows: checked by the host
        const float4 q = *reinterpret_cast<const float4*>(p);
        s[0] = q.x; s[1 % VPL] = q.y; s[2 % VPL] = q.z; s[3 % VPL] = q.w;
      } else {
#pragma unroll
        for (int k = 0; k < VPL; ++k) s[k] = v0 + k < a.nvox ? p[k * a.vs] : 0.f;
      }
      double row[DTIFIT_NP], arow[DTIFIT_NP];
#pragma unroll
      for (int j = 0; j < DTIFIT_NP; ++j) {
        row[j] = lp[m * DTIFIT_NP + j];
        if (METHOD == MI355_DTIFIT_WLS) arow[j] = la[m * DTIFIT_NP + j];
      }
#pragma unroll
      for (int k = 0; k < VPL; ++k) {
        const double y = dtifit_logsig((double)s[k]);
        dtifit_ols_step(beta[k], row, y);
        if (METHOD == MI355_DTIFIT_WLS) dtifit_wls_step(w[k], arow, (double)s[k], y);
      }
    }
  }
  TO* tensor = reinterpret_cast<TO*>(a.tensor);
  TO* s0 = reinterpret_cast<TO*>(a.s0);
#pragma unroll
  for (int k = 0; k < VPL; ++k) {
    const long long v = v0 + k;
    if (v >= a.nvox) break;
    if (live[k]) {
      if (METHOD == MI355_DTIFIT_WLS) dtifit_wls_solve(w[k], beta[k]);     // false: beta keeps the OLS solution
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const double d = a.has_norm ? prep_normalize(beta[k][c], a.lo[c], a.hi[c]) : beta[k][c];
        tensor[c * a.ocs + v * a.ovs] = (TO)d;
      }
      if (s0) s0[v] = (TO)exp(beta[k][6]);
    } else {
#pragma unroll
      for (int c = 0; c < 6; ++c) tensor[c * a.ocs + v * a.ovs] = (TO)0;
      if (s0) s0[v] = (TO)0;
    }
  }
}

template <typename TO, int METHOD, int VPL>
int launch_fit(const FitArgs& a, hipStream_t s) {
  const unsigned blocks = (unsigned)((a.nvox + (long long)kFitThreads * VPL - 1) / ((long long)kFitThreads * VPL));
  const size_t lds = (size_t)a.nmeas * DTIFIT_NP * sizeof(double) * (METHOD == MI355_DTIFIT_WLS ? 2 : 1);   // <= 56 KB
  dtifit_kernel<TO, METHOD, VPL><<<blocks, kFitThreads, lds, s>>>(a);
  return mi355_check_launch("dtifit");
}

}  // namespace

extern "C" int mi355_dtifit(const float* dwi, int64_t nvox, int32_t nmeas, int64_t meas_stride, int64_t vox_stride,
                            const double* design, const double* pinv, int32_t method, const uint8_t* mask, void* tensor,
                            int32_t out_dtype, int64_t out_comp_stride, int64_t out_vox_stride, void* s0, const double* norm,
                            void* stream) {
  MI355_REQUIRE(nmeas >= DTIFIT_NP && nmeas <= MI355_DTIFIT_MAX_MEAS, "dtifit: %d measurements, need 7 .. %d", (int)nmeas,
                MI355_DTIFIT_MAX_MEAS);
  MI355_REQUIRE(method == MI355_DTIFIT_OLS || method == MI355_DTIFIT_WLS, "dtifit: unknown method %d", (int)method);
  MI355_REQUIRE(out_dtype == MI355_DT_F32 || out_dtype == MI355_DT_F64, "dtifit: output dtype must be f32 or f64");
  MI355_REQUIRE(nvox >= 0 && nvox < (1ll << 36), "dtifit: bad voxel count %lld", (long long)nvox);
  MI355_REQUIRE(meas_stride > 0 && vox_stride > 0, "dtifit: input strides must be positive");
  MI355_REQUIRE(out_comp_stride > 0 && out_vox_stride > 0, "dtifit: output strides must be positive");
  MI355_REQUIRE(dwi && design && pinv && tensor, "dtifit: null pointer");
  FitArgs a{dwi, nvox, meas_stride, vox_stride, nmeas, design, pinv, mask, tensor, out_comp_stride, out_vox_stride, s0, 0, {}, {}};
  if (norm) {
    for (int c = 0; c < 6; ++c) {
      a.lo[c] = norm[2 * c];
      a.hi[c] = norm[2 * c + 1];
      MI355_REQUIRE(a.hi[c] > a.lo[c], "dtifit: normalisation range %d is empty or not finite", c);
    }
    a.has_norm = 1;
  }
  if (nvox == 0) return MI355_OK;
  hipStream_t s = (hipStream_t)stream;
  const bool f32 = out_dtype == MI355_DT_F32;
  if (method == MI355_DTIFIT_WLS)
    return f32 ? launch_fit<float, MI355_DTIFIT_WLS, 1>(a, s) : launch_fit<double, MI355_DTIFIT_WLS, 1>(a, s);
  const bool vec = vox_stride == 1 && meas_stride % 4 == 0 && ((uintptr_t)dwi & 15) == 0 && nvox >= 4;
  if (vec) return f32 ? launch_fit<float, MI355_DTIFIT_OLS, 4>(a, s) : launch_fit<double, MI355_DTIFIT_OLS, 4>(a, s);
  return f32 ? launch_fit<float, MI355_DTIFIT_OLS, 1>(a, s) : launch_fit<double, MI355_DTIFIT_OLS, 1>(a, s);
}
