// DTI relative-error table (reference: src/eval.py:154-192 `calc_diff_maps`, :217-317 `calc_error_table` /
// `do_calc_error_avg`): predicted and true tensors -> 12 post-processed relative-error maps (dti_errors_core.h)
// -> per-ROI probseg-weighted means.  Two launches, no atomics, no host synchronisation:
//   pass 1: lanes own voxels (grid-stride); per voxel two f64 eigen-decompositions and 12 diffs, 13 * R f64
//           sums per lane (R weight sums + 12 R weighted column sums); wave butterfly, then the four waves in
//           a fixed order; one partial row of 13 R doubles per block into the workspace.
//   pass 2: one block per ROI sums the partial rows in a fixed order and divides.
// The result is bit-identical from run to run.  Voxels outside the mask contribute exactly 0 (weight 0, all
// columns 0) and skip the decompositions.
#include "common.h"
#include "dti_errors_core.h"

namespace {

constexpr int kErrBlock = 256;
constexpr int kErrMaxBlocks = 2048;
constexpr int kErrRow = DTI_ERR_COLS + 1;    // weight sum, then the 12 weighted column sums

struct ErrArgs {
  const void *pred, *target; long long cs, vs;
  const unsigned char* mask;
  const void* ps; long long prs, pvs;
  long long nvox;
  double scale, offset;
  double* part;
  void* maps[DTI_ERR_COLS];
  int write_maps;
};

int err_blocks(long long nvox) {
  const long long b = (nvox + kErrBlock - 1) / kErrBlock;
  return (int)(b < 1 ? 1 : (b > kErrMaxBlocks ? kErrMaxBlocks : b));
}

template <typename T, typename P, int R>
__global__ __launch_bounds__(kErrBlock) void dti_errors_partial_kernel(ErrArgs a) {
  constexpr int W = kErrRow * R;
  __shared__ double red[kErrBlock / 64][W];
  const T* pr = reinterpret_cast<const T*>(a.pred);
  const T* tg = reinterpret_cast<const T*>(a.target);
  const P* ps = reinterpret_cast<const P*>(a.ps);
  double acc[W];
#pragma unroll
  for (int k = 0; k < W; ++k) acc[k] = 0.0;
  for (long long v = (long long)blockIdx.x * kErrBlock + threadIdx.x; v < a.nvox; v += (long long)gridDim.x * kErrBlock) {
    double col[DTI_ERR_COLS];
    const bool in = a.mask[v] != 0;
    if (in) {
      double p[6], t[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        p[i] = (double)pr[v * a.vs + i * a.cs];
        t[i] = (double)tg[v * a.vs + i * a.cs];
      }
      dti_error_voxel(p, t, a.scale, a.offset, col);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const double w = dti_roi_weight(true, (double)ps[v * a.pvs + r * a.prs]);
        acc[r * kErrRow] += w;
#pragma unroll
        for (int c = 0; c < DTI_ERR_COLS; ++c) acc[r * kErrRow + 1 + c] += w * col[c];   // 0 * NaN = NaN, as in numpy
      }
    } else {
#pragma unroll
      for (int c = 0; c < DTI_ERR_COLS; ++c) col[c] = 0.0;
    }
    if (a.write_maps) {
#pragma unroll
      for (int c = 0; c < DTI_ERR_COLS; ++c) reinterpret_cast<T*>(a.maps[c])[v] = (T)col[c];
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < W; ++k) {
    double s = acc[k];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < W) {
    double s = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kErrBlock / 64; ++w) s += red[w][threadIdx.x];
    a.part[(long long)blockIdx.x * W + threadIdx.x] = s;
  }
}

__device__ __forceinline__ double err_block_sum(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// block r: the 13 sums of ROI r over `nparts` partial rows of `width` doubles, then table[r][c] = S_c / W
__global__ __launch_bounds__(kErrBlock) void dti_errors_final_kernel(const double* __restrict__ part, int nparts, int width,
                                                                      double* __restrict__ table) {
  __shared__ double red[kErrBlock / 64];
  double tot[kErrRow];
  const double* p = part + blockIdx.x * kErrRow;
#pragma unroll
  for (int j = 0; j < kErrRow; ++j) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += kErrBlock) s += p[(long long)i * width + j];
    tot[j] = err_block_sum(s, red);
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < DTI_ERR_COLS; ++c) table[blockIdx.x * DTI_ERR_COLS + c] = tot[1 + c] / tot[0];   // 0/0 -> NaN like numpy
  }
}

template <typename T, typename P>
void launch_partial(const ErrArgs& a, int nroi, int blocks, hipStream_t s) {
  switch (nroi) {
    case 1: dti_errors_partial_kernel<T, P, 1><<<blocks, kErrBlock, 0, s>>>(a); break;
    case 2: dti_errors_partial_kernel<T, P, 2><<<blocks, kErrBlock, 0, s>>>(a); break;
    case 3: dti_errors_partial_kernel<T, P, 3><<<blocks, kErrBlock, 0, s>>>(a); break;
    default: dti_errors_partial_kernel<T, P, 4><<<blocks, kErrBlock, 0, s>>>(a); break;
  }
}

}  // namespace

extern "C" int64_t mi355_dti_errors_workspace_bytes(int64_t nvox, int32_t nroi) {
  if (nvox < 0 || nroi < 1 || nroi > DTI_ERR_MAX_ROI) return -1;
  return (int64_t)err_blocks(nvox) * kErrRow * nroi * (int64_t)sizeof(double);
}

extern "C" int mi355_dti_errors(const void* pred, const void* target, int32_t dtype, int64_t comp_stride,
                                int64_t vox_stride, const uint8_t* mask, const void* probseg, int32_t probseg_dtype,
                                int64_t roi_stride, int64_t probseg_vox_stride, int64_t nvox, int32_t nroi, double scale,
                                double offset, void* workspace, int64_t workspace_bytes, double* table_out,
                                void* const* maps, void* stream) {
  MI355_REQUIRE(dtype == MI355_DT_F32 || dtype == MI355_DT_F64, "dti_errors: pred/target dtype must be f32 or f64");
  MI355_REQUIRE(probseg_dtype == MI355_DT_F32 || probseg_dtype == MI355_DT_F64, "dti_errors: probseg dtype must be f32 or f64");
  MI355_REQUIRE(nroi >= 1 && nroi <= DTI_ERR_MAX_ROI, "dti_errors: %d tissue maps, supported 1..%d", (int)nroi, DTI_ERR_MAX_ROI);
  MI355_REQUIRE(nvox >= 0 && nvox < (1ll << 40), "dti_errors: bad voxel count %lld", (long long)nvox);
  MI355_REQUIRE(comp_stride > 0 && vox_stride > 0 && roi_stride > 0 && probseg_vox_stride > 0,
                "dti_errors: strides must be positive");
  MI355_REQUIRE(workspace && table_out, "dti_errors: null workspace or table");
  MI355_REQUIRE(workspace_bytes >= mi355_dti_errors_workspace_bytes(nvox, nroi), "dti_errors: workspace too small (%lld < %lld bytes)",
                (long long)workspace_bytes, (long long)mi355_dti_errors_workspace_bytes(nvox, nroi));
  ErrArgs a{};
  a.pred = pred; a.target = target; a.cs = comp_stride; a.vs = vox_stride;
  a.mask = mask; a.ps = probseg; a.prs = roi_stride; a.pvs = probseg_vox_stride;
  a.nvox = nvox; a.scale = scale; a.offset = offset;
  a.part = (double*)workspace;
  a.write_maps = maps != nullptr && nvox > 0;
  if (nvox > 0) MI355_REQUIRE(pred && target && mask && probseg, "dti_errors: null input pointer");
  if (a.write_maps) {
    for (int c = 0; c < DTI_ERR_COLS; ++c) {
      MI355_REQUIRE(maps[c], "dti_errors: null pointer for diff map %d", c);
      a.maps[c] = maps[c];
    }
  }
  const int blocks = err_blocks(nvox);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MI355_DT_F32) {
    if (probseg_dtype == MI355_DT_F32) launch_partial<float, float>(a, nroi, blocks, s);
    else launch_partial<float, double>(a, nroi, blocks, s);
  } else {
    if (probseg_dtype == MI355_DT_F32) launch_partial<double, float>(a, nroi, blocks, s);
    else launch_partial<double, double>(a, nroi, blocks, s);
  }
  dti_errors_final_kernel<<<nroi, kErrBlock, 0, s>>>((const double*)workspace, blocks, kErrRow * nroi, table_out);
  return mi355_check_launch("dti_errors");
}
