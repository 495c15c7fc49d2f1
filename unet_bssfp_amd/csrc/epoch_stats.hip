// Epoch statistics of a fit loop (unet_bssfp_amd/trainer.py): every `self.log(..., on_epoch=True, sync_dist=True)` of the
// reference (src/model.py:178, 205, 210, 218, 266, 276, 286) is an epoch mean of a scalar that lives in device memory and
// that the next graph replay overwrites.  One single-wave launch per step adds the step's scalars, times the batch weight,
// into f64 sums that stay on the device until the epoch ends: no host read per step, no stack / cat / add chain of
// scalar-sized torch launches.
//   acc[k]         += weight * *src[k]        k < n      (lane k)
//   acc[n]         += weight                             (lane n)
//   acc[n + 1 + k] += 1 where *src[k] is NaN or +-inf    (lane k)
// The source pointers travel by value in the kernel arguments (as the patch locations of patches.hip and the tensor
// pointers of mi355_adamw_multi do): no device table, so the launch can be recorded into a hipGraph.  Plain loads and
// stores of one lane per address: no atomics, no LDS, no workspace; two identical call sequences are bit-identical.
#include "common.h"

namespace {

__global__ __launch_bounds__(64) void epoch_accumulate_kernel(mi355_scalar_table t, int n, double weight,
                                                              double* __restrict__ acc) {
  const int k = threadIdx.x;
  if (k < n) {
    const float v = *t.src[k];
    acc[k] += weight * (double)v;                       // a non-finite v enters the sum as IEEE carries it ...
    if (!(fabsf(v) <= 3.402823466e+38f)) acc[n + 1 + k] += 1.0;   // ... and is counted (NaN fails every comparison)
  } else if (k == n) {
    acc[n] += weight;
  }
}

}  // namespace

extern "C" int mi355_epoch_accumulate(const mi355_scalar_table* table, int32_t n, double weight, double* acc, void* stream) {
  MI355_REQUIRE(table && acc, "epoch_accumulate: null pointer");
  MI355_REQUIRE(n >= 1 && n <= MI355_EPOCH_MAX_SCALARS, "epoch_accumulate: %d scalars, need 1..%d", n, MI355_EPOCH_MAX_SCALARS);
  mi355_scalar_table t;
  for (int k = 0; k < MI355_EPOCH_MAX_SCALARS; ++k) {
    MI355_REQUIRE(k >= n || table->src[k], "epoch_accumulate: null pointer (source %d)", k);
    t.src[k] = k < n ? table->src[k] : nullptr;         // lanes >= n read no source
  }
  epoch_accumulate_kernel<<<1, 64, 0, (hipStream_t)stream>>>(t, n, weight, acc);
  return mi355_check_launch("epoch_accumulate");
}
