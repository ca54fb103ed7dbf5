// The closing launch of the record kernels (isdf_sdf_metrics, isdf_region_metrics, isdf_nn_distance, isdf_tri_distance): one block
// combines the per-block partial records in the fixed order of block_reduce.h.
#include "isdf_common.h"
#include "launchers.h"
#include "block_reduce.h"

namespace isdf {

// out[v], v < width <= 64 = the nPart partial records' column v: thread k takes partials k, k + 256, .. in ascending order, then
// the block's fixed order.  Bit v of max_mask: the column is a maximum (from 0.0) instead of a sum.
__global__ __launch_bounds__(256) void reduce_partials_kernel(const double* __restrict__ part, int64_t nPart, int width,
                                                              uint64_t max_mask, double* __restrict__ out) {
  __shared__ double sh[4];
  for (int v = 0; v < width; ++v) {
    const bool mx = (max_mask >> v) & 1u;
    double t = 0.0;
    for (int64_t b = threadIdx.x; b < nPart; b += 256) t = mx ? fmax(t, part[b * width + v]) : t + part[b * width + v];
    t = mx ? wave_reduce<RedMax>(t) : wave_reduce<RedSum>(t);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0)
      out[v] = mx ? waves_combine<RedMax>(sh[0], sh[1], sh[2], sh[3]) : waves_combine<RedSum>(sh[0], sh[1], sh[2], sh[3]);
  }
}

int launch_reduce_partials(const double* part, int64_t nPart, int width, uint64_t max_mask, double* out, hipStream_t st) {
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, st, part, nPart, width, max_mask, out);
  return isdf_launch_status();
}

}  // namespace isdf
