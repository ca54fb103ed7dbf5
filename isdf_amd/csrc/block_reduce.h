// THE reduction order of the record kernels (sdf_metrics, region_metrics, nn_distance, pose_system, traj_step, tri_distance):
// the 64 lanes of a wave by shuffle, offsets 32, 16, .., 1; the four waves of a 256-thread block in wave order; one partial per
// block; the partials by reduce.hip (or, per pose, pose.hip's serial close).  include/isdf_hip.h promises the resulting bytes, and
// tests/reduce_model.py restates the order for the exact tests: a change here changes every record.
#pragma once
#include "isdf_common.h"

namespace isdf {

struct RedSum {
  template <typename T> static __device__ __forceinline__ T two(T a, T b) { return a + b; }
  template <typename T> static __device__ __forceinline__ T four(T a, T b, T c, T d) { return ((a + b) + c) + d; }
};
struct RedMin {
  static __device__ __forceinline__ double two(double a, double b) { return fmin(a, b); }
  static __device__ __forceinline__ double four(double a, double b, double c, double d) { return fmin(fmin(a, b), fmin(c, d)); }
};
struct RedMax {
  static __device__ __forceinline__ double two(double a, double b) { return fmax(a, b); }
  static __device__ __forceinline__ double four(double a, double b, double c, double d) { return fmax(fmax(a, b), fmax(c, d)); }
};

// lane 0 of each wave receives the wave's result
template <typename Op, typename T>
__device__ __forceinline__ T wave_reduce(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = Op::two(v, __shfl_down(v, o, 64));
  return v;
}

// the four waves' results a, b, c, d (wave order) into the block's
template <typename Op, typename T>
__device__ __forceinline__ T waves_combine(T a, T b, T c, T d) {
  return Op::four(a, b, c, d);
}

// the tail of an all-sum record: acc[v] of the block's 256 threads summed into out[v], v < N, through sh (one barrier)
template <int N>
__device__ __forceinline__ void block_record_sum(const double (&acc)[N], double (*sh)[N], double* __restrict__ out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int v = 0; v < N; ++v) {
    const double t = wave_reduce<RedSum>(acc[v]);
    if (lane == 0) sh[wave][v] = t;
  }
  __syncthreads();
  if (threadIdx.x < N)
    out[threadIdx.x] = waves_combine<RedSum>(sh[0][threadIdx.x], sh[1][threadIdx.x], sh[2][threadIdx.x], sh[3][threadIdx.x]);
}

}  // namespace isdf
