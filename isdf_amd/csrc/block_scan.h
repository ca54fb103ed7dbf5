// The block-level scan the ordered compactions share (mesh.hip's vertex / face emit, band.hip's point lists): positions come from
// prefix sums, never from an atomic, so two runs write the same bytes.
#pragma once
#include "isdf_common.h"

namespace isdf {

// block-wide exclusive scan of one int per thread (NT threads, wave64); *total = the block's sum
template <int NT, typename T>
__device__ inline T block_exclusive_scan(T x, T* lds, T* total) {
  constexpr int NW = NT / 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T s = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T y = __shfl_up(s, o, 64);
    if (lane >= o) s += y;
  }
  if (lane == 63) lds[w] = s;
  __syncthreads();
  T off = 0, tot = 0;
#pragma unroll
  for (int q = 0; q < NW; ++q) {
    const T b = lds[q];
    off += q < w ? b : T(0);
    tot += b;
  }
  __syncthreads();      // lds is free again for the caller's next scan
  *total = tot;
  return off + s - x;
}

}  // namespace isdf
