// SDF slice images (Trainer.compute_slices / obj_slices_vis / get_sdf_grid_pc, trainer.py:1446-1481,1558-1707,1775-1815)
// after the network, in ONE pass over the points:
//   ScalarMappable.to_rgba(v, bytes=False) then (.. * 255).astype(uint8)[..., :3]   the colour of a value, by table
//   sdf_util.eval_sdf_interp(handle_oob='fill')    isdf/datasets/sdf_util.py:183-216  (gt_volume_dev.h, shared with eval.hip)
//   metrics.chomp_cost on a float32 array          isdf/eval/metrics.py:95-104
// and the points of a plane (isdf_plane_points).  Built with -ffp-contract=off (build.py): every operation below is rounded to
// fp32 on its own, so numpy float32 models (tests/slice_model.py) equal the colour index, the cost and the points bit for bit.
#include "isdf_common.h"
#include "launchers.h"
#include "gt_volume_dev.h"

namespace isdf {

// matplotlib's Normalize on a float32 array, then Colormap.__call__: x = ((v - vmin) / range) * N in fp32 (a true division);
// NaN -> bad, x < 0 -> under, x == N -> N - 1, x > N -> over, else the truncated x.  lut: N colours, then under, over, bad.
__device__ __forceinline__ uint32_t colour_of(const uint32_t* lut, int N, float vmin, float range, float v) {
  const float fN = (float)N;
  const float x = __fmul_rn(__fdiv_rn(__fsub_rn(v, vmin), range), fN);
  const bool inside = x >= 0.f && x < fN;                 // false for NaN
  int k = (int)(inside ? x : 0.f);
  k = x == fN ? N - 1 : k;
  k = x < 0.f ? N : k;
  k = x > fN ? N + 1 : k;
  k = x != x ? N + 2 : k;
  return lut[k];
}

// metrics.chomp_cost in float32, numpy's order: -s + e/2; where s > 0: (1/(2e)) * ((s - e) * (s - e)); where s > e: 0
__device__ __forceinline__ float chomp32(float s, float eps, float half_eps, float inv_2eps) {
  float c = __fadd_rn(-s, half_eps);
  const float d = __fsub_rn(s, eps);
  if (s > 0.f) c = __fmul_rn(inv_2eps, __fmul_rn(d, d));
  if (s > eps) c = 0.f;
  return c;
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// four consecutive floats of thread quad q: one 16-byte access where the quad is whole and the base aligned, else one by one
__device__ __forceinline__ void load4(const float* __restrict__ src, int64_t i0, int cnt, float v[4]) {
  if (cnt == 4 && aligned16(src)) {
    const float4 t = *reinterpret_cast<const float4*>(src + i0);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < cnt ? src[i0 + j] : 0.f;
  }
}

__device__ __forceinline__ void store4(float* __restrict__ dst, int64_t i0, int cnt, const float v[4]) {
  if (cnt == 4 && aligned16(dst)) {
    *reinterpret_cast<float4*>(dst + i0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) dst[i0 + j] = v[j];
  }
}

// the 12 colour bytes of four consecutive points (c = R | G << 8 | B << 16): three dwords where the quad is whole and the
// base dword-aligned (12 * q then is too), else byte by byte
__device__ __forceinline__ void store_rgb4(uint8_t* __restrict__ dst, int64_t i0, int cnt, const uint32_t c[4]) {
  if (cnt == 4 && ((uintptr_t)dst & 3) == 0) {
    uint32_t* o = reinterpret_cast<uint32_t*>(dst + i0 * 3);
    o[0] = c[0] | (c[1] << 24);
    o[1] = (c[1] >> 8) | (c[2] << 16);
    o[2] = (c[2] >> 16) | (c[3] << 8);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) {
        uint8_t* o = dst + (i0 + j) * 3;
        o[0] = (uint8_t)c[j]; o[1] = (uint8_t)(c[j] >> 8); o[2] = (uint8_t)(c[j] >> 16);
      }
  }
}

// Thread q of the grid owns points 4q .. 4q + 3.  The colour table sits in LDS (a few hundred entries, read at a
// data-dependent index: from global memory that would be a divergent load per lane and output).
template <bool GT>
__global__ __launch_bounds__(256) void slice_images_kernel(const isdf_colormap cm, const isdf_gt_volume vol,
                                                           const float* __restrict__ pts, const float* __restrict__ sdf,
                                                           int64_t n, float oob_fill, float eps, float half_eps, float inv_2eps,
                                                           uint8_t* __restrict__ pred_rgb, float* __restrict__ gt_out,
                                                           uint8_t* __restrict__ gt_rgb, float* __restrict__ pred_cost,
                                                           float* __restrict__ gt_cost) {
  extern __shared__ uint32_t lut[];
  const int N = cm.n_colors;
  if (cm.lut)
    for (int k = threadIdx.x; k < N + 3; k += 256) lut[k] = cm.lut[k] & 0xffffffu;
  __syncthreads();
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= n) return;
  const int cnt = n - i0 < 4 ? (int)(n - i0) : 4;
  uint32_t c[4];
  float v[4];
  if (sdf) {
    float s[4];
    load4(sdf, i0, cnt, s);
    if (pred_rgb) {
#pragma unroll
      for (int j = 0; j < 4; ++j) c[j] = colour_of(lut, N, cm.vmin, cm.range, s[j]);
      store_rgb4(pred_rgb, i0, cnt, c);
    }
    if (pred_cost) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = chomp32(s[j], eps, half_eps, inv_2eps);
      store4(pred_cost, i0, cnt, v);
    }
  }
  if (GT) {
    float p[12], g[4];
    if (cnt == 4 && aligned16(pts)) {                     // 48 bytes per thread: three 16-byte loads
      const float4* src = reinterpret_cast<const float4*>(pts + i0 * 3);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float4 t = src[j];
        p[4 * j] = t.x; p[4 * j + 1] = t.y; p[4 * j + 2] = t.z; p[4 * j + 3] = t.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 12; ++j) p[j] = j < 3 * cnt ? pts[i0 * 3 + j] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bool inb;
      g[j] = gt_trilinear(vol, p[3 * j], p[3 * j + 1], p[3 * j + 2], oob_fill, &inb);
    }
    if (gt_out) store4(gt_out, i0, cnt, g);
    if (gt_rgb) {
#pragma unroll
      for (int j = 0; j < 4; ++j) c[j] = colour_of(lut, N, cm.vmin, cm.range, g[j]);
      store_rgb4(gt_rgb, i0, cnt, c);
    }
    if (gt_cost) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = chomp32(g[j], eps, half_eps, inv_2eps);
      store4(gt_cost, i0, cnt, v);
    }
  }
}

struct PlaneArgs { float origin[3], du[3], dv[3]; };

// p[i][j] = (origin + (float)i * du) + (float)j * dv, thread q the four points 4q .. 4q + 3 of the row-major [H, W] raster
__global__ __launch_bounds__(256) void plane_points_kernel(const PlaneArgs a, uint32_t W, uint32_t total,
                                                           float* __restrict__ out) {
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= total) return;
  const int cnt = total - i0 < 4 ? (int)(total - i0) : 4;
  float p[12];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t idx = (uint32_t)i0 + k;               // (past the end in a partial quad: computed, never stored)
    const uint32_t i = idx / W, j = idx - i * W;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax)
      p[3 * k + ax] = __fadd_rn(__fadd_rn(a.origin[ax], __fmul_rn((float)i, a.du[ax])), __fmul_rn((float)j, a.dv[ax]));
  }
  if (cnt == 4 && aligned16(out)) {
    float4* dst = reinterpret_cast<float4*>(out + i0 * 3);
#pragma unroll
    for (int k = 0; k < 3; ++k) dst[k] = make_float4(p[4 * k], p[4 * k + 1], p[4 * k + 2], p[4 * k + 3]);
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k < 3 * cnt) out[i0 * 3 + k] = p[k];
  }
}

int launch_slice_images(const isdf_colormap* cmap, const isdf_gt_volume* vol, const float* pts, const float* sdf, int64_t n,
                        float oob_fill, float chomp_eps, uint8_t* pred_rgb, float* gt_out, uint8_t* gt_rgb, float* pred_cost,
                        float* gt_cost, hipStream_t st) {
  isdf_colormap cm = {};
  if (cmap) cm = *cmap;
  isdf_gt_volume v = {};
  if (vol) v = *vol;
  const size_t lds = cmap ? (size_t)(cm.n_colors + 3) * 4 : 0;
  const int64_t blocks = ((n + 3) / 4 + 255) / 256;
  // numpy's scalars: epsilon / 2. and 1 / (2 * epsilon) are Python floats, rounded to float32 where they meet the array
  const float half_eps = (float)((double)chomp_eps / 2.0), inv_2eps = chomp_eps > 0.f ? (float)(1.0 / (2.0 * (double)chomp_eps)) : 0.f;
  if (vol)
    hipLaunchKernelGGL(slice_images_kernel<true>, dim3((unsigned)blocks), dim3(256), lds, st, cm, v, pts, sdf, n, oob_fill,
                       chomp_eps, half_eps, inv_2eps, pred_rgb, gt_out, gt_rgb, pred_cost, gt_cost);
  else
    hipLaunchKernelGGL(slice_images_kernel<false>, dim3((unsigned)blocks), dim3(256), lds, st, cm, v, pts, sdf, n, oob_fill,
                       chomp_eps, half_eps, inv_2eps, pred_rgb, gt_out, gt_rgb, pred_cost, gt_cost);
  return isdf_launch_status();
}

int launch_plane_points(const float* origin, const float* du, const float* dv, int32_t H, int32_t W, float* pts_out,
                        hipStream_t st) {
  PlaneArgs a;
  for (int k = 0; k < 3; ++k) { a.origin[k] = origin[k]; a.du[k] = du[k]; a.dv[k] = dv[k]; }
  const int64_t total = (int64_t)H * W;
  const int64_t blocks = ((total + 3) / 4 + 255) / 256;
  hipLaunchKernelGGL(plane_points_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, (uint32_t)W, (uint32_t)total, pts_out);
  return isdf_launch_status();
}

}  // namespace isdf
