// Rendered views of the map: the sample generation and the normal pass of Trainer.render_depth_vis /
// render_normals_vis / latest_frame_vis (trainer.py:1055-1147,1225-1280).  The network runs through the library's own
// forward (isdf_sdf_eval's chain), the first crossing through render_depth_kernel (ingest.hip); this file holds the rest:
//   transform.origin_dirs_W                 isdf/geometry/transform.py:36-41
//   sample.stratified_sample                isdf/modules/sample.py:77-128   (n_stratified_samples bins, no surface samples)
//   sample.sample_along_rays (pc)           isdf/modules/sample.py:131-178
//   render.render_normals                   isdf/modules/render.py:38-57
// plus the two resamplings the trainer puts in front of a pass: cv2.resize(INTER_LINEAR) of a keyframe's depth
// (trainer.py:1239-1241) and F.interpolate(bilinear, align_corners=True) of the coarse pass (trainer.py:1105-1109).
// Arithmetic is the reference's, operation by operation; the file is built with -ffp-contract=off (build.py), so no
// multiply-add is fused.
#include "isdf_common.h"
#include "launchers.h"

namespace isdf {

// OpenCV INTER_LINEAR source coordinate of output index d (src = (d + 0.5) * scale - 0.5, scale = n_src / n_dst computed in
// double and the coordinate rounded to float; clamped at both borders, where the weight of the second tap becomes 0)
__device__ __forceinline__ void cv_linear_tap(int d, int n_src, int n_dst, int& s0, int& s1, float& f) {
  const double scale = 1.0 / ((double)n_dst / (double)n_src);
  float x = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(x);
  x -= (float)s;
  if (s < 0) { s = 0; x = 0.f; }
  if (s >= n_src - 1) { s = n_src - 1; x = 0.f; }
  s0 = s; s1 = s + 1 < n_src ? s + 1 : n_src - 1; f = x;
}

// torch upsample_bilinear2d(align_corners=True) source index / weight of output index d
__device__ __forceinline__ void ac_linear_tap(int d, int n_src, int n_dst, int& s0, int& s1, float& f) {
  const float scale = n_dst > 1 ? (float)(n_src - 1) / (float)(n_dst - 1) : 0.f;
  const float x = __fmul_rn(scale, (float)d);
  int s = (int)floorf(x);
  if (s > n_src - 1) s = n_src - 1;
  const float l = fminf(fmaxf(__fadd_rn(x, -(float)s), 0.f), 1.f);
  s0 = s; s1 = s < n_src - 1 ? s + 1 : s; f = l;
}

// (row 0 blend) * (1 - fy) + (row 1 blend) * fy: OpenCV's horizontal-then-vertical pass and torch's nested form alike
__device__ __forceinline__ float bilerp(const float* __restrict__ img, int W, int y0, int y1, float fy, int x0, int x1, float fx) {
  const float ax = __fadd_rn(1.f, -fx), ay = __fadd_rn(1.f, -fy);
  const float r0 = __fadd_rn(__fmul_rn(img[(int64_t)y0 * W + x0], ax), __fmul_rn(img[(int64_t)y0 * W + x1], fx));
  const float r1 = __fadd_rn(__fmul_rn(img[(int64_t)y1 * W + x0], ax), __fmul_rn(img[(int64_t)y1 * W + x1], fx));
  return __fadd_rn(__fmul_rn(r0, ay), __fmul_rn(r1, fy));
}

// origin and world-frame direction of ray r of view b (transform.py:36-41: (R * d).sum(-1), no fused multiply-add)
__device__ __forceinline__ void ray_W(const float* __restrict__ T, const float* __restrict__ dirs_C, int64_t r, float o[3],
                                      float d[3]) {
  const float dx = dirs_C[r * 3], dy = dirs_C[r * 3 + 1], dz = dirs_C[r * 3 + 2];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    d[i] = __fadd_rn(__fadd_rn(__fmul_rn(T[i * 4], dx), __fmul_rn(T[i * 4 + 1], dy)), __fmul_rn(T[i * 4 + 2], dz));
    o[i] = T[i * 4 + 3];
  }
}

// One thread per sample point n = (b * R + r) * S + s: the ray's depth range from its source, the bin's lower limit, the
// uniform (injected or Philox), z and pc.  Per-ray work (a 4-tap resample, nine products) is repeated per sample: it reads
// L1-resident data and the pass is store-bound (16 B per point).
__global__ __launch_bounds__(256) void render_samples_kernel(const isdf_render_args a, int64_t n_points, float* __restrict__ z_out,
                                                             float* __restrict__ pc_out) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_points) return;
  const int S = a.n_samples;
  const int64_t R = (int64_t)a.H * a.W;
  const int64_t ray = n / S;
  const int s = (int)(n - ray * S);
  const int b = (int)(ray / R);
  const int64_t r = ray - (int64_t)b * R;
  const int i = (int)(r / a.W), j = (int)(r - (int64_t)i * a.W);

  float lim, blen;
  if (a.range_mode == ISDF_RANGE_SCALAR) {
    // torch.linspace(min, max, S + 1)[s] (two-sided, step in fp32), bin_length the host's double rounded to fp32
    const float step = __fadd_rn(a.max_depth, -a.min_depth) / (float)S;
    lim = s < (S + 1) / 2 ? __fadd_rn(a.min_depth, __fmul_rn(step, (float)s))
                          : __fadd_rn(a.max_depth, -__fmul_rn(step, (float)(S - s)));
    blen = a.bin_length;
  } else {
    float lo, hi;
    const float* src = a.src_depth + (int64_t)b * a.src_H * a.src_W;
    int y0, y1, x0, x1;
    float fy, fx;
    if (a.range_mode == ISDF_RANGE_DEPTH) {    // [min_depth, resize(depth) + 0.8]  (trainer.py:1239-1246)
      cv_linear_tap(i, a.src_H, a.H, y0, y1, fy);
      cv_linear_tap(j, a.src_W, a.W, x0, x1, fx);
      lo = a.min_depth;
      hi = __fadd_rn(bilerp(src, a.src_W, y0, y1, fy, x0, x1, fx), a.depth_offset);
    } else {                                   // [d - 0.1, d + 0.1] around the align-corners upsample (trainer.py:1105-1119)
      ac_linear_tap(i, a.src_H, a.H, y0, y1, fy);
      ac_linear_tap(j, a.src_W, a.W, x0, x1, fx);
      const float d = bilerp(src, a.src_W, y0, y1, fy, x0, x1, fx);
      lo = __fadd_rn(d, -a.depth_offset);
      hi = __fadd_rn(d, a.depth_offset);
    }
    // torch.linspace(0, 1, S + 1)[s] * (max - min) + min, bin_length = (max - min) / S  (sample.py:94-105)
    const float stp = 1.f / (float)S;
    const float lin = s < (S + 1) / 2 ? __fmul_rn(stp, (float)s) : __fadd_rn(1.f, -__fmul_rn(stp, (float)(S - s)));
    const float range = __fadd_rn(hi, -lo);
    lim = __fadd_rn(__fmul_rn(lin, range), lo);
    blen = range / (float)S;
  }
  float U;
  if (a.rng_mode == 0) {
    U = a.draw_u[n];
  } else {   // Philox4x32-10, counter (ray group, view, render counter): one call per four consecutive samples of a ray
    const uint4 w = philox4x32_10(make_uint4((uint32_t)(r * ((S + 3) / 4) + s / 4), (uint32_t)b, (uint32_t)a.counter,
                                             (uint32_t)(a.counter >> 32)),
                                  make_uint2((uint32_t)a.seed, (uint32_t)(a.seed >> 32)));
    const int q = s & 3;
    U = u01(q == 0 ? w.x : (q == 1 ? w.y : (q == 2 ? w.z : w.w)));
  }
  const float z = __fadd_rn(lim, __fmul_rn(U, blen));          // sample.py:123-126
  float o[3], d[3];
  ray_W(a.T_WC + (int64_t)b * 16, a.dirs_C, r, o, d);
  z_out[n] = z;
#pragma unroll
  for (int k = 0; k < 3; ++k) pc_out[n * 3 + k] = __fadd_rn(o[k], __fmul_rn(d[k], z));   // sample.py:176
}

// render_normals, first half (render.py:39-43): the point at the ray's depth (a ray with depth 0 gives its origin)
__global__ __launch_bounds__(256) void normal_points_kernel(const float* __restrict__ T_WC, const float* __restrict__ dirs_C,
                                                            int64_t R, int64_t n_rays, const float* __restrict__ depth,
                                                            float* __restrict__ pts) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_rays) return;
  const int64_t b = n / R, r = n - b * R;
  float o[3], d[3];
  ray_W(T_WC + b * 16, dirs_C, r, o, d);
  const float z = depth[n];
#pragma unroll
  for (int k = 0; k < 3; ++k) pts[n * 3 + k] = __fadd_rn(o[k], __fmul_rn(d[k], z));
}

// render_normals, second half (render.py:44-55): n_W = -g / (|g| + 1e-4), n_C = R_CW n_W with R_CW the general inverse of
// the pose's 3x3 block (tracked poses are not exactly orthonormal, so not its transpose): adjugate / determinant in double,
// rounded to fp32 like torch's fp32 inverse
__global__ __launch_bounds__(256) void normal_finish_kernel(const float* __restrict__ T_WC, int64_t R, int64_t n_rays,
                                                            const float* __restrict__ grad, float* __restrict__ normals) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_rays) return;
  const float* T = T_WC + (n / R) * 16;
  double m[9], cof[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) m[q] = (double)T[(q / 3) * 4 + q % 3];
#pragma unroll
  for (int rr = 0; rr < 3; ++rr)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int r1 = (rr + 1) % 3, r2 = (rr + 2) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
      cof[3 * rr + c] = m[3 * r1 + c1] * m[3 * r2 + c2] - m[3 * r1 + c2] * m[3 * r2 + c1];
    }
  const double det = m[0] * cof[0] + m[1] * cof[1] + m[2] * cof[2];
  const float gx = grad[n * 3], gy = grad[n * 3 + 1], gz = grad[n * 3 + 2];
  const float den = __fadd_rn(sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy)), __fmul_rn(gz, gz))), 1e-4f);
  const float w0 = -gx / den, w1 = -gy / den, w2 = -gz / den;
#pragma unroll
  for (int rr = 0; rr < 3; ++rr) {   // inverse[rr][c] = cof[c][rr] / det
    const float i0 = (float)(cof[rr] / det), i1 = (float)(cof[3 + rr] / det), i2 = (float)(cof[6 + rr] / det);
    normals[n * 3 + rr] = __fadd_rn(__fadd_rn(__fmul_rn(i0, w0), __fmul_rn(i1, w1)), __fmul_rn(i2, w2));
  }
}

int launch_render_samples(const isdf_render_args& a, float* z, float* pc, hipStream_t st) {
  const int64_t n = (int64_t)a.n_views * a.H * a.W * a.n_samples;
  hipLaunchKernelGGL(render_samples_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, n, z, pc);
  return isdf_launch_status();
}

int launch_normal_points(const float* T_WC, const float* dirs_C, int64_t R, int64_t n_rays, const float* depth, float* pts,
                         hipStream_t st) {
  hipLaunchKernelGGL(normal_points_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, st, T_WC, dirs_C, R, n_rays,
                     depth, pts);
  return isdf_launch_status();
}

int launch_normal_finish(const float* T_WC, int64_t R, int64_t n_rays, const float* grad, float* normals, hipStream_t st) {
  hipLaunchKernelGGL(normal_finish_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, st, T_WC, R, n_rays, grad,
                     normals);
  return isdf_launch_status();
}

}  // namespace isdf
