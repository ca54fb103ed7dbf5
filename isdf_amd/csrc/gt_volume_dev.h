// Trilinear lookup of an isdf_gt_volume, shared by eval.hip (sdf_metrics_kernel) and slices.hip (slice_images_kernel): what
// scipy's linear RegularGridInterpolator computes on an evenly spaced grid (sdf_util.py:151-216), in fp32.  Both files are
// built with -ffp-contract=off (build.py); the blend asks for its fused multiply-adds by name, so the two kernels give the
// same bits for the same point.
#pragma once
#include "isdf_common.h"

namespace isdf {

// grid coordinate u = (p - origin) / spacing per axis; in bounds iff 0 <= u <= n - 1 on every axis (faces inclusive, NaN is out).
// Returns the interpolated value, oob_fill where the point is out of bounds; *inb says which.
__device__ __forceinline__ float gt_trilinear(const isdf_gt_volume& vol, float px, float py, float pz, float oob_fill,
                                              bool* inb_out) {
  const int nx = vol.nx, ny = vol.ny, nz = vol.nz;
  const float ux = (px - vol.origin[0]) / vol.spacing[0];
  const float uy = (py - vol.origin[1]) / vol.spacing[1];
  const float uz = (pz - vol.origin[2]) / vol.spacing[2];
  const bool inb = ux >= 0.f && ux <= (float)(nx - 1) && uy >= 0.f && uy <= (float)(ny - 1) && uz >= 0.f &&
                   uz <= (float)(nz - 1);
  float gt = oob_fill;
  if (inb) {
    // cell index clamped to [0, n - 2] (a point on the upper face interpolates inside the last cell with t = 1)
    const int ix = min((int)ux, nx - 2), iy = min((int)uy, ny - 2), iz = min((int)uz, nz - 2);
    const float tx = ux - (float)ix, ty = uy - (float)iy, tz = uz - (float)iz;
    const float* c = vol.values + ((int64_t)ix * ny + iy) * nz + iz;
    const int64_t sx = (int64_t)ny * nz, sy = nz;
    const float c00 = fmaf(tz, c[1] - c[0], c[0]);
    const float c01 = fmaf(tz, c[sy + 1] - c[sy], c[sy]);
    const float c10 = fmaf(tz, c[sx + 1] - c[sx], c[sx]);
    const float c11 = fmaf(tz, c[sx + sy + 1] - c[sx + sy], c[sx + sy]);
    const float c0 = fmaf(ty, c01 - c00, c00), c1 = fmaf(ty, c11 - c10, c10);
    gt = fmaf(tx, c1 - c0, c0);
  }
  *inb_out = inb;
  return gt;
}

// The same lookup in double, for isdf_region_metrics (eval.hip): the reference evaluates eval_pts.fixed_pts_eval's ground truth
// and its central differences in float64 on the fp32 points.  spacing / origin are the grid's doubles (the struct's own are
// fp32); the values are the volume's fp32 ones, widened.  Returns NaN out of bounds.
__device__ __forceinline__ double gt_trilinear_f64(const isdf_gt_volume& vol, const double* spacing, const double* origin,
                                                   double px, double py, double pz, bool* inb_out) {
  const int nx = vol.nx, ny = vol.ny, nz = vol.nz;
  const double ux = (px - origin[0]) / spacing[0];
  const double uy = (py - origin[1]) / spacing[1];
  const double uz = (pz - origin[2]) / spacing[2];
  const bool inb = ux >= 0.0 && ux <= (double)(nx - 1) && uy >= 0.0 && uy <= (double)(ny - 1) && uz >= 0.0 &&
                   uz <= (double)(nz - 1);
  double gt = __builtin_nan("");
  if (inb) {
    const int ix = min((int)ux, nx - 2), iy = min((int)uy, ny - 2), iz = min((int)uz, nz - 2);
    const double tx = ux - (double)ix, ty = uy - (double)iy, tz = uz - (double)iz;
    const float* c = vol.values + ((int64_t)ix * ny + iy) * nz + iz;
    const int64_t sx = (int64_t)ny * nz, sy = nz;
    const double v000 = c[0], v001 = c[1], v010 = c[sy], v011 = c[sy + 1];
    const double v100 = c[sx], v101 = c[sx + 1], v110 = c[sx + sy], v111 = c[sx + sy + 1];
    const double c00 = v000 + tz * (v001 - v000), c01 = v010 + tz * (v011 - v010);
    const double c10 = v100 + tz * (v101 - v100), c11 = v110 + tz * (v111 - v110);
    const double c0 = c00 + ty * (c01 - c00), c1 = c10 + ty * (c11 - c10);
    gt = c0 + tx * (c1 - c0);
  }
  *inb_out = inb;
  return gt;
}

}  // namespace isdf
