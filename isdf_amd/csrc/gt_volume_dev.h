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

}  // namespace isdf
