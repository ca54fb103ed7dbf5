// The per-pair sequence of the triangle-mesh kernels (include/isdf_hip.h: isdf_tri_distance), shared by the brute-force kernel
// (tri.hip) and the tile-culled one (tri_tiles.hip): both must produce the same bits per pair, so both include these functions and
// are built with the same flags (build.py: nothing contracted, nothing SLP-vectorised).
#pragma once
#include "isdf_common.h"

namespace isdf {

constexpr int TRI_Q = 4;                      // queries per thread
constexpr int TRI_TILE = ISDF_TRI_TILE;       // triangles per LDS tile
constexpr int TRI_SLOT = ISDF_TRI_SLOT_FLOATS;   // floats per packed triangle (six float4)
constexpr int TRI_REC = ISDF_TRI_RECORD;

// ---- the per-pair sequence (the header writes it out) ---------------------------------------------------------------------
struct TriCore { float ax, ay, az, a00, abx, aby, abz, a01, acx, acy, acz, a11, nx, ny, nz; };

// barycentric weights (v, w) of the point of the triangle nearest to p, from ap = p - a; face: that point is inside the triangle
__device__ __forceinline__ void tri_weights(const TriCore& t, float apx, float apy, float apz, float& v, float& w, bool& face) {
  const float d1 = (t.abx * apx + t.aby * apy) + t.abz * apz;
  const float d2 = (t.acx * apx + t.acy * apy) + t.acz * apz;
  const float d3 = d1 - t.a00, d4 = d2 - t.a01, d5 = d1 - t.a01, d6 = d2 - t.a11;
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const float e43 = d4 - d3, e56 = d5 - d6;
  // lowest priority first, so the last assignment that applies is the first region of the usual if-chain.  The edge tests are
  // strict: a point whose projection lies ON an edge line stays with the face (its plane distance is exact on axis-aligned faces)
  float den = (va + vb) + vc, nv = vb, nw = vc;                                             // face
  face = true;
  if (va < 0.f && e43 >= 0.f && e56 >= 0.f) { den = e43 + e56; nv = e56; nw = e43; face = false; }   // edge BC
  if (vb < 0.f && d2 >= 0.f && d6 <= 0.f) { den = d2 - d6; nv = 0.f; nw = d2; face = false; }        // edge AC
  if (d6 >= 0.f && d5 <= d6) { den = 1.f; nv = 0.f; nw = 1.f; face = false; }                         // vertex C
  if (vc < 0.f && d1 >= 0.f && d3 <= 0.f) { den = d1 - d3; nv = d1; nw = 0.f; face = false; }        // edge AB
  if (d3 >= 0.f && d4 <= d3) { den = 1.f; nv = 1.f; nw = 0.f; face = false; }                         // vertex B
  if (d1 <= 0.f && d2 <= 0.f) { den = 1.f; nv = 0.f; nw = 0.f; face = false; }                        // vertex A
  const float r = __fdiv_rn(1.f, den);
  v = nv * r;
  w = nw * r;
}

__device__ __forceinline__ float tri_dist2(const TriCore& t, float apx, float apy, float apz) {
  float v, w;
  bool face;
  tri_weights(t, apx, apy, apz, v, w, face);
  const float dx = apx - (t.abx * v + t.acx * w), dy = apy - (t.aby * v + t.acy * w), dz = apz - (t.abz * v + t.acz * w);
  // inside the triangle the distance is the one to its plane: exactly 0 on an axis-aligned face, where the in-plane residual
  // of v and w would leave 1e-7
  const float dn = (t.nx * apx + t.ny * apy) + t.nz * apz;
  return face ? dn * dn : (dx * dx + dy * dy) + dz * dz;
}

// solid angle of the triangle seen from p, with a, b, c the vertices minus the point (Van Oosterom and Strackee).  The lengths by
// the hardware square root (within one ulp): the winding number is compared with a float64 model, not bit for bit
__device__ __forceinline__ float tri_solid_angle(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy,
                                                 float cz) {
  const float la = __fsqrt_rn((ax * ax + ay * ay) + az * az), lb = __fsqrt_rn((bx * bx + by * by) + bz * bz),
              lc = __fsqrt_rn((cx * cx + cy * cy) + cz * cz);
  const float det = (ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz)) + az * (bx * cy - by * cx);
  const float ab = (ax * bx + ay * by) + az * bz, bc = (bx * cx + by * cy) + bz * cz, ca = (cx * ax + cy * ay) + cz * az;
  const float den = ((la * lb * lc + ab * lc) + bc * la) + ca * lb;
  return 2.f * atan2f(det, den);
}

}  // namespace isdf
