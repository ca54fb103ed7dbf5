// Marching cubes over a dense fp32 volume (isdf_marching_cubes, include/isdf_hip.h): an indexed mesh with one vertex per
// sign-changing grid edge, in a deterministic order that no atomic decides.
//
//   count   one thread per grid point: the vertices it owns (its +i, +j, +k edges) and the triangles of the cell it is the
//           origin of; per-block sums
//   scan    one block: exclusive offsets of the per-block sums, the totals to the caller's counts[2]
//   verts   the block-level exclusive scan again, plus the block's offset: each point writes its vertices (axis order i < j < k)
//           and its first vertex id to the workspace
//   faces   likewise for the triangles; a triangle's edge (owner point q, axis a) is vertex vbase[q] + (vertices q owns on axes < a)
//
// Vertices are thereby ordered by owning point, then axis; faces by cell, then table order.  The two emit passes run only when
// the whole mesh fits the caller's buffers (they read the totals the scan left in the workspace), so no host round trip sits
// between the passes.  Every workspace word is written before it is read in the same call: the workspace needs no zeroing.
#include "isdf_common.h"
#include "launchers.h"
#include "block_scan.h"
#include "mc_tables.h"

namespace isdf {

namespace {

constexpr int MC_BLOCK = 256;     // threads (= grid points) per block of the count / emit passes
constexpr int MC_SCAN = 1024;     // threads of the one-block scan

struct McGeom {
  int32_t D0, D1, D2;
  int64_t P;              // points
  int64_t s0, s1;         // strides of i and j (k: 1)
  float level;
  int has_xf;
  float A[12];            // index -> world affine, rows of [3 x 4]
  float N[9];             // inverse transpose of A's 3x3 part, rows
};

struct McWs {
  int32_t* blockCnt;      // [nBlocks][2]  vertices, faces
  int64_t* blockOff;      // [nBlocks][2]  exclusive offsets
  int64_t* total;         // [2]
  int32_t* vbase;         // [P] first vertex id of each point
  int64_t nBlocks;
};

__device__ inline bool finite_f(float x) { return __builtin_isfinite(x); }

// the edge of point `idx` (coordinates i, j, k) along `axis` carries a vertex: in range, both ends finite, the sign changes
__device__ inline bool edge_vertex(const float* __restrict__ v, const McGeom& g, int64_t idx, int i, int j, int k, int axis, float f0) {
  int64_t nb;
  if (axis == 0) { if (i + 1 >= g.D0) return false; nb = idx + g.s0; }
  else if (axis == 1) { if (j + 1 >= g.D1) return false; nb = idx + g.s1; }
  else { if (k + 1 >= g.D2) return false; nb = idx + 1; }
  const float f1 = v[nb];
  return finite_f(f0) && finite_f(f1) && ((f0 < g.level) != (f1 < g.level));
}

__device__ inline void coords(const McGeom& g, int64_t idx, int& i, int& j, int& k) {
  i = (int)(idx / g.s0);
  const int64_t r = idx - (int64_t)i * g.s0;
  j = (int)(r / g.s1);
  k = (int)(r - (int64_t)j * g.s1);
}

// case index of the cell whose origin is (i, j, k), or -1: no cell there, or a corner is not finite
__device__ inline int cell_case(const float* __restrict__ v, const McGeom& g, int64_t idx, int i, int j, int k) {
  if (i + 1 >= g.D0 || j + 1 >= g.D1 || k + 1 >= g.D2) return -1;
  int c = 0;
  bool ok = true;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float f = v[idx + (q & 1 ? g.s0 : 0) + (q & 2 ? g.s1 : 0) + (q & 4 ? 1 : 0)];
    ok = ok && finite_f(f);
    c |= (f < g.level ? 1 : 0) << q;
  }
  return ok ? c : -1;
}

__device__ inline int point_vertices(const float* __restrict__ v, const McGeom& g, int64_t idx, int i, int j, int k) {
  const float f0 = v[idx];
  return (int)edge_vertex(v, g, idx, i, j, k, 0, f0) + (int)edge_vertex(v, g, idx, i, j, k, 1, f0) +
         (int)edge_vertex(v, g, idx, i, j, k, 2, f0);
}

__global__ __launch_bounds__(MC_BLOCK) void mc_count_kernel(const float* __restrict__ vol, McGeom g, McWs ws) {
  __shared__ int lds[MC_BLOCK / 64];
  const int64_t idx = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  int nv = 0, nf = 0;
  if (idx < g.P) {
    int i, j, k;
    coords(g, idx, i, j, k);
    nv = point_vertices(vol, g, idx, i, j, k);
    const int c = cell_case(vol, g, idx, i, j, k);
    nf = c < 0 ? 0 : (int)mc::kTriCount[c];
  }
  int tv, tf;
  block_exclusive_scan<MC_BLOCK>(nv, lds, &tv);
  block_exclusive_scan<MC_BLOCK>(nf, lds, &tf);
  if (threadIdx.x == 0) {
    ws.blockCnt[2 * blockIdx.x] = tv;
    ws.blockCnt[2 * blockIdx.x + 1] = tf;
  }
}

__global__ __launch_bounds__(MC_SCAN) void mc_scan_kernel(McWs ws, int64_t* __restrict__ counts) {
  __shared__ int64_t lds[MC_SCAN / 64];
  const int64_t per = (ws.nBlocks + MC_SCAN - 1) / MC_SCAN;
  const int64_t b0 = (int64_t)threadIdx.x * per;
  const int64_t b1 = b0 + per < ws.nBlocks ? b0 + per : ws.nBlocks;
  int64_t sv = 0, sf = 0;
  for (int64_t b = b0; b < b1; ++b) {
    sv += ws.blockCnt[2 * b];
    sf += ws.blockCnt[2 * b + 1];
  }
  int64_t tv, tf;
  int64_t ov = block_exclusive_scan<MC_SCAN>(sv, lds, &tv);
  int64_t of = block_exclusive_scan<MC_SCAN>(sf, lds, &tf);
  for (int64_t b = b0; b < b1; ++b) {
    ws.blockOff[2 * b] = ov;
    ws.blockOff[2 * b + 1] = of;
    ov += ws.blockCnt[2 * b];
    of += ws.blockCnt[2 * b + 1];
  }
  if (threadIdx.x == 0) {
    counts[0] = tv; counts[1] = tf;
    ws.total[0] = tv; ws.total[1] = tf;
  }
}

__device__ inline bool mesh_fits(const McWs& ws, int64_t max_verts, int64_t max_faces) {
  const int64_t nv = ws.total[0], nf = ws.total[1];
  return nv <= max_verts && nf <= max_faces && nv <= 0x7fffffff;    // vertex ids are int32
}

// d value / d index at a grid point: central differences inside, one-sided at the borders
__device__ inline void grad_at(const float* __restrict__ v, const McGeom& g, int64_t idx, int i, int j, int k, float* out) {
  const int d[3] = {g.D0, g.D1, g.D2};
  const int c[3] = {i, j, k};
  const int64_t s[3] = {g.s0, g.s1, 1};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (c[a] == 0) out[a] = v[idx + s[a]] - v[idx];
    else if (c[a] == d[a] - 1) out[a] = v[idx] - v[idx - s[a]];
    else out[a] = (v[idx + s[a]] - v[idx - s[a]]) * 0.5f;
  }
}

__global__ __launch_bounds__(MC_BLOCK) void mc_verts_kernel(const float* __restrict__ vol, McGeom g, McWs ws,
                                                            float* __restrict__ verts, float* __restrict__ normals,
                                                            int64_t max_verts, int64_t max_faces) {
  if (!mesh_fits(ws, max_verts, max_faces)) return;
  __shared__ int lds[MC_BLOCK / 64];
  const int64_t idx = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  int i = 0, j = 0, k = 0, nv = 0;
  bool e[3] = {false, false, false};
  float f0 = 0.f;
  if (idx < g.P) {
    coords(g, idx, i, j, k);
    f0 = vol[idx];
#pragma unroll
    for (int a = 0; a < 3; ++a) e[a] = edge_vertex(vol, g, idx, i, j, k, a, f0);
    nv = (int)e[0] + (int)e[1] + (int)e[2];
  }
  int tv;
  const int pre = block_exclusive_scan<MC_BLOCK>(nv, lds, &tv);
  if (idx >= g.P) return;
  const int64_t base = ws.blockOff[2 * blockIdx.x] + pre;
  ws.vbase[idx] = (int32_t)base;
  if (nv == 0) return;
  float ga[3];
  grad_at(vol, g, idx, i, j, k, ga);
  int64_t out = base;
  const int64_t st[3] = {g.s0, g.s1, 1};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!e[a]) continue;
    const int64_t nb = idx + st[a];
    const float f1 = vol[nb];
    const float t = (g.level - f0) / (f1 - f0);
    float p[3] = {(float)i, (float)j, (float)k};
    p[a] = p[a] + t;
    float gb[3];
    grad_at(vol, g, nb, i + (a == 0), j + (a == 1), k + (a == 2), gb);
    float n[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) n[q] = ga[q] + t * (gb[q] - ga[q]);
    float r = 1.f / sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
#pragma unroll
    for (int q = 0; q < 3; ++q) n[q] *= r;
    if (g.has_xf) {
      float w[3], m[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        w[q] = g.A[4 * q] * p[0] + g.A[4 * q + 1] * p[1] + g.A[4 * q + 2] * p[2] + g.A[4 * q + 3];
        m[q] = g.N[3 * q] * n[0] + g.N[3 * q + 1] * n[1] + g.N[3 * q + 2] * n[2];
      }
      r = 1.f / sqrtf(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
#pragma unroll
      for (int q = 0; q < 3; ++q) { p[q] = w[q]; n[q] = m[q] * r; }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) verts[3 * out + q] = p[q];
    if (normals) {
#pragma unroll
      for (int q = 0; q < 3; ++q) normals[3 * out + q] = n[q];
    }
    ++out;
  }
}

// vertex id of edge `e` of the cell at (idx; i, j, k)
__device__ inline int32_t edge_vertex_id(const float* __restrict__ vol, const McGeom& g, const McWs& ws, int64_t idx, int i, int j,
                                         int k, int e) {
  const int axis = e >> 2;
  const int c = mc::kEdgeCorners[e][0];
  const int qi = i + (c & 1), qj = j + (c >> 1 & 1), qk = k + (c >> 2 & 1);
  const int64_t q = idx + (c & 1 ? g.s0 : 0) + (c & 2 ? g.s1 : 0) + (c & 4 ? 1 : 0);
  int32_t id = ws.vbase[q];
  if (axis > 0) {
    const float f0 = vol[q];
    id += (int32_t)edge_vertex(vol, g, q, qi, qj, qk, 0, f0);
    if (axis > 1) id += (int32_t)edge_vertex(vol, g, q, qi, qj, qk, 1, f0);
  }
  return id;
}

__global__ __launch_bounds__(MC_BLOCK) void mc_faces_kernel(const float* __restrict__ vol, McGeom g, McWs ws,
                                                            int32_t* __restrict__ faces, int64_t max_verts, int64_t max_faces) {
  if (!mesh_fits(ws, max_verts, max_faces)) return;
  __shared__ int lds[MC_BLOCK / 64];
  const int64_t idx = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  int i = 0, j = 0, k = 0, c = -1, nf = 0;
  if (idx < g.P) {
    coords(g, idx, i, j, k);
    c = cell_case(vol, g, idx, i, j, k);
    nf = c < 0 ? 0 : (int)mc::kTriCount[c];
  }
  int tf;
  const int pre = block_exclusive_scan<MC_BLOCK>(nf, lds, &tf);
  if (nf == 0) return;
  const int64_t base = ws.blockOff[2 * blockIdx.x + 1] + pre;
  for (int t = 0; t < nf; ++t)
    for (int q = 0; q < 3; ++q)
      faces[3 * (base + t) + q] = edge_vertex_id(vol, g, ws, idx, i, j, k, mc::kTriTable[c][3 * t + q]);
}

}  // namespace

// workspace layout (bytes); nBlocks out
int64_t mesh_ws_layout(int64_t P, int64_t* nBlocks, int64_t* offOff, int64_t* offTot, int64_t* offVbase) {
  const int64_t nb = (P + MC_BLOCK - 1) / MC_BLOCK;
  auto up = [](int64_t x) { return (x + 255) / 256 * 256; };
  const int64_t oOff = up(nb * 2 * 4);
  const int64_t oTot = oOff + up(nb * 2 * 8);
  const int64_t oVb = oTot + 256;
  if (nBlocks) *nBlocks = nb;
  if (offOff) *offOff = oOff;
  if (offTot) *offTot = oTot;
  if (offVbase) *offVbase = oVb;
  return oVb + up(P * 4);
}

int launch_marching_cubes(const float* vol, int32_t D0, int32_t D1, int32_t D2, float level, const float* A, const float* N,
                          int64_t* counts, float* verts, float* normals, int64_t max_verts, int32_t* faces, int64_t max_faces,
                          void* workspace, hipStream_t st) {
  McGeom g = {};
  g.D0 = D0; g.D1 = D1; g.D2 = D2;
  g.s1 = D2; g.s0 = (int64_t)D1 * D2; g.P = (int64_t)D0 * g.s0;
  g.level = level;
  g.has_xf = A != nullptr;
  for (int q = 0; q < 12; ++q) g.A[q] = A ? A[q] : 0.f;
  for (int q = 0; q < 9; ++q) g.N[q] = N ? N[q] : 0.f;
  McWs ws = {};
  int64_t oOff, oTot, oVb;
  mesh_ws_layout(g.P, &ws.nBlocks, &oOff, &oTot, &oVb);
  char* base = (char*)workspace;
  ws.blockCnt = (int32_t*)base;
  ws.blockOff = (int64_t*)(base + oOff);
  ws.total = (int64_t*)(base + oTot);
  ws.vbase = (int32_t*)(base + oVb);
  const dim3 grid((unsigned)ws.nBlocks);
  hipLaunchKernelGGL(mc_count_kernel, grid, dim3(MC_BLOCK), 0, st, vol, g, ws);
  hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(MC_SCAN), 0, st, ws, counts);
  hipLaunchKernelGGL(mc_verts_kernel, grid, dim3(MC_BLOCK), 0, st, vol, g, ws, verts, normals, max_verts, max_faces);
  hipLaunchKernelGGL(mc_faces_kernel, grid, dim3(MC_BLOCK), 0, st, vol, g, ws, faces, max_verts, max_faces);
  return isdf_launch_status();
}

void mc_tables_host(int32_t* edge_corners, int8_t* tri_table) {
  if (edge_corners)
    for (int e = 0; e < 12; ++e) { edge_corners[2 * e] = mc::kEdgeCorners[e][0]; edge_corners[2 * e + 1] = mc::kEdgeCorners[e][1]; }
  if (tri_table)
    for (int c = 0; c < 256; ++c)
      for (int q = 0; q < mc::kTriWidth; ++q) tri_table[c * mc::kTriWidth + q] = mc::kTriTable[c][q];
}

}  // namespace isdf
