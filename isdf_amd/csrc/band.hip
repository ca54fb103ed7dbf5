// Narrow-band selection for surface extraction (isdf_band_*, include/isdf_hip.h): which lattice points of a D0 x D1 x D2 grid the
// network has to be evaluated at so that marching cubes of the result equals marching cubes of the dense grid.
//
// The hierarchy is a set of DENSE byte grids, one per stride s = coarse, coarse / 2, ..., 2, holding "cell kept" for every cell
// of that stride; a cell is a candidate iff its parent (>> 1 per axis) is kept.  Dense flags instead of compacted cell lists:
// the candidates of a level are then ordered by construction, the passes need no list of their own, and the finest grid costs
// P / 8 bytes -- small next to the P floats of the volume that marching cubes needs anyway.
//
//   fill     the volume <- BD_UNSET, a quiet NaN whose payload says "not evaluated"
//   select   one thread per lattice point of the stride (stride 1: per grid point): needed by a candidate cell and still
//            BD_UNSET?  per-block sums, then the one-block scan: exclusive block offsets, the total to the caller's counts
//   emit     the same test again, the block-level scan, plus the block's offset: the point's linear index and its world
//            position go to slot `offset`; the list is ordered by lattice index, no atomic decides a position
//   update   scatter the caller's values into the volume, then one thread per cell of the stride: candidate?  kept?
//   leaks    one thread per unit cell: every corner evaluated, the surface crosses it, and its stride-2 cell is not kept
//
// Every workspace word is written before it is read within one select / emit / update sequence: the workspace needs no zeroing.
// Built without floating-point contraction: d and the world positions are the documented fp32 chains (fmaf by name).
#include "isdf_common.h"
#include "launchers.h"
#include "block_scan.h"

namespace isdf {

namespace {

constexpr int BD_BLOCK = 256;              // threads per block of every pass
constexpr int BD_SCAN = 1024;              // threads of the one-block scan
constexpr uint32_t BD_UNSET = 0x7fe15df0u; // "not evaluated"; a field value with these very bits is stored as the default NaN
constexpr uint32_t BD_NAN = 0x7fc00000u;

struct BandGeom {
  int32_t D0, D1, D2;
  int32_t s;              // stride of the pass; 1: the finest fill (cells below are then those of stride 2)
  int32_t n0, n1, n2;     // cells per axis
  int32_t p1, p2;         // parent cells along j and k (stride 2s)
  int32_t t1, t2, tshift; // stride 1: cells of the coarsest stride along j and k; stride-2 cell index >> tshift = its coarsest ancestor
  int64_t P, s0, s1;      // grid points; strides of i and j (k: 1)
  int64_t T;              // threads of the select / emit pass
  float level, slack;
  float A[12];
};

struct BandWs {
  uint8_t* kept;          // cell flags of this stride (stride 1: of stride 2)
  const uint8_t* parent;  // cell flags of stride 2s; null at the coarsest stride
  const uint8_t* top;     // stride 1: cell flags of the coarsest stride
  int32_t* blockCnt;      // [nBlocks][2]
  int64_t* blockOff;      // [nBlocks][2] exclusive offsets
  int64_t nBlocks;
};

__device__ inline uint32_t bits_of(float x) { return __float_as_uint(x); }
__device__ inline int min_i(int a, int b) { return a < b ? a : b; }
__device__ inline int max_i(int a, int b) { return a > b ? a : b; }

__device__ inline bool candidate(const BandGeom& g, const uint8_t* __restrict__ parent, int ci, int cj, int ck) {
  return parent == nullptr || parent[((int64_t)(ci >> 1) * g.p1 + (cj >> 1)) * g.p2 + (ck >> 1)] != 0;
}

// thread t of a select / emit pass: does its point have to be evaluated now?  lin: its linear index in the volume
__device__ inline bool point_wanted(const BandGeom& g, const BandWs& ws, const float* __restrict__ vol, int64_t t, int64_t* lin) {
  bool need = false;
  if (g.s == 1) {       // every point of [2c - 1, 2c + 3] per axis around a kept stride-2 cell c
    const int i = (int)(t / g.s0);
    const int64_t r = t - (int64_t)i * g.s0;
    const int j = (int)(r / g.s1), k = (int)(r - (int64_t)j * g.s1);
    *lin = t;
    if (bits_of(vol[t]) != BD_UNSET) return false;
    const int a0 = max_i((i - 2) >> 1, 0), a1 = min_i((i + 1) >> 1, g.n0 - 1);
    const int b0 = max_i((j - 2) >> 1, 0), b1 = min_i((j + 1) >> 1, g.n1 - 1);
    const int c0 = max_i((k - 2) >> 1, 0), c1 = min_i((k + 1) >> 1, g.n2 - 1);
    // a kept cell has kept ancestors: most points are ruled out by the few coarsest cells around them, a grid that stays in cache
    bool near = false;
    for (int a = a0 >> g.tshift; a <= a1 >> g.tshift; ++a)
      for (int b = b0 >> g.tshift; b <= b1 >> g.tshift; ++b)
        for (int c = c0 >> g.tshift; c <= c1 >> g.tshift; ++c) near = near || ws.top[((int64_t)a * g.t1 + b) * g.t2 + c] != 0;
    if (!near) return false;
    for (int a = a0; a <= a1; ++a)
      for (int b = b0; b <= b1; ++b)
        for (int c = c0; c <= c1; ++c) need = need || ws.kept[((int64_t)a * g.n1 + b) * g.n2 + c] != 0;
    return need;
  }
  // lattice point (pi, pj, pk) of the stride, the last one clipped to the grid's last index: a corner of up to eight cells
  const int64_t m1 = g.n2 + 1, m0 = (int64_t)(g.n1 + 1) * m1;
  const int pi = (int)(t / m0);
  const int64_t r = t - (int64_t)pi * m0;
  const int pj = (int)(r / m1), pk = (int)(r - (int64_t)pj * m1);
  const int i = min_i(pi * g.s, g.D0 - 1), j = min_i(pj * g.s, g.D1 - 1), k = min_i(pk * g.s, g.D2 - 1);
  *lin = (int64_t)i * g.s0 + (int64_t)j * g.s1 + k;
  if (bits_of(vol[*lin]) != BD_UNSET) return false;
  for (int a = max_i(pi - 1, 0); a <= min_i(pi, g.n0 - 1); ++a)
    for (int b = max_i(pj - 1, 0); b <= min_i(pj, g.n1 - 1); ++b)
      for (int c = max_i(pk - 1, 0); c <= min_i(pk, g.n2 - 1); ++c) need = need || candidate(g, ws.parent, a, b, c);
  return need;
}

__global__ __launch_bounds__(BD_BLOCK) void band_fill_kernel(float* __restrict__ vol, int64_t P) {
  const int64_t t = (int64_t)blockIdx.x * BD_BLOCK + threadIdx.x;
  if (t < P) vol[t] = __uint_as_float(BD_UNSET);
}

__global__ __launch_bounds__(BD_BLOCK) void band_select_kernel(const float* __restrict__ vol, BandGeom g, BandWs ws) {
  __shared__ int lds[BD_BLOCK / 64];
  const int64_t t = (int64_t)blockIdx.x * BD_BLOCK + threadIdx.x;
  int64_t lin;
  const int want = t < g.T && point_wanted(g, ws, vol, t, &lin) ? 1 : 0;
  int tot;
  block_exclusive_scan<BD_BLOCK>(want, lds, &tot);
  if (threadIdx.x == 0) {
    ws.blockCnt[2 * blockIdx.x] = tot;
    ws.blockCnt[2 * blockIdx.x + 1] = 0;
  }
}

// exclusive offsets of the per-block sums (both columns), the totals to counts[0..1]
__global__ __launch_bounds__(BD_SCAN) void band_scan_kernel(BandWs ws, int64_t* __restrict__ counts) {
  __shared__ int64_t lds[BD_SCAN / 64];
  const int64_t per = (ws.nBlocks + BD_SCAN - 1) / BD_SCAN;
  const int64_t b0 = (int64_t)threadIdx.x * per;
  const int64_t b1 = b0 + per < ws.nBlocks ? b0 + per : ws.nBlocks;
  int64_t sa = 0, sb = 0;
  for (int64_t b = b0; b < b1; ++b) {
    sa += ws.blockCnt[2 * b];
    sb += ws.blockCnt[2 * b + 1];
  }
  int64_t ta, tb;
  int64_t oa = block_exclusive_scan<BD_SCAN>(sa, lds, &ta);
  int64_t ob = block_exclusive_scan<BD_SCAN>(sb, lds, &tb);
  for (int64_t b = b0; b < b1; ++b) {
    ws.blockOff[2 * b] = oa;
    ws.blockOff[2 * b + 1] = ob;
    oa += ws.blockCnt[2 * b];
    ob += ws.blockCnt[2 * b + 1];
  }
  if (threadIdx.x == 0 && counts) { counts[0] = ta; counts[1] = tb; }
}

// index -> world: per row r, fma(A[r][2], k, fma(A[r][1], j, fma(A[r][0], i, A[r][3]))) -- the one chain of the sparse list and the
// full grid
__device__ inline void index_to_world(const float* A, int64_t lin, int64_t s0, int64_t s1, float* __restrict__ out) {
  const int i = (int)(lin / s0);
  const int64_t r = lin - (int64_t)i * s0;
  const int j = (int)(r / s1), k = (int)(r - (int64_t)j * s1);
  const float fi = (float)i, fj = (float)j, fk = (float)k;
#pragma unroll
  for (int q = 0; q < 3; ++q) out[q] = fmaf(A[4 * q + 2], fk, fmaf(A[4 * q + 1], fj, fmaf(A[4 * q], fi, A[4 * q + 3])));
}

__global__ __launch_bounds__(BD_BLOCK) void band_emit_kernel(const float* __restrict__ vol, BandGeom g, BandWs ws,
                                                             const float* __restrict__ points, int32_t* __restrict__ index_out,
                                                             float* __restrict__ pts_out, int64_t n) {
  __shared__ int lds[BD_BLOCK / 64];
  const int64_t t = (int64_t)blockIdx.x * BD_BLOCK + threadIdx.x;
  int64_t lin = 0;
  const int want = t < g.T && point_wanted(g, ws, vol, t, &lin) ? 1 : 0;
  int tot;
  const int pre = block_exclusive_scan<BD_BLOCK>(want, lds, &tot);
  if (!want) return;
  const int64_t pos = ws.blockOff[2 * blockIdx.x] + pre;
  if (pos >= n) return;         // the caller's list is shorter than the count select reported: write nothing past it
  index_out[pos] = (int32_t)lin;
  float p[3];
  if (points) {
#pragma unroll
    for (int q = 0; q < 3; ++q) p[q] = points[3 * lin + q];
  } else {
    index_to_world(g.A, lin, g.s0, g.s1, p);
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) pts_out[3 * pos + q] = p[q];
}

__global__ __launch_bounds__(BD_BLOCK) void band_scatter_kernel(float* __restrict__ vol, int64_t P, const int32_t* __restrict__ index,
                                                                const float* __restrict__ values, int64_t n) {
  const int64_t t = (int64_t)blockIdx.x * BD_BLOCK + threadIdx.x;
  if (t >= n) return;
  const int64_t lin = index[t];
  if (lin < 0 || lin >= P) return;
  const float v = values[t];
  vol[lin] = bits_of(v) == BD_UNSET ? __uint_as_float(BD_NAN) : v;
}

// the cell whose corners are (lo, hi) per axis: any corner non-finite, the corners not all on one side, or all within slack * d
__device__ inline bool cell_kept(const float* __restrict__ vol, const BandGeom& g, const int* lo, const int* hi) {
  bool bad = false;
  int inside = 0;
  float m = 0.f;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float f = vol[(int64_t)(q & 1 ? hi[0] : lo[0]) * g.s0 + (int64_t)(q & 2 ? hi[1] : lo[1]) * g.s1 + (q & 4 ? hi[2] : lo[2])];
    bad = bad || !__builtin_isfinite(f);
    inside += f < g.level ? 1 : 0;
    m = fmaxf(m, fabsf(f - g.level));
  }
  const float e0 = (float)(hi[0] - lo[0]), e1 = (float)(hi[1] - lo[1]), e2 = (float)(hi[2] - lo[2]);
  float w[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) w[q] = fmaf(g.A[4 * q + 2], e2, fmaf(g.A[4 * q + 1], e1, g.A[4 * q] * e0));
  const float d = sqrtf(fmaf(w[2], w[2], fmaf(w[1], w[1], w[0] * w[0])));
  return bad || (inside != 0 && inside != 8) || m <= g.slack * d;
}

__global__ __launch_bounds__(BD_BLOCK) void band_test_kernel(const float* __restrict__ vol, BandGeom g, BandWs ws) {
  __shared__ int lds[BD_BLOCK / 64];
  const int64_t c = (int64_t)blockIdx.x * BD_BLOCK + threadIdx.x;
  int cand = 0, keep = 0;
  if (c < g.T) {
    const int64_t m0 = (int64_t)g.n1 * g.n2;
    const int ci = (int)(c / m0);
    const int64_t r = c - (int64_t)ci * m0;
    const int cj = (int)(r / g.n2), ck = (int)(r - (int64_t)cj * g.n2);
    if (candidate(g, ws.parent, ci, cj, ck)) {
      cand = 1;
      const int lo[3] = {ci * g.s, cj * g.s, ck * g.s};
      const int hi[3] = {min_i(lo[0] + g.s, g.D0 - 1), min_i(lo[1] + g.s, g.D1 - 1), min_i(lo[2] + g.s, g.D2 - 1)};
      keep = cell_kept(vol, g, lo, hi) ? 1 : 0;
    }
    ws.kept[c] = (uint8_t)keep;
  }
  int tc, tk;
  block_exclusive_scan<BD_BLOCK>(cand, lds, &tc);
  block_exclusive_scan<BD_BLOCK>(keep, lds, &tk);
  if (threadIdx.x == 0) {
    ws.blockCnt[2 * blockIdx.x] = tc;
    ws.blockCnt[2 * blockIdx.x + 1] = tk;
  }
}

__global__ __launch_bounds__(BD_BLOCK) void band_leak_kernel(const float* __restrict__ vol, BandGeom g, BandWs ws) {
  __shared__ int lds[BD_BLOCK / 64];
  const int64_t t = (int64_t)blockIdx.x * BD_BLOCK + threadIdx.x;
  int leak = 0;
  if (t < g.P && bits_of(vol[t]) != BD_UNSET) {
    const int i = (int)(t / g.s0);
    const int64_t r = t - (int64_t)i * g.s0;
    const int j = (int)(r / g.s1), k = (int)(r - (int64_t)j * g.s1);
    if (i + 1 < g.D0 && j + 1 < g.D1 && k + 1 < g.D2 && ws.kept[((int64_t)(i >> 1) * g.n1 + (j >> 1)) * g.n2 + (k >> 1)] == 0) {
      bool ok = true;
      int inside = 0;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float f = vol[t + (q & 1 ? g.s0 : 0) + (q & 2 ? g.s1 : 0) + (q & 4 ? 1 : 0)];
        ok = ok && __builtin_isfinite(f);         // BD_UNSET is a NaN: an unevaluated corner ends here too
        inside += f < g.level ? 1 : 0;
      }
      leak = ok && inside != 0 && inside != 8 ? 1 : 0;
    }
  }
  int tot;
  block_exclusive_scan<BD_BLOCK>(leak, lds, &tot);
  if (threadIdx.x == 0) {
    ws.blockCnt[2 * blockIdx.x] = tot;
    ws.blockCnt[2 * blockIdx.x + 1] = 0;
  }
}

__global__ __launch_bounds__(BD_BLOCK) void grid_points_kernel(BandGeom g, float* __restrict__ pts_out) {
  const int64_t t = (int64_t)blockIdx.x * BD_BLOCK + threadIdx.x;
  if (t >= g.P) return;
  float p[3];
  index_to_world(g.A, t, g.s0, g.s1, p);
#pragma unroll
  for (int q = 0; q < 3; ++q) pts_out[3 * t + q] = p[q];
}

int64_t up256(int64_t x) { return (x + 255) / 256 * 256; }
int32_t cells(int32_t D, int32_t s) { return (D - 1 + s - 1) / s; }
int level_of(int32_t s) { int l = 0; while ((1 << (l + 1)) < s) ++l; return l; }     // 2 -> 0, 4 -> 1, ...

struct BandLayout { int64_t flags[31]; int64_t cnt, off, total; int64_t nBlocks; };

BandLayout band_layout(int32_t D0, int32_t D1, int32_t D2, int32_t coarse) {
  BandLayout L = {};
  int64_t o = 0;
  for (int32_t s = 2; s <= coarse && s > 0; s <<= 1) {
    L.flags[level_of(s)] = o;
    o += up256((int64_t)cells(D0, s) * cells(D1, s) * cells(D2, s));
  }
  L.nBlocks = ((int64_t)D0 * D1 * D2 + BD_BLOCK - 1) / BD_BLOCK;      // every pass has at most one thread per grid point
  L.cnt = o; o += up256(L.nBlocks * 2 * 4);
  L.off = o; o += up256(L.nBlocks * 2 * 8);
  L.total = o + 256;
  return L;
}

// geometry and workspace pointers of the pass at `stride` (1: the finest fill and the leak count, on the stride-2 cells)
void band_setup(const isdf_band_args& a, int32_t stride, void* workspace, BandGeom* g, BandWs* ws) {
  const int32_t cs = stride == 1 ? 2 : stride;
  *g = {};
  g->D0 = a.D0; g->D1 = a.D1; g->D2 = a.D2; g->s = stride;
  g->n0 = cells(a.D0, cs); g->n1 = cells(a.D1, cs); g->n2 = cells(a.D2, cs);
  const bool has_parent = stride > 1 && stride < a.coarse;
  if (has_parent) { g->p1 = cells(a.D1, 2 * cs); g->p2 = cells(a.D2, 2 * cs); }
  g->s1 = a.D2; g->s0 = (int64_t)a.D1 * a.D2; g->P = (int64_t)a.D0 * g->s0;
  g->T = stride == 1 ? g->P : (int64_t)(g->n0 + 1) * (g->n1 + 1) * (g->n2 + 1);
  g->level = a.level; g->slack = a.slack;
  static const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  for (int q = 0; q < 12; ++q) g->A[q] = a.has_transform ? a.index_to_world[q] : I[q];
  const BandLayout L = band_layout(a.D0, a.D1, a.D2, a.coarse);
  char* base = (char*)workspace;
  ws->kept = (uint8_t*)(base + L.flags[level_of(cs)]);
  ws->parent = has_parent ? (const uint8_t*)(base + L.flags[level_of(2 * cs)]) : nullptr;
  g->t1 = cells(a.D1, a.coarse); g->t2 = cells(a.D2, a.coarse); g->tshift = level_of(a.coarse);
  ws->top = (const uint8_t*)(base + L.flags[level_of(a.coarse)]);
  ws->blockCnt = (int32_t*)(base + L.cnt);
  ws->blockOff = (int64_t*)(base + L.off);
  ws->nBlocks = 0;
}

unsigned blocks_for(BandWs* ws, int64_t threads) {
  ws->nBlocks = (threads + BD_BLOCK - 1) / BD_BLOCK;
  return (unsigned)ws->nBlocks;
}

}  // namespace

int64_t band_ws_bytes(int32_t D0, int32_t D1, int32_t D2, int32_t coarse) { return band_layout(D0, D1, D2, coarse).total; }

int launch_band_fill(float* vol, int64_t P, hipStream_t st) {
  hipLaunchKernelGGL(band_fill_kernel, dim3((unsigned)((P + BD_BLOCK - 1) / BD_BLOCK)), dim3(BD_BLOCK), 0, st, vol, P);
  return isdf_launch_status();
}

int launch_band_select(const isdf_band_args& a, int32_t stride, const float* vol, int64_t* counts, void* workspace, hipStream_t st) {
  BandGeom g; BandWs ws;
  band_setup(a, stride, workspace, &g, &ws);
  const dim3 grid(blocks_for(&ws, g.T));
  hipLaunchKernelGGL(band_select_kernel, grid, dim3(BD_BLOCK), 0, st, vol, g, ws);
  hipLaunchKernelGGL(band_scan_kernel, dim3(1), dim3(BD_SCAN), 0, st, ws, counts);
  return isdf_launch_status();
}

int launch_band_emit(const isdf_band_args& a, int32_t stride, const float* vol, int32_t* index_out, float* pts_out, int64_t n,
                     void* workspace, hipStream_t st) {
  BandGeom g; BandWs ws;
  band_setup(a, stride, workspace, &g, &ws);
  const dim3 grid(blocks_for(&ws, g.T));
  hipLaunchKernelGGL(band_emit_kernel, grid, dim3(BD_BLOCK), 0, st, vol, g, ws, a.points, index_out, pts_out, n);
  return isdf_launch_status();
}

int launch_band_update(const isdf_band_args& a, int32_t stride, float* vol, const int32_t* index, const float* values, int64_t n,
                       int64_t* counts, void* workspace, hipStream_t st) {
  BandGeom g; BandWs ws;
  band_setup(a, stride, workspace, &g, &ws);
  if (n > 0)
    hipLaunchKernelGGL(band_scatter_kernel, dim3((unsigned)((n + BD_BLOCK - 1) / BD_BLOCK)), dim3(BD_BLOCK), 0, st, vol, g.P, index,
                       values, n);
  if (stride > 1) {
    g.T = (int64_t)g.n0 * g.n1 * g.n2;
    const dim3 grid(blocks_for(&ws, g.T));
    hipLaunchKernelGGL(band_test_kernel, grid, dim3(BD_BLOCK), 0, st, (const float*)vol, g, ws);
    hipLaunchKernelGGL(band_scan_kernel, dim3(1), dim3(BD_SCAN), 0, st, ws, counts);
  }
  return isdf_launch_status();
}

int launch_band_leaks(const isdf_band_args& a, const float* vol, int64_t* counts, void* workspace, hipStream_t st) {
  BandGeom g; BandWs ws;
  band_setup(a, 1, workspace, &g, &ws);
  const dim3 grid(blocks_for(&ws, g.P));
  hipLaunchKernelGGL(band_leak_kernel, grid, dim3(BD_BLOCK), 0, st, vol, g, ws);
  hipLaunchKernelGGL(band_scan_kernel, dim3(1), dim3(BD_SCAN), 0, st, ws, counts);
  return isdf_launch_status();
}

int launch_grid_points(int32_t D0, int32_t D1, int32_t D2, const float* A, float* pts_out, hipStream_t st) {
  BandGeom g = {};
  g.D0 = D0; g.D1 = D1; g.D2 = D2;
  g.s1 = D2; g.s0 = (int64_t)D1 * D2; g.P = (int64_t)D0 * g.s0;
  for (int q = 0; q < 12; ++q) g.A[q] = A[q];
  hipLaunchKernelGGL(grid_points_kernel, dim3((unsigned)((g.P + BD_BLOCK - 1) / BD_BLOCK)), dim3(BD_BLOCK), 0, st, g, pts_out);
  return isdf_launch_status();
}

}  // namespace isdf
