// Where to look next: the frontier between known-free and unknown voxels (isdf_frontier_init), its 26-connected components
// (isdf_frontier_relax), their records (isdf_frontier_clusters) and the unknown voxels a camera pose would see (isdf_view_gain).
// The reference has no counterpart; include/isdf_hip.h states every rule and the walk operation by operation.  Labels, records
// and counts are integers and the depth is one float32 from a stated sequence, so everything is compared bit for bit.
//
// Labels.  label[p] <- min(label[p], label[q] over the 26 neighbours q) for frontier voxels; the others hold ISDF_FRONTIER_NONE in
// the volume itself, a neighbour nobody takes (route.hip's blocked voxels).  Built as route_tile_kernel is: a workgroup owns 8^3
// voxels, loads them with their one-voxel halo (faces, edges and corners) into LDS rows of 24 words (conflict-free for the four
// rows of eight k a half-wave reads), and repeats the update until the tile is quiet or FRONTIER_INNER sweeps are done; a
// thread owns two voxels adjacent in i and reads their shared 4 x 9 neighbourhood once per sweep.  Every value written is the
// index of a voxel of the same component and values only decrease: the fixed point is the component's least linear index,
// whatever the tile, the cap or the number of launches.
//
// Clusters.  Roots (label[p] == p) are compacted in ascending index order by prefix sums (block_scan.h), never by an atomic;
// a root's slot is parked in a 4 B / voxel volume, and every frontier voxel adds itself to its root's record with 64-bit
// integer atomics -- sums, minima and maxima of integers do not depend on the order.
//
// View gain.  One thread per ray, a wave = an 8 x 8 pixel tile of one view: neighbouring rays pass the same lines of the u8
// volume.  The walk chooses its axis with selects (no per-axis array is indexed at run time: no scratch).
#include "isdf_common.h"
#include "launchers.h"
#include "block_scan.h"
#include "block_reduce.h"

namespace isdf {

constexpr int FR_TILE = ISDF_ROUTE_TILE;
constexpr int FR_INNER = 8;                             // sweeps inside a tile per launch, at most
constexpr int FR_HALO = FR_TILE + 2;
constexpr int FR_ROW = 24;                              // words per LDS row (route.hip)
constexpr int FR_PLANE = FR_HALO * FR_ROW;
constexpr int FR_CELLS = FR_HALO * FR_HALO * FR_HALO;
constexpr int32_t FR_NONE = ISDF_FRONTIER_NONE;
constexpr int FR_SCAN = 1024;
static_assert(FR_TILE == 8, "the thread -> voxel map below is written for 8^3 tiles and 256 threads");

__global__ __launch_bounds__(256) void frontier_init_kernel(const uint8_t* __restrict__ state, int nx, int ny, int nz,
                                                            int32_t* __restrict__ label) {
  const int32_t n = nx * ny * nz;
  const int32_t p = (int32_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int k = p % nz, j = (p / nz) % ny, i = p / (nz * ny);
  bool f = false;
  if (state[p] == ISDF_VOXEL_FREE) {
    const int32_t si = ny * nz;
    f = (i > 0 && state[p - si] == ISDF_VOXEL_UNKNOWN) || (i + 1 < nx && state[p + si] == ISDF_VOXEL_UNKNOWN) ||
        (j > 0 && state[p - nz] == ISDF_VOXEL_UNKNOWN) || (j + 1 < ny && state[p + nz] == ISDF_VOXEL_UNKNOWN) ||
        (k > 0 && state[p - 1] == ISDF_VOXEL_UNKNOWN) || (k + 1 < nz && state[p + 1] == ISDF_VOXEL_UNKNOWN);
  }
  label[p] = f ? p : FR_NONE;
}

int launch_frontier_init(const uint8_t* state, int32_t nx, int32_t ny, int32_t nz, int32_t* label, hipStream_t st) {
  const int32_t n = nx * ny * nz;
  hipLaunchKernelGGL(frontier_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, state, nx, ny, nz, label);
  return isdf_launch_status();
}

// the least of one i-plane of a voxel's neighbourhood and `best`
__device__ __forceinline__ int32_t min9(int32_t best, const int32_t (&v)[3][3]) {
#pragma unroll
  for (int b = 0; b < 3; ++b)
#pragma unroll
    for (int c = 0; c < 3; ++c) best = v[b][c] < best ? v[b][c] : best;
  return best;
}

__global__ __launch_bounds__(256) void frontier_tile_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out, int nx, int ny,
                                                            int nz, int tiles_j, int tiles_k, int32_t* changed) {
  __shared__ int32_t s[FR_HALO * FR_PLANE];
  const int tid = threadIdx.x;
  const int tile = (int)blockIdx.x;
  const int tk = tile % tiles_k, tj = (tile / tiles_k) % tiles_j, ti = tile / (tiles_k * tiles_j);
  const int i0 = ti * FR_TILE, j0 = tj * FR_TILE, k0 = tk * FR_TILE;
  // the tile and its halo; NONE outside the grid
  for (int t = tid; t < FR_CELLS; t += 256) {
    const int c = t % FR_HALO, b = (t / FR_HALO) % FR_HALO, a = t / (FR_HALO * FR_HALO);
    const int gi = i0 + a - 1, gj = j0 + b - 1, gk = k0 + c - 1;
    const bool inside = gi >= 0 && gj >= 0 && gk >= 0 && gi < nx && gj < ny && gk < nz;
    s[a * FR_PLANE + b * FR_ROW + c] = inside ? in[(gi * ny + gj) * nz + gk] : FR_NONE;
  }
  // this thread's two voxels: (2 * ip, j, k) and (2 * ip + 1, j, k) of the tile
  const int k = tid & 7, j = (tid >> 3) & 7, ip = tid >> 6;
  const int gi = i0 + 2 * ip, gj = j0 + j, gk = k0 + k;
  const bool in0 = gi < nx && gj < ny && gk < nz, in1 = gi + 1 < nx && gj < ny && gk < nz;
  const int32_t g0 = in0 ? (gi * ny + gj) * nz + gk : 0, g1 = in1 ? g0 + ny * nz : 0;      // in1 implies in0
  const int at = (2 * ip) * FR_PLANE + j * FR_ROW + k;      // LDS word of the neighbourhood's low corner
  __syncthreads();
  const int32_t first0 = s[at + FR_PLANE + FR_ROW + 1], first1 = s[at + 2 * FR_PLANE + FR_ROW + 1];
  const bool live0 = in0 && first0 < FR_NONE, live1 = in1 && first1 < FR_NONE;             // NONE stays NONE
  int32_t cur0 = first0, cur1 = first1;
  for (int it = 0; it < FR_INNER; ++it) {
    int32_t v[4][3][3];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[a][b][c] = s[at + a * FR_PLANE + b * FR_ROW + c];
    const int32_t mid = min9(min9(cur0 < cur1 ? cur0 : cur1, v[1]), v[2]);     // the two planes both voxels see
    const int32_t n0 = min9(mid, v[0]), n1 = min9(mid, v[3]);
    const bool low0 = live0 && n0 < cur0, low1 = live1 && n1 < cur1;
    // the barrier of the vote: every read of this sweep is done before any write below
    if (!__syncthreads_or(low0 || low1)) break;
    if (low0) s[at + FR_PLANE + FR_ROW + 1] = cur0 = n0;
    if (low1) s[at + 2 * FR_PLANE + FR_ROW + 1] = cur1 = n1;
    __syncthreads();
  }
  if (in0) out[g0] = cur0;
  if (in1) out[g1] = cur1;
  if (__syncthreads_or(cur0 < first0 || cur1 < first1) && tid == 0) *changed = 1;      // every block that stores, stores 1
}

static int64_t up256(int64_t x) { return (x + 255) / 256 * 256; }

int64_t frontier_ws_bytes(int32_t nx, int32_t ny, int32_t nz) {
  const int64_t n = (int64_t)nx * ny * nz;
  return up256(4 * n) + up256(4 * ((n + 255) / 256));
}

// one round: label -> ws -> label; changed[r] <- 1 iff either launch of round r lowered a label
int launch_frontier_relax(int32_t* label, int32_t nx, int32_t ny, int32_t nz, int32_t* ws, int32_t rounds, int32_t* changed,
                          hipStream_t st) {
  const hipError_t e = hipMemsetAsync(changed, 0, (size_t)rounds * sizeof(int32_t), st);
  if (e != hipSuccess) { g_isdf_last_hip_error = (int)e; return ISDF_EHIP; }
  const int ti = (nx + FR_TILE - 1) / FR_TILE, tj = (ny + FR_TILE - 1) / FR_TILE, tk = (nz + FR_TILE - 1) / FR_TILE;
  for (int32_t r = 0; r < rounds; ++r)
    for (int half = 0; half < 2; ++half) {
      const int32_t* in = half ? ws : label;
      int32_t* out = half ? label : ws;
      hipLaunchKernelGGL(frontier_tile_kernel, dim3((unsigned)(ti * tj * tk)), dim3(256), 0, st, in, out, nx, ny, nz, tj, tk,
                         changed + r);
      const int rc = isdf_launch_status();
      if (rc) return rc;
    }
  return ISDF_OK;
}

// ---- clusters ---------------------------------------------------------------------------------------------------------------
// a frontier voxel: 0 <= label < NONE (one unsigned compare); its root q = label[p] is one iff q < n and label[q] == q
__device__ __forceinline__ bool fr_is_frontier(int32_t l) { return (uint32_t)l < (uint32_t)FR_NONE; }
__device__ __forceinline__ bool fr_root_ok(const int32_t* __restrict__ label, int32_t n, int32_t q) { return q < n && label[q] == q; }

__global__ __launch_bounds__(256) void cluster_count_kernel(const int32_t* __restrict__ label, int32_t n, int32_t* __restrict__ blockCnt,
                                                            int32_t* counts) {
  __shared__ int32_t sh[3][4];
  const int32_t p = (int32_t)blockIdx.x * 256 + threadIdx.x;
  int32_t root = 0, front = 0, orphan = 0;
  if (p < n) {
    const int32_t l = label[p];
    if (fr_is_frontier(l)) {
      front = 1;
      root = l == p;
      orphan = !root && !fr_root_ok(label, n, l);
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int32_t r = wave_reduce<RedSum>(root), f = wave_reduce<RedSum>(front), o = wave_reduce<RedSum>(orphan);
  if (lane == 0) { sh[0][wave] = r; sh[1][wave] = f; sh[2][wave] = o; }
  __syncthreads();
  if (threadIdx.x == 0) {
    blockCnt[blockIdx.x] = waves_combine<RedSum>(sh[0][0], sh[0][1], sh[0][2], sh[0][3]);
    const int32_t bf = waves_combine<RedSum>(sh[1][0], sh[1][1], sh[1][2], sh[1][3]);
    const int32_t bo = waves_combine<RedSum>(sh[2][0], sh[2][1], sh[2][2], sh[2][3]);
    if (bf) atomicAdd(counts + 1, bf);      // integer sums: the order does not matter
    if (bo) atomicAdd(counts + 2, bo);
  }
}

// blockCnt -> its exclusive prefix sums, in place; counts[0] <- the number of roots
__global__ __launch_bounds__(FR_SCAN) void cluster_scan_kernel(int32_t* __restrict__ blockCnt, int32_t nBlocks, int32_t* counts) {
  __shared__ int32_t lds[FR_SCAN / 64];
  const int32_t per = (nBlocks + FR_SCAN - 1) / FR_SCAN;
  const int32_t b0 = (int32_t)threadIdx.x * per < nBlocks ? (int32_t)threadIdx.x * per : nBlocks;
  const int32_t b1 = b0 + per < nBlocks ? b0 + per : nBlocks;
  int32_t sum = 0;
  for (int32_t b = b0; b < b1; ++b) sum += blockCnt[b];
  int32_t total;
  int32_t off = block_exclusive_scan<FR_SCAN>(sum, lds, &total);
  for (int32_t b = b0; b < b1; ++b) {
    const int32_t c = blockCnt[b];
    blockCnt[b] = off;
    off += c;
  }
  if (threadIdx.x == 0) counts[0] = total;
}

__global__ __launch_bounds__(256) void cluster_emit_kernel(const int32_t* __restrict__ label, int32_t n, int ny, int nz,
                                                           const int32_t* __restrict__ blockOff, const int32_t* __restrict__ counts,
                                                           int32_t max_clusters, int32_t* __restrict__ slot, int64_t* __restrict__ records) {
  if (counts[0] > max_clusters) return;      // uniform over the grid: the counts are written, the records are not
  __shared__ int32_t lds[4];
  const int32_t p = (int32_t)blockIdx.x * 256 + threadIdx.x;
  const int32_t root = p < n && label[p] == p;
  int32_t total;
  const int32_t pre = block_exclusive_scan<256>(root, lds, &total);
  if (!root) return;
  const int32_t sl = blockOff[blockIdx.x] + pre;
  slot[p] = sl;
  int64_t* r = records + (int64_t)sl * ISDF_FRONTIER_RECORD;
  r[0] = p;
  r[1] = r[2] = r[3] = r[4] = 0;
  r[5] = r[6] = r[7] = INT64_MAX;
  r[8] = r[9] = r[10] = -1;
  r[11] = 0;
}

__global__ __launch_bounds__(256) void cluster_add_kernel(const int32_t* __restrict__ label, int32_t n, int ny, int nz,
                                                          const int32_t* __restrict__ counts, int32_t max_clusters,
                                                          const int32_t* __restrict__ slot, int64_t* records) {
  if (counts[0] > max_clusters) return;
  const int32_t p = (int32_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int32_t q = label[p];
  if (!fr_is_frontier(q) || !fr_root_ok(label, n, q)) return;      // orphans join nothing
  const unsigned long long k = p % nz, j = (p / nz) % ny, i = p / (nz * ny);
  unsigned long long* r = (unsigned long long*)(records + (int64_t)slot[q] * ISDF_FRONTIER_RECORD);      // every value is >= 0
  atomicAdd(r + 1, 1ull);
  atomicAdd(r + 2, i);
  atomicAdd(r + 3, j);
  atomicAdd(r + 4, k);
  atomicMin(r + 5, i);
  atomicMin(r + 6, j);
  atomicMin(r + 7, k);
  atomicMax((long long*)r + 8, (long long)i);
  atomicMax((long long*)r + 9, (long long)j);
  atomicMax((long long*)r + 10, (long long)k);
}

int launch_frontier_clusters(const int32_t* label, int32_t nx, int32_t ny, int32_t nz, void* ws, int32_t max_clusters, int32_t* counts,
                             int64_t* records, hipStream_t st) {
  const int32_t n = nx * ny * nz, nBlocks = (n + 255) / 256;
  int32_t* slot = (int32_t*)ws;
  int32_t* blockCnt = (int32_t*)((char*)ws + up256(4 * (int64_t)n));
  const hipError_t e = hipMemsetAsync(counts, 0, 3 * sizeof(int32_t), st);
  if (e != hipSuccess) { g_isdf_last_hip_error = (int)e; return ISDF_EHIP; }
  hipLaunchKernelGGL(cluster_count_kernel, dim3((unsigned)nBlocks), dim3(256), 0, st, label, n, blockCnt, counts);
  int rc = isdf_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(cluster_scan_kernel, dim3(1), dim3(FR_SCAN), 0, st, blockCnt, nBlocks, counts);
  if ((rc = isdf_launch_status()) || max_clusters == 0) return rc;
  hipLaunchKernelGGL(cluster_emit_kernel, dim3((unsigned)nBlocks), dim3(256), 0, st, label, n, ny, nz, blockCnt, counts, max_clusters,
                     slot, records);
  if ((rc = isdf_launch_status())) return rc;
  hipLaunchKernelGGL(cluster_add_kernel, dim3((unsigned)nBlocks), dim3(256), 0, st, label, n, ny, nz, counts, max_clusters, slot,
                     records);
  return isdf_launch_status();
}

// ---- view gain --------------------------------------------------------------------------------------------------------------
constexpr int VG_TILE = 8;      // a wave is an 8 x 8 pixel tile of one view

struct ViewGainParams {
  const uint8_t* state;
  int nx, ny, nz;
  float ox, oy, oz, sx, sy, sz;
  const float* T_WC;
  int B, H, W, tiles_w, tiles;      // tiles: per view
  float fx, fy, cx, cy, t_min, t_max;
  int32_t* unknown;
  float* depth;
  uint32_t* bitmap;                 // NULL: no distinct count
  int64_t words;                    // per view
};

// one axis of the clip; false = the ray misses the grid
__device__ __forceinline__ bool vg_clip(float g0, float dg, int n, float& t0, float& t1) {
  const float hi = (float)n - 0.5f;
  if (dg == 0.f) return !(g0 < -0.5f || g0 >= hi);
  const float ta = (-0.5f - g0) / dg, tb = (hi - g0) / dg;
  t0 = fmaxf(t0, fminf(ta, tb));
  t1 = fminf(t1, fmaxf(ta, tb));
  return true;
}

__device__ __forceinline__ int vg_start(float g0, float dg, float t0, int n) {
  const float c = floorf((g0 + t0 * dg) + 0.5f);
  return (int)fminf(fmaxf(c, 0.f), (float)(n - 1));      // clamped as a float: the cast is always defined
}

__device__ __forceinline__ float vg_tmax(int c, int step, float g0, float dg, float inv) {
  return dg == 0.f ? INFINITY : (((float)c + 0.5f * (float)step) - g0) * inv;
}

__global__ __launch_bounds__(256) void view_gain_kernel(ViewGainParams q) {
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (wave >= (int64_t)q.B * q.tiles) return;
  const int b = (int)(wave / q.tiles), tile = (int)(wave % q.tiles);
  const int r = (tile / q.tiles_w) * VG_TILE + (lane >> 3), c = (tile % q.tiles_w) * VG_TILE + (lane & 7);
  if (r >= q.H || c >= q.W) return;
  const float* T = q.T_WC + (int64_t)b * 16;
  const float x = ((float)c - q.cx) / q.fx, y = ((float)r - q.cy) / q.fy;
  const float dwx = (T[0] * x + T[1] * y) + T[2], dwy = (T[4] * x + T[5] * y) + T[6], dwz = (T[8] * x + T[9] * y) + T[10];
  const float gx = (T[3] - q.ox) / q.sx, gy = (T[7] - q.oy) / q.sy, gz = (T[11] - q.oz) / q.sz;
  const float dx = dwx / q.sx, dy = dwy / q.sy, dz = dwz / q.sz;
  int32_t count = 0;
  float depth = 0.f;
  float t0 = q.t_min, t1 = q.t_max;
  bool hit = __builtin_isfinite(gx) && __builtin_isfinite(gy) && __builtin_isfinite(gz) && __builtin_isfinite(dx) &&
             __builtin_isfinite(dy) && __builtin_isfinite(dz);
  hit = hit && vg_clip(gx, dx, q.nx, t0, t1) && vg_clip(gy, dy, q.ny, t0, t1) && vg_clip(gz, dz, q.nz, t0, t1) && t0 < t1;
  if (hit) {
    int ci = vg_start(gx, dx, t0, q.nx), cj = vg_start(gy, dy, t0, q.ny), ck = vg_start(gz, dz, t0, q.nz);
    const int si = dx > 0.f ? 1 : -1, sj = dy > 0.f ? 1 : -1, sk = dz > 0.f ? 1 : -1;
    const float ix = 1.f / dx, iy = 1.f / dy, iz = 1.f / dz;
    float mx = vg_tmax(ci, si, gx, dx, ix), my = vg_tmax(cj, sj, gy, dy, iy), mz = vg_tmax(ck, sk, gz, dz, iz);
    float t_in = t0;
    uint32_t* bits = q.bitmap ? q.bitmap + (int64_t)b * q.words : nullptr;
    for (int it = q.nx + q.ny + q.nz; it > 0; --it) {
      const int32_t p = (ci * q.ny + cj) * q.nz + ck;
      const uint8_t s = q.state[p];
      if (s == ISDF_VOXEL_UNKNOWN) {
        ++count;
        if (bits) atomicOr(bits + (p >> 5), 1u << (p & 31));
      } else if (s >= ISDF_VOXEL_OCCUPIED) {
        depth = t_in;
        break;
      }
      // the axis with the least tMax; on ties the lowest axis
      const bool ay = my < mx;
      const float mxy = ay ? my : mx;
      const bool az = mz < mxy;
      t_in = az ? mz : mxy;
      if (!(t_in < t1)) break;
      if (az) {
        ck += sk;
        if (ck < 0 || ck >= q.nz) break;
        mz = vg_tmax(ck, sk, gz, dz, iz);
      } else if (ay) {
        cj += sj;
        if (cj < 0 || cj >= q.ny) break;
        my = vg_tmax(cj, sj, gy, dy, iy);
      } else {
        ci += si;
        if (ci < 0 || ci >= q.nx) break;
        mx = vg_tmax(ci, si, gx, dx, ix);
      }
    }
  }
  const int64_t o = ((int64_t)b * q.H + r) * q.W + c;
  q.unknown[o] = count;
  q.depth[o] = depth;
}

constexpr int VG_POP_BLOCKS = 64;      // blocks per view of the popcount, at most

__global__ __launch_bounds__(256) void view_popcount_kernel(const uint32_t* __restrict__ bitmap, int64_t words, int blocks_per_view,
                                                            int32_t* distinct) {
  __shared__ int32_t sh[4];
  const int b = (int)blockIdx.x / blocks_per_view, part = (int)blockIdx.x % blocks_per_view;
  const uint32_t* w = bitmap + (int64_t)b * words;
  int32_t sum = 0;
  for (int64_t t = (int64_t)part * 256 + threadIdx.x; t < words; t += (int64_t)blocks_per_view * 256) sum += __popc(w[t]);
  sum = wave_reduce<RedSum>(sum);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int32_t t = waves_combine<RedSum>(sh[0], sh[1], sh[2], sh[3]);
    if (t) atomicAdd(distinct + b, t);      // an integer sum: the order does not matter
  }
}

int64_t view_gain_words(int32_t nx, int32_t ny, int32_t nz) { return ((int64_t)nx * ny * nz + 31) / 32; }

int launch_view_gain(const uint8_t* state, int32_t nx, int32_t ny, int32_t nz, const float* origin, const float* spacing,
                     const float* T_WC, int32_t B, float fx, float fy, float cx, float cy, int32_t H, int32_t W, float t_min,
                     float t_max, int32_t* unknown, float* depth, int32_t* distinct, void* ws, hipStream_t st) {
  if (B == 0) return ISDF_OK;
  ViewGainParams q;
  q.state = state;
  q.nx = nx, q.ny = ny, q.nz = nz;
  q.ox = origin[0], q.oy = origin[1], q.oz = origin[2];
  q.sx = spacing[0], q.sy = spacing[1], q.sz = spacing[2];
  q.T_WC = T_WC;
  q.B = B, q.H = H, q.W = W;
  q.tiles_w = (W + VG_TILE - 1) / VG_TILE;
  q.tiles = q.tiles_w * ((H + VG_TILE - 1) / VG_TILE);
  q.fx = fx, q.fy = fy, q.cx = cx, q.cy = cy, q.t_min = t_min, q.t_max = t_max;
  q.unknown = unknown, q.depth = depth;
  q.bitmap = distinct ? (uint32_t*)ws : nullptr;
  q.words = view_gain_words(nx, ny, nz);
  if (distinct) {
    hipError_t e = hipMemsetAsync(ws, 0, (size_t)(q.words * B) * sizeof(uint32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(distinct, 0, (size_t)B * sizeof(int32_t), st);
    if (e != hipSuccess) { g_isdf_last_hip_error = (int)e; return ISDF_EHIP; }
  }
  const int64_t blocks = ((int64_t)B * q.tiles + 3) / 4;
  hipLaunchKernelGGL(view_gain_kernel, dim3((unsigned)blocks), dim3(256), 0, st, q);
  int rc = isdf_launch_status();
  if (rc || !distinct) return rc;
  const int64_t want = (q.words + 255) / 256;
  const int bpv = (int)(want < VG_POP_BLOCKS ? want : VG_POP_BLOCKS);
  hipLaunchKernelGGL(view_popcount_kernel, dim3((unsigned)((int64_t)B * bpv)), dim3(256), 0, st, (const uint32_t*)ws, q.words, bpv,
                     distinct);
  return isdf_launch_status();
}

}  // namespace isdf
