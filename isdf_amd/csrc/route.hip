// Routing through the map: the geodesic distance field of a free-space mask (isdf_route_init, isdf_route_relax) and the steepest
// descent through it (isdf_route_trace).  The reference has no counterpart; include/isdf_hip.h states the graph, the update and the
// neighbour order.  Everything is int32, so the converged field is THE shortest-path distance and is compared bit for bit.
//
// Relaxation.  out[p] = min(in[p], min over the 26 neighbours q of in[q] + w(p, q)) is a Jacobi sweep: one launch moves the wave
// front by one voxel, and a field across a 256^3 room needs several hundred of them, each reading and writing the whole volume.
// So a workgroup owns a tile of ROUTE_TILE^3 voxels, loads it with its one-voxel halo (faces, edges AND corners: a corner move
// crosses a tile corner) into LDS and iterates the same update there until the tile stops changing or ROUTE_INNER sweeps are done:
// one launch then moves the front by up to a tile, for one read and one write of the volume.  Every value ever written is the
// cost of a real path and values only decrease, so tile shape, inner cap and launch count change how fast the fixed point is
// reached, never what it is.  A blocked voxel holds ISDF_ROUTE_NONE in the volume itself (the init sets it, the sweep never
// lowers it), which makes it a neighbour nobody takes: NONE + w >= NONE >= in[p].  Only p's own mask byte is read.
//
// The tile in LDS is [T+2][T+2] rows of ROUTE_ROW = 24 words: with lanes 0..31 of a wave on four consecutive rows of eight k, rows
// 24 words apart start at banks 0, 24, 16, 8 -- every ds_read_b32 of the sweep is conflict-free (a row stride of T+2 = 10 is 2-way
// on six banks).  A thread owns two voxels adjacent in i and reads their 4 x 9 shared neighbourhood once per sweep (36 LDS reads
// for two voxels instead of 54), all into registers; the barrier that also carries the "anything lowered?" vote separates these
// reads from the writes of the new values, so no lane reads a word another lane is writing.  Measured choices: DESIGN 25.
//
// Trace.  One wave per path: lanes 0..25 each read one neighbour, a ballot finds the first lane (= the first neighbour in the
// header's order) whose value explains the current one, and the wave steps there.  dist drops by >= 3 per step, so the walk ends.
#include "isdf_common.h"
#include "launchers.h"

namespace isdf {

constexpr int ROUTE_TILE = ISDF_ROUTE_TILE;
constexpr int ROUTE_INNER = 8;                          // sweeps inside a tile per launch, at most
constexpr int ROUTE_HALO = ROUTE_TILE + 2;
constexpr int ROUTE_ROW = 24;                           // words per LDS row (see above)
constexpr int ROUTE_PLANE = ROUTE_HALO * ROUTE_ROW;
constexpr int ROUTE_CELLS = ROUTE_HALO * ROUTE_HALO * ROUTE_HALO;
constexpr int32_t ROUTE_NONE = ISDF_ROUTE_NONE;
static_assert(ROUTE_TILE == 8, "the thread -> voxel map below is written for 8^3 tiles and 256 threads");

__global__ __launch_bounds__(256) void route_fill_kernel(int32_t* dist, int32_t n) {
  const int32_t p = (int32_t)blockIdx.x * 256 + threadIdx.x;
  if (p < n) dist[p] = ROUTE_NONE;
}

__global__ __launch_bounds__(256) void route_goals_kernel(const uint8_t* __restrict__ free, int nx, int ny, int nz,
                                                          const int32_t* __restrict__ goals, int32_t n_goals, int32_t* dist) {
  const int32_t g = (int32_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n_goals) return;
  const int i = goals[3 * (int64_t)g], j = goals[3 * (int64_t)g + 1], k = goals[3 * (int64_t)g + 2];
  if (i < 0 || j < 0 || k < 0 || i >= nx || j >= ny || k >= nz) return;
  const int32_t p = (i * ny + j) * nz + k;
  if (free[p]) dist[p] = 0;      // several goals on one voxel all store 0
}

int launch_route_init(const uint8_t* free, int32_t nx, int32_t ny, int32_t nz, const int32_t* goals, int32_t n_goals, int32_t* dist,
                      hipStream_t st) {
  const int32_t n = nx * ny * nz;
  hipLaunchKernelGGL(route_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dist, n);
  int rc = isdf_launch_status();
  if (rc || n_goals == 0) return rc;
  hipLaunchKernelGGL(route_goals_kernel, dim3((unsigned)((n_goals + 255) / 256)), dim3(256), 0, st, free, nx, ny, nz, goals, n_goals,
                     dist);
  return isdf_launch_status();
}

// one i-plane of a voxel's neighbourhood folded into `best`; w(p, q) = 2 + the number of coordinates that differ
__device__ __forceinline__ int32_t relax3(int32_t best, const int32_t (&v)[3][3], bool centre_is_self) {
  // v[dj+1][dk+1] of one i-plane; centre_is_self: the plane is the voxel's own (di = 0), whose centre is the voxel itself
  const int32_t face = v[1][1];
  int32_t edge = v[0][1] < v[2][1] ? v[0][1] : v[2][1];
  const int32_t e2 = v[1][0] < v[1][2] ? v[1][0] : v[1][2];
  edge = e2 < edge ? e2 : edge;
  int32_t corner = v[0][0] < v[0][2] ? v[0][0] : v[0][2];
  const int32_t c2 = v[2][0] < v[2][2] ? v[2][0] : v[2][2];
  corner = c2 < corner ? c2 : corner;
  // own plane: centre = self (+0), its in-plane faces +3, in-plane edges +4; a neighbouring plane: +3, +4, +5
  const int32_t base = centre_is_self ? 0 : 3;
  int32_t m = centre_is_self ? best : face + 3;
  m = m < best ? m : best;
  const int32_t a = edge + base + (centre_is_self ? 3 : 1);
  m = a < m ? a : m;
  const int32_t b = corner + base + (centre_is_self ? 4 : 2);
  return b < m ? b : m;
}

__global__ __launch_bounds__(256) void route_tile_kernel(const uint8_t* __restrict__ free, const int32_t* __restrict__ in,
                                                         int32_t* __restrict__ out, int nx, int ny, int nz, int tiles_j, int tiles_k,
                                                         int32_t* changed) {
  __shared__ int32_t s[ROUTE_HALO * ROUTE_PLANE];
  const int tid = threadIdx.x;
  const int tile = (int)blockIdx.x;
  const int tk = tile % tiles_k, tj = (tile / tiles_k) % tiles_j, ti = tile / (tiles_k * tiles_j);
  const int i0 = ti * ROUTE_TILE, j0 = tj * ROUTE_TILE, k0 = tk * ROUTE_TILE;
  // the tile and its halo; NONE outside the grid
  for (int t = tid; t < ROUTE_CELLS; t += 256) {
    const int c = t % ROUTE_HALO, b = (t / ROUTE_HALO) % ROUTE_HALO, a = t / (ROUTE_HALO * ROUTE_HALO);
    const int gi = i0 + a - 1, gj = j0 + b - 1, gk = k0 + c - 1;
    const bool inside = gi >= 0 && gj >= 0 && gk >= 0 && gi < nx && gj < ny && gk < nz;
    s[a * ROUTE_PLANE + b * ROUTE_ROW + c] = inside ? in[(gi * ny + gj) * nz + gk] : ROUTE_NONE;
  }
  // this thread's two voxels: (2 * ip, j, k) and (2 * ip + 1, j, k) of the tile
  const int k = tid & 7, j = (tid >> 3) & 7, ip = tid >> 6;
  const int gi = i0 + 2 * ip, gj = j0 + j, gk = k0 + k;
  const bool in0 = gi < nx && gj < ny && gk < nz, in1 = gi + 1 < nx && gj < ny && gk < nz;
  const int32_t g0 = in0 ? (gi * ny + gj) * nz + gk : 0, g1 = in1 ? g0 + ny * nz : 0;      // in1 implies in0
  const bool live0 = in0 && free[g0] != 0, live1 = in1 && free[g1] != 0;
  const int at = (2 * ip) * ROUTE_PLANE + j * ROUTE_ROW + k;      // LDS word of (a, b, c) = (2 ip, j, k): the neighbourhood's low corner
  __syncthreads();
  const int32_t first0 = s[at + ROUTE_PLANE + ROUTE_ROW + 1], first1 = s[at + 2 * ROUTE_PLANE + ROUTE_ROW + 1];
  int32_t cur0 = first0, cur1 = first1;
  for (int it = 0; it < ROUTE_INNER; ++it) {
    int32_t v[4][3][3];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[a][b][c] = s[at + a * ROUTE_PLANE + b * ROUTE_ROW + c];
    int32_t n0 = relax3(cur0, v[0], false);
    n0 = relax3(n0, v[1], true);
    n0 = relax3(n0, v[2], false);
    int32_t n1 = relax3(cur1, v[1], false);
    n1 = relax3(n1, v[2], true);
    n1 = relax3(n1, v[3], false);
    const bool low0 = live0 && n0 < cur0, low1 = live1 && n1 < cur1;
    // the barrier of the vote: every read of this sweep is done before any write below
    if (!__syncthreads_or(low0 || low1)) break;
    if (low0) s[at + ROUTE_PLANE + ROUTE_ROW + 1] = cur0 = n0;
    if (low1) s[at + 2 * ROUTE_PLANE + ROUTE_ROW + 1] = cur1 = n1;
    __syncthreads();
  }
  if (in0) out[g0] = cur0;
  if (in1) out[g1] = cur1;
  if (__syncthreads_or(cur0 < first0 || cur1 < first1) && tid == 0) *changed = 1;      // every block that stores, stores 1
}

int64_t route_volume_bytes(int32_t nx, int32_t ny, int32_t nz) { return ((int64_t)nx * ny * nz * 4 + 255) / 256 * 256; }

// one round: dist -> ws -> dist; changed[r] <- 1 iff either launch of round r lowered a voxel
int launch_route_relax(const uint8_t* free, int32_t nx, int32_t ny, int32_t nz, int32_t* dist, int32_t* ws, int32_t rounds,
                       int32_t* changed, hipStream_t st) {
  const hipError_t e = hipMemsetAsync(changed, 0, (size_t)rounds * sizeof(int32_t), st);
  if (e != hipSuccess) { g_isdf_last_hip_error = (int)e; return ISDF_EHIP; }
  const int ti = (nx + ROUTE_TILE - 1) / ROUTE_TILE, tj = (ny + ROUTE_TILE - 1) / ROUTE_TILE, tk = (nz + ROUTE_TILE - 1) / ROUTE_TILE;
  for (int32_t r = 0; r < rounds; ++r)
    for (int half = 0; half < 2; ++half) {
      const int32_t* in = half ? ws : dist;
      int32_t* out = half ? dist : ws;
      hipLaunchKernelGGL(route_tile_kernel, dim3((unsigned)(ti * tj * tk)), dim3(256), 0, st, free, in, out, nx, ny, nz, tj, tk,
                         changed + r);
      const int rc = isdf_launch_status();
      if (rc) return rc;
    }
  return ISDF_OK;
}

// neighbour m of 26 in the header's order: (di, dj, dk) lexicographic over -1..1 without (0, 0, 0)
__device__ __forceinline__ void route_neighbour(int m, int& di, int& dj, int& dk) {
  const int c = m < 13 ? m : m + 1;
  di = c / 9 - 1;
  dj = (c / 3) % 3 - 1;
  dk = c % 3 - 1;
}

__global__ __launch_bounds__(64) void route_trace_kernel(const int32_t* __restrict__ dist, int nx, int ny, int nz,
                                                         const int32_t* __restrict__ starts, int32_t max_len, int32_t* path,
                                                         int32_t* len) {
  const int b = (int)blockIdx.x, lane = threadIdx.x;
  int i = starts[3 * (int64_t)b], j = starts[3 * (int64_t)b + 1], k = starts[3 * (int64_t)b + 2];
  int32_t* row = path + (int64_t)b * max_len;
  if (i < 0 || j < 0 || k < 0 || i >= nx || j >= ny || k >= nz || dist[(i * ny + j) * nz + k] >= ROUTE_NONE) {
    if (lane == 0) len[b] = 0;
    return;
  }
  int ldi, ldj, ldk;
  route_neighbour(lane < 26 ? lane : 0, ldi, ldj, ldk);
  const int32_t lw = 2 + (ldi != 0) + (ldj != 0) + (ldk != 0);
  int32_t n = 0, result;
  for (;;) {                                 // everything below is wave-uniform except the neighbour reads
    if (n == max_len) { result = -1; break; }
    const int32_t p = (i * ny + j) * nz + k;
    if (lane == 0) row[n] = p;
    ++n;
    const int32_t d = dist[p];
    if (d == 0) { result = n; break; }
    const int qi = i + ldi, qj = j + ldj, qk = k + ldk;
    bool match = false;
    if (lane < 26 && qi >= 0 && qj >= 0 && qk >= 0 && qi < nx && qj < ny && qk < nz)
      match = dist[(qi * ny + qj) * nz + qk] + lw == d;
    const unsigned long long mask = __ballot(match);
    if (mask == 0) { result = -1; break; }
    int di, dj, dk;
    route_neighbour(__ffsll(mask) - 1, di, dj, dk);
    i += di, j += dj, k += dk;
  }
  if (lane == 0) len[b] = result;
}

int launch_route_trace(const int32_t* dist, int32_t nx, int32_t ny, int32_t nz, const int32_t* starts, int32_t B, int32_t max_len,
                       int32_t* path, int32_t* len, hipStream_t st) {
  if (B == 0) return ISDF_OK;
  hipLaunchKernelGGL(route_trace_kernel, dim3((unsigned)B), dim3(64), 0, st, dist, nx, ny, nz, starts, max_len, path, len);
  return isdf_launch_status();
}

}  // namespace isdf
