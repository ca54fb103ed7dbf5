// Exact mesh distance at scan scale (include/isdf_hip.h: isdf_tri_tiles_build, isdf_tri_distance_tiles): a flat index with one box
// and one dipole per tile of ISDF_TRI_TILE triangles, and the brute-force kernel's loop (tri.hip) over the tiles that survive a
// conservative test against the query block's box.
//   build     one workgroup per tile of the caller's `order`: every entry checked, then the valid slots' box, area vector N,
//             area-weighted centroid c, radius r about c, area, count and extent; the sums in double through block_reduce.h's order.
//   distance  one block per 1024 entries of `qperm` (TRI_Q per thread, as tri.hip).  The block's box, then the header's rule: a seed
//             tile, U = the block's worst running best dist2, and every further tile staged iff its box may still hold a triangle
//             no farther than sqrt(U).  A staged tile is gathered through `order_clean` into tri.hip's LDS layout, the slot index
//             beside it; the per-pair sequence is tri_dev.h's, so dist2 has tri.hip's bits, and the winner is the (dist2, index)
//             minimum, which no visiting order changes.  Winding number: a tile far from the block's box adds its dipole term per
//             query, a near one is staged and adds tri.hip's fp32 solid angles; visiting order, then slot order, in a double per query.
//   finish    tri.hip's tri_finish_kernel and the record's closing launch, unchanged (launch_tri_finish), with one winding partial.
#include "isdf_common.h"
#include "launchers.h"
#include "block_reduce.h"
#include "tri_dev.h"

namespace isdf {

constexpr int TILE_REC = ISDF_TRI_TILE_RECORD;
constexpr double TILE_EPS = ISDF_TRI_TILE_EPS;

// lo <- the block's minimum, hi <- its maximum, in every thread (a minimum and a maximum have no order to fix); two barriers
__device__ __forceinline__ void block_box(float (&lo)[3], float (&hi)[3], float (*shb)[6]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo[k] = fminf(lo[k], __shfl_xor(lo[k], o, 64));
      hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o, 64));
    }
  }
  __syncthreads();                                                     // earlier readers of shb are done
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { shb[threadIdx.x >> 6][k] = lo[k]; shb[threadIdx.x >> 6][3 + k] = hi[k]; }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = fminf(fminf(shb[0][k], shb[1][k]), fminf(shb[2][k], shb[3][k]));
    hi[k] = fmaxf(fmaxf(shb[0][3 + k], shb[1][3 + k]), fmaxf(shb[2][3 + k], shb[3][3 + k]));
  }
}

// ---- build ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tri_tiles_build_kernel(const float* __restrict__ packed, int64_t slots,
                                                              const int32_t* __restrict__ order, double* __restrict__ tiles,
                                                              int32_t* __restrict__ order_clean, int32_t* __restrict__ counts) {
  __shared__ double sh[4][7];
  __shared__ double res[7];
  __shared__ double sh2[4][2];
  __shared__ float shb[4][6];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t i = (int64_t)blockIdx.x * TRI_TILE + tid;
  const int32_t e = order[i];
  // the entry is checked before anything is read through it
  const bool listed = e >= 0 && (int64_t)e < slots;
  double p[3][3] = {};
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  bool valid = false;
  if (listed) {
    const float4* s = (const float4*)(packed + (int64_t)e * TRI_SLOT);
    const float4 A = s[0], D = s[3], E = s[4];
    valid = D.w != 0.f;
    if (valid) {
      const float f[3][3] = {{A.x, A.y, A.z}, {D.x, D.y, D.z}, {E.x, E.y, E.z}};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          p[c][k] = (double)f[c][k];
          lo[k] = fminf(lo[k], f[c][k]);
          hi[k] = fmaxf(hi[k], f[c][k]);
        }
      }
    }
  }
  order_clean[i] = valid ? e : -1;
  const int n_bad = __syncthreads_count(!listed && e != -1);
  const int n_valid = __syncthreads_count(valid);
  if (tid == 0) {
    if (n_bad) atomicAdd(&counts[0], n_bad);
    if (n_valid) atomicAdd(&counts[1], n_valid);
  }
  block_box(lo, hi, shb);
  // N = sum of the area vectors, area * centroid, area: zero terms for the slots that are not valid
  const double abx = p[1][0] - p[0][0], aby = p[1][1] - p[0][1], abz = p[1][2] - p[0][2];
  const double acx = p[2][0] - p[0][0], acy = p[2][1] - p[0][1], acz = p[2][2] - p[0][2];
  const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
  const double area = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
  const double acc[7] = {0.5 * nx, 0.5 * ny, 0.5 * nz, area * (((p[0][0] + p[1][0]) + p[2][0]) / 3.0),
                         area * (((p[0][1] + p[1][1]) + p[2][1]) / 3.0), area * (((p[0][2] + p[1][2]) + p[2][2]) / 3.0), area};
  block_record_sum<7>(acc, sh, res);
  __syncthreads();
  const double cx = n_valid ? res[3] / res[6] : 0.0, cy = n_valid ? res[4] / res[6] : 0.0, cz = n_valid ? res[5] / res[6] : 0.0;
  // r^2 = the largest squared distance of a valid slot's vertex from c; extent = one past the last valid slot of the tile
  double far2 = 0.0;
  if (valid) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double dx = p[c][0] - cx, dy = p[c][1] - cy, dz = p[c][2] - cz;
      far2 = fmax(far2, (dx * dx + dy * dy) + dz * dz);
    }
  }
  const double acc2[2] = {far2, valid ? (double)(tid + 1) : 0.0};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double t = wave_reduce<RedMax>(acc2[k]);
    if (lane == 0) sh2[wave][k] = t;
  }
  __syncthreads();
  if (tid == 0) {
    double* rec = tiles + (int64_t)blockIdx.x * TILE_REC;
    const double r2 = waves_combine<RedMax>(sh2[0][0], sh2[1][0], sh2[2][0], sh2[3][0]);
    rec[0] = (double)lo[0]; rec[1] = (double)lo[1]; rec[2] = (double)lo[2];
    rec[3] = (double)hi[0]; rec[4] = (double)hi[1]; rec[5] = (double)hi[2];
    rec[6] = res[0]; rec[7] = res[1]; rec[8] = res[2];
    rec[9] = cx; rec[10] = cy; rec[11] = cz;
    rec[12] = sqrt(r2);
    rec[13] = res[6];
    rec[14] = (double)n_valid;
    rec[15] = waves_combine<RedMax>(sh2[0][1], sh2[1][1], sh2[2][1], sh2[3][1]);
  }
}

// ---- the rule (the header states it) ----------------------------------------------------------------------------------------
// mind and maxd between the block's box [bl, bh] and the tile's, each sum as (x + y) + z
__device__ __forceinline__ void tile_bounds(const double* __restrict__ rec, const double (&bl)[3], const double (&bh)[3], double& mind,
                                            double& maxd) {
  double g[3], h[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double tl = rec[k], th = rec[3 + k];
    g[k] = fmax(0.0, fmax(tl - bh[k], bl[k] - th));
    h[k] = fmax(fabs(th - bl[k]), fabs(bh[k] - tl));
  }
  mind = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
  maxd = sqrt((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]);
}

// one staged tile against the thread's queries: the distance (DOD), the fp32 solid angles (DOW), or both
template <bool DOD, bool DOW>
__device__ __forceinline__ void tile_pass(const float4* __restrict__ sh, const uint32_t* __restrict__ shi, int extent,
                                          const float (&px)[TRI_Q], const float (&py)[TRI_Q], const float (&pz)[TRI_Q],
                                          float (&best)[TRI_Q], uint32_t (&bi)[TRI_Q], double (&wsum)[TRI_Q]) {
  for (int k = 0; k < extent; ++k) {
    const float4 A = sh[k * 6], B = sh[k * 6 + 1], Cc = sh[k * 6 + 2], D = sh[k * 6 + 3], E = sh[k * 6 + 4], N = sh[k * 6 + 5];
    const TriCore t = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w, Cc.x, Cc.y, Cc.z, Cc.w, N.x, N.y, N.z};
    const bool valid = D.w != 0.f;
    const uint32_t idx = shi[k];
#pragma unroll
    for (int j = 0; j < TRI_Q; ++j) {
      const float apx = px[j] - t.ax, apy = py[j] - t.ay, apz = pz[j] - t.az;
      if (DOD) {
        float d2 = tri_dist2(t, apx, apy, apz);
        d2 = valid ? d2 : INFINITY;                                    // a skipped or padding slot never wins
        // the minimum of (dist2, index): what tri.hip's ascending strict loop and its atomic minimum leave
        if (d2 < best[j] || (d2 == best[j] && idx < bi[j])) { best[j] = d2; bi[j] = idx; }
      }
      if (DOW) {
        const float om = tri_solid_angle(-apx, -apy, -apz, D.x - px[j], D.y - py[j], D.z - pz[j], E.x - px[j], E.y - py[j],
                                         E.z - pz[j]);
        wsum[j] += (double)(valid ? om : 0.f);
      }
    }
  }
}

template <bool WIND>
__global__ __launch_bounds__(256) void tri_tiles_distance_kernel(const float* __restrict__ pts, int64_t n,
                                                                 const int32_t* __restrict__ qperm, const float* __restrict__ packed,
                                                                 int64_t slots, const double* __restrict__ tiles,
                                                                 const int32_t* __restrict__ order_clean, int n_tiles, double beta,
                                                                 unsigned long long* __restrict__ keys, double* __restrict__ wpart,
                                                                 unsigned long long* __restrict__ stats) {
  __shared__ float4 sh[TRI_TILE * (TRI_SLOT / 4)];
  __shared__ uint32_t shi[TRI_TILE];
  __shared__ float shb[4][6];
  __shared__ float shu[4];
  __shared__ double shm[4];
  __shared__ int sht[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t i0 = (int64_t)blockIdx.x * (256 * TRI_Q) + tid;
  float px[TRI_Q], py[TRI_Q], pz[TRI_Q], best[TRI_Q];
  uint32_t bi[TRI_Q];
  int32_t qi[TRI_Q];
  double wsum[TRI_Q];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  int skipped = 0;
#pragma unroll
  for (int j = 0; j < TRI_Q; ++j) {
    const int64_t i = i0 + j * 256;
    int32_t q = -1;
    if (i < n) {
      q = qperm[i];
      // the entry is checked before anything is read or written through it
      if (q < 0 || (int64_t)q >= n) { q = -1; ++skipped; }
    }
    float x = 0.f, y = 0.f, z = 0.f;
    if (q >= 0) { x = pts[(int64_t)q * 3]; y = pts[(int64_t)q * 3 + 1]; z = pts[(int64_t)q * 3 + 2]; }
    // a non-finite point takes no part: tri_finish_kernel writes its NaN from the point itself
    if (!(q >= 0 && isfinite(x) && isfinite(y) && isfinite(z))) { q = -1; x = y = z = 0.f; }
    qi[j] = q; px[j] = x; py[j] = y; pz[j] = z;
    best[j] = INFINITY; bi[j] = 0xffffffffu; wsum[j] = 0.0;
    if (q >= 0) {
      lo[0] = fminf(lo[0], x); lo[1] = fminf(lo[1], y); lo[2] = fminf(lo[2], z);
      hi[0] = fmaxf(hi[0], x); hi[1] = fmaxf(hi[1], y); hi[2] = fmaxf(hi[2], z);
    }
  }
  if (stats && skipped) atomicAdd(&stats[3], (unsigned long long)skipped);
  if (stats && tid == 0) atomicAdd(&stats[2], 1ull);
  block_box(lo, hi, shb);
  if (!(lo[0] <= hi[0])) return;                                       // no finite query in the block: nothing is staged
  const double bl[3] = {(double)lo[0], (double)lo[1], (double)lo[2]}, bh[3] = {(double)hi[0], (double)hi[1], (double)hi[2]};

  // the seed: the lowest non-empty tile with the least maxd
  double sm = INFINITY;
  int stile = 0x7fffffff;
  for (int t = tid; t < n_tiles; t += 256) {
    const double* rec = tiles + (int64_t)t * TILE_REC;
    if (rec[14] > 0.0) {
      double mind, maxd;
      tile_bounds(rec, bl, bh, mind, maxd);
      if (maxd < sm) { sm = maxd; stile = t; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double om = __shfl_xor(sm, o, 64);
    const int ot = __shfl_xor(stile, o, 64);
    if (om < sm || (om == sm && ot < stile)) { sm = om; stile = ot; }
  }
  if (lane == 0) { shm[wave] = sm; sht[wave] = stile; }
  __syncthreads();
  sm = shm[0]; stile = sht[0];
#pragma unroll
  for (int w = 1; w < 4; ++w)
    if (shm[w] < sm || (shm[w] == sm && sht[w] < stile)) { sm = shm[w]; stile = sht[w]; }
  const int seed = __builtin_amdgcn_readfirstlane(stile);
  if (seed == 0x7fffffff) return;                                      // no valid face is listed

  const float4* __restrict__ src = (const float4*)packed;
  float U = INFINITY;
  unsigned long long n_dist = 0, n_near = 0;
  for (int v = -1; v < n_tiles; ++v) {
    if (v == seed) continue;
    const int t = v < 0 ? seed : v;
    const double* rec = tiles + (int64_t)t * TILE_REC;
    if (!(rec[14] > 0.0)) continue;                                    // an empty tile is never visited
    double mind, maxd;
    tile_bounds(rec, bl, bh, mind, maxd);
    const bool do_dist = v < 0 || mind - TILE_EPS * maxd <= sqrt((double)U);
    bool near = false;
    if (WIND) {
      const double cx = rec[9], cy = rec[10], cz = rec[11];
      const double ex = fmax(0.0, fmax(cx - bh[0], bl[0] - cx)), ey = fmax(0.0, fmax(cy - bh[1], bl[1] - cy)),
                   ez = fmax(0.0, fmax(cz - bh[2], bl[2] - cz));
      const double dc = sqrt((ex * ex + ey * ey) + ez * ez);
      near = !(beta > 0.0) || !(dc >= beta * rec[12]);
      if (!near) {
        const double Nx = rec[6], Ny = rec[7], Nz = rec[8];
#pragma unroll
        for (int j = 0; j < TRI_Q; ++j) {
          const double dx = cx - (double)px[j], dy = cy - (double)py[j], dz = cz - (double)pz[j];
          const double r2 = (dx * dx + dy * dy) + dz * dz;
          wsum[j] += ((Nx * dx + Ny * dy) + Nz * dz) / (r2 * sqrt(r2));
        }
      }
    }
    if (!do_dist && !near) continue;
    n_dist += do_dist; n_near += near;
    __syncthreads();                                                   // the previous tile's readers are done
    const int64_t base = (int64_t)t * TRI_TILE;
#pragma unroll
    for (int j = 0; j < TRI_SLOT / 4; ++j) {
      const int f = tid + j * 256;
      const int32_t e = order_clean[base + f / (TRI_SLOT / 4)];
      // checked again here: nothing is read through an entry outside the packed buffer, whoever wrote order_clean
      sh[f] = (e >= 0 && (int64_t)e < slots) ? src[(int64_t)e * (TRI_SLOT / 4) + f % (TRI_SLOT / 4)] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    shi[tid] = (uint32_t)order_clean[base + tid];
    __syncthreads();
    int extent = (int)rec[15];
    extent = extent < 0 ? 0 : extent > TRI_TILE ? TRI_TILE : extent;
    if (do_dist && near) tile_pass<true, WIND>(sh, shi, extent, px, py, pz, best, bi, wsum);
    else if (do_dist) tile_pass<true, false>(sh, shi, extent, px, py, pz, best, bi, wsum);
    else tile_pass<false, WIND>(sh, shi, extent, px, py, pz, best, bi, wsum);
    if (do_dist) {
      // U: the largest running best dist2 over the block's finite queries
      float u = -INFINITY;
#pragma unroll
      for (int j = 0; j < TRI_Q; ++j) u = qi[j] >= 0 ? fmaxf(u, best[j]) : u;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) u = fmaxf(u, __shfl_xor(u, o, 64));
      if (lane == 0) shu[wave] = u;
      __syncthreads();
      U = fmaxf(fmaxf(shu[0], shu[1]), fmaxf(shu[2], shu[3]));
    }
  }
#pragma unroll
  for (int j = 0; j < TRI_Q; ++j) {
    if (qi[j] >= 0) {
      if (!(best[j] < INFINITY)) bi[j] = 0xffffffffu;                  // an infinite dist2 never wins (tri.hip's strict comparison)
      keys[qi[j]] = ((unsigned long long)__float_as_uint(best[j]) << 32) | bi[j];
      if (WIND) wpart[qi[j]] = wsum[j];
    }
  }
  if (stats && tid == 0) {
    atomicAdd(&stats[0], n_dist);
    atomicAdd(&stats[1], n_near);
  }
}

int launch_tri_tiles_build(const float* packed, int64_t m, const int32_t* order, int64_t n_order, double* tiles, int32_t* order_clean,
                           int32_t* counts, hipStream_t st) {
  const hipError_t e = hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), st);
  if (e != hipSuccess) { g_isdf_last_hip_error = (int)e; return ISDF_EHIP; }
  if (n_order == 0) return ISDF_OK;
  const int64_t slots = (m + TRI_TILE - 1) / TRI_TILE * TRI_TILE;
  hipLaunchKernelGGL(tri_tiles_build_kernel, dim3((unsigned)(n_order / TRI_TILE)), dim3(256), 0, st, packed, slots, order, tiles,
                     order_clean, counts);
  return isdf_launch_status();
}

int launch_tri_distance_tiles(const float* pts, int64_t n, const int32_t* qperm, const float* packed, int64_t m, const double* tiles,
                              const int32_t* order_clean, int64_t n_tiles, double beta, float* dist, int32_t* index, float* closest,
                              float* winding, double* record, int64_t* stats, void* workspace, hipStream_t st) {
  unsigned long long* keys = (unsigned long long*)workspace;
  double* wpart = (double*)(keys + n);
  double* part = wpart + n;
  hipError_t e = stats ? hipMemsetAsync(stats, 0, 4 * sizeof(int64_t), st) : hipSuccess;
  // every key starts above any (distance, index); a query that qperm does not list keeps that and a winding sum of zero
  if (e == hipSuccess && n > 0) e = hipMemsetAsync(keys, 0xff, (size_t)n * 8, st);
  if (e == hipSuccess && n > 0 && winding) e = hipMemsetAsync(wpart, 0, (size_t)n * 8, st);
  if (e != hipSuccess) { g_isdf_last_hip_error = (int)e; return ISDF_EHIP; }
  if (n > 0 && n_tiles > 0) {
    const int64_t slots = (m + TRI_TILE - 1) / TRI_TILE * TRI_TILE;
    const dim3 grid((unsigned)((n + 256 * TRI_Q - 1) / (256 * TRI_Q)));
    if (winding)
      hipLaunchKernelGGL(tri_tiles_distance_kernel<true>, grid, dim3(256), 0, st, pts, n, qperm, packed, slots, tiles, order_clean,
                         (int)n_tiles, beta, keys, wpart, (unsigned long long*)stats);
    else
      hipLaunchKernelGGL(tri_tiles_distance_kernel<false>, grid, dim3(256), 0, st, pts, n, qperm, packed, slots, tiles, order_clean,
                         (int)n_tiles, beta, keys, wpart, (unsigned long long*)stats);
    const int rc = isdf_launch_status();
    if (rc) return rc;
  }
  return launch_tri_finish(pts, n, packed, keys, wpart, 1, dist, index, closest, winding, record, part, st);
}

}  // namespace isdf
