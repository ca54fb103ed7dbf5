// Ground truth from a triangle mesh (include/isdf_hip.h: isdf_tri_pack, isdf_tri_distance): for every query point the distance to
// the nearest triangle and the generalised winding number of the mesh, by brute force over points x triangles -- the exact
// version of the reference's voxelise / fill / two distance transforms (sdf_util.py:388-457, sdf_from_mesh*).
//   pack      one thread per slot: index check, gather, optional affine, validity, the per-triangle constants of the sequence
//   distance  block (x, y): TRI_Q queries per thread (1024 per block) against the tiles of triangle chunk y.  A tile of TRI_TILE
//             packed triangles sits in LDS; every lane reads the SAME address (broadcast ds_read_b128, six per triangle), and each
//             triangle feeds the TRI_Q queries held in registers.  Squared distance and index go into the query's 64-bit key by an
//             integer atomic minimum, as eval.hip's nn_kernel does; the solid angles are summed in a double per query, in
//             triangle order, one partial per chunk.
//   finish    key -> distance, index, the closest point recomputed with the same sequence; the chunks' winding partials added in
//             chunk order; the record's per-block partials, combined in block order by a closing block.
// The chunking is a function of n and m alone (tri_splits), so every output repeats bit for bit run to run.
#include "isdf_common.h"
#include "launchers.h"
#include "block_reduce.h"
#include "tri_dev.h"

namespace isdf {

struct TriAffine { float a[12]; };

// the header's split rule: about 1024 blocks, never more chunks than tiles
int64_t tri_splits(int64_t n, int64_t m) {
  const int64_t qblocks = (n + 256 * TRI_Q - 1) / (256 * TRI_Q);
  const int64_t tiles = (m + TRI_TILE - 1) / TRI_TILE;
  int64_t splits = qblocks > 0 ? (1024 + qblocks - 1) / qblocks : 1;
  if (splits > tiles) splits = tiles;
  if (splits > 65535) splits = 65535;
  if (splits < 1) splits = 1;
  const int64_t chunk_tiles = tiles > 0 ? (tiles + splits - 1) / splits : 1;
  return tiles > 0 ? (tiles + chunk_tiles - 1) / chunk_tiles : 1;
}

static int64_t tri_chunk_tiles(int64_t n, int64_t m) {
  const int64_t tiles = (m + TRI_TILE - 1) / TRI_TILE;
  const int64_t splits = tri_splits(n, m);
  return (tiles + splits - 1) / splits;
}

// ---- pack ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tri_pack_kernel(const float* __restrict__ verts, int64_t nv, const int32_t* __restrict__ faces,
                                                       int64_t m, int64_t slots, int has_T, const TriAffine T,
                                                       float* __restrict__ packed, int32_t* __restrict__ counts) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= slots) return;
  float o[TRI_SLOT];
#pragma unroll
  for (int k = 0; k < TRI_SLOT; ++k) o[k] = 0.f;
  if (s < m) {
    const int64_t i0 = faces[s * 3], i1 = faces[s * 3 + 1], i2 = faces[s * 3 + 2];
    // the indices are checked before anything is read through them
    bool ok = i0 >= 0 && i0 < nv && i1 >= 0 && i1 < nv && i2 >= 0 && i2 < nv;
    float p[3][3];
    if (ok) {
      const int64_t id[3] = {i0, i1, i2};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float x = verts[id[c] * 3], y = verts[id[c] * 3 + 1], z = verts[id[c] * 3 + 2];
        if (has_T) {
#pragma unroll
          for (int r = 0; r < 3; ++r) p[c][r] = ((T.a[r * 4] * x + T.a[r * 4 + 1] * y) + T.a[r * 4 + 2] * z) + T.a[r * 4 + 3];
        } else {
          p[c][0] = x; p[c][1] = y; p[c][2] = z;
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) ok = ok && isfinite(p[c][r]);
      }
    }
    if (!ok) {
      atomicAdd(&counts[0], 1);
    } else {
      const float abx = p[1][0] - p[0][0], aby = p[1][1] - p[0][1], abz = p[1][2] - p[0][2];
      const float acx = p[2][0] - p[0][0], acy = p[2][1] - p[0][1], acz = p[2][2] - p[0][2];
      const float nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
      const float nn = (nx * nx + ny * ny) + nz * nz;
      if (!(nn > 0.f)) {
        atomicAdd(&counts[1], 1);
      } else {
        o[0] = p[0][0]; o[1] = p[0][1]; o[2] = p[0][2]; o[3] = (abx * abx + aby * aby) + abz * abz;
        o[4] = abx; o[5] = aby; o[6] = abz; o[7] = (abx * acx + aby * acy) + abz * acz;
        o[8] = acx; o[9] = acy; o[10] = acz; o[11] = (acx * acx + acy * acy) + acz * acz;
        o[12] = p[1][0]; o[13] = p[1][1]; o[14] = p[1][2]; o[15] = 1.f;
        o[16] = p[2][0]; o[17] = p[2][1]; o[18] = p[2][2];
        // the unit normal: sqrtf(fl(x * x)) == |x|, so an axis-aligned face gets +-1 and zeros exactly
        const float ln = sqrtf(nn);
        o[20] = __fdiv_rn(nx, ln); o[21] = __fdiv_rn(ny, ln); o[22] = __fdiv_rn(nz, ln);
      }
    }
  }
  float4* dst = (float4*)(packed + s * TRI_SLOT);
#pragma unroll
  for (int k = 0; k < TRI_SLOT / 4; ++k) dst[k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
}

template <bool WIND>
__global__ __launch_bounds__(256) void tri_distance_kernel(const float* __restrict__ pts, int64_t n, const float* __restrict__ packed,
                                                           int64_t slots, int64_t chunk, unsigned long long* __restrict__ keys,
                                                           double* __restrict__ wpart) {
  __shared__ float4 sh[TRI_TILE * (TRI_SLOT / 4)];
  const int64_t q0 = (int64_t)blockIdx.x * (256 * TRI_Q) + threadIdx.x;
  float px[TRI_Q], py[TRI_Q], pz[TRI_Q], best[TRI_Q];
  uint32_t bi[TRI_Q];
  double wsum[TRI_Q];
#pragma unroll
  for (int j = 0; j < TRI_Q; ++j) {
    const int64_t q = q0 + j * 256;
    const bool ok = q < n;
    px[j] = ok ? pts[q * 3] : 0.f; py[j] = ok ? pts[q * 3 + 1] : 0.f; pz[j] = ok ? pts[q * 3 + 2] : 0.f;
    best[j] = INFINITY; bi[j] = 0xffffffffu; wsum[j] = 0.0;
  }
  const int64_t t0 = (int64_t)blockIdx.y * chunk;                    // chunk is a multiple of TRI_TILE, slots too
  const int64_t t1 = t0 + chunk < slots ? t0 + chunk : slots;
  const float4* __restrict__ src = (const float4*)packed;
  for (int64_t base = t0; base < t1; base += TRI_TILE) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TRI_SLOT / 4; ++j) sh[threadIdx.x + j * 256] = src[base * (TRI_SLOT / 4) + threadIdx.x + j * 256];
    __syncthreads();
    for (int k = 0; k < TRI_TILE; ++k) {
      const float4 A = sh[k * 6], B = sh[k * 6 + 1], Cc = sh[k * 6 + 2], D = sh[k * 6 + 3], E = sh[k * 6 + 4], N = sh[k * 6 + 5];
      const TriCore t = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w, Cc.x, Cc.y, Cc.z, Cc.w, N.x, N.y, N.z};
      const bool valid = D.w != 0.f;
      const uint32_t idx = (uint32_t)(base + k);
#pragma unroll
      for (int j = 0; j < TRI_Q; ++j) {
        const float apx = px[j] - t.ax, apy = py[j] - t.ay, apz = pz[j] - t.az;
        float d2 = tri_dist2(t, apx, apy, apz);
        d2 = valid ? d2 : INFINITY;                                  // a skipped or padding slot never wins
        if (d2 < best[j]) { best[j] = d2; bi[j] = idx; }             // ascending index, strict: the lowest index of a tie
        if (WIND) {
          const float om = tri_solid_angle(-apx, -apy, -apz, D.x - px[j], D.y - py[j], D.z - pz[j], E.x - px[j], E.y - py[j],
                                           E.z - pz[j]);
          wsum[j] += (double)(valid ? om : 0.f);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < TRI_Q; ++j) {
    const int64_t q = q0 + j * 256;
    if (q < n) {
      atomicMin(&keys[q], ((unsigned long long)__float_as_uint(best[j]) << 32) | bi[j]);
      if (WIND) wpart[(int64_t)blockIdx.y * n + q] = wsum[j];
    }
  }
}

__global__ __launch_bounds__(256) void tri_finish_kernel(const float* __restrict__ pts, int64_t n, const float* __restrict__ packed,
                                                         const unsigned long long* __restrict__ keys,
                                                         const double* __restrict__ wpart, int64_t splits, float* __restrict__ dist,
                                                         int32_t* __restrict__ index, float* __restrict__ closest,
                                                         float* __restrict__ winding, double* __restrict__ part) {
  __shared__ double sh[4][TRI_REC];
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double acc[TRI_REC] = {0.0, 0.0, 0.0, 0.0};
  if (q < n) {
    const float x = pts[q * 3], y = pts[q * 3 + 1], z = pts[q * 3 + 2];
    const unsigned long long key = keys[q];
    const uint32_t bi = (uint32_t)key;
    // no valid triangle (the key may still be the initial all-ones pattern of an empty mesh): +inf.  sqrtf is the correctly
    // rounded square root here; __fsqrt_rn is the hardware's, which measured one ulp low at one point in nine
    float d = bi != 0xffffffffu ? sqrtf(__uint_as_float((uint32_t)(key >> 32))) : INFINITY;
    float cx = NAN, cy = NAN, cz = NAN, wn = 0.f;
    int32_t id = -1;
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) {
      d = NAN; wn = NAN;
      acc[2] = 1.0;
    } else {
      if (bi != 0xffffffffu) {
        id = (int32_t)bi;
        const float4* s = (const float4*)(packed + (int64_t)bi * TRI_SLOT);
        const float4 A = s[0], B = s[1], Cc = s[2];
        const TriCore t = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w, Cc.x, Cc.y, Cc.z, Cc.w, 0.f, 0.f, 0.f};
        float v, w;
        bool face;
        tri_weights(t, x - t.ax, y - t.ay, z - t.az, v, w, face);
        cx = t.ax + (t.abx * v + t.acx * w); cy = t.ay + (t.aby * v + t.acy * w); cz = t.az + (t.abz * v + t.acz * w);
      }
      if (winding) {
        double s = 0.0;
        for (int64_t c = 0; c < splits; ++c) s += wpart[c * n + q];          // chunk order
        wn = (float)(s / 12.566370614359172);                                // 4 pi
      }
      acc[0] = (double)d; acc[1] = 1.0; acc[3] = (double)d;
    }
    if (dist) dist[q] = d;
    if (index) index[q] = id;
    if (closest) { closest[q * 3] = cx; closest[q * 3 + 1] = cy; closest[q * 3 + 2] = cz; }
    if (winding) winding[q] = wn;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int v = 0; v < TRI_REC; ++v) {
    const double t = v == 3 ? wave_reduce<RedMax>(acc[v]) : wave_reduce<RedSum>(acc[v]);
    if (lane == 0) sh[wave][v] = t;
  }
  __syncthreads();
  if (threadIdx.x < TRI_REC) {
    const int v = threadIdx.x;
    part[(int64_t)blockIdx.x * TRI_REC + v] = v == 3 ? waves_combine<RedMax>(sh[0][v], sh[1][v], sh[2][v], sh[3][v])
                                                     : waves_combine<RedSum>(sh[0][v], sh[1][v], sh[2][v], sh[3][v]);
  }
}

int launch_tri_pack(const float* verts, int64_t nv, const int32_t* faces, int64_t m, const float* T, float* packed, int32_t* counts,
                    hipStream_t st) {
  const hipError_t e = hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), st);
  if (e != hipSuccess) { g_isdf_last_hip_error = (int)e; return ISDF_EHIP; }
  const int64_t slots = (m + TRI_TILE - 1) / TRI_TILE * TRI_TILE;
  if (slots == 0) return ISDF_OK;
  TriAffine A = {};
  if (T)
    for (int k = 0; k < 12; ++k) A.a[k] = T[k];
  hipLaunchKernelGGL(tri_pack_kernel, dim3((unsigned)(slots / 256 + (slots % 256 != 0))), dim3(256), 0, st, verts, nv, faces, m, slots,
                     T ? 1 : 0, A, packed, counts);
  return isdf_launch_status();
}

// key -> outputs, then the record: the closing launches of both the brute-force and the tile-culled distance (tri_tiles.hip)
int launch_tri_finish(const float* pts, int64_t n, const float* packed, const unsigned long long* keys, const double* wpart,
                      int64_t splits, float* dist, int32_t* index, float* closest, float* winding, double* record, double* part,
                      hipStream_t st) {
  const int64_t fin = (n + 255) / 256;
  if (n > 0) {
    hipLaunchKernelGGL(tri_finish_kernel, dim3((unsigned)fin), dim3(256), 0, st, pts, n, packed, keys, wpart, splits, dist, index,
                       closest, winding, part);
    const int rc = isdf_launch_status();
    if (rc) return rc;
  }
  return launch_reduce_partials(part, fin, TRI_REC, 1u << 3, record, st);      // the three sums, and the maximum of entry 3
}

int launch_tri_distance(const float* pts, int64_t n, const float* packed, int64_t m, float* dist, int32_t* index, float* closest,
                        float* winding, double* record, void* workspace, hipStream_t st) {
  unsigned long long* keys = (unsigned long long*)workspace;
  const int64_t splits = tri_splits(n, m);
  double* wpart = (double*)(keys + n);
  double* part = wpart + splits * n;
  const int64_t slots = (m + TRI_TILE - 1) / TRI_TILE * TRI_TILE;
  if (n > 0) {
    const hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)n * 8, st);   // every key starts above any (distance, index)
    if (e != hipSuccess) { g_isdf_last_hip_error = (int)e; return ISDF_EHIP; }
    if (slots > 0) {
      const int64_t qblocks = (n + 256 * TRI_Q - 1) / (256 * TRI_Q);
      const int64_t chunk = tri_chunk_tiles(n, m) * TRI_TILE;
      const dim3 grid((unsigned)qblocks, (unsigned)splits);
      if (winding)
        hipLaunchKernelGGL(tri_distance_kernel<true>, grid, dim3(256), 0, st, pts, n, packed, slots, chunk, keys, wpart);
      else
        hipLaunchKernelGGL(tri_distance_kernel<false>, grid, dim3(256), 0, st, pts, n, packed, slots, chunk, keys, wpart);
      const int rc = isdf_launch_status();
      if (rc) return rc;
    }
  }
  // an empty mesh launches no distance kernel: the finish reads no winding partial then
  return launch_tri_finish(pts, n, packed, keys, wpart, slots > 0 ? splits : 0, dist, index, closest, winding, record, part, st);
}

}  // namespace isdf
