// Evaluation of the map against ground truth (Trainer.eval_sdf / eval_object_sdf / eval_traj_cost / eval_mesh,
// trainer.py:1819-2064):
//   sdf_util.eval_sdf_interp(handle_oob='mask')   isdf/datasets/sdf_util.py:183-216  (scipy's linear RegularGridInterpolator
//                                                 over an axis-aligned grid, sdf_util.py:151-180)
//   metrics.binned_losses                         isdf/eval/metrics.py:133-158
//   metrics.chomp_cost                            isdf/eval/metrics.py:95-104
//   metrics.accuracy / completion                 isdf/eval/metrics.py:48-59        (nearest-neighbour distances, brute force)
// Both reductions are deterministic: per-block partial sums in double (block_reduce.h), combined in block order by one closing
// block (reduce.hip); the nearest neighbour is a minimum over integer keys (squared distance bits, then index), which no order can
// change.
#include "isdf_common.h"
#include "launchers.h"
#include "gt_volume_dev.h"
#include "block_reduce.h"

namespace isdf {

constexpr int REC = ISDF_METRICS_RECORD;          // doubles per record
constexpr int MAXB = ISDF_METRICS_MAX_BLOCKS;     // per-block partial records in the workspace

// CHOMP collision cost (metrics.py:95-104): -s + e/2; where s > 0: (s - e)^2 / (2e); where s > e: 0 (the last assignment wins)
__device__ __forceinline__ double chomp(double s, double e) {
  double c = -s + 0.5 * e;
  if (s > 0.0) c = (1.0 / (2.0 * e)) * (s - e) * (s - e);
  if (s > e) c = 0.0;
  return c;
}

// One thread per point (grid-stride): grid coordinate, in-bounds test with the faces inclusive, trilinear value (all three
// in gt_volume_dev.h, shared with slices.hip), validity, and this point's share of the 24 sums.  Block b writes its partial
// record to part[b].
__global__ __launch_bounds__(256) void sdf_metrics_kernel(const isdf_gt_volume vol, const float* __restrict__ pts,
                                                          const float* __restrict__ sdf, int64_t n, int exclude_zero,
                                                          float oob_fill, float* __restrict__ gt_out,
                                                          uint8_t* __restrict__ valid_out, double* __restrict__ part) {
  __shared__ double sh[4][REC];
  double acc[REC];
#pragma unroll
  for (int v = 0; v < REC; ++v) acc[v] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    bool inb;
    const float gt = gt_trilinear(vol, pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2], oob_fill, &inb);
    const bool valid = inb && (gt != 0.f || !exclude_zero);
    if (gt_out) gt_out[i] = gt;
    if (valid_out) valid_out[i] = valid ? 1 : 0;
    acc[1] += inb ? 1.0 : 0.0;
    if (valid) {
      const double s = (double)sdf[i], g = (double)gt;
      const double d = fabs(s - g);
      acc[0] += 1.0;
      acc[2] += d;
      // metrics.binned_losses: limits -inf, 0, 0.1, 0.2, 0.5, 1, +inf, strict on both sides (compared in fp32 against the fp32
      // ground truth; the limits are the doubles rounded to fp32)
      const float lim[7] = {-INFINITY, 0.f, 0.1f, 0.2f, 0.5f, 1.f, INFINITY};
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        const bool in = gt > lim[b] && gt < lim[b + 1];
        acc[3 + b] += in ? d : 0.0;
        acc[9 + b] += in ? 1.0 : 0.0;
      }
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const double eps = 1.0 + 0.5 * e;
        const double cp = chomp(s, eps), cg = chomp(g, eps);
        acc[15 + 3 * e] += fabs(cp - cg);
        acc[16 + 3 * e] += cp;
        acc[17 + 3 * e] += cg;
      }
    }
  }
  block_record_sum(acc, sh, part + (int64_t)blockIdx.x * REC);
}

// ---- region metrics (eval_pts.fixed_pts_eval, eval_pts.py:96-299) -------------------------------------------------------
// One thread per point (grid-stride), everything in double.  A point's flag byte says which of the two sets (vis, vox) count its
// |sdf - gt| figures (bits 1, 2) and its cosine distance (bits 4, 8).  The point's own contribution is formed once, in
// registers, and added to each set's accumulators under a select: both sets are indexed statically, nothing lives in scratch.
constexpr int RREC = ISDF_REGION_RECORD;

// one lookup of eval_pts.eval_grad(is_gt_sdf=True): NaN out of bounds or where the value is == 0 (eval_pts.py:79-82)
__device__ __forceinline__ double grad_lookup(const isdf_gt_volume& vol, const isdf_region_args& a, double x, double y, double z) {
  bool inb;
  const double f = gt_trilinear_f64(vol, a.spacing, a.origin, x, y, z, &inb);
  return (inb && f != 0.0) ? f : __builtin_nan("");
}

__global__ __launch_bounds__(256) void region_metrics_kernel(const isdf_gt_volume vol, const isdf_region_args a, int has_vol,
                                                             double* __restrict__ part) {
  __shared__ double sh[4][2 * RREC];
  double acc[2 * RREC];                   // set k's entry v at k * RREC + v, as in the record
#pragma unroll
  for (int v = 0; v < 2 * RREC; ++v) acc[v] = 0.0;
  const float* __restrict__ pts = a.pts;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
    const unsigned f = (a.flags ? a.flags[i] : 3u) & (a.grad_sets ? 15u : 3u);
    double c[RREC];
#pragma unroll
    for (int v = 0; v < RREC; ++v) c[v] = 0.0;
    const double px = (double)pts[i * 3], py = (double)pts[i * 3 + 1], pz = (double)pts[i * 3 + 2];
    if (f & 3u) {
      bool inb = true;
      double g;
      if (has_vol) g = gt_trilinear_f64(vol, a.spacing, a.origin, px, py, pz, &inb);
      else g = a.gt_in[i];
      if (inb) {
        const double s = (double)a.sdf[i];
        const double d = fabs(s - g);
        c[0] = 1.0; c[1] = 1.0; c[2] = d;
        // metrics.binned_losses on the float64 ground truth: limits -inf, 0, 0.1, 0.2, 0.5, 1, +inf, strict on both sides
        const double lim[7] = {-INFINITY, 0.0, 0.1, 0.2, 0.5, 1.0, INFINITY};
#pragma unroll
        for (int b = 0; b < 6; ++b) {
          const bool in = g > lim[b] && g < lim[b + 1];
          c[3 + b] = in ? d : 0.0;
          c[9 + b] = in ? 1.0 : 0.0;
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          const double eps = 1.0 + 0.5 * e;
          const double cp = chomp(s, eps), cg = chomp(g, eps);
          c[15 + 3 * e] = fabs(cp - cg);
          c[16 + 3 * e] = cp;
          c[17 + 3 * e] = cg;
        }
      }
    }
    if (f & 12u) {
      // eval_pts.eval_grad: grad_i = (f(p + d e_i) - f(p - d e_i)) / (2 d), six lookups at (double)p +- delta
      const double dl = a.delta;
      const double gx = (grad_lookup(vol, a, px + dl, py, pz) - grad_lookup(vol, a, px - dl, py, pz)) / (2.0 * dl);
      const double gy = (grad_lookup(vol, a, px, py + dl, pz) - grad_lookup(vol, a, px, py - dl, pz)) / (2.0 * dl);
      const double gz = (grad_lookup(vol, a, px, py, pz + dl) - grad_lookup(vol, a, px, py, pz - dl)) / (2.0 * dl);
      c[24] = 1.0;
      if (isfinite(gx) && isfinite(gy) && isfinite(gz)) {
        // torch.nn.CosineSimilarity(dim=1, eps=1e-6): x.y / (max(|x|, eps) * max(|y|, eps))
        const double x0 = (double)a.sdf_grad[i * 3], x1 = (double)a.sdf_grad[i * 3 + 1], x2 = (double)a.sdf_grad[i * 3 + 2];
        const double nx = sqrt((x0 * x0 + x1 * x1) + x2 * x2), ny = sqrt((gx * gx + gy * gy) + gz * gz);
        const double cs = ((x0 * gx + x1 * gy) + x2 * gz) / (fmax(nx, 1e-6) * fmax(ny, 1e-6));
        c[25] = 1.0 - cs;
      } else {
        c[26] = 1.0;
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const bool in_sdf = (f >> k) & 1u, in_grad = (f >> (2 + k)) & 1u;
#pragma unroll
      for (int v = 0; v < 24; ++v) acc[k * RREC + v] += in_sdf ? c[v] : 0.0;
#pragma unroll
      for (int v = 24; v < RREC; ++v) acc[k * RREC + v] += in_grad ? c[v] : 0.0;
    }
  }
  block_record_sum(acc, sh, part + (int64_t)blockIdx.x * (2 * RREC));
}

int launch_region_metrics(const isdf_region_args& a, double* records, double* part, hipStream_t st) {
  // as launch_sdf_metrics: the grid is a function of n alone
  int64_t blocks = (a.n + 255) / 256;
  if (blocks > MAXB) blocks = MAXB;
  if (blocks > 0) {
    isdf_gt_volume vol = {};
    if (a.vol) vol = *a.vol;
    hipLaunchKernelGGL(region_metrics_kernel, dim3((unsigned)blocks), dim3(256), 0, st, vol, a, a.vol ? 1 : 0, part);
    const int rc = isdf_launch_status();
    if (rc) return rc;
  }
  return launch_reduce_partials(part, blocks, 2 * RREC, 0, records, st);
}

// ---- nearest neighbour, brute force -----------------------------------------------------------------------------------
// Block (x, y): NN_Q queries per thread (1024 per block) against target chunk y.  A tile of NN_TILE targets sits in LDS one
// axis per array, four targets per float4: every lane reads the SAME address (a broadcast ds_read_b128, no bank conflict),
// three reads bring four targets, and each feeds all NN_Q queries held in registers -- 8 VALU operations per pair plus half a
// v_min3 without the index, a compare and two selects with it, against 3/16 of an LDS read.  The squared distance is
// (dx*dx + dy*dy) + dz*dz with every operation rounded to fp32 (the file is built with -ffp-contract=off, build.py), so it
// equals a numpy float32 model bit for bit.  A chunk's result goes into the query's 64-bit key (distance bits << 32 | index)
// by an integer atomic minimum: squared distances are >= 0, their bit patterns order like the values, and the lowest index
// wins a tie whatever order the chunks finish in.
constexpr int NN_Q = 4;
constexpr int NN_TILE = 1024;

template <bool IDX>
__global__ __launch_bounds__(256) void nn_kernel(const float* __restrict__ query, int64_t n, const float* __restrict__ target,
                                                 int64_t m, int64_t chunk, unsigned long long* __restrict__ keys) {
  __shared__ float4 tx[NN_TILE / 4], ty[NN_TILE / 4], tz[NN_TILE / 4];   // four targets per 16-byte read and axis
  const int64_t q0 = (int64_t)blockIdx.x * (256 * NN_Q) + threadIdx.x;
  float qx[NN_Q], qy[NN_Q], qz[NN_Q], best[NN_Q];
  uint32_t bi[NN_Q];
#pragma unroll
  for (int j = 0; j < NN_Q; ++j) {
    const int64_t q = q0 + j * 256;
    const bool ok = q < n;
    qx[j] = ok ? query[q * 3] : 0.f; qy[j] = ok ? query[q * 3 + 1] : 0.f; qz[j] = ok ? query[q * 3 + 2] : 0.f;
    best[j] = INFINITY; bi[j] = 0xffffffffu;
  }
  const int64_t t0 = (int64_t)blockIdx.y * chunk;
  const int64_t t1 = t0 + chunk < m ? t0 + chunk : m;
  for (int64_t base = t0; base < t1; base += NN_TILE) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NN_TILE / 256; ++j) {
      const int k = threadIdx.x + j * 256;
      const int64_t t = base + k;
      // slots past the chunk hold +inf: their squared distance is +inf (or NaN) and never below the running minimum
      const bool ok = t < t1;
      ((float*)tx)[k] = ok ? target[t * 3] : INFINITY;
      ((float*)ty)[k] = ok ? target[t * 3 + 1] : INFINITY;
      ((float*)tz)[k] = ok ? target[t * 3 + 2] : INFINITY;
    }
    __syncthreads();
#pragma unroll 2
    for (int k4 = 0; k4 < NN_TILE / 4; ++k4) {
      const float4 X = tx[k4], Y = ty[k4], Z = tz[k4];
      const float px[4] = {X.x, X.y, X.z, X.w}, py[4] = {Y.x, Y.y, Y.z, Y.w}, pz[4] = {Z.x, Z.y, Z.z, Z.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int j = 0; j < NN_Q; ++j) {
          const float dx = __fsub_rn(qx[j], px[c]), dy = __fsub_rn(qy[j], py[c]), dz = __fsub_rn(qz[j], pz[c]);
          const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
          if (IDX) {   // ascending index, strict: the lowest index of a tie
            if (d2 < best[j]) { best[j] = d2; bi[j] = (uint32_t)(base + k4 * 4 + c); }
          } else {
            best[j] = fminf(best[j], d2);
          }
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NN_Q; ++j) {
    const int64_t q = q0 + j * 256;
    if (q < n) atomicMin(&keys[q], ((unsigned long long)__float_as_uint(best[j]) << 32) | bi[j]);
  }
}

// key -> distance (correctly rounded square root), index, and the block's partial sum of the distances
__global__ __launch_bounds__(256) void nn_finish_kernel(const unsigned long long* __restrict__ keys, int64_t n,
                                                        float* __restrict__ dist, int32_t* __restrict__ index,
                                                        double* __restrict__ part) {
  __shared__ double sh[4][1];
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double d[1] = {0.0};
  if (q < n) {
    const unsigned long long k = keys[q];
    const float r = __fsqrt_rn(__uint_as_float((uint32_t)(k >> 32)));
    if (dist) dist[q] = r;
    if (index) index[q] = (int32_t)(uint32_t)k;
    d[0] = (double)r;
  }
  block_record_sum(d, sh, part + blockIdx.x);
}

int launch_sdf_metrics(const isdf_gt_volume& vol, const float* pts, const float* sdf, int64_t n, int exclude_zero,
                       float oob_fill, double* record, float* gt_out, uint8_t* valid_out, double* part, hipStream_t st) {
  // the grid is a function of n alone, so the partial sums -- and with them every bit of the record -- repeat run to run
  int64_t blocks = (n + 255) / 256;
  if (blocks > MAXB) blocks = MAXB;
  if (blocks > 0) {
    hipLaunchKernelGGL(sdf_metrics_kernel, dim3((unsigned)blocks), dim3(256), 0, st, vol, pts, sdf, n, exclude_zero, oob_fill,
                       gt_out, valid_out, part);
    const int rc = isdf_launch_status();
    if (rc) return rc;
  }
  return launch_reduce_partials(part, blocks, REC, 0, record, st);
}

int launch_nn_distance(const float* query, int64_t n, const float* target, int64_t m, float* dist, int32_t* index,
                       double* dist_sum, unsigned long long* keys, double* part, hipStream_t st) {
  const int64_t fin = (n + 255) / 256;
  if (n > 0) {
    const hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)n * 8, st);   // every key starts above any (distance, index)
    if (e != hipSuccess) { g_isdf_last_hip_error = (int)e; return ISDF_EHIP; }
    // grid from the CU count: about four blocks (of four waves) per CU, reached by splitting the target set into chunks
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus < 1)
      cus = 256;
    const int64_t qblocks = (n + 256 * NN_Q - 1) / (256 * NN_Q);
    const int64_t tiles = (m + NN_TILE - 1) / NN_TILE;
    int64_t splits = (4 * (int64_t)cus + qblocks - 1) / qblocks;
    if (splits > tiles) splits = tiles;
    if (splits > 65535) splits = 65535;
    if (splits < 1) splits = 1;
    const int64_t chunk = (tiles + splits - 1) / splits * NN_TILE;
    splits = (m + chunk - 1) / chunk;
    const dim3 grid((unsigned)qblocks, (unsigned)splits);
    if (index)
      hipLaunchKernelGGL(nn_kernel<true>, grid, dim3(256), 0, st, query, n, target, m, chunk, keys);
    else
      hipLaunchKernelGGL(nn_kernel<false>, grid, dim3(256), 0, st, query, n, target, m, chunk, keys);
    int rc = isdf_launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(nn_finish_kernel, dim3((unsigned)fin), dim3(256), 0, st, keys, n, dist, index, part);
    if ((rc = isdf_launch_status())) return rc;
  }
  return launch_reduce_partials(part, fin, 1, 0, dist_sum, st);
}

}  // namespace isdf
