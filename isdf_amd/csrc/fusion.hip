// The voxel baseline beside the neural map: TSDF fusion of posed depth frames (isdf_tsdf_integrate), the exact squared Euclidean
// distance transform (isdf_distance_transform) and the reference's sdf_from_occupancy on top of it (isdf_occupancy_sdf,
// datasets/sdf_util.py:371-385).  The reference scores a "GPU fusion" result beside the net (eval/plot_utils.py:108-130) but does
// not ship the fusion; include/isdf_hip.h states the arithmetic of all three operation by operation.
//
// Fusion.  Per voxel and frame one random 4-byte gather out of the depth batch behind ~50 VALU operations (two IEEE divisions), then a
// running average whose result depends on the ORDER of the frames: latency-bound and sequential in f.  So: one thread per voxel
// (threadIdx.x along k: the two volumes are read once and written once, coalesced), the voxel's (tsdf, w) in registers across ALL
// frames of the call, the frames in the inner loop TSDF_UNROLL at a time -- the address arithmetic of the group first, then
// TSDF_UNROLL independent loads in flight per lane, then their updates in index order.  A lane whose pair fails before the gather
// reads depth[0]: no divergent branch around the load, one hot cache line.  The twelve coefficients of a frame are the same for
// every lane: a block stages up to TSDF_STAGE frames in LDS and reads each row as one broadcast ds_read_b128.  Stage slots past the
// last frame hold zeros: zc = 0 fails `zc > 0`, so the padded iterations of the unrolled loop need no test of their own.  No voxel's
// frames are ever split over blocks and nothing is combined by atomics, so F frames in one call equal the same frames in any
// sequence of calls, bit for bit.  The file is built with -ffp-contract=off (build.py): every operation is rounded on its own.
//
// Distance transform.  Three separable min-plus passes (z, y, x) over int32 squared distances: out[p] = min over q of the line of
// in[q] + (p - q)^2, by brute force, which is exact by construction.  A workgroup owns EDT_LANES lines and EDT_PC outputs of each;
// it walks the whole line in chunks of EDT_QC staged in LDS as [q][lane] (row padded to 65 words: the z pass fills it lane-major
// and reads it q-major without a bank conflict).  Wave w of the four holds outputs p0 + 16 w .. + 15 in registers, so (p - q) is
// the same for the whole wave and a staged value is read once for 16 outputs.  A line of 1024 int32 x 64 lanes is 256 KB and does
// not fit the 160 KB of LDS, hence the chunks and, since other workgroups read the line while this one would write it, a second
// volume instead of an update in place.  Global memory is touched in runs of 64 consecutive k in every pass: the y and x passes
// take 64 neighbouring lines (consecutive k) per row of the stage, the z pass loads and stores whole lines and turns them in LDS.
// Values saturate at ISDF_EDT_NONE = 2^30: the accumulator starts there and in[q] + (p - q)^2 <= 2^30 + 1023^2 < 2^31.
#include "isdf_common.h"
#include "launchers.h"

namespace isdf {

constexpr int TSDF_STAGE = 64;    // frames whose coefficients a block holds in LDS at once (3 KB)
constexpr int TSDF_UNROLL = 8;    // independent gathers in flight per lane

__global__ __launch_bounds__(256) void tsdf_integrate_kernel(isdf_tsdf_args a, int64_t n) {
  __shared__ float4 rows[TSDF_STAGE * 3];
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = p < n;
  const int64_t pp = live ? p : 0;
  const int k = (int)(pp % a.nz), j = (int)((pp / a.nz) % a.ny), i = (int)(pp / ((int64_t)a.nz * a.ny));
  const float x = a.origin[0] + (float)i * a.spacing[0];
  const float y = a.origin[1] + (float)j * a.spacing[1];
  const float z = a.origin[2] + (float)k * a.spacing[2];
  const float fW = (float)a.W, fH = (float)a.H;
  const int64_t HW = (int64_t)a.H * a.W;
  const float fx = a.fx, fy = a.fy, cx = a.cx, cy = a.cy, trunc = a.trunc, ntrunc = -a.trunc;
  const float* __restrict__ depth = a.depth;
  float tsdf = live ? a.tsdf[p] : 0.f, w = live ? a.weight[p] : 0.f;
  for (int base = 0, m; base < a.F; base += m) {
    m = a.F - base < TSDF_STAGE ? a.F - base : TSDF_STAGE;
    const int padded = (m + TSDF_UNROLL - 1) / TSDF_UNROLL * TSDF_UNROLL;
    __syncthreads();
    for (int t = threadIdx.x; t < padded * 12; t += 256) {
      const int fr = t / 12, e = t - fr * 12;
      ((float*)rows)[t] = fr < m ? a.T_CW[(int64_t)(base + fr) * 16 + e] : 0.f;
    }
    __syncthreads();
    // kept as written (see visible.hip): vectorised over k0 the compiler waits for the first group's loads inside the second
#pragma clang loop vectorize(disable) unroll(disable)
    for (int k0 = 0; k0 < padded; k0 += TSDF_UNROLL) {
      float zc[TSDF_UNROLL], d[TSDF_UNROLL];
      bool need[TSDF_UNROLL];
#pragma unroll
      for (int g = 0; g < TSDF_UNROLL; ++g) {
        const float4 r0 = rows[(k0 + g) * 3], r1 = rows[(k0 + g) * 3 + 1], r2 = rows[(k0 + g) * 3 + 2];
        const float xc = ((r0.x * x + r0.y * y) + r0.z * z) + r0.w;
        const float yc = ((r1.x * x + r1.y * y) + r1.z * z) + r1.w;
        zc[g] = ((r2.x * x + r2.y * y) + r2.z * z) + r2.w;
        const float u = __fdiv_rn(fx * xc + cx * zc[g], zc[g]);
        const float v = __fdiv_rn(fy * yc + cy * zc[g], zc[g]);
        const float uc = u + 0.5f, vc = v + 0.5f;
        // `&`, not `&&`: straight-line selects instead of a chain of exec-masked branches in front of every load
        need[g] = live & (uc >= 0.f) & (uc < fW) & (vc >= 0.f) & (vc < fH) & (zc[g] > 0.f);
        // 0 <= uc < W and 0 <= vc < H here, so the truncated pixel is inside the frame; every other lane reads depth[0]
        const int col = (int)(need[g] ? uc : 0.f), row = (int)(need[g] ? vc : 0.f);
        const int64_t off = need[g] ? (int64_t)(base + k0 + g) * HW + (row * a.W + col) : 0;
        d[g] = depth[off];
      }
#pragma unroll
      for (int g = 0; g < TSDF_UNROLL; ++g) {
        const float s = d[g] - zc[g];
        const bool ok = need[g] & (d[g] > a.min_depth) & (d[g] < a.max_depth) & (s >= ntrunc);
        const float t = s < trunc ? s : trunc;
        const float w1 = w + 1.0f;
        const float nt = __fdiv_rn(tsdf * w + t, w1);
        tsdf = ok ? nt : tsdf;
        w = ok ? fminf(w1, a.max_weight) : w;
      }
    }
  }
  if (live) {
    a.tsdf[p] = tsdf;
    a.weight[p] = w;
  }
}

int launch_tsdf_integrate(const isdf_tsdf_args& a, hipStream_t st) {
  if (a.F == 0) return ISDF_OK;
  const int64_t n = (int64_t)a.nx * a.ny * a.nz;
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, n);
  return isdf_launch_status();
}

// ---- exact squared Euclidean distance transform
constexpr int EDT_LANES = 64;   // lines per workgroup: one per lane of a wave
constexpr int EDT_PC = 64;      // outputs per line and workgroup: 16 per wave
constexpr int EDT_PW = EDT_PC / 4;
constexpr int EDT_QC = 128;     // inputs per line staged at once
constexpr int EDT_ROW = EDT_LANES + 1;   // LDS row in words: [q][lane], padded
constexpr int32_t EDT_NONE = ISDF_EDT_NONE;

// One pass along an axis of L points and stride `inner`; line l of nLines starts at (l / inner) * L * inner + l % inner.
// FIRST: `in` is the u8 feature volume (0 where (feature != 0) != invert, EDT_NONE elsewhere); else int32.
// CONTIG: inner == 1 (the z pass): a line is L consecutive words, so the stage is filled and the result stored line by line.
template <bool FIRST, bool CONTIG>
__global__ __launch_bounds__(256) void edt_pass_kernel(const void* __restrict__ in, int32_t* __restrict__ out, int64_t nLines, int L,
                                                       int64_t inner, int invert) {
  __shared__ int32_t stage[EDT_QC * EDT_ROW];
  __shared__ int64_t lineBase[EDT_LANES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t l0 = (int64_t)blockIdx.x * EDT_LANES;
  const int p0 = blockIdx.y * EDT_PC;
  if (tid < EDT_LANES) {
    const int64_t l = l0 + tid;
    lineBase[tid] = l < nLines ? (l / inner) * L * inner + l % inner : -1;
  }
  int32_t acc[EDT_PW];
#pragma unroll
  for (int m = 0; m < EDT_PW; ++m) acc[m] = EDT_NONE;
  const int pw = p0 + wave * EDT_PW;          // this wave's first output
  for (int q0 = 0; q0 < L; q0 += EDT_QC) {
    const int cnt = L - q0 < EDT_QC ? L - q0 : EDT_QC;
    __syncthreads();                          // lineBase written; the previous chunk read
    for (int t = tid; t < EDT_QC * EDT_LANES; t += 256) {
      const int ln = CONTIG ? t / EDT_QC : t % EDT_LANES, q = CONTIG ? t % EDT_QC : t / EDT_LANES;
      const int64_t b = lineBase[ln];
      int32_t v = EDT_NONE;
      if (b >= 0 && q < cnt) {
        const int64_t at = b + (int64_t)(q0 + q) * inner;
        if (FIRST) v = ((((const uint8_t*)in)[at] != 0) != (invert != 0)) ? 0 : EDT_NONE;
        else v = ((const int32_t*)in)[at];
      }
      stage[q * EDT_ROW + ln] = v;
    }
    __syncthreads();
    int dq = pw - q0;                         // p - q of output 0 against the chunk's first input; wave-uniform
    for (int q = 0; q < cnt; ++q, --dq) {
      const int32_t v = stage[q * EDT_ROW + lane];
#pragma unroll
      for (int m = 0; m < EDT_PW; ++m) {
        const int32_t c = v + (dq + m) * (dq + m);
        acc[m] = c < acc[m] ? c : acc[m];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < EDT_PW; ++m) stage[(wave * EDT_PW + m) * EDT_ROW + lane] = acc[m];
  __syncthreads();
  for (int t = tid; t < EDT_PC * EDT_LANES; t += 256) {
    const int ln = CONTIG ? t / EDT_PC : t % EDT_LANES, pp = CONTIG ? t % EDT_PC : t / EDT_LANES;
    const int64_t b = lineBase[ln];
    if (b >= 0 && p0 + pp < L) out[b + (int64_t)(p0 + pp) * inner] = stage[pp * EDT_ROW + ln];
  }
}

template <bool FIRST, bool CONTIG>
static int edt_pass(const void* in, int32_t* out, int64_t nLines, int L, int64_t inner, int invert, hipStream_t st) {
  const dim3 grid((unsigned)((nLines + EDT_LANES - 1) / EDT_LANES), (unsigned)((L + EDT_PC - 1) / EDT_PC));
  hipLaunchKernelGGL((edt_pass_kernel<FIRST, CONTIG>), grid, dim3(256), 0, st, in, out, nLines, L, inner, invert);
  return isdf_launch_status();
}

int64_t edt_volume_bytes(int32_t nx, int32_t ny, int32_t nz) { return ((int64_t)nx * ny * nz * 4 + 255) / 256 * 256; }

// z: feature -> dist2, y: dist2 -> scratch, x: scratch -> dist2
int launch_distance_transform(const uint8_t* feature, int32_t nx, int32_t ny, int32_t nz, int invert, int32_t* dist2, int32_t* scratch,
                              hipStream_t st) {
  int rc = edt_pass<true, true>(feature, dist2, (int64_t)nx * ny, nz, 1, invert, st);
  if (rc) return rc;
  rc = edt_pass<false, false>(dist2, scratch, (int64_t)nx * nz, ny, nz, 0, st);
  if (rc) return rc;
  return edt_pass<false, false>(scratch, dist2, (int64_t)ny * nz, nx, (int64_t)ny * nz, 0, st);
}

// out[p] holds b (int32 bits) on entry and the signed distance on exit
__global__ __launch_bounds__(256) void occupancy_sdf_kernel(const int32_t* __restrict__ a2, float* out, int64_t n, double voxel) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int32_t a = a2[p], b = ((const int32_t*)out)[p];
  float r;
  if (a == EDT_NONE) r = __builtin_inff();
  else if (b == EDT_NONE) r = -__builtin_inff();
  else r = (float)((sqrt((double)a) - sqrt((double)b)) * voxel);
  out[p] = r;
}

int launch_occupancy_sdf(const uint8_t* occ, int32_t nx, int32_t ny, int32_t nz, double voxel, float* out, void* ws, hipStream_t st) {
  int32_t* a2 = (int32_t*)ws;
  int32_t* scratch = (int32_t*)((char*)ws + edt_volume_bytes(nx, ny, nz));
  int rc = launch_distance_transform(occ, nx, ny, nz, 0, a2, scratch, st);
  if (rc) return rc;
  rc = launch_distance_transform(occ, nx, ny, nz, 1, (int32_t*)out, scratch, st);
  if (rc) return rc;
  const int64_t n = (int64_t)nx * ny * nz;
  hipLaunchKernelGGL(occupancy_sdf_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a2, out, n, voxel);
  return isdf_launch_status();
}

}  // namespace isdf
