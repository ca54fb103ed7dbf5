// Visibility of world points against posed depth frames (isdf_visible_points): the use_projection=True branch of
// geometry.frustum.is_visible_torch (isdf/geometry/frustum.py:87-133), which Trainer.eval_object_sdf (trainer.py:1976-1981) and
// the visible-region masks of the slice figures (eval/figs/slices.py:274) call -- "in front of the frame, inside its image, and no
// more than trunc metres behind the surface" -- for every (frame, point) pair in ONE pass, a per-point count the only mandatory
// output.  Per pair, with (a_rc) the frame's camera-from-world matrix, every operation rounded to fp32 and nothing fused (the file is
// built with -ffp-contract=off, build.py), so the result equals a numpy float32 model bit for bit:
//   xc = ((a00*x + a01*y) + a02*z) + a03, yc and zc alike from rows 1 and 2                       torch.matmul(T_CW, homog_points)
//   u = (fx*xc + cx*zc) / zc, v = (fy*yc + cy*zc) / zc   (IEEE division)                          torch.matmul(K, points_C), uv / z
//   inside = u > 0 && u < (float)W && v > 0 && v < (float)H   (NaN and +-inf compare false)       x_valid, y_valid
//   pixel = ((int)v, (int)u), truncated                                                            uv.long()
//   visible = inside && zc > 0 && zc < depth[f][row][col] + trunc                                  z_valid (a pixel of 0 or NaN: no case)
//
// Shape.  The work is one random 4-byte gather per pair out of up to ~2 GB of depth and ~50 VALU operations (two IEEE divisions) in
// front of it: latency-bound.  One thread per point keeps the point in registers; the frames run in the inner loop, VIS_UNROLL at a
// time: the address arithmetic of all of them first, then VIS_UNROLL independent loads in flight per lane, then the compares.  A
// lane whose pair fails before the gather (outside the image or behind the camera) reads depth[0] instead -- no divergent branch
// around the load, one hot cache line.  The twelve coefficients of a frame are the same for every lane: a block stages up to
// VIS_STAGE frames in LDS and reads each row as one broadcast ds_read_b128.  Stage slots past the block's last frame hold zeros: zc
// = 0 fails `zc > 0`, so the padded iterations of the unrolled loop need no test of their own.
// Frames are split over blockIdx.y (launch_visible_points) so that a small point set still fills the chip; a block adds its share to
// count[i] with an integer atomic, and the points seen are counted from the finished counts by a second launch: integer adds only,
// so the bytes do not depend on the split or on arrival order.
#include "isdf_common.h"
#include "launchers.h"
#include "block_reduce.h"

namespace isdf {

constexpr int VIS_STAGE = 64;    // frames whose coefficients a block holds in LDS at once (3 KB)
constexpr int VIS_UNROLL = 8;    // independent gathers in flight per lane
constexpr int VIS_BLOCKS = 2048; // blocks aimed at when the frames are split: 8 per CU
constexpr int64_t VIS_LAUNCH_BLOCKS = (int64_t)1 << 22;   // point blocks per launch (2^30 threads: a launch takes fewer than 2^32)

template <bool MASK>
__global__ __launch_bounds__(256) void visible_kernel(const float* __restrict__ pts, int64_t i0, int64_t n, const float* __restrict__ T_CW,
                                                      const float* __restrict__ depth, int F, int frames_per_block, int H, int W,
                                                      float fx, float fy, float cx, float cy, float trunc,
                                                      int32_t* __restrict__ count, uint8_t* __restrict__ mask) {
  __shared__ float4 rows[VIS_STAGE * 3];
  const int64_t i = i0 + (int64_t)blockIdx.x * 256 + threadIdx.x;      // i0: the first point of this launch
  const bool live = i < n;
  const float x = live ? pts[i * 3] : 0.f, y = live ? pts[i * 3 + 1] : 0.f, z = live ? pts[i * 3 + 2] : 0.f;
  const float fW = (float)W, fH = (float)H;
  const int64_t HW = (int64_t)H * W;
  const int f0 = blockIdx.y * frames_per_block;                                  // < F: the launcher's grid
  const int f1 = F - f0 < frames_per_block ? F : f0 + frames_per_block;          // no sum that could pass INT_MAX
  int seen = 0;
  for (int base = f0, m; base < f1; base += m) {
    m = f1 - base < VIS_STAGE ? f1 - base : VIS_STAGE;
    const int padded = (m + VIS_UNROLL - 1) / VIS_UNROLL * VIS_UNROLL;
    __syncthreads();
    for (int t = threadIdx.x; t < padded * 12; t += 256) {
      const int fr = t / 12, e = t - fr * 12;
      ((float*)rows)[t] = fr < m ? T_CW[(int64_t)(base + fr) * 16 + e] : 0.f;
    }
    __syncthreads();
    // kept as written: vectorised over k0 the compiler pairs two groups into packed fp32 operations and waits for the first
    // group's loads in the middle of the second
#pragma clang loop vectorize(disable) unroll(disable)
    for (int k0 = 0; k0 < padded; k0 += VIS_UNROLL) {
      float zc[VIS_UNROLL], d[VIS_UNROLL];
      bool need[VIS_UNROLL];
#pragma unroll
      for (int j = 0; j < VIS_UNROLL; ++j) {
        const float4 r0 = rows[(k0 + j) * 3], r1 = rows[(k0 + j) * 3 + 1], r2 = rows[(k0 + j) * 3 + 2];
        const float xc = ((r0.x * x + r0.y * y) + r0.z * z) + r0.w;
        const float yc = ((r1.x * x + r1.y * y) + r1.z * z) + r1.w;
        zc[j] = ((r2.x * x + r2.y * y) + r2.z * z) + r2.w;
        const float u = __fdiv_rn(fx * xc + cx * zc[j], zc[j]);
        const float v = __fdiv_rn(fy * yc + cy * zc[j], zc[j]);
        // `&`, not `&&`: straight-line selects instead of a chain of exec-masked branches in front of every load
        const bool inside = (u > 0.f) & (u < fW) & (v > 0.f) & (v < fH);
        need[j] = live & inside & (zc[j] > 0.f);
        // 0 < u < W and 0 < v < H here, so the truncated pixel is inside the frame; every other lane reads depth[0]
        const int col = (int)(need[j] ? u : 0.f), row = (int)(need[j] ? v : 0.f);
        const int64_t off = need[j] ? (int64_t)(base + k0 + j) * HW + (row * W + col) : 0;
        d[j] = depth[off];
      }
#pragma unroll
      for (int j = 0; j < VIS_UNROLL; ++j) {
        const bool vis = need[j] & (zc[j] < d[j] + trunc);
        seen += vis ? 1 : 0;
        if (MASK && live && k0 + j < m) mask[(int64_t)(base + k0 + j) * n + i] = vis ? 1 : 0;
      }
    }
  }
  if (live && seen) atomicAdd(&count[i], seen);
}

// n_seen += the points of this block's grid-stride share whose finished count is > 0
__global__ __launch_bounds__(256) void visible_seen_kernel(const int32_t* __restrict__ count, int64_t n,
                                                           unsigned long long* __restrict__ n_seen) {
  __shared__ int sh[4];
  int c = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) c += count[i] > 0 ? 1 : 0;
  c = wave_reduce<RedSum>(c);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = waves_combine<RedSum>(sh[0], sh[1], sh[2], sh[3]);
    if (t) atomicAdd(n_seen, (unsigned long long)t);
  }
}

int launch_visible_points(const float* pts, int64_t n, const float* T_CW, const float* depth, int32_t F, int32_t H, int32_t W,
                          float fx, float fy, float cx, float cy, float trunc, int32_t* count, uint8_t* mask, int64_t* n_seen,
                          hipStream_t st) {
  hipError_t e = hipSuccess;
  if (n > 0) e = hipMemsetAsync(count, 0, (size_t)n * 4, st);
  if (e == hipSuccess && n_seen) e = hipMemsetAsync(n_seen, 0, 8, st);
  if (e != hipSuccess) { g_isdf_last_hip_error = (int)e; return ISDF_EHIP; }
  if (n == 0 || F == 0) return ISDF_OK;
  // the split is a function of (n, F) alone; the outputs are integers, so it could be any other without changing a byte
  const int64_t pblocks = (n + 255) / 256;
  int64_t splits = (VIS_BLOCKS + pblocks - 1) / pblocks;
  const int64_t most = ((int64_t)F + VIS_UNROLL - 1) / VIS_UNROLL;
  if (splits > most) splits = most;
  if (splits > 65535) splits = 65535;
  int64_t fpb = (((int64_t)F + splits - 1) / splits + VIS_UNROLL - 1) / VIS_UNROLL * VIS_UNROLL;
  if (fpb > F) fpb = F;                       // one block row: the kernel pads its last group itself, and F fits an int
  splits = ((int64_t)F + fpb - 1) / fpb;
  // one thread per point; beyond VIS_LAUNCH_BLOCKS point blocks (2^30 points) the launch repeats with the next points
  for (int64_t b0 = 0; b0 < pblocks; b0 += VIS_LAUNCH_BLOCKS) {
    const int64_t nb = pblocks - b0 < VIS_LAUNCH_BLOCKS ? pblocks - b0 : VIS_LAUNCH_BLOCKS;
    const dim3 grid((unsigned)nb, (unsigned)splits);
    if (mask)
      hipLaunchKernelGGL(visible_kernel<true>, grid, dim3(256), 0, st, pts, b0 * 256, n, T_CW, depth, F, (int)fpb, H, W, fx, fy, cx,
                         cy, trunc, count, mask);
    else
      hipLaunchKernelGGL(visible_kernel<false>, grid, dim3(256), 0, st, pts, b0 * 256, n, T_CW, depth, F, (int)fpb, H, W, fx, fy, cx,
                         cy, trunc, count, mask);
    const int rc = isdf_launch_status();
    if (rc) return rc;
  }
  if (!n_seen) return ISDF_OK;
  const int64_t sblocks = pblocks < 1024 ? pblocks : 1024;
  hipLaunchKernelGGL(visible_seen_kernel, dim3((unsigned)sblocks), dim3(256), 0, st, count, n, (unsigned long long*)n_seen);
  return isdf_launch_status();
}

}  // namespace isdf
