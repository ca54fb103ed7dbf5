// Frame-to-map pose alignment (isdf_pose_points, isdf_pose_system): one Gauss-Newton linearisation of "where was this depth frame
// really taken?" against the map.  Reference: none -- the reference reads T_WC from a tracker or from robot kinematics and never
// corrects it; the back-projection restates pointcloud_from_depth_torch (isdf/geometry/transform.py:189-190) op by op.
//   pose_points_kernel   lattice pixel -> world point under the pose guess, fp32, every operation rounded on its own (the file is
//                        built with -ffp-contract=off, build.py), so the points equal a numpy float32 model bit for bit
//   pose_system_kernel   per pose the record of include/isdf_hip.h (counts, costs, sum w r J, upper triangle of sum w J J^T), all
//                        in double on the fp32 inputs widened, reduced like eval.hip's records: a grid-stride share per thread,
//                        then block_reduce.h's order, one partial record per block
//   pose_close_kernel    a pose's partial records in block order
// The grid is (blocks per pose, poses of the chunk) with blocks per pose a function of n_pix alone, capped at ISDF_POSE_MAX_BLOCKS:
// a pose's record does not depend on the run or on its neighbours in the call.  Poses and frame indices come from the host and
// travel as launch arguments, POSE_CHUNK poses per launch: no copy, nothing the host could not check before the launch.
// Shape: a few thousand pixels per pose and ~150 double operations per pixel -- launch-bound next to the field call between the
// two kernels; the 32 accumulators are indexed statically throughout (64 VGPRs, nothing in scratch).
#include "isdf_common.h"
#include "launchers.h"
#include "block_reduce.h"

namespace isdf {

constexpr int PREC = ISDF_POSE_RECORD;
constexpr int POSE_CHUNK = 32;        // poses per launch: 32 x (12 floats + 1 index) = 1.7 KB of launch arguments

struct PoseChunk {
  float T[POSE_CHUNK][12];            // rows of the 3 x 4 pose
  int32_t frame[POSE_CHUNK];
};

struct PoseCam {
  const float* depth;
  int32_t H, W, stride, ncols;
  int64_t n_pix;
  float fx, fy, cx, cy, min_depth, max_depth;
};

// THE definition of a usable depth pixel
__device__ __forceinline__ bool depth_valid(float z, float min_depth, float max_depth) {
  return isfinite(z) && z != 0.f && z >= min_depth && z <= max_depth;
}

// depth of lattice pixel i of frame f, and its column and row
__device__ __forceinline__ float lattice_depth(const PoseCam& cam, int f, int64_t i, int* col, int* row) {
  const int lr = (int)(i / cam.ncols), lc = (int)(i - (int64_t)lr * cam.ncols);
  *row = lr * cam.stride;                 // < H and < W: i < n_pix = ceil(H / stride) * ceil(W / stride)
  *col = lc * cam.stride;
  return cam.depth[(int64_t)f * ((int64_t)cam.H * cam.W) + ((int64_t)*row * cam.W + *col)];
}

__global__ __launch_bounds__(256) void pose_points_kernel(const PoseCam cam, const PoseChunk chunk, int64_t pose0,
                                                          float* __restrict__ pts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= cam.n_pix) return;
  const float* T = chunk.T[blockIdx.y];
  int col, row;
  const float z = lattice_depth(cam, chunk.frame[blockIdx.y], i, &col, &row);
  const bool ok = depth_valid(z, cam.min_depth, cam.max_depth);
  const float xc = __fdiv_rn(z * ((float)col - cam.cx), cam.fx);
  const float yc = __fdiv_rn(z * ((float)row - cam.cy), cam.fy);
  float* o = pts + ((pose0 + blockIdx.y) * cam.n_pix + i) * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float w = ((T[4 * k] * xc + T[4 * k + 1] * yc) + T[4 * k + 2] * z) + T[4 * k + 3];
    o[k] = ok ? w : T[4 * k + 3];
  }
}

// block (x, y): the grid-stride share x of pose pose0 + y; its partial record goes to part[pose][x]
__global__ __launch_bounds__(256) void pose_system_kernel(const PoseCam cam, const PoseChunk chunk, int64_t pose0,
                                                          const float* __restrict__ pts, const float* __restrict__ sdf,
                                                          const float* __restrict__ grad, float huber_f, float trunc_f,
                                                          double* __restrict__ part) {
  __shared__ double sh[4][PREC];
  double acc[PREC];
#pragma unroll
  for (int v = 0; v < PREC; ++v) acc[v] = 0.0;
  const int64_t pose = pose0 + blockIdx.y;
  const int frame = chunk.frame[blockIdx.y];
  const double c0 = (double)chunk.T[blockIdx.y][3], c1 = (double)chunk.T[blockIdx.y][7], c2 = (double)chunk.T[blockIdx.y][11];
  const double huber = (double)huber_f, trunc = (double)trunc_f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cam.n_pix; i += (int64_t)gridDim.x * 256) {
    int col, row;
    const bool ok = depth_valid(lattice_depth(cam, frame, i, &col, &row), cam.min_depth, cam.max_depth);
    const int64_t p = pose * cam.n_pix + i;
    const double r = (double)sdf[p], a = fabs(r);
    const bool used = ok && a <= trunc;           // a NaN residual compares false: never used
    acc[1] += ok ? 1.0 : 0.0;
    if (used) {
      const bool quad = a <= huber;
      const double w = quad ? 1.0 : huber / a;
      const double g0 = (double)grad[p * 3], g1 = (double)grad[p * 3 + 1], g2 = (double)grad[p * 3 + 2];
      const double d0 = (double)pts[p * 3] - c0, d1 = (double)pts[p * 3 + 1] - c1, d2 = (double)pts[p * 3 + 2] - c2;
      const double J[6] = {g0, g1, g2, d1 * g2 - d2 * g1, d2 * g0 - d0 * g2, d0 * g1 - d1 * g0};
      const double wr = w * r;
      acc[0] += 1.0;
      acc[2] += wr * r;
      acc[3] += quad ? 0.5 * (r * r) : huber * (a - 0.5 * huber);
      acc[31] += a;
#pragma unroll
      for (int m = 0; m < 6; ++m) {
        acc[4 + m] += wr * J[m];
        const double wj = w * J[m];
#pragma unroll
        for (int n = m; n < 6; ++n) acc[10 + 6 * m - m * (m - 1) / 2 + (n - m)] += wj * J[n];   // row m of the upper triangle
      }
    }
  }
  block_record_sum(acc, sh, part + (pose * ISDF_POSE_MAX_BLOCKS + blockIdx.x) * PREC);
}

// block = pose, thread v < PREC: records[pose][v] = its nPart partial records in block order
__global__ __launch_bounds__(64) void pose_close_kernel(const double* __restrict__ part, int nPart, double* __restrict__ records) {
  if (threadIdx.x >= PREC) return;
  const double* p = part + (int64_t)blockIdx.x * ISDF_POSE_MAX_BLOCKS * PREC + threadIdx.x;
  double t = 0.0;
  for (int b = 0; b < nPart; ++b) t += p[(int64_t)b * PREC];
  records[(int64_t)blockIdx.x * PREC + threadIdx.x] = t;
}

static PoseCam pose_cam(const isdf_pose_args& a) {
  PoseCam cam;
  cam.depth = a.depth;
  cam.H = a.H; cam.W = a.W; cam.stride = a.stride;
  cam.ncols = (a.W + a.stride - 1) / a.stride;      // no sum past INT_MAX: capi.hip bounds stride by max(H, W)
  cam.n_pix = (int64_t)((a.H + a.stride - 1) / a.stride) * cam.ncols;
  cam.fx = a.fx; cam.fy = a.fy; cam.cx = a.cx; cam.cy = a.cy;
  cam.min_depth = a.min_depth; cam.max_depth = a.max_depth;
  return cam;
}

// poses b0 .. b0 + m - 1 of the call as launch arguments (unused slots: pose 0 of the chunk again, never indexed)
static void pose_chunk(const isdf_pose_args& a, int32_t b0, int m, PoseChunk* c) {
  for (int j = 0; j < POSE_CHUNK; ++j) {
    const int32_t b = b0 + (j < m ? j : 0);
    for (int k = 0; k < 12; ++k) c->T[j][k] = a.T_WC[(int64_t)b * 12 + k];
    c->frame[j] = a.frame_of_pose ? a.frame_of_pose[b] : b;
  }
}

int launch_pose_points(const isdf_pose_args& a, float* pts, hipStream_t st) {
  const PoseCam cam = pose_cam(a);
  const unsigned blocks = (unsigned)((cam.n_pix + 255) / 256);
  PoseChunk chunk;
  for (int32_t b0 = 0; b0 < a.B; b0 += POSE_CHUNK) {
    const int m = a.B - b0 < POSE_CHUNK ? a.B - b0 : POSE_CHUNK;
    pose_chunk(a, b0, m, &chunk);
    hipLaunchKernelGGL(pose_points_kernel, dim3(blocks, (unsigned)m), dim3(256), 0, st, cam, chunk, (int64_t)b0, pts);
    const int rc = isdf_launch_status();
    if (rc) return rc;
  }
  return ISDF_OK;
}

int launch_pose_system(const isdf_pose_args& a, const float* pts, const float* sdf, const float* grad, float huber, float trunc,
                       double* records, double* part, hipStream_t st) {
  const PoseCam cam = pose_cam(a);
  // the grid is a function of n_pix alone, so every bit of a pose's record repeats
  int64_t blocks = (cam.n_pix + 255) / 256;
  if (blocks > ISDF_POSE_MAX_BLOCKS) blocks = ISDF_POSE_MAX_BLOCKS;
  PoseChunk chunk;
  for (int32_t b0 = 0; b0 < a.B; b0 += POSE_CHUNK) {
    const int m = a.B - b0 < POSE_CHUNK ? a.B - b0 : POSE_CHUNK;
    pose_chunk(a, b0, m, &chunk);
    hipLaunchKernelGGL(pose_system_kernel, dim3((unsigned)blocks, (unsigned)m), dim3(256), 0, st, cam, chunk, (int64_t)b0, pts, sdf,
                       grad, huber, trunc, part);
    const int rc = isdf_launch_status();
    if (rc) return rc;
  }
  hipLaunchKernelGGL(pose_close_kernel, dim3((unsigned)a.B), dim3(64), 0, st, part, (int)blocks, records);
  return isdf_launch_status();
}

}  // namespace isdf
