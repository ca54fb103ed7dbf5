// Planning against the map (isdf_traj_points, isdf_traj_step): one iteration of covariant gradient descent on B trajectories.
// Reference: none -- the reference scores a recorded camera path with metrics.chomp_cost (metrics.py:95-104) and never moves one;
// the cost c(d) restates it as eval.hip does.  The mathematics, operation by operation, is the header's (include/isdf_hip.h).
//   traj_points_kernel   q[b][t][s] = x[b][t] + o_s, fp32, one thread per query point
//   traj_step_kernel     one 256-thread workgroup per trajectory, everything in double on the fp32 inputs widened (the file is
//                        built with -ffp-contract=off, build.py: every product and sum is rounded on its own, so a host model
//                        written in the same order has the same terms bit for bit):
//     1  thread k takes waypoints k, k + 256, ..: its S samples (s ascending) give C_t and G_t, its neighbours in x the speed;
//        C_t vh_t and sigma_t G_t go to LDS, the scalar sums, minimum and counts stay in registers
//     2  grad_t from the neighbours' C vh in LDS; the record's sums: lanes by shuffle, the four waves in wave order
//     3  (moving trajectories only) K^-1 grad by the closed-form inverse, one lane per coordinate, then m = max |Delta_t| over
//        all threads
//     4  state, record, the new x and the next iteration's query points
//   The cost, the sums, the solve, the state rule and the record are descent_dev.h's, shared with arm.hip.
// LDS: 6 doubles per waypoint, allocated per launch for the T of the call (48 T bytes: 3 KB at T = 64, 48 KB at T = 1024), and
// 40 doubles of scalars, so that short trajectories share a CU up to the wave limit.  Coordinates are planes of T doubles: a
// wave's 64 consecutive waypoints are 64 consecutive doubles, conflict-free.  Offsets and radii are launch arguments (512 B).
// Nothing is indexed dynamically in registers: no scratch.
#include "isdf_common.h"
#include "launchers.h"
#include "block_reduce.h"
#include "descent_dev.h"

namespace isdf {

constexpr int TMAXS = ISDF_TRAJ_MAX_SPHERES;

struct TrajBody {
  float off[TMAXS][3];
  float rad[TMAXS];
};

struct TrajParams {
  int32_t T, S;
  float eps, w_obs, w_smooth, eta, max_step, tol;
};

__global__ __launch_bounds__(256) void traj_points_kernel(const float* __restrict__ x, const TrajBody body, int32_t S, int64_t n,
                                                          float* __restrict__ q) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // (b * T + t) * S + s
  if (i >= n) return;
  const int64_t bt = i / S;
  const int s = (int)(i - bt * S);
#pragma unroll
  for (int k = 0; k < 3; ++k) q[i * 3 + k] = x[bt * 3 + k] + body.off[s][k];
}

__device__ __forceinline__ double traj_norm(double a, double b, double c) { return sqrt((a * a + b * b) + c * c); }

__global__ __launch_bounds__(256) void traj_step_kernel(const TrajParams p, const TrajBody body, float* __restrict__ x,
                                                        int32_t* __restrict__ state, const float* __restrict__ sdf,
                                                        const float* __restrict__ grad, double* __restrict__ records,
                                                        float* __restrict__ q_out, double* __restrict__ grad_out) {
  extern __shared__ double lds[];         // cv [3][T]: C_t vh_t, then P;  nab [3][T]: sigma_t G_t, then grad_t, then y_t
  __shared__ double sh[4][DSLOTS];
  __shared__ double shm[4];
  const int T = p.T, S = p.S, n = T - 2, tid = threadIdx.x;
  double* cv = lds;
  double* nab = lds + 3 * T;
  const int64_t b = blockIdx.x;
  float* xb = x + b * T * 3;
  const int state_in = state[b];
  const double eps = (double)p.eps, w_obs = (double)p.w_obs, ws = (double)p.w_smooth * (double)(T - 1);

  DescentSums sums;
  for (int t = tid; t < T; t += 256) {
    const bool interior = t > 0 && t < T - 1;
    double C = 0.0, G0 = 0.0, G1 = 0.0, G2 = 0.0;
    const int64_t i0 = (b * T + t) * S;
    for (int s = 0; s < S; ++s) {
      const double sd = (double)sdf[i0 + s];
      const double g0 = (double)grad[(i0 + s) * 3], g1 = (double)grad[(i0 + s) * 3 + 1], g2 = (double)grad[(i0 + s) * 3 + 2];
      const int bad = (isfinite(sd) ? 0 : 1) + (isfinite(g0) ? 0 : 1) + (isfinite(g1) ? 0 : 1) + (isfinite(g2) ? 0 : 1);
      if (bad) {
        sums.n_bad += (double)bad;
        continue;
      }
      const double d = sd - (double)body.rad[s];
      sums.clearance(d, eps);
      double c, cp;
      descent_cost(d, eps, c, cp);
      if (interior) {
        C += c;
        G0 += cp * g0;
        G1 += cp * g1;
        G2 += cp * g2;
      }
    }
    const double c0 = (double)xb[t * 3], c1 = (double)xb[t * 3 + 1], c2 = (double)xb[t * 3 + 2];
    if (t < T - 1) {
      const double e0 = (double)xb[t * 3 + 3] - c0, e1 = (double)xb[t * 3 + 4] - c1, e2 = (double)xb[t * 3 + 5] - c2;
      const double q = (e0 * e0 + e1 * e1) + e2 * e2;
      sums.seg2 += q;
      sums.len += sqrt(q);
    }
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (interior) {
      const double v0 = ((double)xb[t * 3 + 3] - (double)xb[t * 3 - 3]) * 0.5, v1 = ((double)xb[t * 3 + 4] - (double)xb[t * 3 - 2]) * 0.5,
                   v2 = ((double)xb[t * 3 + 5] - (double)xb[t * 3 - 1]) * 0.5;
      const double sigma = traj_norm(v0, v1, v2);
      const bool go = sigma > 0.0;
      const double h0 = go ? v0 / sigma : 0.0, h1 = go ? v1 / sigma : 0.0, h2 = go ? v2 / sigma : 0.0;
      a0 = C * h0; a1 = C * h1; a2 = C * h2;
      s0 = sigma * G0; s1 = sigma * G1; s2 = sigma * G2;
      sums.f_obs += C * sigma;
    }
    cv[t] = a0; cv[T + t] = a1; cv[2 * T + t] = a2;
    nab[t] = s0; nab[T + t] = s1; nab[2 * T + t] = s2;
  }
  __syncthreads();

  for (int t = tid; t < T; t += 256) {
    double r0 = 0.0, r1 = 0.0, r2 = 0.0;
    if (t > 0 && t < T - 1) {
      const double o0 = nab[t] + (cv[t - 1] - cv[t + 1]) * 0.5, o1 = nab[T + t] + (cv[T + t - 1] - cv[T + t + 1]) * 0.5,
                   o2 = nab[2 * T + t] + (cv[2 * T + t - 1] - cv[2 * T + t + 1]) * 0.5;
      const double m0 = (2.0 * (double)xb[t * 3] - (double)xb[t * 3 - 3]) - (double)xb[t * 3 + 3],
                   m1 = (2.0 * (double)xb[t * 3 + 1] - (double)xb[t * 3 - 2]) - (double)xb[t * 3 + 4],
                   m2 = (2.0 * (double)xb[t * 3 + 2] - (double)xb[t * 3 - 1]) - (double)xb[t * 3 + 5];
      r0 = w_obs * o0 + ws * m0;
      r1 = w_obs * o1 + ws * m1;
      r2 = w_obs * o2 + ws * m2;
      sums.gsq += (r0 * r0 + r1 * r1) + r2 * r2;
    }
    nab[t] = r0; nab[T + t] = r1; nab[2 * T + t] = r2;        // only waypoint t's own entries of nab are read above
    if (grad_out) {
      double* go = grad_out + (b * T + t) * 3;
      go[0] = r0; go[1] = r1; go[2] = r2;
    }
  }

  const double bad_total = descent_reduce(sums, sh);          // a barrier: sh, and every grad_t in nab; cv is free from here

  double m = 0.0;
  if (state_in == 0) {                    // uniform over the workgroup
    if (tid < 3) descent_solve(nab + tid * T, cv + tid * T, n);
    __syncthreads();
    const double scale = (double)p.eta * (double)(T - 1);
    for (int t = tid; t < T; t += 256) {
      double d0 = 0.0, d1 = 0.0, d2 = 0.0;
      if (t > 0 && t < T - 1) {
        d0 = -(nab[t] / scale); d1 = -(nab[T + t] / scale); d2 = -(nab[2 * T + t] / scale);
      }
      nab[t] = d0; nab[T + t] = d1; nab[2 * T + t] = d2;
      m = fmax(m, traj_norm(d0, d1, d2));
    }
    m = wave_reduce<RedMax>(m);
    if ((tid & 63) == 0) shm[tid >> 6] = m;         // lane 0 of each wave
    __syncthreads();
    m = waves_combine<RedMax>(shm[0], shm[1], shm[2], shm[3]);
  }

  const DescentClose cl = descent_close(state_in, bad_total, m, (double)p.tol, (double)p.max_step);
  descent_record(sh, T, m, bad_total, state_in, cl, 0.0, records + b * DREC, state + b);

  // every read of x above is complete: the values went into LDS and registers before the barriers
  if (!cl.apply && !q_out) return;
  for (int t = tid; t < T; t += 256) {
    float y0 = xb[t * 3], y1 = xb[t * 3 + 1], y2 = xb[t * 3 + 2];
    if (cl.apply && t > 0 && t < T - 1) {
      y0 = (float)((double)y0 + cl.kappa * nab[t]);
      y1 = (float)((double)y1 + cl.kappa * nab[T + t]);
      y2 = (float)((double)y2 + cl.kappa * nab[2 * T + t]);
      xb[t * 3] = y0; xb[t * 3 + 1] = y1; xb[t * 3 + 2] = y2;
    }
    if (q_out) {
      float* q = q_out + (b * T + t) * S * 3;
      for (int s = 0; s < S; ++s) {
        q[s * 3] = y0 + body.off[s][0];
        q[s * 3 + 1] = y1 + body.off[s][1];
        q[s * 3 + 2] = y2 + body.off[s][2];
      }
    }
  }
}

static void traj_body(const isdf_traj_args& a, TrajBody* body) {
  for (int s = 0; s < TMAXS; ++s) {
    const int r = s < a.S ? s : 0;            // unused slots: sphere 0 again, never indexed
    for (int k = 0; k < 3; ++k) body->off[s][k] = a.offsets[r * 3 + k];
    body->rad[s] = a.radii[r];
  }
}

int launch_traj_points(const isdf_traj_args& a, float* q_out, hipStream_t st) {
  TrajBody body;
  traj_body(a, &body);
  const int64_t n = (int64_t)a.B * a.T * a.S;         // <= 2^31 - 1 (capi.hip)
  hipLaunchKernelGGL(traj_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a.x, body, a.S, n, q_out);
  return isdf_launch_status();
}

int launch_traj_step(const isdf_traj_args& a, const float* sdf, const float* grad, double* records, float* q_out, double* grad_out,
                     hipStream_t st) {
  TrajBody body;
  traj_body(a, &body);
  TrajParams p;
  p.T = a.T; p.S = a.S;
  p.eps = a.eps; p.w_obs = a.w_obs; p.w_smooth = a.w_smooth; p.eta = a.eta; p.max_step = a.max_step; p.tol = a.tol;
  const size_t lds_bytes = (size_t)6 * a.T * sizeof(double);       // <= 48 KB at ISDF_TRAJ_MAX_WAYPOINTS
  hipLaunchKernelGGL(traj_step_kernel, dim3((unsigned)a.B), dim3(256), lds_bytes, st, p, body, a.x, a.state, sdf, grad, records, q_out,
                     grad_out);
  return isdf_launch_status();
}

}  // namespace isdf
