// Planning for articulated robots (isdf_arm_points, isdf_arm_step): one iteration of covariant gradient descent on B trajectories in
// the joint space of a serial chain whose links carry collision spheres.  Reference: none (as traj.hip).  The mathematics,
// operation by operation, is the header's (include/isdf_hip.h); the file is built with -ffp-contract=off (build.py), so a host
// model written in the same order has the same terms bit for bit wherever no sin or cos enters.
//   arm_points_kernel   one thread per (b, t): the chain's frames in double, link by link, and the S query points in fp32
//   arm_step_kernel     one 256-thread workgroup per trajectory, everything in double on the fp32 inputs widened:
//     1  thread k takes waypoints k, k + 256, ..: the frames of its waypoint give a_j and p_j; its S samples (s ascending) give
//        the counts, sigma c and the workspace force r, which is summed per link as (sum r, sum q x r); a suffix sum over the
//        links and one dot product per joint give grad_t.  The neighbours' c h are RECOMPUTED from the inputs (the same
//        operations on the same values: the same bits), so no per-sample value crosses threads and nothing waits.
//        grad_t goes to LDS; the scalar sums, minimum and counts stay in registers
//     2  the record's sums: lanes by shuffle, the four waves in wave order (block_reduce.h)
//     3  (moving trajectories only) K^-1 grad by the closed-form inverse, one lane per joint; then the projected step Delta',
//        its infinity norm m and the number of clamped entries over all threads
//     4  state, record, the new theta and the query points of the theta the call leaves (the frames once more)
//   The cost, the sums, the solve, the state rule and the record are descent_dev.h's, shared with traj.hip.
// LDS: 2 J doubles per waypoint (grad / y / Delta', and P), allocated per launch: 16 J T bytes, 48 KB at J = 8 and
// ISDF_ARM_MAX_WAYPOINTS = 384 -- traj.hip's ceiling, which leaves the 64 KB a workgroup may ask for without an opt-in room for
// the 44 doubles of scalars.  Planes of T doubles per joint: a wave's 64 consecutive waypoints are 64 consecutive doubles.
// The chain travels as launch arguments (1.9 KB).  Every loop over joints and links is unrolled to ISDF_ARM_MAX_JOINTS with the
// joint index a constant (a joint beyond J is a uniform branch not taken), and a sphere finds its link's accumulator through
// uniform branches on its link number: nothing is indexed dynamically in registers, no scratch.
#include "isdf_common.h"
#include "launchers.h"
#include "block_reduce.h"
#include "descent_dev.h"

namespace isdf {

constexpr int AJ = ISDF_ARM_MAX_JOINTS;
constexpr int AS = ISDF_ARM_MAX_SPHERES;

struct ArmChain {
  float base[12];
  float X[AJ][12];
  float axis[AJ][3];
  float lo[AJ], hi[AJ];
  int32_t kind[AJ];
  int32_t link[AS];
  float ctr[AS][3];
  float rad[AS];
};

struct ArmParams {
  int32_t T, J, S;
  float eps, w_obs, w_smooth, eta, max_step, tol;
};

__device__ __forceinline__ double arm_dot(double a0, double a1, double a2, double b0, double b1, double b2) {
  return (a0 * b0 + a1 * b1) + a2 * b2;
}

// An entry of the chain, widened.  The entries are uniform and the same for every waypoint: left to itself the compiler widens all
// 150 of them once, ahead of the waypoint loops, and holds 300 registers of doubles through the kernel.  The empty statement pins
// each conversion to its place of use; the value stays in its scalar register.
__device__ __forceinline__ double arm_wide(float v) {
  asm volatile("" : "+s"(v));
  return (double)v;
}

// the query points of the spheres on link l under the frame (R, t)
__device__ __forceinline__ void arm_emit(const ArmChain& ch, int S, int l, const double (&R)[9], const double (&t)[3], float* q) {
  for (int s = 0; s < S; ++s) {
    if (ch.link[s] != l) continue;                      // uniform
    const double o0 = arm_wide(ch.ctr[s][0]), o1 = arm_wide(ch.ctr[s][1]), o2 = arm_wide(ch.ctr[s][2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) q[s * 3 + r] = (float)(arm_dot(R[3 * r], R[3 * r + 1], R[3 * r + 2], o0, o1, o2) + t[r]);
  }
}

// the frames of one configuration, link by link: joint(j, a, p) receives every joint's world axis and origin (j a constant after
// unrolling), EMIT writes the query points q[S][3]
template <bool EMIT, class F>
__device__ __forceinline__ void arm_fk(const ArmChain& ch, int J, int S, const double (&th)[AJ], float* q, F&& joint) {
  double R[9], t[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) R[3 * r + c] = arm_wide(ch.base[4 * r + c]);
    t[r] = arm_wide(ch.base[4 * r + 3]);
  }
  if (EMIT) arm_emit(ch, S, 0, R, t, q);
#pragma unroll
  for (int j = 0; j < AJ; ++j) {
    if (j < J) {                                        // uniform
      double X[12], A[9], p[3], a[3];
#pragma unroll
      for (int i = 0; i < 12; ++i) X[i] = arm_wide(ch.X[j][i]);
      const double u0 = arm_wide(ch.axis[j][0]), u1 = arm_wide(ch.axis[j][1]), u2 = arm_wide(ch.axis[j][2]);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) A[3 * r + c] = arm_dot(R[3 * r], R[3 * r + 1], R[3 * r + 2], X[c], X[4 + c], X[8 + c]);
        p[r] = arm_dot(R[3 * r], R[3 * r + 1], R[3 * r + 2], X[3], X[7], X[11]) + t[r];
      }
#pragma unroll
      for (int r = 0; r < 3; ++r) a[r] = arm_dot(A[3 * r], A[3 * r + 1], A[3 * r + 2], u0, u1, u2);
      joint(j, a, p);
      if (ch.kind[j] == 0) {                            // revolute: Rodrigues about u
        const double sn = sin(th[j]), cs = cos(th[j]), k = 1.0 - cs;
        double M[9];
        M[0] = cs + k * (u0 * u0);      M[1] = k * (u0 * u1) - sn * u2; M[2] = k * (u0 * u2) + sn * u1;
        M[3] = k * (u1 * u0) + sn * u2; M[4] = cs + k * (u1 * u1);      M[5] = k * (u1 * u2) - sn * u0;
        M[6] = k * (u2 * u0) - sn * u1; M[7] = k * (u2 * u1) + sn * u0; M[8] = cs + k * (u2 * u2);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int c = 0; c < 3; ++c) R[3 * r + c] = arm_dot(A[3 * r], A[3 * r + 1], A[3 * r + 2], M[c], M[3 + c], M[6 + c]);
          t[r] = p[r];
        }
      } else {                                          // prismatic: along a_j
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = A[i];
#pragma unroll
        for (int r = 0; r < 3; ++r) t[r] = p[r] + th[j] * a[r];
      }
      if (EMIT) arm_emit(ch, S, j + 1, R, t, q);
    }
  }
}

struct ArmNoJoint {
  __device__ __forceinline__ void operator()(int, const double (&)[3], const double (&)[3]) const {}
};

__global__ __launch_bounds__(256) void arm_points_kernel(const float* __restrict__ theta, const ArmChain ch, int32_t J, int32_t S,
                                                         int64_t n, float* __restrict__ q) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // b * T + t
  if (i >= n) return;
  double th[AJ];
#pragma unroll
  for (int j = 0; j < AJ; ++j) th[j] = j < J ? (double)theta[i * J + j] : 0.0;
  arm_fk<true>(ch, J, S, th, q + i * S * 3, ArmNoJoint());
}

// sample (t, s) of one trajectory: bad = how many of its four field values are not finite; for a sample that is not bad its
// clearance d and, at an interior t, the cost c, its slope cp and the speed sigma and direction h of its body point from the
// neighbours' query points (all 0 otherwise)
struct ArmSample { double d, c, cp, sigma, h[3], g[3]; int bad; };

__device__ __forceinline__ void arm_sample(const float* qb, const float* __restrict__ sdfb, const float* __restrict__ gradb, int t,
                                           int s, int S, double eps, double rad, bool interior, ArmSample& o) {
  const int64_t i = (int64_t)t * S + s;
  const double sd = (double)sdfb[i];
  o.g[0] = (double)gradb[i * 3]; o.g[1] = (double)gradb[i * 3 + 1]; o.g[2] = (double)gradb[i * 3 + 2];
  o.bad = (isfinite(sd) ? 0 : 1) + (isfinite(o.g[0]) ? 0 : 1) + (isfinite(o.g[1]) ? 0 : 1) + (isfinite(o.g[2]) ? 0 : 1);
  o.d = sd - rad;
  o.c = 0.0; o.cp = 0.0; o.sigma = 0.0;
  o.h[0] = 0.0; o.h[1] = 0.0; o.h[2] = 0.0;
  if (o.bad || !interior) return;
  descent_cost(o.d, eps, o.c, o.cp);
  const int64_t ip = (i + S) * 3, im = (i - S) * 3;
  const double v0 = ((double)qb[ip] - (double)qb[im]) * 0.5, v1 = ((double)qb[ip + 1] - (double)qb[im + 1]) * 0.5,
               v2 = ((double)qb[ip + 2] - (double)qb[im + 2]) * 0.5;
  o.sigma = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
  if (o.sigma > 0.0) {
    o.h[0] = v0 / o.sigma; o.h[1] = v1 / o.sigma; o.h[2] = v2 / o.sigma;
  }
}

__global__ __launch_bounds__(256) void arm_step_kernel(const ArmParams p, const ArmChain ch, float* theta, int32_t* __restrict__ state,
                                                       const float* q, const float* __restrict__ sdf, const float* __restrict__ grad,
                                                       double* __restrict__ records, float* q_out, double* __restrict__ grad_out) {
  extern __shared__ double lds[];         // gy [J][T]: grad_t, then y_t, then Delta'_t;  P [J][T]
  __shared__ double sh[4][DSLOTS];
  __shared__ double shm[4];
  const int T = p.T, J = p.J, S = p.S, n = T - 2, tid = threadIdx.x;
  double* gy = lds;
  double* Pp = lds + J * T;
  const int64_t b = blockIdx.x;
  float* thb = theta + b * T * J;
  const float* qb = q + b * T * S * 3;
  const float* sdfb = sdf + b * T * S;
  const float* gradb = grad + b * T * S * 3;
  const int state_in = state[b];
  const double eps = (double)p.eps, w_obs = (double)p.w_obs, ws = (double)p.w_smooth * (double)(T - 1);

  DescentSums sums;
  for (int t = tid; t < T; t += 256) {
    const bool interior = t > 0 && t < T - 1;
    double th[AJ], gt[AJ];                 // gt: the smoothness term first, then grad_t
    double qd = 0.0;
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      th[j] = 0.0; gt[j] = 0.0;
      if (j < J) {
        th[j] = (double)thb[t * J + j];
        if (t < T - 1) {
          const double e = (double)thb[(t + 1) * J + j] - th[j];
          qd = qd + e * e;
        }
        if (interior) gt[j] = (2.0 * th[j] - (double)thb[(t - 1) * J + j]) - (double)thb[(t + 1) * J + j];
      }
    }
    if (t < T - 1) {
      sums.seg2 += qd;
      sums.len += sqrt(qd);
    }

    double Rl[AJ][3], Ml[AJ][3];            // per link 1 .. J: sum r, sum q x r
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { Rl[j][k] = 0.0; Ml[j][k] = 0.0; }
    }
    double fo = 0.0;
    for (int s = 0; s < S; ++s) {
      const double rad = (double)ch.rad[s];
      ArmSample me;
      arm_sample(qb, sdfb, gradb, t, s, S, eps, rad, interior, me);
      if (me.bad) {
        sums.n_bad += (double)me.bad;
        continue;
      }
      sums.clearance(me.d, eps);
      if (!interior) continue;
      fo = fo + me.c * me.sigma;
      ArmSample lo, hi;                     // the neighbours in t: c = 0 and h = 0 at a fixed waypoint and for a bad sample
      arm_sample(qb, sdfb, gradb, t - 1, s, S, eps, rad, t - 1 > 0, lo);
      arm_sample(qb, sdfb, gradb, t + 1, s, S, eps, rad, t + 1 < T - 1, hi);
      const double e = me.sigma * me.cp;
      const double r0 = e * me.g[0] + (lo.c * lo.h[0] - hi.c * hi.h[0]) * 0.5, r1 = e * me.g[1] + (lo.c * lo.h[1] - hi.c * hi.h[1]) * 0.5,
                   r2 = e * me.g[2] + (lo.c * lo.h[2] - hi.c * hi.h[2]) * 0.5;
      const int64_t i = ((int64_t)t * S + s) * 3;
      const double q0 = (double)qb[i], q1 = (double)qb[i + 1], q2 = (double)qb[i + 2];
      const double x0 = q1 * r2 - q2 * r1, x1 = q2 * r0 - q0 * r2, x2 = q0 * r1 - q1 * r0;
      const int link = ch.link[s];          // uniform: a link-0 sphere is static and pulls on no joint
#pragma unroll
      for (int j = 0; j < AJ; ++j) {
        if (link == j + 1) {
          Rl[j][0] += r0; Rl[j][1] += r1; Rl[j][2] += r2;
          Ml[j][0] += x0; Ml[j][1] += x1; Ml[j][2] += x2;
        }
      }
    }

    double g2 = 0.0;
    if (interior) {
      sums.f_obs += fo;
#pragma unroll
      for (int j = AJ - 2; j >= 0; --j) {                 // suffix sums over the links, in place
        if (j + 1 < J) {
#pragma unroll
          for (int k = 0; k < 3; ++k) { Rl[j][k] = Rl[j + 1][k] + Rl[j][k]; Ml[j][k] = Ml[j + 1][k] + Ml[j][k]; }
        }
      }
      arm_fk<false>(ch, J, S, th, nullptr, [&](int j, const double (&a)[3], const double (&pj)[3]) __attribute__((always_inline)) {
        double o;
        if (ch.kind[j] == 0) {
          const double w0 = Ml[j][0] - (pj[1] * Rl[j][2] - pj[2] * Rl[j][1]), w1 = Ml[j][1] - (pj[2] * Rl[j][0] - pj[0] * Rl[j][2]),
                       w2 = Ml[j][2] - (pj[0] * Rl[j][1] - pj[1] * Rl[j][0]);
          o = arm_dot(a[0], a[1], a[2], w0, w1, w2);
        } else {
          o = arm_dot(a[0], a[1], a[2], Rl[j][0], Rl[j][1], Rl[j][2]);
        }
        gt[j] = w_obs * o + ws * gt[j];
      });
#pragma unroll
      for (int j = 0; j < AJ; ++j)
        if (j < J) g2 = g2 + gt[j] * gt[j];
      sums.gsq += g2;
    }
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      if (j < J) {
        gy[j * T + t] = gt[j];
        if (grad_out) grad_out[(b * T + t) * J + j] = gt[j];
      }
    }
  }

  const double bad_total = descent_reduce(sums, sh);          // a barrier: sh, and every grad_t in gy; every read of q is complete

  double m = 0.0, n_cut = 0.0;
  if (state_in == 0) {                    // uniform over the workgroup
    if (tid < J) descent_solve(gy + tid * T, Pp + tid * T, n);
    __syncthreads();
    const double scale = (double)p.eta * (double)(T - 1);
    for (int t = tid; t < T; t += 256) {
      const bool interior = t > 0 && t < T - 1;
#pragma unroll
      for (int j = 0; j < AJ; ++j) {
        if (j < J) {
          double dp = 0.0;
          if (interior) {
            const double th = (double)thb[t * J + j];
            const double z0 = th + -(gy[j * T + t] / scale);
            const double z = fmin(fmax(z0, (double)ch.lo[j]), (double)ch.hi[j]);
            dp = z - th;
            n_cut += z != z0 ? 1.0 : 0.0;
            m = fmax(m, fabs(dp));
          }
          gy[j * T + t] = dp;             // only thread t's own entries of gy are read above
        }
      }
    }
    m = wave_reduce<RedMax>(m);
    n_cut = wave_reduce<RedSum>(n_cut);
    if ((tid & 63) == 0) {                // lane 0 of each wave
      shm[tid >> 6] = m;
      sh[tid >> 6][8] = n_cut;
    }
    __syncthreads();
    m = waves_combine<RedMax>(shm[0], shm[1], shm[2], shm[3]);
    n_cut = descent_sum4(sh, 8);
  }

  const DescentClose cl = descent_close(state_in, bad_total, m, (double)p.tol, (double)p.max_step);
  descent_record(sh, T, m, bad_total, state_in, cl, n_cut, records + b * DREC, state + b);

  // every read of theta's neighbours and of q lies before the barriers above: thread t now rewrites row t alone
  if (!cl.apply && !q_out) return;
  for (int t = tid; t < T; t += 256) {
    const bool move = cl.apply && t > 0 && t < T - 1;
    double th[AJ];
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      th[j] = 0.0;
      if (j < J) {
        float y = thb[t * J + j];
        if (move) {
          y = (float)((double)y + cl.kappa * gy[j * T + t]);
          thb[t * J + j] = y;
        }
        th[j] = (double)y;
      }
    }
    if (q_out) arm_fk<true>(ch, J, S, th, q_out + (b * T + t) * S * 3, ArmNoJoint());
  }
}

static void arm_chain(const isdf_arm_args& a, ArmChain* ch) {
  for (int i = 0; i < 12; ++i) ch->base[i] = a.base[i];
  for (int j = 0; j < AJ; ++j) {
    const int r = j < a.J ? j : 0;            // unused slots: joint 0 again, never reached
    for (int i = 0; i < 12; ++i) ch->X[j][i] = a.X[r * 12 + i];
    for (int k = 0; k < 3; ++k) ch->axis[j][k] = a.axes[r * 3 + k];
    ch->kind[j] = a.kinds[r];
    ch->lo[j] = a.lo ? a.lo[r] : -INFINITY;
    ch->hi[j] = a.hi ? a.hi[r] : INFINITY;
  }
  for (int s = 0; s < AS; ++s) {
    const int r = s < a.S ? s : 0;
    for (int k = 0; k < 3; ++k) ch->ctr[s][k] = a.centres[r * 3 + k];
    ch->rad[s] = a.radii[r];
    ch->link[s] = a.links[r];
  }
}

int launch_arm_points(const isdf_arm_args& a, float* q_out, hipStream_t st) {
  ArmChain ch;
  arm_chain(a, &ch);
  const int64_t n = (int64_t)a.B * a.T;
  hipLaunchKernelGGL(arm_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a.theta, ch, a.J, a.S, n, q_out);
  return isdf_launch_status();
}

int launch_arm_step(const isdf_arm_args& a, const float* q, const float* sdf, const float* grad, double* records, float* q_out,
                    double* grad_out, hipStream_t st) {
  ArmChain ch;
  arm_chain(a, &ch);
  ArmParams p;
  p.T = a.T; p.J = a.J; p.S = a.S;
  p.eps = a.eps; p.w_obs = a.w_obs; p.w_smooth = a.w_smooth; p.eta = a.eta; p.max_step = a.max_step; p.tol = a.tol;
  const size_t lds_bytes = (size_t)2 * a.J * a.T * sizeof(double);       // <= 48 KB at ISDF_ARM_MAX_JOINTS x ISDF_ARM_MAX_WAYPOINTS
  hipLaunchKernelGGL(arm_step_kernel, dim3((unsigned)a.B), dim3(256), lds_bytes, st, p, ch, a.theta, a.state, q, sdf, grad, records,
                     q_out, grad_out);
  return isdf_launch_status();
}

}  // namespace isdf
