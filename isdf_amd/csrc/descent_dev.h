// Phases 2 to 4 of one covariant gradient-descent step, the part traj.hip and arm.hip do identically (include/isdf_hip.h states
// the mathematics): the cost of a clearance, the per-thread sums of the record and their block reduction, the closed-form K^-1
// solve of one coordinate plane, the state rule with its clamp factor, and the record and state stores.  What differs between
// the planners -- the linearisation, the step length, the write-back and the query points -- stays in their files.  Every piece is
// inlined into a 256-thread workgroup's kernel; LDS planes arrive as pointers, scalars by value, nothing is indexed dynamically
// in registers.  Both files are built with -ffp-contract=off: each product and sum below is rounded on its own, in this order.
#pragma once
#include "isdf_common.h"
#include "block_reduce.h"

namespace isdf {

constexpr int DREC = ISDF_TRAJ_RECORD;
constexpr int DSLOTS = 9;                 // sh[wave][0..7]: the sums below; [8]: the caller's (arm.hip: entries a limit cut)

// c(d) and c'(d) of the clearance d
__device__ __forceinline__ void descent_cost(double d, double eps, double& c, double& cp) {
  c = 0.0; cp = 0.0;
  if (d < 0.0) {
    c = -d + eps * 0.5;
    cp = -1.0;
  } else if (d <= eps) {
    const double u = d - eps;
    c = (u * u) / (2.0 * eps);
    cp = u / eps;
  }
}

// slot v of the four waves, in wave order
__device__ __forceinline__ double descent_sum4(const double (*sh)[DSLOTS], int v) {
  return waves_combine<RedSum>(sh[0][v], sh[1][v], sh[2][v], sh[3][v]);
}

// what a thread gathers over its waypoints for the record
struct DescentSums {
  double f_obs = 0.0, seg2 = 0.0, len = 0.0, gsq = 0.0, mind = (double)INFINITY, n_neg = 0.0, n_act = 0.0, n_bad = 0.0;
  // a sample whose four field values are finite, of clearance d
  __device__ __forceinline__ void clearance(double d, double eps) {
    mind = fmin(mind, d);
    n_neg += d < 0.0 ? 1.0 : 0.0;
    n_act += d < eps ? 1.0 : 0.0;
  }
};

// the lanes by shuffle, lane 0 of each wave into its row of sh, ONE BARRIER; returns the block's count of bad field values
__device__ __forceinline__ double descent_reduce(const DescentSums& a, double (*sh)[DSLOTS]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double v0 = wave_reduce<RedSum>(a.f_obs), v1 = wave_reduce<RedSum>(a.seg2), v2 = wave_reduce<RedMin>(a.mind),
               v3 = wave_reduce<RedSum>(a.n_neg), v4 = wave_reduce<RedSum>(a.n_act), v5 = wave_reduce<RedSum>(a.gsq),
               v6 = wave_reduce<RedSum>(a.n_bad), v7 = wave_reduce<RedSum>(a.len);
  if (lane == 0) {
    sh[wave][0] = v0; sh[wave][1] = v1; sh[wave][2] = v2; sh[wave][3] = v3;
    sh[wave][4] = v4; sh[wave][5] = v5; sh[wave][6] = v6; sh[wave][7] = v7;
  }
  __syncthreads();
  return descent_sum4(sh, 6);
}

// g[1..n] <- A^-1 g for A = tridiag(-1, 2, -1) by the closed-form inverse: two ordered prefix sums, P[1..n] the scratch plane --
// 2 n dependent adds, no division on the chain; one lane per coordinate plane
__device__ __forceinline__ void descent_solve(double* g, double* P, int n) {
  double acc = 0.0;
  for (int i = 1; i <= n; ++i) {
    acc = acc + (double)i * g[i];
    P[i] = acc;
  }
  acc = 0.0;
  const double n1 = (double)(n + 1);
  for (int i = n; i >= 1; --i) {
    const double gi = g[i], w = (double)(n + 1 - i);
    g[i] = (w * P[i] + (double)i * acc) / n1;
    acc = acc + w * gi;
  }
}

struct DescentClose { int state_out; double kappa; bool apply; };         // kappa: the clamp factor applied, 0: no step

// a moving trajectory with a bad field value becomes invalid, one whose step length m is below tol converged; otherwise it moves
__device__ __forceinline__ DescentClose descent_close(int state_in, double bad_total, double m, double tol, double max_step) {
  DescentClose c = {state_in, 0.0, false};
  if (state_in == 0) {
    if (bad_total > 0.0) c.state_out = 2;
    else if (m < tol) c.state_out = 1;
    else c.kappa = m <= max_step ? 1.0 : max_step / m;
  }
  c.apply = state_in == 0 && c.state_out == 0;
  return c;
}

// the record rec[0..15], one entry per thread (extra: entry 11), and the state if it changed
__device__ __forceinline__ void descent_record(const double (*sh)[DSLOTS], int T, double m, double bad_total, int state_in,
                                               const DescentClose& c, double extra, double* __restrict__ rec,
                                               int32_t* __restrict__ state) {
  const int tid = threadIdx.x;
  if (tid < DREC) {
    double v = 0.0;
    if (tid == 2) v = waves_combine<RedMin>(sh[0][2], sh[1][2], sh[2][2], sh[3][2]);
    else if (tid == 0) v = descent_sum4(sh, 0);
    else if (tid == 1) v = (0.5 * (double)(T - 1)) * descent_sum4(sh, 1);
    else if (tid == 3) v = descent_sum4(sh, 3);
    else if (tid == 4) v = descent_sum4(sh, 4);
    else if (tid == 5) v = descent_sum4(sh, 5);
    else if (tid == 6) v = m;
    else if (tid == 7) v = c.kappa;
    else if (tid == 8) v = bad_total;
    else if (tid == 9) v = (double)c.state_out;
    else if (tid == 10) v = descent_sum4(sh, 7);
    else if (tid == 11) v = extra;
    rec[tid] = v;
  }
  if (tid == 0 && c.state_out != state_in) *state = c.state_out;
}

}  // namespace isdf
