"""Planning against the map on the device (include/isdf_hip.h: isdf_traj_points, isdf_traj_step).

"Here is a map, a start and a goal; how do I get there without touching anything?" -- covariant (CHOMP-style) gradient descent on B
trajectories at once.  The reference has no counterpart: its `eval_traj_cost` scores a recorded camera path, it never moves one.

    trajectory_step         one linearisation of B trajectories on a copy of x: costs, clearances, step length (TrajStep)
    optimise_trajectories   the loop; per iteration ONE field call over all B * T * S query points and ONE step launch, nothing
                            in between and no host synchronisation; every `check_every` iterations one copy of B x 16 doubles
    seed_trajectories       the straight line and sinusoidal bulges of it
    plan_path               seeds, one batch, and the cheapest trajectory that is free of collision

Conventions.  A trajectory is T waypoints x[t] in the world frame, fp32; waypoints 0 and T-1 are fixed.  The robot is S spheres
(offset o_s, radius r_s) that translate with the waypoint: query points q[t][s] = x[t] + o_s, clearance d = sdf(q) - r_s.  Cost
c(d) = -d + eps/2 for d < 0, (d - eps)^2 / (2 eps) for 0 <= d <= eps, 0 beyond (metrics.chomp_cost).  With v_t = (x_{t+1} -
x_{t-1}) / 2, sigma_t = |v_t| and C_t = sum_s c:  F_obs = sum_t C_t sigma_t (the arc-length integral of the cost), F_smooth =
(T-1)/2 sum_t |x_{t+1} - x_t|^2; the factor T-1 makes both, and the loop, independent of the resolution T.  The gradient is the
exact gradient of w_obs F_obs + w_smooth F_smooth; the step is -(1/eta) K^-1 grad with K = (T-1) tridiag(-1, 2, -1), scaled so
that no waypoint moves further than max_step.  State per trajectory: 0 moving, 1 converged (longest waypoint step < tol; x is
left as the record describes it), 2 invalid (a field value that is not finite; x is left alone).  No step rejection, no line
search, no rotation.  Module-level functions only: nothing is added to HotPath or HipState.
"""
import collections

import numpy as np
import torch

from . import _ffi
from .engine import host_array

REC = _ffi.TRAJ_RECORD
MOVING, CONVERGED, INVALID = 0, 1, 2

TrajStep = collections.namedtuple("TrajStep", "cost_obs cost_smooth min_clearance in_collision active grad_sq step scale bad state "
                                              "length records")
TrajStep.__doc__ = """One linearisation, float64 numpy, one entry per trajectory: cost_obs = F_obs, cost_smooth = F_smooth,
min_clearance (+inf without a finite sample), in_collision = samples with d < 0, active = samples with d < eps, grad_sq = sum
|grad_t|^2, step = the longest waypoint step before the clamp, scale = the clamp factor applied (0: no step), bad = non-finite
field values, state after the call, length of the path, records [B,16] as the kernel wrote them."""

PlanResult = collections.namedtuple("PlanResult", "x state reason iterations records")
PlanResult.__doc__ = """x [B,T,3] float32 on the device; state int [B] (0 moving, 1 converged, 2 invalid), reason (list of str:
"converged", "max_iters", "invalid_field"), iterations (int: step launches issued), records: the TrajStep of the last launch --
for a converged trajectory it describes exactly the x returned."""

_REASON = {MOVING: "max_iters", CONVERGED: "converged", INVALID: "invalid_field"}
DEFAULTS = dict(eps=0.2, w_obs=8.0, w_smooth=1.0, eta=8.0, max_step=0.05, tol=1e-5)


class _Scratch:
    """per-device records and the pinned host mirror they are copied through"""

    def __init__(self, device):
        self.device = device
        self.records = None
        self.pinned = None

    def reserve(self, B):
        if self.records is None or self.records.shape[0] < B:
            self.records = torch.empty(B, REC, dtype=torch.float64, device=self.device)
            self.pinned = torch.empty(B, REC, dtype=torch.float64, pin_memory=self.device.type == "cuda")
        return self.records[:B]

    def fetch(self, records):
        """the records on the host: ONE copy into the pinned buffer, then the stream's end"""
        B = int(records.shape[0])
        if records.device.type != "cuda":
            return records.detach().numpy().astype(np.float64).reshape(B, REC)
        host = self.pinned[:B]
        host.copy_(records, non_blocking=True)
        torch.cuda.current_stream(records.device).synchronize()
        return host.numpy().copy()


_SCRATCH = {}


def _scratch(device):
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None or device.type != "cuda" else torch.cuda.current_device())
    s = _SCRATCH.get(key)
    if s is None:
        s = _SCRATCH[key] = _Scratch(device)
    return s


def _engine(obj):
    """an Engine, or anything that has one as `.engine` (SDFMapHIP, a grafted trainer)"""
    return getattr(obj, "engine", obj)


def unpack_records(records):
    """TrajStep of records [B, 16] (float64, host)"""
    r = np.asarray(records, np.float64).reshape(-1, REC)
    return TrajStep(*(r[:, k].copy() for k in range(11)), r)


def _setup(obj, x, offsets, radii, field):
    """(engine, a float32 device COPY of x [B,T,3], offsets [S,3], radii [S], field)"""
    eng = _engine(obj)
    x = torch.as_tensor(x)
    if x.dim() == 2:
        x = x[None]
    if x.dim() != 3 or x.shape[-1] != 3:
        raise ValueError("trajectories must be [B, T, 3] or [T, 3] (got %s)" % (tuple(x.shape),))
    x = x.detach().to(device=eng.device, dtype=torch.float32).contiguous().clone()
    off = np.zeros((1, 3), np.float32) if offsets is None else np.ascontiguousarray(
        host_array(offsets, np.float32)).reshape(-1, 3)
    rad = host_array(radii, np.float32).reshape(-1)
    rad = np.ascontiguousarray(np.broadcast_to(rad, (off.shape[0],)) if rad.size == 1 else rad)
    if rad.size != off.shape[0]:
        raise ValueError("%d offsets but %d radii" % (off.shape[0], rad.size))
    return eng, x, off, rad, default_field(eng) if field is None else field


def default_field(eng):
    """the engine's own map as a field: device points [N,3] -> `eng.sdf_eval(pts, want_grad=True)`, outside autograd"""
    def field(pts):
        with torch.no_grad():
            return eng.sdf_eval(pts, want_grad=True)
    return field


def one_step(var, points, step, field, want_grad, **params):
    """trajectory_step and kinematics.joint_step after their set-up: var [B,T,K] the device copy, every trajectory moving;
    points() -> q, step(state, q, sdf, grad, **kw) the engine's step call on var.  TrajStep, with want_grad also the gradient."""
    state = torch.zeros(var.shape[0], dtype=torch.int32, device=var.device)
    q = points()
    sdf, grad = field(q)
    out = step(state, q, sdf, grad, out=_scratch(var.device).reserve(var.shape[0]), want_grad=want_grad, **params)
    rec, g = out if want_grad else (out, None)
    res = unpack_records(_scratch(var.device).fetch(rec))
    return (res, g.detach().cpu().numpy()) if want_grad else res


def descend(var, points, step, field, iters, check_every, **params):
    """the loop of optimise_trajectories and kinematics.optimise_joint_trajectories on var [B,T,K], the device copy (points and
    step as in `one_step`; the step rewrites q in place): PlanResult"""
    B = int(var.shape[0])
    scratch = _scratch(var.device)
    rec = scratch.reserve(B)
    state = torch.zeros(B, dtype=torch.int32, device=var.device)
    q = points()
    iters, check_every = int(iters), max(1, int(check_every))
    host, done = None, 0
    while done < iters:
        sdf, grad = field(q)
        step(state, q, sdf, grad, out=rec, q_out=q, **params)
        done += 1
        if done % check_every == 0 or done == iters:
            host = scratch.fetch(rec)
            if not (host[:, 9] == MOVING).any():
                break
    if host is None:                      # iters < 1: nothing was launched
        host = np.zeros((B, REC))
    res = unpack_records(host)
    st = res.state.astype(np.int64)
    return PlanResult(var, st, [_REASON.get(int(s), "invalid_field") for s in st], done, res)


def best_trajectory(res, clearance, kw, defaults):
    """the index of the trajectory of the PlanResult with the lowest w_obs cost_obs + w_smooth cost_smooth (the weights from kw,
    else from defaults) among those whose state is not invalid, that have no sample in collision and whose least clearance is
    at least `clearance`; None if there is none"""
    r = res.records
    total = kw.get("w_obs", defaults["w_obs"]) * r.cost_obs + kw.get("w_smooth", defaults["w_smooth"]) * r.cost_smooth
    ok = (res.state != INVALID) & (r.in_collision == 0) & (r.min_clearance >= clearance) & np.isfinite(total)
    return int(np.argmin(np.where(ok, total, np.inf))) if ok.any() else None


def trajectory_step(engine, x, offsets=None, radii=0.0, eps=0.2, w_obs=8.0, w_smooth=1.0, eta=8.0, max_step=0.05, tol=1e-5,
                    field=None, want_grad=False):
    """TrajStep of ONE linearisation of the trajectories x [B,T,3] (or [T,3]), every one taken as moving; x itself is not touched
    (the step is applied to a copy).  offsets [S,3] (None: one sphere at the waypoint), radii [S] or a scalar.  field: callable,
    device points [N,3] -> (sdf [N], grad [N,3]) on the device; default `engine.sdf_eval(pts, want_grad=True)`.  With want_grad
    also the gradient of w_obs F_obs + w_smooth F_smooth, float64 numpy [B,T,3]."""
    eng, xc, off, rad, field = _setup(engine, x, offsets, radii, field)
    return one_step(xc, lambda: eng.traj_points(xc, off, rad), lambda state, q, sdf, grad, **kw: eng.traj_step(xc, state, off, rad, sdf, grad, **kw),
                    field, want_grad, eps=eps, w_obs=w_obs, w_smooth=w_smooth, eta=eta, max_step=max_step, tol=tol)


def optimise_trajectories(engine_or_sdf_map_or_trainer, x0, offsets=None, radii=0.0, eps=0.2, w_obs=8.0, w_smooth=1.0, eta=8.0,
                          max_step=0.05, tol=1e-5, iters=150, check_every=10, field=None):
    """PlanResult: the trajectories x0 [B,T,3] (or [T,3]; copied) after at most `iters` iterations of `Engine.traj_step`.

    The query points are computed once; then every iteration is `field(q)` and one step launch that also rewrites q for the
    next one.  Nothing is read back inside the loop: every `check_every` iterations, and at the end, the B x 16 doubles of the
    last launch are copied once through a pinned buffer, and the loop is left when no trajectory is moving any more.  The
    result does not depend on `check_every`: a trajectory that has stopped is left bit for bit by every later launch.

    The defaults are the values at which a float64 host prototype of this loop converged on the analytic room of
    `isdf_amd.synthetic`; they are not tuned on a trained map."""
    eng, x, off, rad, field = _setup(engine_or_sdf_map_or_trainer, x0, offsets, radii, field)
    return descend(x, lambda: eng.traj_points(x, off, rad), lambda state, q, sdf, grad, **kw: eng.traj_step(x, state, off, rad, sdf, grad, **kw),
                   field, iters, check_every, eps=eps, w_obs=w_obs, w_smooth=w_smooth, eta=eta, max_step=max_step, tol=tol)


def seed_trajectories(start, goal, T, n_seeds, spread=0.5, seed=0):
    """x [n_seeds, T, 3] float32 numpy: seed 0 is the straight line start -> goal at T evenly spaced waypoints; seed k is the line
    plus a_k sin(pi s) u_k (s in [0, 1] along the line) with u_k a unit vector perpendicular to goal - start and a_k uniform in
    (-spread, spread), all drawn from numpy.random.RandomState(seed).  Every seed starts at `start` and ends at `goal` exactly."""
    start, goal = np.asarray(start, np.float64).reshape(3), np.asarray(goal, np.float64).reshape(3)
    T, n_seeds = int(T), int(n_seeds)
    s = np.linspace(0.0, 1.0, T)
    line = start[None] + s[:, None] * (goal - start)[None]
    x = np.repeat(line[None], n_seeds, 0)
    rng = np.random.RandomState(seed)
    axis = goal - start
    norm = np.linalg.norm(axis)
    axis = axis / norm if norm > 0 else np.array([1.0, 0.0, 0.0])
    bulge = np.sin(np.pi * s)
    for k in range(1, n_seeds):
        u = rng.standard_normal(3)
        u = u - (u @ axis) * axis
        u = u / np.linalg.norm(u)
        x[k] += rng.uniform(-spread, spread) * bulge[:, None] * u[None]
    x = x.astype(np.float32)
    x[:, 0], x[:, -1] = start.astype(np.float32), goal.astype(np.float32)
    return x


def plan_path(obj, start, goal, T=64, n_seeds=32, clearance=0.0, spread=0.5, seed=0, **kw):
    """(PlanResult, best): `seed_trajectories(start, goal, T, n_seeds, spread, seed)` optimised as one batch (**kw goes to
    `optimise_trajectories`); best is the index of the trajectory with the lowest w_obs cost_obs + w_smooth cost_smooth among
    those whose state is not invalid, that have no sample in collision and whose least clearance is at least `clearance`;
    None if there is none."""
    res = optimise_trajectories(obj, seed_trajectories(start, goal, T, n_seeds, spread, seed), **kw)
    return res, best_trajectory(res, clearance, kw, DEFAULTS)
