"""Planning for articulated robots on the device (include/isdf_hip.h: isdf_arm_points, isdf_arm_step).

`isdf_amd.planning` moves S spheres that translate with a waypoint.  This module plans for a robot that has joints: a serial
kinematic chain with collision spheres on its links -- an arm on a fixed base, a free-flying rigid body (three prismatic and three
revolute joints), a mobile base with yaw (two prismatic joints and one revolute).  The cost, the preconditioner, the states and the
loop are planning's; the trajectory lives in joint space and the gradient is pulled back through the chain's Jacobian.

    Chain                          the robot: joints, fixed transforms, collision spheres, limits; validated on the host
    joint_step                     one linearisation of B joint-space trajectories on a copy of theta (TrajStep)
    optimise_joint_trajectories    the loop; per iteration ONE field call over all B * T * S query points and ONE step launch,
                                   nothing in between and no host synchronisation; every `check_every` iterations one copy of
                                   B x 16 doubles
    seed_joint_trajectories        the straight line in joint space and sinusoidal bulges of it
    plan_joint_path                seeds, one batch, and the cheapest trajectory that is free of collision

Conventions.  A trajectory is T configurations theta[t] (J joint values: radians for a revolute joint, metres for a prismatic
one), fp32; rows 0 and T-1 are fixed.  Frames: F_0 = base, A_j = F_{j-1} X_j, F_j = A_j M_j(theta_j) with M the rotation about the
joint's axis u_j (Rodrigues) or the translation theta_j u_j.  Sphere s sits on link l_s at the local centre o_s: q_s = F_{l_s} o_s,
clearance d = sdf(q_s) - r_s; a sphere on link 0 never moves.  F_obs = sum_t sum_s c(d) sigma with sigma the speed of the BODY
POINT, |q_{t+1,s} - q_{t-1,s}| / 2 (CHOMP's own form), F_smooth = (T-1)/2 sum_t |theta_{t+1} - theta_t|^2.  The step is
-(1/eta) K^-1 grad, projected onto the joint limits and scaled so that no joint value moves further than max_step (the infinity
norm: radians and metres are not mixed into a 2-norm).  States as in planning.  No branches, no closed loops, no self-collision,
no per-joint weights.  Module-level functions and one small class: nothing is added to HotPath or HipState.
"""
import numpy as np
import torch

from . import _ffi
from .planning import (CONVERGED, INVALID, MOVING, REC, PlanResult, TrajStep, _REASON, _engine, _scratch,  # noqa: F401
                       best_trajectory, default_field, descend, one_step, unpack_records)

REVOLUTE, PRISMATIC = 0, 1
# planning.DEFAULTS but for eta: at planning's eta = 8 a float64 host prototype of this loop fell into a period-2 oscillation across
# the medial surface between the floor and an obstacle (the step length constant at 0.0886 for 1 200 iterations, in a state that was
# already free of collision); at 32 every scenario it was tried on converged.
DEFAULTS = dict(eps=0.2, w_obs=8.0, w_smooth=1.0, eta=32.0, max_step=0.05, tol=1e-5)


def _pose(m, what):
    m = np.asarray(m, np.float64)
    if m.shape == (4, 4):
        m = m[:3]
    if m.shape != (3, 4):
        raise ValueError("%s must be a 3x4 (or 4x4) rigid transform (got %s)" % (what, m.shape))
    return m


class Chain:
    """A serial kinematic chain with collision spheres.

    base [3,4] (or [4,4]): the world pose of link 0.  X [J,3,4]: joint j's fixed transform from the previous link's frame (a
    fixed joint is folded into the next X by the caller: X = X_fixed @ X_next).  kinds [J]: 0 revolute, 1 prismatic.  axes [J,3]:
    the joint's unit axis in its own frame.  links [S] in [0, J], centres [S,3], radii [S] (or a scalar): the spheres.  lo, hi
    [J] (None: no limits; +-inf: none for that joint).  Everything is kept as contiguous float32 / int32 host arrays, the
    form the device call reads; ValueError for what isdf_arm_step would refuse."""

    def __init__(self, base, X, kinds, axes, links, centres, radii, lo=None, hi=None):
        self.base = np.ascontiguousarray(_pose(base, "base"), np.float32)
        X = np.asarray(X, np.float64)
        if X.ndim != 3 or X.shape[1:] not in ((3, 4), (4, 4)):
            raise ValueError("X must be [J, 3, 4] (got %s)" % (X.shape,))
        self.X = np.ascontiguousarray(X[:, :3], np.float32)
        J = self.J = int(X.shape[0])
        if not 1 <= J <= _ffi.ARM_MAX_JOINTS:
            raise ValueError("%d joints: a chain has 1 .. %d" % (J, _ffi.ARM_MAX_JOINTS))
        self.kinds = np.ascontiguousarray(np.asarray(kinds).reshape(-1), np.int32)
        self.axes = np.ascontiguousarray(np.asarray(axes, np.float64).reshape(-1, 3), np.float32)
        if self.kinds.size != J or self.axes.shape[0] != J:
            raise ValueError("%d joints but %d kinds and %d axes" % (J, self.kinds.size, self.axes.shape[0]))
        if not np.isin(self.kinds, (REVOLUTE, PRISMATIC)).all():
            raise ValueError("kinds are 0 (revolute) or 1 (prismatic)")
        u = self.axes
        n2 = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
        if not (np.abs(n2 - np.float32(1)) <= np.float32(1e-5)).all():
            raise ValueError("axes must be unit vectors (|u|^2 = %s)" % n2)
        self.links = np.ascontiguousarray(np.asarray(links).reshape(-1), np.int32)
        S = self.S = int(self.links.size)
        if not 1 <= S <= _ffi.ARM_MAX_SPHERES:
            raise ValueError("%d spheres: a chain has 1 .. %d" % (S, _ffi.ARM_MAX_SPHERES))
        self.centres = np.ascontiguousarray(np.asarray(centres, np.float64).reshape(-1, 3), np.float32)
        rad = np.asarray(radii, np.float32).reshape(-1)
        self.radii = np.ascontiguousarray(np.broadcast_to(rad, (S,)) if rad.size == 1 else rad)
        if self.centres.shape[0] != S or self.radii.size != S:
            raise ValueError("%d links but %d centres and %d radii" % (S, self.centres.shape[0], self.radii.size))
        if (self.links < 0).any() or (self.links > J).any():
            raise ValueError("links must lie in [0, %d]" % J)
        if not (np.isfinite(self.base).all() and np.isfinite(self.X).all() and np.isfinite(self.centres).all()):
            raise ValueError("base, X and centres must be finite")
        if not (np.isfinite(self.radii).all() and (self.radii >= 0).all()):
            raise ValueError("radii must be finite and not negative")
        self.lo = self.hi = None
        if lo is not None or hi is not None:
            self.lo = np.ascontiguousarray(np.broadcast_to(np.asarray(-np.inf if lo is None else lo, np.float32).reshape(-1), (J,)))
            self.hi = np.ascontiguousarray(np.broadcast_to(np.asarray(np.inf if hi is None else hi, np.float32).reshape(-1), (J,)))
            if not (self.lo <= self.hi).all():
                raise ValueError("limits need lo <= hi, neither NaN")

    @classmethod
    def free_body(cls, centres, radii, lo=None, hi=None):
        """a free-flying rigid body: theta = (x, y, z, then rotations about the body's y, x and z axes in that order), every
        sphere on link 6; at theta = 0 the body frame is the world frame"""
        eye = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (6, 1, 1))
        axes = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, 1]]
        c = np.asarray(centres, np.float64).reshape(-1, 3)
        return cls(eye[0], eye, [1, 1, 1, 0, 0, 0], axes, np.full(len(c), 6), c, radii, lo, hi)

    @classmethod
    def planar_base(cls, centres, radii, base=None, lo=None, hi=None):
        """a mobile base in the plane: theta = (x, y along the base frame's x and y axes, yaw about its z axis), every sphere on
        link 3; `base` (default: the identity) places and orients the plane in the world"""
        eye = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (3, 1, 1))
        c = np.asarray(centres, np.float64).reshape(-1, 3)
        return cls(eye[0] if base is None else base, eye, [1, 1, 0], [[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.full(len(c), 3), c, radii, lo, hi)

    def forward(self, theta, frames=False):
        """float64 numpy forward kinematics of theta [..., J]: the spheres' world centres q [..., S, 3]; with frames=True also
        the link frames F [..., J + 1, 3, 4] (F[..., 0] is the base).  The chain's float32 entries widened; plain matrix
        products (the device's order of operations is the header's; the two agree to a few ulp of double)."""
        th = np.asarray(theta, np.float64)
        if th.shape[-1] != self.J:
            raise ValueError("theta must be [..., %d] (got %s)" % (self.J, th.shape))
        lead = th.shape[:-1]
        R = np.broadcast_to(self.base[:, :3].astype(np.float64), lead + (3, 3))
        t = np.broadcast_to(self.base[:, 3].astype(np.float64), lead + (3,))
        F = [np.concatenate([R, t[..., None]], -1)]
        for j in range(self.J):
            X = self.X[j].astype(np.float64)
            u = self.axes[j].astype(np.float64)
            A = R @ X[:, :3]
            p = R @ X[:, 3] + t
            a = A @ u
            if self.kinds[j] == REVOLUTE:
                s, c = np.sin(th[..., j])[..., None, None], np.cos(th[..., j])[..., None, None]
                K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
                R, t = A @ (c * np.eye(3) + s * K + (1.0 - c) * np.outer(u, u)), p
            else:
                R, t = A, p + th[..., j, None] * a
            F.append(np.concatenate([R, t[..., None]], -1))
        F = np.stack(F, -3)
        Fs = F[..., self.links, :, :]                                   # [..., S, 3, 4]
        q = (Fs[..., :3] @ self.centres.astype(np.float64)[:, :, None])[..., 0] + Fs[..., 3]
        return (q, F) if frames else q


def _setup(obj, chain, theta, field):
    """(engine, a float32 device COPY of theta [B,T,J], field)"""
    eng = _engine(obj)
    theta = torch.as_tensor(theta)
    if theta.dim() == 2:
        theta = theta[None]
    if theta.dim() != 3 or theta.shape[-1] != chain.J:
        raise ValueError("trajectories must be [B, T, %d] or [T, %d] (got %s)" % (chain.J, chain.J, tuple(theta.shape)))
    theta = theta.detach().to(device=eng.device, dtype=torch.float32).contiguous().clone()
    return eng, theta, default_field(eng) if field is None else field


def joint_step(engine, chain, theta, eps=0.2, w_obs=8.0, w_smooth=1.0, eta=32.0, max_step=0.05, tol=1e-5, field=None,
               want_grad=False):
    """TrajStep of ONE linearisation of the joint-space trajectories theta [B,T,J] (or [T,J]), every one taken as moving; theta
    itself is not touched (the step is applied to a copy).  field: callable, device points [N,3] -> (sdf [N], grad [N,3]) on the
    device; default `engine.sdf_eval(pts, want_grad=True)`.  TrajStep.length is the joint-space path length, .step the largest
    joint move before the clamp; records[:, 11] counts the entries of the step a limit cut.  With want_grad also the gradient
    of w_obs F_obs + w_smooth F_smooth, float64 numpy [B,T,J]."""
    eng, th, field = _setup(engine, chain, theta, field)
    return one_step(th, lambda: eng.arm_points(th, chain), lambda state, q, sdf, grad, **kw: eng.arm_step(th, state, chain, q, sdf, grad, **kw),
                    field, want_grad, eps=eps, w_obs=w_obs, w_smooth=w_smooth, eta=eta, max_step=max_step, tol=tol)


def optimise_joint_trajectories(engine_or_sdf_map_or_trainer, chain, theta0, eps=0.2, w_obs=8.0, w_smooth=1.0, eta=32.0,
                                max_step=0.05, tol=1e-5, iters=400, check_every=10, field=None):
    """PlanResult (x: theta [B,T,J] float32 on the device): the trajectories theta0 [B,T,J] (or [T,J]; copied) after at most
    `iters` iterations of `Engine.arm_step`.

    As `planning.optimise_trajectories`: the query points are computed once; then every iteration is `field(q)` and one step
    launch that also rewrites q in place for the next one.  Nothing is read back inside the loop: every `check_every`
    iterations, and at the end, the B x 16 doubles of the last launch are copied once through a pinned buffer, and the loop is
    left when no trajectory is moving any more.  The result does not depend on `check_every`."""
    eng, th, field = _setup(engine_or_sdf_map_or_trainer, chain, theta0, field)
    return descend(th, lambda: eng.arm_points(th, chain), lambda state, q, sdf, grad, **kw: eng.arm_step(th, state, chain, q, sdf, grad, **kw),
                   field, iters, check_every, eps=eps, w_obs=w_obs, w_smooth=w_smooth, eta=eta, max_step=max_step, tol=tol)


def seed_joint_trajectories(start, goal, T, n_seeds, spread=0.5, seed=0, lo=None, hi=None):
    """theta [n_seeds, T, J] float32 numpy: seed 0 is the straight line start -> goal in joint space at T evenly spaced rows; seed
    k is the line plus a_k sin(pi s) u_k (s in [0, 1] along the line) with u_k a unit vector of joint space perpendicular to
    goal - start and a_k uniform in (-spread, spread), all drawn from numpy.random.RandomState(seed); with limits, clipped to
    [lo, hi].  Every seed starts at `start` and ends at `goal` exactly."""
    start, goal = np.asarray(start, np.float64).reshape(-1), np.asarray(goal, np.float64).reshape(-1)
    if start.size != goal.size:
        raise ValueError("start has %d joints, goal %d" % (start.size, goal.size))
    T, n_seeds, J = int(T), int(n_seeds), start.size
    s = np.linspace(0.0, 1.0, T)
    line = start[None] + s[:, None] * (goal - start)[None]
    th = np.repeat(line[None], n_seeds, 0)
    rng = np.random.RandomState(seed)
    axis = goal - start
    norm = np.linalg.norm(axis)
    axis = axis / norm if norm > 0 else np.zeros(J)
    bulge = np.sin(np.pi * s)
    for k in range(1, n_seeds):
        u = rng.standard_normal(J)
        u = u - (u @ axis) * axis
        nu = np.linalg.norm(u)
        a = rng.uniform(-spread, spread)
        if nu > 0:                        # J = 1 with distinct ends: nothing is perpendicular, the seed stays the line
            th[k] += a * bulge[:, None] * (u / nu)[None]
    if lo is not None or hi is not None:
        th = np.clip(th, -np.inf if lo is None else np.asarray(lo, np.float64), np.inf if hi is None else np.asarray(hi, np.float64))
    th = th.astype(np.float32)
    th[:, 0], th[:, -1] = start.astype(np.float32), goal.astype(np.float32)
    return th


def plan_joint_path(obj, chain, start, goal, T=64, n_seeds=32, clearance=0.0, spread=0.5, seed=0, **kw):
    """(PlanResult, best): `seed_joint_trajectories(start, goal, T, n_seeds, spread, seed, chain.lo, chain.hi)` optimised as one
    batch (**kw goes to `optimise_joint_trajectories`); best is the index of the trajectory with the lowest w_obs cost_obs +
    w_smooth cost_smooth among those whose state is not invalid, that have no sample in collision and whose least clearance is at
    least `clearance`; None if there is none."""
    res = optimise_joint_trajectories(obj, chain, seed_joint_trajectories(start, goal, T, n_seeds, spread, seed, chain.lo, chain.hi), **kw)
    return res, best_trajectory(res, clearance, kw, DEFAULTS)
