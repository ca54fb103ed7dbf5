"""Routing through the map on the device (include/isdf_hip.h: isdf_route_init, isdf_route_relax, isdf_route_trace).

`isdf_amd.planning` deforms a seed trajectory and cannot change which side of an obstacle the seed passes: with start and goal on
opposite sides of a wall, every bulge of the straight line stays in collision.  This is the global half -- a shortest route over
the free voxels of a grid, which then seeds the local optimiser.  The reference has no counterpart.

    free_space          a field on a grid -> the uint8 mask of voxels a robot of a given radius may occupy
    map_free_space      the same from the net, evaluated on mesh.grid_points
    volume_free_space   the same from the voxel baseline (fusion.TsdfVolume); unobserved voxels are blocked by default
    distance_field      the geodesic distance to the goals on the mask (RouteField): relaxation rounds in groups, ONE copy of
                        `check_every` ints per group, stops at the first group whose last round changed nothing
    trace               voxel paths from starts down a converged field
    route / routes      world-frame polylines from start(s) to a goal
    resample            T points evenly spaced along a polyline
    plan_route          route -> seeds -> planning.optimise_trajectories as one batch -> the best trajectory free of collision

The graph: voxels 26-connected with integer chamfer weights 3 / 4 / 5 for face / edge / corner moves, a move exists iff both
voxels are free.  All int32, so a converged field IS the shortest-path distance: it does not depend on the tile, on how often
the host looked, or on the run.  A route is a staircase of voxel centres; the optimiser smooths it.  No rotation, no any-angle
shortening.  Module-level functions only: nothing is added to HotPath or HipState.
"""
import collections
import math

import numpy as np
import torch

from . import _ffi, mesh, planning
from .engine import host_array

NONE = _ffi.ROUTE_NONE

RouteField = collections.namedtuple("RouteField", "dist rounds converged")
RouteField.__doc__ = """dist: int32 [nx,ny,nz] on the device, chamfer cost to the nearest goal (3 per face move), _ffi.ROUTE_NONE
where blocked or unreachable; rounds: relaxation rounds up to and including the first that changed nothing (all that were
issued when not converged); converged: whether such a round was seen."""


def _engine(obj):
    """an Engine, or anything that has one as `.engine` (SDFMapHIP, a grafted trainer)"""
    return getattr(obj, "engine", obj)


def margin(voxel):
    """(sqrt(3) / 2) * voxel: half the longest move of the graph, the corner move"""
    return 0.5 * math.sqrt(3.0) * float(voxel)


def free_space(values, clearance, voxel=None):
    """uint8 mask of `values > clearance` (a tensor of any shape, or array-like); NaN counts as blocked.

    The margin.  A signed distance field is 1-Lipschitz and the longest move between two voxels is the corner move, sqrt(3) *
    voxel, so every point of a move lies within (sqrt(3) / 2) * voxel of one of its two ends.  With both ends above
    radius + (sqrt(3) / 2) * voxel on an exact field, every point of every segment of a route is further than `radius` from the
    surface -- and so is the segment from a point to the centre of the voxel it snaps to.  With `voxel` given that term is
    added to `clearance` here (`margin(voxel)`); without it the threshold is `clearance` as passed."""
    v = torch.as_tensor(values)
    c = float(clearance) + (margin(voxel) if voxel is not None else 0.0)
    return (v > c).to(torch.uint8)


def map_free_space(obj, dims, index_to_world, clearance, voxel=None):
    """uint8 [D0,D1,D2] on the device: `free_space` of the net (obj: an Engine or anything with one as `.engine`) evaluated by
    `sdf_eval` on `mesh.grid_points(dims, index_to_world)`.  The net is not an exact field: `clearance` wants the map's own
    error on top of the robot's radius."""
    eng = _engine(obj)
    d = mesh._dims3(dims)
    with torch.no_grad():
        sdf = eng.sdf_eval(mesh.grid_points(d, index_to_world, eng.device))
    return free_space(sdf.reshape(d), clearance, voxel).contiguous()


def volume_free_space(engine, vol, clearance, voxel=None, unknown_free=False):
    """uint8 [nx,ny,nz] on the device: `free_space` of the voxel baseline's full-range field (`fusion.full_sdf(engine, vol)`, vol a
    fusion.TsdfVolume with cubic voxels).  Voxels no frame measured (weight == 0) are blocked unless `unknown_free`."""
    from . import fusion
    free = free_space(fusion.full_sdf(engine, vol), clearance, voxel)
    if not unknown_free:
        free = free * (vol.weight > 0).to(torch.uint8)
    return free.contiguous()


class _Scratch:
    """per-device round flags and the pinned host mirror they are copied through (as planning._Scratch)"""

    def __init__(self, device):
        self.device = device
        self.changed = None
        self.pinned = None

    def reserve(self, n):
        if self.changed is None or self.changed.numel() < n:
            self.changed = torch.empty(n, dtype=torch.int32, device=self.device)
            self.pinned = torch.empty(n, dtype=torch.int32, pin_memory=True) if self.device.type == "cuda" else None
        return self.changed[:n]

    def fetch(self, changed):
        """the flags on the host: ONE copy into the pinned buffer, then the stream's end (a host-side stand-in for an Engine, as
        the CPU tests use, has its flags on the host already)"""
        if self.pinned is None:
            return changed.numpy().copy()
        host = self.pinned[:changed.numel()]
        host.copy_(changed, non_blocking=True)
        torch.cuda.current_stream(changed.device).synchronize()
        return host.numpy().copy()


_SCRATCH = {}


def _scratch(device):
    device = torch.device(device)
    key = "cpu" if device.type != "cuda" else device.index if device.index is not None else torch.cuda.current_device()
    s = _SCRATCH.get(key)
    if s is None:
        s = _SCRATCH[key] = _Scratch(device)
    return s


def _mask(eng, free):
    f = torch.as_tensor(free)
    if f.dim() != 3:
        raise ValueError("free must be a [nx, ny, nz] mask (got %s)" % (tuple(f.shape),))
    f = f if f.dtype == torch.uint8 else (f != 0)
    return f.to(device=eng.device, dtype=torch.uint8).contiguous()


def distance_field(engine, free, goals, check_every=8, max_rounds=None):
    """RouteField of the mask `free` ([nx,ny,nz], non-zero = free) from `goals` (integer voxel coordinates [n,3]; those outside
    the grid or on a blocked voxel are ignored, none at all is allowed).

    `Engine.route_relax` is issued in groups of `check_every` rounds; after each group the group's `changed` flags are copied
    once through a pinned buffer, and the loop is left at the first group whose last round changed nothing.  Neither dist nor
    `rounds` depends on `check_every`: dist is a fixed point, and rounds counts up to the first round that changed nothing.
    max_rounds: None = the number of voxels (no path has more); a field cut short there has converged = False."""
    eng = _engine(engine)
    f = _mask(eng, free)
    dist = eng.route_init(f, goals)
    check_every = max(1, int(check_every))
    limit = f.numel() if max_rounds is None else int(max_rounds)
    scratch = _scratch(eng.device)
    done = 0
    while done < limit:
        n = min(check_every, limit - done)
        flags = scratch.fetch(eng.route_relax(f, dist, n, changed=scratch.reserve(n)))
        if flags[n - 1] == 0:
            return RouteField(dist, done + int(np.argmin(flags != 0)) + 1, True)
        done += n
    return RouteField(dist, done, False)


def _voxels(v):
    v = host_array(v)
    if v.dtype.kind not in "iu" or v.size % 3 != 0:
        raise ValueError("voxel coordinates must be integers [n, 3]")
    return v.reshape(-1, 3).astype(np.int64)


def trace(engine, field, starts):
    """A list with one int64 numpy [len, 3] voxel path per start (integer voxel coordinates [B,3]), from the start to a goal of
    `field` (a RouteField, or its dist); len = 0 for a start that is outside the grid, blocked or unreachable.  One small
    read-back of dist at the starts sizes the paths (a path of cost c has at most c / 3 + 1 voxels), one launch traces them
    all, one copy brings them back.  RuntimeError if the field is not converged at a voxel on the way."""
    eng = _engine(engine)
    dist = field.dist if isinstance(field, RouteField) else field
    s = _voxels(starts)
    B = s.shape[0]
    if B == 0:
        return []
    dims = np.array(dist.shape, np.int64)
    inside = ((s >= 0) & (s < dims)).all(1)
    lin = np.where(inside, (s[:, 0] * dims[1] + s[:, 1]) * dims[2] + s[:, 2], 0)
    at = dist.reshape(-1)[torch.as_tensor(lin, device=dist.device)].cpu().numpy().astype(np.int64)
    reach = inside & (at < NONE)
    max_len = int(at[reach].max()) // 3 + 1 if reach.any() else 1
    path, length = eng.route_trace(dist, torch.as_tensor(s.astype(np.int32)), max_len)
    path, length = path.cpu().numpy().astype(np.int64), length.cpu().numpy()
    if (length < 0).any():
        raise RuntimeError("route trace: the field is not converged along the path from start %s" % (s[int(np.argmin(length))],))
    out = []
    for b in range(B):
        p = path[b, :length[b]]
        out.append(np.stack([p // (dims[1] * dims[2]), (p // dims[2]) % dims[1], p % dims[2]], -1))
    return out


def _affine(index_to_world):
    A = host_array(index_to_world, np.float64).reshape(3, 4)
    return A[:, :3], A[:, 3]


def snap(index_to_world, points):
    """int64 [n, 3]: the voxel nearest to each world point (the inverse affine, halves rounded up; it may lie outside the grid)"""
    R, t = _affine(index_to_world)
    p = np.asarray(points, np.float64).reshape(-1, 3)
    # row by row with plain sums: a point snaps to the same voxel whichever other points share the call
    return np.floor(((p - t)[:, None, :] * np.linalg.inv(R)[None]).sum(-1) + 0.5).astype(np.int64)


def routes(engine, free, index_to_world, starts, goal, check_every=8):
    """One world-frame polyline (float64 numpy [L, 3]) per start in `starts` [B,3], all from ONE field built from `goal`: the true
    start, the centres of the route's voxels (`index_to_world`, a [3,4] affine, maps voxel (i, j, k) to its centre), the true
    goal.  None in place of a polyline whose start snaps to a voxel that is outside, blocked or cut off from the goal; all None
    when the goal itself is."""
    R, t = _affine(index_to_world)
    goal = np.asarray(goal, np.float64).reshape(3)
    starts = np.asarray(starts, np.float64).reshape(-1, 3)
    field = distance_field(engine, free, snap(index_to_world, goal), check_every=check_every)
    out = []
    for s, vox in zip(starts, trace(engine, field, snap(index_to_world, starts))):
        out.append(None if len(vox) == 0 else np.concatenate([s[None], vox.astype(np.float64) @ R.T + t, goal[None]]))
    return out


def route(engine, free, index_to_world, start, goal, check_every=8):
    """`routes` for one start: the polyline [L, 3], or None when the goal cannot be reached from it."""
    return routes(engine, free, index_to_world, np.asarray(start, np.float64).reshape(1, 3), goal, check_every)[0]


def resample(polyline, T):
    """float32 numpy [T, 3]: T points evenly spaced by arc length along `polyline` [L, 3], the first and last its end points
    exactly.  On the host: it is tiny.  A polyline of zero length gives T copies of its point."""
    p = np.asarray(polyline, np.float64).reshape(-1, 3)
    T = int(T)
    if p.shape[0] < 1 or T < 2:
        raise ValueError("resample: a polyline of at least one point and T >= 2 are needed")
    seg = np.linalg.norm(np.diff(p, axis=0), axis=1)
    keep = np.concatenate([[True], seg > 0])
    p, arc = p[keep], np.concatenate([[0.0], np.cumsum(seg[seg > 0])])
    s = np.linspace(0.0, arc[-1], T)
    x = np.stack([np.interp(s, arc, p[:, k]) for k in range(3)], -1).astype(np.float32)
    x[0], x[-1] = p[0].astype(np.float32), p[-1].astype(np.float32)
    return x


def seed_routes(polyline, T, n_seeds, spread=0.3, seed=0):
    """x [n_seeds, T, 3] float32 numpy: seed 0 is `resample(polyline, T)`; seed k is that plus a_k sin(pi s) u_k, s in [0, 1] by arc
    length, with the draws of `planning.seed_trajectories` -- u_k a unit vector perpendicular to goal - start, a_k uniform in
    (-spread, spread), from numpy.random.RandomState(seed) in the same order.  Every seed keeps the end points exactly."""
    base = resample(polyline, T)
    T, n_seeds = int(T), int(n_seeds)
    x = np.repeat(base.astype(np.float64)[None], n_seeds, 0)
    rng = np.random.RandomState(seed)
    axis = x[0, -1] - x[0, 0]
    norm = np.linalg.norm(axis)
    axis = axis / norm if norm > 0 else np.array([1.0, 0.0, 0.0])
    bulge = np.sin(np.pi * np.linspace(0.0, 1.0, T))
    for k in range(1, n_seeds):
        u = rng.standard_normal(3)
        u = u - (u @ axis) * axis
        u = u / np.linalg.norm(u)
        x[k] += rng.uniform(-spread, spread) * bulge[:, None] * u[None]
    x = x.astype(np.float32)
    x[:, 0], x[:, -1] = base[0], base[-1]
    return x


def hold_weight(length, w_smooth=planning.DEFAULTS["w_smooth"], eps=planning.DEFAULTS["eps"]):
    """The obstacle weight at which a trajectory of `length` metres stays on its side of an obstacle edge it is wrapped round:
    2 * w_smooth * length / eps, and never below planning's default.  F_smooth makes the trajectory an elastic band of tension
    w_smooth * length; round a U-turn both strands pull, 2 * w_smooth * length in all.  The obstacle term pushes back with at
    most w_obs per metre of path inside the eps band (the cost's slope is at most 1), and the arc wrapped round an edge is of
    the order of eps.  Below that weight the band is pulled THROUGH the wall: with planning's w_obs = 8 every seed of a 9.6 m
    route round a partition ended as the straight line through it."""
    return max(planning.DEFAULTS["w_obs"], 2.0 * float(w_smooth) * float(length) / float(eps))


def plan_route(obj, start, goal, free, index_to_world, T=64, n_seeds=8, clearance=0.0, spread=0.3, seed=0, **kw):
    """(PlanResult, best, polyline): the route from `start` to `goal` over the mask `free`, `seed_routes` of it optimised as one
    batch by `planning.optimise_trajectories` (**kw goes there: radii, offsets, field, iters, ...), and best chosen exactly as
    `planning.plan_path` chooses it -- the lowest w_obs cost_obs + w_smooth cost_smooth among the trajectories whose state is
    not invalid, that have no sample in collision and whose least clearance is at least `clearance`; None if there is none.
    (None, None, None) when there is no route.  `free` wants the robot's radius and `margin(voxel)` in its threshold
    (`free_space`); `spread` is smaller than plan_path's because the route already passes the obstacles on the right side.
    w_obs, unless the caller passes one, is `hold_weight` of the route's length: a long detour needs more than planning's
    default to stay where the route put it."""
    line = route(obj, free, index_to_world, start, goal)
    if line is None:
        return None, None, None
    if "w_obs" not in kw:
        length = float(np.linalg.norm(np.diff(line, axis=0), axis=1).sum())
        kw["w_obs"] = hold_weight(length, kw.get("w_smooth", planning.DEFAULTS["w_smooth"]), kw.get("eps", planning.DEFAULTS["eps"]))
    res = planning.optimise_trajectories(obj, seed_routes(line, T, n_seeds, spread, seed), **kw)
    r = res.records
    total = kw["w_obs"] * r.cost_obs + kw.get("w_smooth", planning.DEFAULTS["w_smooth"]) * r.cost_smooth
    ok = (res.state != planning.INVALID) & (r.in_collision == 0) & (r.min_clearance >= clearance) & np.isfinite(total)
    best = int(np.argmin(np.where(ok, total, np.inf))) if ok.any() else None
    return res, best, line
