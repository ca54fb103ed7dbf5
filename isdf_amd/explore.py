"""Where to look next (include/isdf_hip.h: isdf_frontier_init, isdf_frontier_relax, isdf_frontier_clusters, isdf_view_gain;
DESIGN 28).

The map is incomplete, so where should the camera go?  `fusion.TsdfVolume` knows which voxels no frame measured,
`metrics.visible_points` knows the same for the neural map, `routing.distance_field` gives the travel cost to every free voxel.
This module adds the boundary between known-free and unknown space, its grouping into frontiers, and an occlusion-aware count of
the unknown voxels a candidate pose would see.  The reference has no counterpart.

    Grid                an axis-aligned grid: dims, spacing, origin (a fusion.TsdfVolume is accepted wherever one is expected)
    volume_states       the uint8 state volume of a TsdfVolume: UNKNOWN where nothing was measured, OCCUPIED at tsdf <= level
    map_states          the same for the net: known where metrics.visible_points sees the voxel, occupied at sdf <= clearance
    frontiers           frontier voxels labelled by the least linear index of their 26-connected component (Frontiers):
                        relaxation rounds in groups, ONE copy of `check_every` ints per group (routing.distance_field's loop)
    clusters            one record per component, sorted by root: size, centroid, bounding box -- one read-back
    view_gain           per pose: unknown voxels per ray, the depth image of the voxel map, distinct unknown voxels per view
    look_at             a camera-to-world pose in the reference's camera frame (z forward, x right, y down)
    candidate_views     poses on a ring around every cluster's centroid whose eye lies in a FREE voxel (host)
    next_best_view      frontiers -> clusters -> candidates -> view_gain -> ONE routing.distance_field -> the best pose and the
                        route to it

Labels, records and counts are integers and the walk of a ray is a stated fp32 sequence: every result equals
tests/explore_model.py bit for bit and does not depend on the run, on `check_every` or on how the views are chunked.  Grids are
axis-aligned (a rotated one raises ValueError); rays walk voxels, never the neural field.  Module-level functions only: nothing is
added to HotPath or HipState, and nothing is written to a trainer.
"""
import collections
import math

import numpy as np
import torch

from . import _ffi, mesh, routing
from .engine import host_array, to_host

UNKNOWN, FREE, OCCUPIED = _ffi.VOXEL_UNKNOWN, _ffi.VOXEL_FREE, _ffi.VOXEL_OCCUPIED
NONE = _ffi.FRONTIER_NONE

Grid = collections.namedtuple("Grid", "dims spacing origin")
Grid.__doc__ = """dims: (nx, ny, nz); spacing, origin: three floats each -- voxel (i, j, k) is centred at origin + (i, j, k) * spacing."""

Frontiers = collections.namedtuple("Frontiers", "label rounds converged")
Frontiers.__doc__ = """label: int32 [nx,ny,nz] on the device, per frontier voxel the least linear index (i * ny + j) * nz + k of its
26-connected component, _ffi.FRONTIER_NONE elsewhere; rounds: relaxation rounds up to and including the first that changed nothing
(all that were issued when not converged); converged: whether such a round was seen."""

Clusters = collections.namedtuple("Clusters", "root size centroid lo hi")
Clusters.__doc__ = """numpy arrays sorted by root: root int64 [m] (the component's least linear index), size int64 [m], centroid
float64 [m,3] (index coordinates: the integer sums / size), lo, hi int64 [m,3] (the bounding box, inclusive)."""

ViewGain = collections.namedtuple("ViewGain", "unknown depth distinct")
ViewGain.__doc__ = """unknown int32 [B,H,W], depth float32 [B,H,W], distinct int32 [B] or None, on the device (Engine.view_gain)."""

Candidates = collections.namedtuple("Candidates", "T_WC cluster voxel")
Candidates.__doc__ = """T_WC float64 [m,4,4] camera-to-world; cluster int64 [m], the row of `clusters` each pose looks at; voxel int64
[m,3], the voxel of each eye."""

NbvTable = collections.namedtuple("NbvTable", "T_WC cluster voxel distinct cost utility")
NbvTable.__doc__ = """one row per REACHABLE candidate, in candidate order: the pose, its cluster, the eye's voxel, the distinct unknown
voxels it sees (int64), the travel cost in metres (float64) and utility = distinct * exp(-lam * cost)."""

NextBestView = collections.namedtuple("NextBestView", "T_WC gain cost route table")
NextBestView.__doc__ = """T_WC float64 [4,4], gain (distinct unknown voxels), cost (metres), route (float64 [L,3] world polyline from the
robot to the eye) of the candidate of highest utility, and the whole NbvTable; the first four are None when there is no frontier
or no reachable candidate (table is None when there was no candidate at all)."""

_engine = routing._engine


def _grid(grid):
    """the checked Grid of a Grid or of anything with dims / spacing / origin (fusion.TsdfVolume)"""
    if hasattr(grid, "dims") and hasattr(grid, "spacing") and hasattr(grid, "origin"):
        dims, spacing, origin = grid.dims, grid.spacing, grid.origin
    else:
        raise ValueError("a Grid(dims, spacing, origin) or a fusion.TsdfVolume is needed (got %r)" % (type(grid).__name__,))
    dims = tuple(int(d) for d in np.broadcast_to(np.asarray(dims).reshape(-1), (3,)))
    spacing = np.asarray(spacing, np.float64)
    if spacing.ndim == 2:
        raise ValueError("rotated (non-axis-aligned) grids are not supported: spacing must be one number or three")
    spacing = tuple(float(x) for x in np.broadcast_to(spacing.reshape(-1), (3,)))
    origin = tuple(float(x) for x in np.asarray(origin, np.float64).reshape(3))
    if not all(np.isfinite(x) and x > 0 for x in spacing) or not all(np.isfinite(x) for x in origin) or min(dims) < 1:
        raise ValueError("grid: sides >= 1, spacing positive and finite, origin finite (got %s, %s, %s)" % (dims, spacing, origin))
    return Grid(dims, spacing, origin)


def grid_from_affine(dims, index_to_world):
    """Grid of a [3,4] (or [4,4]) index-to-world affine; ValueError if it rotates or shears (rotated grids are out of scope)"""
    A = host_array(index_to_world, np.float64).reshape(-1, 4)[:3]
    if np.any(A[:, :3] != np.diag(np.diag(A[:, :3]))):
        raise ValueError("rotated (non-axis-aligned) grids are not supported (index_to_world = %s)" % (A.tolist(),))
    return _grid(Grid(mesh._dims3(dims), tuple(np.diag(A[:, :3])), tuple(A[:, 3])))


def index_to_world(grid):
    """[3,4] float64 affine of the grid (voxel index -> its centre), what routing.snap and mesh.grid_points take"""
    g = _grid(grid)
    A = np.zeros((3, 4))
    A[:, :3], A[:, 3] = np.diag(g.spacing), g.origin
    return A


def to_world(grid, index_points):
    """float64 [..., 3]: origin + index_points * spacing"""
    g = _grid(grid)
    return np.asarray(g.origin) + np.asarray(index_points, np.float64) * np.asarray(g.spacing)


def volume_states(vol, level=0.0):
    """uint8 [nx,ny,nz] on vol's device: UNKNOWN where weight == 0, else OCCUPIED where tsdf <= level, else FREE (torch ops)."""
    known = torch.where(vol.tsdf <= float(level), torch.full_like(vol.tsdf, OCCUPIED, dtype=torch.uint8),
                        torch.full_like(vol.tsdf, FREE, dtype=torch.uint8))
    return torch.where(vol.weight == 0, torch.full_like(known, UNKNOWN), known).contiguous()


def map_states(obj, grid, T_WC, depth, cam, trunc=0.2, clearance=0.0):
    """uint8 [nx,ny,nz] on the device for the neural map (obj: an Engine or anything with one as `.engine`): a voxel is known iff
    `metrics.visible_points` counts at least one of the posed depth frames (T_WC [F,4,4], depth [F,H,W]) seeing its centre, and a
    known voxel is OCCUPIED iff `sdf_eval` <= clearance there."""
    from . import metrics
    eng, g = _engine(obj), _grid(grid)
    pts = mesh.grid_points(g.dims, index_to_world(g).astype(np.float32), eng.device)
    count = metrics.visible_points(eng, pts, T_WC, depth, cam, trunc=trunc)[0].reshape(g.dims)
    with torch.no_grad():
        sdf = eng.sdf_eval(pts).reshape(g.dims)
    known = torch.where(sdf <= float(clearance), torch.full_like(count, OCCUPIED, dtype=torch.uint8),
                        torch.full_like(count, FREE, dtype=torch.uint8))
    return torch.where(count > 0, known, torch.full_like(known, UNKNOWN)).contiguous()


def _state(eng, state):
    s = torch.as_tensor(state)
    if s.dim() != 3 or s.dtype != torch.uint8:
        raise ValueError("state must be a uint8 [nx, ny, nz] volume (got %s %s)" % (s.dtype, tuple(s.shape)))
    return s.to(device=eng.device).contiguous()


def frontiers(engine, state, check_every=8, max_rounds=None):
    """Frontiers of the state volume (uint8 [nx,ny,nz]: UNKNOWN / FREE / >= OCCUPIED).  `Engine.frontier_relax` is issued in groups
    of `check_every` rounds; after each group its `changed` flags are copied once through a pinned buffer, and the loop is left
    at the first group whose last round changed nothing.  Neither label nor `rounds` depends on `check_every`.  max_rounds: None =
    the number of voxels; labels cut short there have converged = False."""
    eng = _engine(engine)
    s = _state(eng, state)
    label = eng.frontier_init(s)
    check_every = max(1, int(check_every))
    limit = s.numel() if max_rounds is None else int(max_rounds)
    scratch = routing._scratch(eng.device)
    done = 0
    while done < limit:
        n = min(check_every, limit - done)
        flags = scratch.fetch(eng.frontier_relax(label, n, changed=scratch.reserve(n)))
        if flags[n - 1] == 0:
            return Frontiers(label, done + int(np.argmin(flags != 0)) + 1, True)
        done += n
    return Frontiers(label, done, False)


_CAPACITY = {}      # device -> the record rows the last call on it needed (a grow-only guess, as mesh.Mesher keeps one)


def clusters(engine, fr, min_size=1):
    """Clusters of `fr` (a Frontiers, or its label volume) with at least `min_size` voxels.  One launch group at the cached
    capacity and ONE read-back of counts and records; one re-launch only when there are more clusters than that capacity.
    RuntimeError if any frontier voxel's label is not a root (labels that were not relaxed to convergence)."""
    eng = _engine(engine)
    label = fr.label if isinstance(fr, Frontiers) else fr
    key = str(eng.device)
    cap = _CAPACITY.get(key, 1024)
    counts, records = to_host(*eng.frontier_clusters(label, cap))
    m = int(counts[0])
    if m > cap:
        cap = _CAPACITY[key] = m + m // 4
        counts, records = to_host(*eng.frontier_clusters(label, cap))
    if int(counts[2]) != 0:
        raise RuntimeError("clusters: %d of %d frontier voxels carry a label that is not a root: the labels are not converged"
                           % (int(counts[2]), int(counts[1])))
    r = records[:m].astype(np.int64)
    r = r[r[:, 1] >= int(min_size)]
    return Clusters(r[:, 0].copy(), r[:, 1].copy(), r[:, 2:5] / r[:, 1:2].astype(np.float64), r[:, 5:8].copy(), r[:, 8:11].copy())


def view_gain(engine, state, grid, T_WC, cam, H, W, t_min=0.0, t_max=float("inf"), distinct=True, ws_budget=256 << 20):
    """ViewGain of the camera-to-world poses T_WC [B,4,4] over `state` on `grid`: Engine.view_gain in chunks of views whose bitmaps
    (one bit per voxel and view, only with `distinct`) stay within `ws_budget` bytes; at least one view per chunk.  The result
    does not depend on the chunking.  cam: anything with fx, fy, cx, cy."""
    eng, g = _engine(engine), _grid(grid)
    s = _state(eng, state)
    if tuple(s.shape) != g.dims:
        raise ValueError("view_gain: state is %s, the grid %s" % (tuple(s.shape), g.dims))
    T = (T_WC if torch.is_tensor(T_WC) else torch.as_tensor(np.asarray(T_WC, np.float32))).to(torch.float32).reshape(-1, 4, 4)
    B = int(T.shape[0])
    per_view = 4 * ((s.numel() + 31) // 32)
    chunk = max(1, int(ws_budget) // per_view) if distinct else max(B, 1)
    parts = [eng.view_gain(s, g.origin, g.spacing, T[a:a + chunk], cam, H, W, t_min, t_max, distinct)
             for a in range(0, B, chunk)] or [eng.view_gain(s, g.origin, g.spacing, T, cam, H, W, t_min, t_max, distinct)]
    if len(parts) == 1:
        return ViewGain(*parts[0])
    return ViewGain(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]),
                    torch.cat([p[2] for p in parts]) if distinct else None)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """float64 [4,4] camera-to-world pose in the reference's camera frame (x right, y down, z forward): z = normalise(target - eye),
    x = normalise(z cross up), y = z cross x, translation eye.  ValueError when target == eye or the view is parallel to up."""
    eye, target, up = (np.asarray(v, np.float64).reshape(3) for v in (eye, target, up))
    z = target - eye
    nz = np.linalg.norm(z)
    x = np.cross(z, up)
    nx = np.linalg.norm(x)
    if not nz > 0 or not nx > 1e-12 * nz * max(np.linalg.norm(up), 1e-300):
        raise ValueError("look_at: target equals eye, or the view direction is parallel to up")
    z, x = z / nz, x / nx
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T


def _ring_basis(up):
    """two unit vectors spanning the plane perpendicular to `up`: deterministic, from the axis `up` is least aligned with"""
    up = np.asarray(up, np.float64).reshape(3)
    n = up / np.linalg.norm(up)
    e = np.zeros(3)
    e[int(np.argmin(np.abs(n)))] = 1.0
    u = np.cross(n, e)
    u /= np.linalg.norm(u)
    return u, np.cross(n, u)


def voxel_of(grid, points):
    """int64 [n,3]: the voxel whose cell [a - 0.5, a + 0.5) holds each world point (it may lie outside the grid)"""
    g = _grid(grid)
    p = np.asarray(points, np.float64).reshape(-1, 3)
    return np.floor((p - np.asarray(g.origin)) / np.asarray(g.spacing) + 0.5).astype(np.int64)


def candidate_views(state, grid, clusters, n_per_cluster=8, radius=1.0, seed=0, up=(0.0, 0.0, 1.0)):
    """Candidates for the clusters (a Clusters), on the host: per cluster, in order, `n_per_cluster` angles uniform in [0, 2 pi) from
    numpy.random.RandomState(seed); eye = the centroid's world position + radius * (cos a * u + sin a * v), (u, v) spanning the
    plane perpendicular to `up`; an eye is kept iff its voxel is inside the grid and FREE; every kept eye looks at the centroid
    (`look_at` with `up`)."""
    g = _grid(grid)
    s = host_array(state)
    if s.shape != g.dims:
        raise ValueError("candidate_views: state is %s, the grid %s" % (s.shape, g.dims))
    u, v = _ring_basis(up)
    rng = np.random.RandomState(seed)
    poses, which, voxels = [], [], []
    for c, centroid in enumerate(to_world(g, clusters.centroid)):
        for a in rng.uniform(0.0, 2.0 * math.pi, int(n_per_cluster)):
            eye = centroid + float(radius) * (math.cos(a) * u + math.sin(a) * v)
            vox = voxel_of(g, eye)[0]
            if (vox >= 0).all() and (vox < g.dims).all() and s[tuple(vox)] == FREE:
                poses.append(look_at(eye, centroid, up))
                which.append(c)
                voxels.append(vox)
    return Candidates(np.array(poses, np.float64).reshape(-1, 4, 4), np.array(which, np.int64), np.array(voxels, np.int64).reshape(-1, 3))


def next_best_view(engine, state, grid, position, cam, H, W, free=None, lam=0.25, min_size=1, n_per_cluster=8, radius=1.0, seed=0,
                   up=(0.0, 0.0, 1.0), t_min=0.0, t_max=float("inf"), check_every=8, ws_budget=256 << 20):
    """NextBestView for a robot at the world point `position`: frontiers -> clusters (of at least `min_size` voxels) ->
    candidate_views -> view_gain -> ONE routing.distance_field over `free` (uint8 mask, default state == FREE) whose goal is the
    robot's voxel.  cost = dist[eye voxel] / 3 * voxel metres (cubic voxels only: ValueError otherwise); candidates whose eye is
    unreachable are dropped; utility = distinct * exp(-lam * cost); the first candidate of highest utility wins.  The route is
    routing.trace from the eye's voxel down the field, reversed: the robot's position, the voxel centres, the eye.  Nothing is
    written to a trainer."""
    eng, g = _engine(engine), _grid(grid)
    if not (abs(g.spacing[0] - g.spacing[1]) <= 1e-9 * g.spacing[0] and abs(g.spacing[0] - g.spacing[2]) <= 1e-9 * g.spacing[0]):
        raise ValueError("next_best_view: cubic voxels are needed for the travel cost (got %s)" % (g.spacing,))
    s = _state(eng, state)
    none = NextBestView(None, None, None, None, None)
    cl = clusters(eng, frontiers(eng, s, check_every=check_every), min_size=min_size)
    if len(cl.root) == 0:
        return none
    cand = candidate_views(s, g, cl, n_per_cluster, radius, seed, up)
    if len(cand.cluster) == 0:
        return none
    gain = view_gain(eng, s, g, cand.T_WC, cam, H, W, t_min, t_max, True, ws_budget)
    free = (s == FREE).to(torch.uint8) if free is None else free
    field = routing.distance_field(eng, free, voxel_of(g, position), check_every=check_every)
    lin = (cand.voxel[:, 0] * g.dims[1] + cand.voxel[:, 1]) * g.dims[2] + cand.voxel[:, 2]
    at = field.dist.reshape(-1)[torch.as_tensor(lin, device=field.dist.device)]
    distinct, at = (a.astype(np.int64) for a in to_host(gain.distinct, at))
    keep = at < routing.NONE
    cost = at[keep] / 3.0 * g.spacing[0]
    utility = distinct[keep] * np.exp(-float(lam) * cost)
    table = NbvTable(cand.T_WC[keep], cand.cluster[keep], cand.voxel[keep], distinct[keep], cost, utility)
    if not keep.any():
        return none._replace(table=table)
    best = int(np.argmax(utility))
    path = routing.trace(eng, field, table.voxel[best:best + 1])[0][::-1]
    route = np.concatenate([np.asarray(position, np.float64).reshape(1, 3), to_world(g, path), table.T_WC[best, :3, 3][None]])
    return NextBestView(table.T_WC[best], int(table.distinct[best]), float(cost[best]), route, table)
