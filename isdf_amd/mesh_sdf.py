"""Ground truth from a triangle mesh (include/isdf_hip.h: isdf_tri_pack, isdf_tri_distance).

Every evaluation path scores the map against a ground-truth SDF volume; the reference builds that volume offline from the scene
mesh with trimesh (voxelise, fill, two distance transforms: sdf_util.py:388-457), which carries a voxel of error and needs a
watertight mesh.  Here the exact version: per query point the distance to the nearest triangle and the generalised winding number
of the mesh, which gives the sign on open and non-manifold meshes as well.  Brute force over points x triangles on the device.

    PackedMesh                  a mesh gathered once into the layout the kernel reads
    surface_distance            unsigned distance to the surface (and the nearest face / point)
    mesh_sdf                    signed distance and winding number
    mesh_volume                 the signed distance on a grid, as a metrics.GtVolume: every consumer of a ground-truth volume
                                (sdf_metrics, region_metrics, the slices, fusion.baseline_metrics) then works from a mesh
    sample_surface              area-weighted points on a mesh (what trimesh.sample.sample_surface draws)
    mesh_accuracy_completion    accuracy / completion measured to the SURFACE instead of to a second point sample
    tile_order                  the default order of a mesh's tile index: large faces apart, the rest along a Morton curve
    PackedMesh.tiles / accel="tiles"   the same results from a flat tile index with conservative culling: distance,
                                index, nearest point and record bit for bit; the winding number with a far-field term per tile

Module-level functions and one small class: nothing is added to HotPath or HipState.  `engine` is an isdf_amd.engine.Engine (or
anything that has one as `.engine`).
"""
import numpy as np
import torch

from . import metrics
from . import _ffi
from .engine import host_array, morton_codes

CHUNK = 1 << 20      # query points per call of mesh_volume


def _engine(obj):
    """an Engine, or anything that has one as `.engine` (SDFMapHIP, a grafted trainer)"""
    return getattr(obj, "engine", obj)


def tile_order(packed, m, big_fraction=0.125):
    """int32 [(ceil(m / 256) + 1) * 256] on packed's device: the valid slots of a packed mesh of m faces in tile order, -1
    elsewhere.  Faces whose box diagonal exceeds `big_fraction` of the mesh's come first, padded with -1 to whole tiles so that
    they do not spoil the boxes of the others; each group in the Morton order of the face centroids (a stable sort).  Skipped
    faces are not listed.  torch ops, no host synchronisation."""
    m, T, dev = int(m), _ffi.TRI_TILE, packed.device
    order = torch.full(((-(-m // T) + 1) * T,), -1, dtype=torch.int32, device=dev)
    if m == 0:
        return order
    s = packed[:m]
    valid = s[:, 15] != 0
    tri = torch.stack([s[:, 0:3], s[:, 12:15], s[:, 16:19]], 1)                      # [m, 3 vertices, 3]
    lo, hi = tri.amin(1), tri.amax(1)
    inf = torch.tensor(float("inf"), device=dev)
    mesh_diag = torch.linalg.norm(torch.where(valid[:, None], hi, -inf).amax(0) - torch.where(valid[:, None], lo, inf).amin(0))
    big = valid & (torch.linalg.norm(hi - lo, dim=1) > float(big_fraction) * mesh_diag)
    code = morton_codes(torch.where(valid[:, None], tri.mean(1), inf))              # a skipped face: 2^30, behind the others
    rank = torch.sort(code + torch.where(big, 0, 1 << 31), stable=True)[1]           # big first, then the rest, then skipped
    n_big = big.sum()
    i = torch.arange(m, device=dev)
    pos = torch.where(i < n_big, i, i - n_big + (n_big + T - 1) // T * T)
    order[pos] = torch.where(valid[rank], rank, -1).to(torch.int32)
    return order


class PackedMesh:
    """vertices [nv,3] and faces [m,3] (arrays or tensors) packed for the device; transform: None or a [3,4] / [4,4] affine applied
    to the vertices first.  Faces with a non-finite vertex or zero fp32 area are skipped and counted (`n_invalid`,
    `n_degenerate`); a face index outside [0, nv) is an error in the caller's data: ValueError, naming how many.  Reading the
    counters synchronises with the device once, here."""

    def __init__(self, engine, vertices, faces, transform=None):
        eng = _engine(engine)
        self.engine, self.device = eng, eng.device
        self._tiles = None
        v = torch.as_tensor(vertices).detach().to(self.device).reshape(-1, 3)
        f = torch.as_tensor(faces).detach().to(self.device).reshape(-1, 3)
        nv = int(v.shape[0])
        n_bad = int(((f < 0) | (f >= nv)).any(1).sum()) if f.numel() else 0
        if n_bad:
            raise ValueError("PackedMesh: %d of %d faces have a vertex index outside [0, %d)" % (n_bad, f.shape[0], nv))
        self.packed, self.counts, self.n_faces = eng.tri_pack(v, f, transform)
        n_invalid, self.n_degenerate = (int(x) for x in self.counts.tolist())
        self.n_invalid = n_invalid                       # no bad index is left: these have a non-finite vertex
        # what sample_surface reads: the transformed vertices (torch's rounding, not the kernel's chain: sampling only)
        v = v.to(torch.float32)
        if transform is not None:
            A = torch.as_tensor(host_array(transform, np.float32)[:3],
                                device=self.device)
            v = v @ A[:, :3].T + A[:, 3]
        self.vertices, self.faces = v, f.to(torch.int64)

    @property
    def n_valid(self):
        return self.n_faces - self.n_invalid - self.n_degenerate

    def tiles(self, big_fraction=0.125, order=None):
        """(tiles f64 [n_tiles, 16], order_clean i32 [n_tiles * 256]): the flat tile index of the mesh for accel="tiles"
        (Engine.tri_tiles_build), built on first use and kept for the same arguments.  order: None for `tile_order`, or the
        caller's own: every valid slot exactly once, -1 for nothing; anything else is a ValueError.  Reading the build counters
        synchronises with the device once, here."""
        key = (float(big_fraction), None if order is None else id(order))
        if self._tiles is not None and self._tiles[0] == key:
            return self._tiles[1]
        own = order is not None
        o = torch.as_tensor(order).detach().to(self.device).reshape(-1) if own else tile_order(self.packed, self.n_faces, big_fraction)
        tiles, clean, counts = self.engine.tri_tiles_build(self.packed, self.n_faces, o)
        # a slot listed twice: the counters cannot see it when another one is missing
        slots = int(self.packed.shape[0])
        seen = torch.zeros(slots + 1, dtype=torch.int64, device=self.device)
        seen.scatter_add_(0, torch.where((o >= 0) & (o < slots), o, slots).to(torch.int64), torch.ones_like(o, dtype=torch.int64))
        n_bad, n_listed, n_twice = torch.cat([counts.to(torch.int64), (seen[:slots] > 1).sum().reshape(1)]).tolist()
        if n_bad or n_twice or n_listed != self.n_valid:
            raise ValueError("PackedMesh.tiles: order must list each of the %d valid slots once (%d entries outside [0, %d), %d "
                             "slots listed twice, %d valid slots listed)" % (self.n_valid, n_bad, slots, n_twice, n_listed))
        self._tiles = (key, (tiles, clean), order)               # the caller's order is held so that its id stays its own
        return tiles, clean


def _tri_distance(engine, mesh, pts, accel, beta=0.0, **want):
    """Engine.tri_distance, or with accel="tiles" Engine.tri_distance_tiles on the mesh's tile index: the same five outputs"""
    if accel is None:
        return _engine(engine).tri_distance(mesh.packed, mesh.n_faces, pts, **want)
    if accel != "tiles":
        raise ValueError("accel must be None or 'tiles' (got %r)" % (accel,))
    tiles, clean = mesh.tiles()
    return _engine(engine).tri_distance_tiles(mesh.packed, mesh.n_faces, tiles, clean, pts, beta=beta, **want)[:5]


def surface_distance(engine, mesh, pts, want_index=False, want_closest=False, accel=None):
    """(dist [n] f32, index [n] i32 or None, closest [n,3] f32 or None, record f64 [4]) on the device: the exact distance from
    every point to the nearest triangle of `mesh` (a PackedMesh), the lowest face index on ties; +inf / -1 / NaN for a mesh
    without a valid face, NaN / -1 for a non-finite point.  record: sum of dist over the finite points, their number, the number of
    non-finite points, the largest dist.  ONE isdf_tri_distance call without the solid-angle arithmetic; no host synchronisation.
    accel="tiles": the same bits through the mesh's tile index (isdf_tri_distance_tiles; the first use builds the index)."""
    dist, index, closest, _, record = _tri_distance(engine, mesh, pts, accel, want_index=want_index, want_closest=want_closest)
    return dist, index, closest, record


def mesh_sdf(engine, mesh, pts, free_winding=0.0, accel=None, beta=3.0):
    """(sdf [n] f32, winding [n] f32) on the device: the distance to the surface, positive where the point is free -- iff
    |w - free_winding| < 0.5 with w the generalised winding number of the mesh around the point -- and negative elsewhere.
    free_winding = 0: closed objects in open space, normals outward (w = 1 inside an object).  free_winding = -1: a room seen
    from inside with every normal into free space (w = -1 in free space, 0 inside a solid and outside the room).  ONE
    isdf_tri_distance call; no host synchronisation.  accel="tiles": the same magnitude bit for bit through the mesh's tile index;
    the winding number takes one dipole term for every tile farther than `beta` of its radii from a block of queries (DESIGN 27
    has the measured error; beta <= 0: no tile does)."""
    dist, _, _, w, _ = _tri_distance(engine, mesh, pts, accel, beta, want_winding=True)
    free = (w - float(free_winding)).abs() < 0.5
    return torch.where(free, dist, -dist), w


def grid_nodes(origin, spacing, dims, start, stop, device):
    """float32 [stop - start, 3]: nodes start .. stop-1 (row-major, k fastest) of the grid, x = ox + (float)i * sx with both
    operations rounded to fp32 (y, z alike)"""
    flat = torch.arange(start, stop, dtype=torch.int64, device=device)
    k = flat % dims[2]
    j = (flat // dims[2]) % dims[1]
    i = flat // (dims[1] * dims[2])
    o = torch.tensor(origin, dtype=torch.float64, device=device).to(torch.float32)
    s = torch.tensor(spacing, dtype=torch.float64, device=device).to(torch.float32)
    return o[None, :] + torch.stack([i, j, k], 1).to(torch.float32) * s[None, :]


def mesh_volume(engine, mesh, spacing, origin, dims, free_winding=0.0, chunk=CHUNK, accel=None, beta=3.0):
    """A metrics.GtVolume of `mesh_sdf` on the grid of `dims` (one number or three, each >= 2) nodes, node (i, j, k) at origin +
    (i, j, k) * spacing (the node positions as `grid_nodes` rounds them).  The nodes are produced and queried `chunk` at a time,
    so nothing but the volume itself grows with the grid.  No host synchronisation.  accel, beta: as for `mesh_sdf`."""
    eng = _engine(engine)
    dims = (int(dims),) * 3 if np.ndim(dims) == 0 else tuple(int(d) for d in dims)
    spacing = tuple(float(x) for x in np.broadcast_to(np.asarray(spacing, np.float64).reshape(-1), (3,)))
    origin = tuple(float(x) for x in np.asarray(origin, np.float64).reshape(3))
    if len(dims) != 3 or min(dims) < 2 or int(chunk) < 1:
        raise ValueError("mesh_volume: three sides >= 2 and chunk >= 1 are needed (got %r, %r)" % (dims, chunk))
    total = dims[0] * dims[1] * dims[2]
    values = torch.empty(total, dtype=torch.float32, device=eng.device)
    for start in range(0, total, int(chunk)):
        stop = min(start + int(chunk), total)
        values[start:stop] = mesh_sdf(eng, mesh, grid_nodes(origin, spacing, dims, start, stop, eng.device), free_winding, accel,
                                      beta)[0]
    return metrics.GtVolume(values.view(dims), spacing, origin, eng.device)


def sample_surface(vertices, faces, n, generator=None):
    """(points [n,3], face [n] int64): n points drawn uniformly by area from the mesh, in torch ops on the device (and in the
    dtype) of `vertices`: a face by torch.multinomial over the areas (at most 2^24 faces), then p = (1 - r) a + r (1 - t) b + r t c
    with r = sqrt(u), (u, t) uniform in [0, 1).  Faces of zero or non-finite area are never drawn."""
    v = torch.as_tensor(vertices)
    v = v if v.is_floating_point() else v.to(torch.float32)
    f = torch.as_tensor(faces).to(device=v.device, dtype=torch.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * torch.linalg.norm(torch.linalg.cross(b - a, c - a), dim=1)
    area = torch.where(torch.isfinite(area), area, torch.zeros_like(area))
    if int(n) > 0 and not bool(area.sum() > 0):
        raise ValueError("sample_surface: the mesh has no face of positive area")
    face = torch.multinomial(area, int(n), replacement=True, generator=generator) if int(n) > 0 else f.new_zeros(0)
    ut = torch.rand(int(n), 2, dtype=v.dtype, device=v.device, generator=generator)
    r, t = ut[:, 0].sqrt()[:, None], ut[:, 1][:, None]
    return (1 - r) * a[face] + (r * (1 - t)) * b[face] + (r * t) * c[face], face


def mesh_accuracy_completion(engine, gt_mesh, rec_mesh, samples=200000, generator=None, accel=None):
    """(acc, comp): the mean distance from `samples` points drawn on the reconstruction to the ground-truth SURFACE, and from
    `samples` points drawn on the ground truth to the reconstructed surface (both PackedMesh; the ground-truth points are drawn
    first).  The reference's metrics.accuracy_comp (metrics.py:48-73), and metrics.accuracy_completion here, measure from sample
    to SAMPLE -- the nearest neighbour in a second point cloud -- which overestimates the distance to the surface by up to the
    sample spacing; this one has no such floor.  Two isdf_tri_distance calls, one copy of two records.  accel="tiles": the same
    floats through the meshes' tile indices."""
    eng = _engine(engine)
    gt_pts, _ = sample_surface(gt_mesh.vertices, gt_mesh.faces, samples, generator)
    rec_pts, _ = sample_surface(rec_mesh.vertices, rec_mesh.faces, samples, generator)
    acc = surface_distance(eng, gt_mesh, rec_pts, accel=accel)[3]
    comp = surface_distance(eng, rec_mesh, gt_pts, accel=accel)[3]
    r = torch.stack([acc, comp]).cpu().numpy()
    return float(metrics._ratio(r[0, 0], r[0, 1])), float(metrics._ratio(r[1, 0], r[1, 1]))
