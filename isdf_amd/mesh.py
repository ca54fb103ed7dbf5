"""Mesh reconstruction on the device: marching cubes of a dense SDF volume (`isdf_marching_cubes`, include/isdf_hip.h) and the
index -> world affine of the reference's `draw3D.draw_mesh` (draw3D.py:128-160).

    verts, faces, normals = marching_cubes(sdf_grid, level=0.0, index_to_world=grid_index_to_world(dim, scale, T))

gives, on the device, the vertices and normals `draw_mesh(sdf_grid, scale, T)` ends up with, and int32 faces.  The mesh is
indexed (one vertex per sign-changing grid edge) and bit-reproducible: vertices are ordered by the grid point owning their edge,
then axis; faces by cell, then table order (tables: isdf_amd/mc_tables.py).

    verts, faces, normals, stats = extract_surface(engine, dim, index_to_world)       # or reconstruct(trainer, grid_dim)

gives the same mesh with the network evaluated only in a narrow band around its level set (`isdf_band_*`): what makes
grids finer than the visualisation grid affordable."""
import ctypes as C

import numpy as np
import torch

from . import _ffi
from .engine import _stream, host_array, to_host


def grid_index_to_world(dim, scene_scale, bounds_transform):
    """[3, 4] float32 affine of draw_mesh's chain on a dim^3 grid: v / (dim - 1) -> - 0.5 -> x 2 -> x scene_scale (per axis) ->
    bounds_transform (4 x 4).  `Trainer.grid_pc` holds exactly these points (make_3D_grid over [-1, 1], trainer.py:141-148)."""
    s = np.broadcast_to(np.asarray(scene_scale, np.float64).reshape(-1), (3,))
    T = np.asarray(bounds_transform, np.float64).reshape(4, 4)
    R = T[:3, :3]
    A = np.empty((3, 4), np.float64)
    A[:, :3] = R * (2.0 * s / (dim - 1))[None, :]
    A[:, 3] = T[:3, 3] - R @ s
    return A.astype(np.float32)


class Mesher:
    """Caller-side state of `isdf_marching_cubes` on one device: the workspace, the device / pinned-host count pair and the
    output capacity, all kept across calls.  Each call makes ONE launch sequence at the current capacity, synchronises once to
    read the counts, and re-launches once with exact capacity only if the mesh did not fit (the capacity then stays grown).
    The returned tensors are fresh (torch's caching allocator): a later call does not overwrite them."""

    def __init__(self, device):
        self.lib = _ffi.lib()
        self.device = torch.device(device)
        self._ws = None
        self.counts = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.counts_host = torch.zeros(2, dtype=torch.int64, pin_memory=True)
        self.cap = None
        self.launches = 0        # marching-cubes launch sequences so far (the overflow path makes two for one call)

    @staticmethod
    def estimate(D0, D1, D2):
        """vertices / faces to allocate before the first call: a surface that crosses every slab of the grid a few times"""
        v = 4 * (D0 * D1 + D1 * D2 + D0 * D2) + 4096
        return v, 2 * v + 4096

    def _launch(self, args, V, F, stream):
        verts = torch.empty(V, 3, dtype=torch.float32, device=self.device)
        normals = torch.empty(V, 3, dtype=torch.float32, device=self.device)
        faces = torch.empty(F, 3, dtype=torch.int32, device=self.device)
        _ffi.check(self.lib.isdf_marching_cubes(C.byref(args), _ffi.ptr(self.counts), _ffi.ptr(verts), _ffi.ptr(normals), V,
                                                _ffi.ptr(faces), F, _ffi.ptr(self._ws), self._ws.numel(), stream),
                   "isdf_marching_cubes")
        self.launches += 1
        self.counts_host.copy_(self.counts, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        nv, nf = (int(x) for x in self.counts_host.tolist())
        return verts, faces, normals, nv, nf

    def __call__(self, volume, level=0.0, index_to_world=None, capacity=None):
        if volume.dim() != 3:
            raise ValueError("marching_cubes takes a [D0, D1, D2] volume (got shape %s)" % (tuple(volume.shape),))
        vol = volume.detach().to(device=self.device, dtype=torch.float32).contiguous()
        D0, D1, D2 = (int(d) for d in vol.shape)
        args = _ffi.McArgs()
        args.volume, args.D0, args.D1, args.D2, args.level = vol.data_ptr(), D0, D1, D2, float(level)
        if index_to_world is not None:
            A = host_array(index_to_world, np.float32).reshape(3, 4)
            args.has_transform = 1
            args.index_to_world[:] = [float(x) for x in A.reshape(-1)]
        nb = self.lib.isdf_mesh_ws_bytes(D0, D1, D2)
        _ffi.check(min(nb, 0), "isdf_mesh_ws_bytes(%d, %d, %d)" % (D0, D1, D2))
        if self._ws is None or self._ws.numel() < nb:
            self._ws = torch.empty(int(nb), dtype=torch.uint8, device=self.device)
        if capacity is not None:
            V, F = capacity
        else:
            est = self.estimate(D0, D1, D2)
            V, F = (est if self.cap is None else (max(self.cap[0], est[0]), max(self.cap[1], est[1])))
        stream = _stream(self.device)
        verts, faces, normals, nv, nf = self._launch(args, V, F, stream)
        if nv > V or nf > F:            # did not fit: nothing was written; once more at the exact size
            V, F = max(nv, 1), max(nf, 1)
            verts, faces, normals, nv2, nf2 = self._launch(args, V, F, stream)
            assert (nv2, nf2) == (nv, nf), ((nv, nf), (nv2, nf2))
        if capacity is None:
            grown = (max(V, nv + nv // 4), max(F, nf + nf // 4))
            self.cap = grown if self.cap is None else (max(self.cap[0], grown[0]), max(self.cap[1], grown[1]))
        return verts[:nv], faces[:nf], normals[:nv]


_MESHERS = {}


def marching_cubes(volume, level=0.0, index_to_world=None):
    """Marching cubes of a device volume [D0, D1, D2] (vol[i][j][k], as `sdf.view(dim, dim, dim)` lays it out) at `level`.

    Returns (verts [V, 3] f32, faces [F, 3] int32, normals [V, 3] f32), all on the volume's device.  A corner is inside iff
    value < level; cells with a non-finite corner are skipped.  Normals are the interpolated central-difference gradient,
    normalised: they point toward increasing value (free space for an SDF), and every face's right-hand normal agrees.
    index_to_world: optional [3, 4] affine applied in the kernel (normals by its inverse transpose), e.g. `grid_index_to_world`."""
    dev = volume.device
    if dev.type != "cuda":
        raise _ffi.IsdfError("isdf_amd marching cubes needs a HIP device (got %s); there is no CPU path" % dev)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    m = _MESHERS.get(key)
    if m is None:
        m = _MESHERS[key] = Mesher(torch.device("cuda", key))
    return m(volume, level, index_to_world)


# ---- narrow-band extraction: the field only near its level set (isdf_band_*, isdf_amd/csrc/band.hip)
DEFAULT_SLACK = 1.5      # max(1.5, 1.5 x the smallest complete slack measured on the trained nets): DESIGN 19
BAND_UNSET_BITS = 0x7fe15df0     # the NaN a band volume holds where the field was not evaluated (band.hip: BD_UNSET)
MAX_WIDEN = 6            # band attempts of extract_surface(widen=True) before the dense grid is evaluated


def _affine_rows(index_to_world):
    A = host_array(index_to_world, np.float32)
    return (C.c_float * 12)(*[float(x) for x in A.reshape(3, 4).reshape(-1)])


def _dims3(dims):
    d = (int(dims),) * 3 if np.ndim(dims) == 0 else tuple(int(x) for x in dims)
    if len(d) != 3:
        raise ValueError("dims: one number or three (got %r)" % (dims,))
    return d


def grid_points(dims, index_to_world, device="cuda"):
    """[D0*D1*D2, 3] float32 on the device: `index_to_world` (a [3, 4] affine, e.g. `grid_index_to_world`) at every lattice point
    (i, j, k), row-major, by isdf_grid_points -- per row r, fma(a_r2, k, fma(a_r1, j, fma(a_r0, i, a_r3))) in float32, the very
    chain the band's sparse lists use: the field on these points is the dense volume a band volume agrees with bit for bit."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _ffi.IsdfError("isdf_amd grid_points needs a HIP device (got %s); there is no CPU path" % dev)
    D0, D1, D2 = _dims3(dims)
    if min(D0, D1, D2) < 2 or D0 * D1 * D2 > 0x7fffffff:
        raise ValueError("grid_points: each dimension >= 2 and at most 2^31 - 1 points (got %r)" % ((D0, D1, D2),))
    pts = torch.empty(D0 * D1 * D2, 3, dtype=torch.float32, device=dev)
    _ffi.check(_ffi.lib().isdf_grid_points(D0, D1, D2, _affine_rows(index_to_world), _ffi.ptr(pts), _stream(pts.device)),
               "isdf_grid_points")
    return pts


class BandSelector:
    """Caller-side state of the isdf_band_* calls on one device: the workspace and the device / pinned-host count table, kept
    across calls.  One call walks the strides coarse, ..., 2 and the closing fill; per level it reads ONE count back (the list
    has to be allocated and the field called at that size), nothing else leaves the device."""

    def __init__(self, device):
        self.lib = _ffi.lib()
        self.device = torch.device(device)
        self._ws = None
        self._counts = self._counts_host = None

    def __call__(self, field, dims, index_to_world=None, points=None, level=0.0, slack=DEFAULT_SLACK, coarse=8):
        D0, D1, D2 = _dims3(dims)
        P = D0 * D1 * D2
        coarse = int(coarse)
        slack = DEFAULT_SLACK if slack is None else float(slack)
        if index_to_world is None and points is None:
            raise ValueError("band_volume: index_to_world or points (or both: the affine then only measures the cells)")
        a = _ffi.BandArgs()
        a.D0, a.D1, a.D2, a.coarse, a.level, a.slack = D0, D1, D2, coarse, float(level), slack
        if index_to_world is not None:
            a.has_transform = 1
            a.index_to_world[:] = list(_affine_rows(index_to_world))
        if points is not None:
            points = points.detach().reshape(-1, 3).to(device=self.device, dtype=torch.float32).contiguous()
            if points.shape[0] != P:
                raise ValueError("band_volume: %d points for a %d x %d x %d grid" % (points.shape[0], D0, D1, D2))
            a.points = points.data_ptr()
        nb = self.lib.isdf_band_ws_bytes(D0, D1, D2, coarse)
        _ffi.check(min(nb, 0), "isdf_band_ws_bytes(%d, %d, %d, coarse=%d)" % (D0, D1, D2, coarse))
        if self._ws is None or self._ws.numel() < nb:
            self._ws = torch.empty(int(nb), dtype=torch.uint8, device=self.device)
        ws, wsn = _ffi.ptr(self._ws), self._ws.numel()
        strides = []
        s = coarse
        while s >= 2:
            strides.append(s)
            s //= 2
        L = len(strides)
        rows = 2 * L + 2                  # select of every stride and of the fill | test of every stride | leaks
        if self._counts is None or self._counts.shape[0] < rows:
            self._counts = torch.zeros(rows, 2, dtype=torch.int64, device=self.device)
            self._counts_host = torch.zeros(rows, 2, dtype=torch.int64, pin_memory=True)
        counts, host = self._counts, self._counts_host
        row = lambda r: C.c_void_p(counts.data_ptr() + 16 * r)
        stream = _stream(self.device)

        def read():
            host[:rows].copy_(counts[:rows], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()

        vol = torch.empty(D0, D1, D2, dtype=torch.float32, device=self.device)
        _ffi.check(self.lib.isdf_band_begin(C.byref(a), _ffi.ptr(vol), stream), "isdf_band_begin")
        evaluated = []
        for li, s in enumerate(strides + [1]):
            _ffi.check(self.lib.isdf_band_select(C.byref(a), s, _ffi.ptr(vol), row(li), ws, wsn, stream), "isdf_band_select")
            read()
            n = int(host[li, 0])
            evaluated.append(n)
            index = torch.empty(n, dtype=torch.int32, device=self.device)
            values = None
            if n > 0:
                pts = torch.empty(n, 3, dtype=torch.float32, device=self.device)
                _ffi.check(self.lib.isdf_band_emit(C.byref(a), s, _ffi.ptr(vol), _ffi.ptr(index), _ffi.ptr(pts), n, ws, wsn, stream),
                           "isdf_band_emit")
                values = field(pts).detach().reshape(-1).to(device=self.device, dtype=torch.float32).contiguous()
                if values.numel() != n:
                    raise ValueError("band_volume: field returned %d values for %d points" % (values.numel(), n))
            _ffi.check(self.lib.isdf_band_update(C.byref(a), s, _ffi.ptr(vol), _ffi.ptr(index) if n else None, _ffi.ptr(values), n,
                                                 row(L + 1 + li) if s > 1 else None, ws, wsn, stream), "isdf_band_update")
        _ffi.check(self.lib.isdf_band_leaks(C.byref(a), _ffi.ptr(vol), row(2 * L + 1), ws, wsn, stream), "isdf_band_leaks")
        read()
        levels = [dict(stride=s, candidates=int(host[L + 1 + li, 0]), kept=int(host[L + 1 + li, 1]), evaluated=evaluated[li])
                  for li, s in enumerate(strides)]
        levels.append(dict(stride=1, evaluated=evaluated[L]))       # the closing fill: cells and halos of the kept stride-2 cells
        total = sum(evaluated)
        stats = dict(levels=levels, evaluated=total, dense=P, fraction=total / P, leaks=int(host[2 * L + 1, 0]), slack=slack,
                     coarse=coarse)
        return vol, stats


def extract_surface(engine_or_sdf_map, dims, index_to_world, level=0.0, slack=None, coarse=8, widen=True, field=None, points=None):
    """(verts, faces, normals, stats) on the device: `Engine.band_volume`, then `Engine.marching_cubes` with `index_to_world` as
    the kernel's affine -- the mesh of the dense grid, with the network evaluated only near its level set.

    engine_or_sdf_map: an `Engine`, or anything with one as `.engine` (SDFMapHIP, a grafted trainer).  slack: None = DEFAULT_SLACK.
    widen: a volume that reports leaks (the surface left the band) is recomputed at twice the slack, up to MAX_WIDEN band attempts;
    after those every cell is kept: the field is evaluated on `grid_points` (or `points`), which is the dense result.  stats: the
    last attempt's, plus `attempts`, every attempt's in order (a dense one has `dense_fallback` set).  field / points: see
    `Engine.band_volume`."""
    eng = getattr(engine_or_sdf_map, "engine", engine_or_sdf_map)
    dims = _dims3(dims)
    fn = eng.sdf_eval if field is None else field
    s = DEFAULT_SLACK if slack is None else float(slack)
    attempts = []
    while True:
        vol, st = eng.band_volume(dims, index_to_world, points, level, s, coarse, fn)
        attempts.append(st)
        if not widen or st["leaks"] == 0:
            break
        if len(attempts) == MAX_WIDEN:
            P = dims[0] * dims[1] * dims[2]
            pts = grid_points(dims, index_to_world, eng.device) if points is None else points.reshape(-1, 3)
            vol = fn(pts).detach().reshape(dims).to(dtype=torch.float32)
            st = dict(levels=[], evaluated=P, dense=P, fraction=1.0, leaks=0, slack=float("inf"), coarse=coarse, dense_fallback=True)
            attempts.append(st)
            break
        s *= 2.0
    verts, faces, normals = eng.marching_cubes(vol, level, index_to_world)
    return verts, faces, normals, dict(st, attempts=attempts)


def reconstruct(trainer, grid_dim=None, **kw):
    """`extract_surface` for a grafted trainer over its bounds box at ANY grid_dim (None: the trainer's): the affine is
    `grid_index_to_world(grid_dim, trainer.scene_scale_np, trainer.bounds_transform_np)`, what mesh_rec uses.  At the trainer's own
    grid_dim the points are gathered from `trainer.grid_pc`, so the values are get_sdf_grid's; at any other the kernel's affine
    makes them.  A module-level function: it adds nothing to the trainer.  kw: level, slack, coarse, widen, field."""
    dim = int(trainer.grid_dim if grid_dim is None else grid_dim)
    A = grid_index_to_world(dim, trainer.scene_scale_np, trainer.bounds_transform_np)
    points = trainer.grid_pc if dim == int(trainer.grid_dim) else None
    with torch.no_grad():
        return extract_surface(trainer.engine, dim, A, points=points, **kw)


class MeshMethods:
    """The trainer-level half (trainer.py:1426-1443,1500-1542): a base class of hot_path.HotPath; `self` is the grafted Trainer."""

    def get_sdf_grid(self):
        """The network on the cached `grid_pc` as a [grid_dim]^3 volume: ONE forward launch over all grid_dim^3 points (the
        reference's fc_map.chunks makes one per 100 000; the kernel's result per point does not depend on the chunking)."""
        d = self.grid_dim
        with torch.no_grad():
            return self.engine.sdf_eval(self.grid_pc).view(d, d, d)

    def _vis_pointcloud(self):
        """world-frame point cloud of the keyframes at visualisation resolution (update_vis_vars + backproject + draw_pc)"""
        ref = self._hip.ref_module
        self.update_vis_vars()
        pcs_cam = ref.geometry.transform.backproject_pointclouds(self.gt_depth_vis, self.fx_vis, self.fy_vis, self.cx_vis,
                                                                 self.cy_vis)
        pc, _ = ref.draw3D.draw_pc(len(self.frames), pcs_cam, self.frames.T_WC_batch_np)
        return pc

    def mesh_rec(self, crop_mesh_with_pc=True):
        """The reconstructed mesh as a trimesh.Trimesh in world coordinates, what the reference's mesh_rec returns.

        Contract kept: a trainer without a GT scene that runs incrementally first re-derives its scene bounds from the keyframes'
        point cloud (set_scene_properties); with crop_mesh_with_pc, faces none of whose vertices lie within crop_dist of that
        point cloud are dropped (a KDTree query on the host) together with the vertices left unreferenced; a pending grid size
        (new_grid_dim / new_grid_pc) is swapped in at the end.  The point cloud is only built when one of the two needs it.

        The mesh itself: get_sdf_grid, then Engine.marching_cubes with draw_mesh's index -> world chain as the kernel's affine
        (isdf_amd.mesh.grid_index_to_world), so vertices and normals come out in world coordinates; ONE device -> host copy;
        flat grey face colours as draw_mesh(..., color_by="none") sets them."""
        ref = self._ref("mesh_rec", "trimesh", "trimesh, KDTree, draw3D")
        rescale = self.gt_scene is False and self.incremental
        pc = self._vis_pointcloud() if (crop_mesh_with_pc or rescale) else None
        if rescale:
            self.set_scene_properties(ref.trimesh.PointCloud(pc))
        sdf = self.get_sdf_grid()
        A = grid_index_to_world(self.grid_dim, self.scene_scale_np, self.bounds_transform_np)
        verts, faces, normals = self.engine.marching_cubes(sdf, 0.0, A)
        nv = verts.shape[0]
        verts_h, normals_h, faces_h = to_host(verts, normals, faces)
        if crop_mesh_with_pc:
            near = ref.KDTree(pc).query(verts_h, k=1)[0] < self.crop_dist
            faces_h = faces_h[near[faces_h].any(axis=1)]
            used = np.zeros(nv, bool)
            used[faces_h.reshape(-1)] = True
            remap = np.cumsum(used) - 1
            verts_h, normals_h, faces_h = verts_h[used], normals_h[used], remap[faces_h].astype(np.int32)
        mesh = ref.trimesh.Trimesh(vertices=verts_h, vertex_normals=normals_h, faces=faces_h)
        mesh.visual.face_colors = [160, 160, 160, 255]
        if self.new_grid_dim is not None:
            self.grid_dim, self.grid_pc = self.new_grid_dim, self.new_grid_pc
            self.new_grid_dim = self.new_grid_pc = None
        return mesh
