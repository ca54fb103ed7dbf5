"""The voxel baseline beside the neural map (include/isdf_hip.h: isdf_tsdf_integrate, isdf_distance_transform, isdf_occupancy_sdf;
DESIGN 22).

"Is the map better than simply fusing the depth frames into voxels?" -- the comparison the reference's evaluation is built around
(eval/plot_utils.py:108-130 reads a "GPU fusion" result and scores it with the net's metrics) without shipping the fusion.

    TsdfVolume          a running (tsdf, weight) pair on the device and its grid
    integrate           posed depth frames -> the volume, in frame order: ONE isdf_tsdf_integrate call
    fuse_frames         integrate over the stored keyframes of a grafted trainer; it RETURNS the volume and writes nothing back
    distance_transform  exact squared Euclidean distances to the nearest feature voxel
    signed_distance     the reference's sdf_from_occupancy (sdf_util.py:371-385) of an occupancy grid
    full_sdf            the baseline's full-range field: signed_distance of the volume's occupancy, the TSDF inside its band
    baseline_metrics    a baseline field scored against ground truth with the record the net is scored with

Module-level functions and one small class: nothing is added to HotPath or HipState.  `engine` is an isdf_amd.engine.Engine (or
anything with its tsdf_integrate / distance_transform / occupancy_sdf / sdf_metrics methods).
"""
import numpy as np
import torch

from . import metrics
from .mesh import grid_index_to_world

INF = float("inf")


def _engine(obj):
    """an Engine, or anything that has one as `.engine` (SDFMapHIP, a grafted trainer)"""
    return getattr(obj, "engine", obj)


class TsdfVolume:
    """`tsdf` and `weight`: float32 [nx, ny, nz] on `device`, zeroed; voxel (i, j, k) at origin + (i, j, k) * spacing.  dims and
    spacing: one number or three.  trunc: the truncation distance in metres; max_weight: where the running average saturates
    (inf: a plain mean over all measurements)."""

    def __init__(self, dims, spacing, origin, trunc, device, max_weight=INF):
        self.dims = (int(dims),) * 3 if np.ndim(dims) == 0 else tuple(int(d) for d in dims)
        self.spacing = tuple(float(x) for x in np.broadcast_to(np.asarray(spacing, np.float64).reshape(-1), (3,)))
        self.origin = tuple(float(x) for x in np.asarray(origin, np.float64).reshape(3))
        self.trunc, self.max_weight = float(trunc), float(max_weight)
        if len(self.dims) != 3 or min(self.dims) < 1 or self.dims[0] * self.dims[1] * self.dims[2] > 0x7fffffff:
            raise ValueError("TsdfVolume: three sides >= 1 and at most 2^31 - 1 voxels (got %r)" % (dims,))
        if not all(np.isfinite(x) and x > 0 for x in self.spacing) or not all(np.isfinite(x) for x in self.origin):
            raise ValueError("TsdfVolume: spacing must be positive and finite, origin finite (got %s, %s)" % (self.spacing, self.origin))
        if not (np.isfinite(self.trunc) and self.trunc > 0) or not self.max_weight >= 1:
            raise ValueError("TsdfVolume: trunc must be positive and finite, max_weight >= 1 (got %s, %s)" % (trunc, max_weight))
        self.device = torch.device(device)
        self.tsdf = torch.zeros(self.dims, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(self.dims, dtype=torch.float32, device=self.device)

    @classmethod
    def from_bounds(cls, lo, hi, voxel, trunc=None, device="cuda", max_weight=INF):
        """The smallest grid of cubic `voxel`-sized cells from `lo` that reaches `hi` on every axis (trunc: None = 4 voxels)."""
        lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
        voxel = float(voxel)
        if not (np.isfinite(voxel) and voxel > 0) or not np.all(hi >= lo):
            raise ValueError("TsdfVolume.from_bounds: voxel > 0 and hi >= lo are needed (got %s, %s, %s)" % (lo, hi, voxel))
        dims = np.ceil((hi - lo) / voxel - 1e-9).astype(np.int64) + 1
        return cls(dims, voxel, lo, 4.0 * voxel if trunc is None else trunc, device, max_weight)

    @classmethod
    def for_trainer(cls, trainer, voxel, trunc=None, max_weight=INF):
        """`from_bounds` over the axis-aligned box around the eight corners of the trainer's own grid (isdf_amd.mesh.
        grid_index_to_world: the box mesh_rec meshes), on the trainer's device."""
        lo, hi = trainer_box(trainer)
        return cls.from_bounds(lo, hi, voxel, trunc, _engine(trainer).device, max_weight)

    def index_to_world(self):
        """[3, 4] float32 affine of the grid, what Engine.marching_cubes takes"""
        A = np.zeros((3, 4), np.float32)
        A[:, :3], A[:, 3] = np.diag(self.spacing), self.origin
        return A

    def values(self):
        """the TSDF with NaN where nothing was measured (weight == 0): `engine.marching_cubes(vol.values(), 0.0,
        vol.index_to_world())` is the fused mesh (marching cubes skips cells with a non-finite corner; a vertex normal whose central
        differences reach an unmeasured voxel is NaN)"""
        return torch.where(self.weight > 0, self.tsdf, torch.full_like(self.tsdf, float("nan")))

    def occupancy(self):
        """uint8 [nx, ny, nz]: measured and on or behind the surface (weight > 0 and tsdf <= 0)"""
        return ((self.weight > 0) & (self.tsdf <= 0)).to(torch.uint8)

    def gt_volume(self, values):
        """`values` [nx, ny, nz] as an isdf_amd.metrics.GtVolume on this grid (every side >= 2)"""
        if tuple(values.shape) != self.dims:
            raise ValueError("TsdfVolume.gt_volume: values are %s, the grid %s" % (tuple(values.shape), self.dims))
        return metrics.GtVolume(values, self.spacing, self.origin, self.device)


def trainer_box(trainer):
    """(lo [3], hi [3]) float64: the axis-aligned box around the eight corners of the trainer's grid"""
    d = int(trainer.grid_dim)
    A = grid_index_to_world(d, trainer.scene_scale_np, trainer.bounds_transform_np).astype(np.float64)
    corners = np.array([[i, j, k, 1.0] for i in (0, d - 1) for j in (0, d - 1) for k in (0, d - 1)]) @ A.T
    return corners.min(0), corners.max(0)


def integrate(engine, vol, depth, T_WC, cam, min_depth=0.0, max_depth=INF):
    """depth [F,H,W] (device) taken at the poses T_WC [F,4,4] fused into `vol` in index order; returns `vol`.  The poses are
    inverted on the device with torch.linalg.inv, as metrics.visible_points inverts them; then ONE isdf_tsdf_integrate call.  cam:
    anything with fx, fy, cx, cy.  A pixel counts iff min_depth < depth < max_depth (0 and NaN never do).  Integrating frames in
    several calls gives the bytes of one call over all of them."""
    eng = _engine(engine)
    T = torch.as_tensor(T_WC).to(device=eng.device, dtype=torch.float32).reshape(-1, 4, 4)
    T_CW = torch.linalg.inv(T) if T.shape[0] else T
    eng.tsdf_integrate(vol.tsdf, vol.weight, depth, T_CW, cam, vol.origin, vol.spacing, vol.trunc, max_weight=vol.max_weight,
                       min_depth=min_depth, max_depth=max_depth)
    return vol


def fuse_frames(trainer, voxel=None, dims=None, idxs=None, trunc=None, max_weight=INF, min_depth=0.0, max_depth=INF):
    """A new TsdfVolume with the stored keyframes of a grafted trainer fused into it: its `frames.depth_batch` and
    `frames.T_WC_batch` (idxs: which keyframes, in that order; None = all) with the trainer's intrinsics, as
    tracking.refine_frames reads them.  The grid covers the trainer's own box (`trainer_box`): cubic cells of `voxel` metres, or
    `dims` (one number or three) lattice points per axis across it.  trunc: None = 4 x the largest spacing.  The keyframe store
    is not written."""
    if (voxel is None) == (dims is None):
        raise ValueError("fuse_frames: exactly one of voxel and dims")
    dev = _engine(trainer).device
    if voxel is not None:
        vol = TsdfVolume.for_trainer(trainer, voxel, trunc, max_weight)
    else:
        lo, hi = trainer_box(trainer)
        d = np.broadcast_to(np.asarray(dims, np.int64).reshape(-1), (3,))
        if d.min() < 2:
            raise ValueError("fuse_frames: dims >= 2 per axis (got %r)" % (dims,))
        spacing = (hi - lo) / (d - 1)
        vol = TsdfVolume(d, spacing, lo, 4.0 * float(spacing.max()) if trunc is None else trunc, dev, max_weight)
    depth, T = trainer.frames.depth_batch, trainer.frames.T_WC_batch
    if idxs is not None:
        ix = torch.as_tensor(np.asarray(idxs, np.int64).reshape(-1), device=depth.device)
        depth, T = depth[ix], T[ix]
    return integrate(trainer, vol, depth, T, trainer, min_depth=min_depth, max_depth=max_depth)


def distance_transform(engine, feature, invert=False):
    """int32 [nx,ny,nz] on the device: per voxel the exact squared distance, in voxels, to the nearest voxel q with
    (feature[q] != 0) != invert; 2^30 (_ffi.EDT_NONE) where there is none."""
    return _engine(engine).distance_transform(feature, invert=invert)


def signed_distance(engine, occ, voxel):
    """float32 [nx,ny,nz] on the device: the reference's sdf_from_occupancy(occ, voxel) -- positive in free space; +inf / -inf
    everywhere when the grid holds no occupied / no free voxel."""
    return _engine(engine).occupancy_sdf(occ, voxel)


def full_sdf(engine, vol, blend=True):
    """The baseline's full-range field, float32 [nx,ny,nz]: `signed_distance(vol.occupancy(), voxel)`, which is quantised to voxel
    centres; with `blend` the TSDF itself wherever it was measured inside its band (weight > 0 and |tsdf| < trunc, trunc as the
    float32 the kernel clamps to: a voxel clamped to +-trunc is outside).  Needs cubic voxels (ValueError otherwise)."""
    sx, sy, sz = vol.spacing
    if not (abs(sx - sy) <= 1e-9 * sx and abs(sx - sz) <= 1e-9 * sx):
        raise ValueError("full_sdf: isotropic spacing is needed (got %s)" % (vol.spacing,))
    sdf = signed_distance(engine, vol.occupancy(), sx)
    if blend:
        sdf = torch.where((vol.weight > 0) & (vol.tsdf.abs() < float(np.float32(vol.trunc))), vol.tsdf, sdf)
    return sdf


def baseline_metrics(engine, field_values, vol, gt_volume, pts):
    """isdf_amd.metrics.SdfMetrics of a baseline field (`field_values` [nx,ny,nz] on `vol`'s grid, e.g. `full_sdf`) at `pts`
    [n,3] against `gt_volume` (a metrics.GtVolume): av_l1, binned_l1 and l1_chomp_costs as eval_sdf reports them for the net.
    The field is looked up trilinearly by ONE Engine.sdf_metrics(..., per_point=True) call with the baseline as the volume; the
    points inside the baseline's grid are then scored by metrics.sdf_metrics."""
    eng = _engine(engine)
    p = torch.as_tensor(pts).to(device=eng.device, dtype=torch.float32).reshape(-1, 3)
    zeros = torch.zeros(p.shape[0], dtype=torch.float32, device=eng.device)
    _, looked, inb = eng.sdf_metrics(vol.gt_volume(field_values), p, zeros, exclude_zero_gt=False, per_point=True)
    keep = inb.to(torch.bool)
    return metrics.sdf_metrics(eng, gt_volume, p[keep], looked[keep], exclude_zero_gt=True)
