"""Evaluation of the map against ground truth on the device (include/isdf_hip.h: isdf_sdf_metrics, isdf_region_metrics,
isdf_nn_distance).

    GtVolume              the ground-truth SDF grid resident on the device (what the reference keeps behind a scipy
                          RegularGridInterpolator, sdf_util.py:174-180)
    sdf_metrics           av_l1, the six distance bins and the CHOMP cost figures of Trainer.eval_sdf / eval_object_sdf /
                          eval_traj_cost (trainer.py:1831-1866,1993-2003,2026-2050): one launch pair, one host copy
    region_metrics        the per-region figures of eval_pts.fixed_pts_eval (eval_pts.py:96-299): av_l1, bins, CHOMP, av_cossim for
                          the vis and vox sets in one launch pair, one host copy
    accuracy_completion   metrics.accuracy / completion (metrics.py:48-59): mean nearest-neighbour distance both ways

`engine` is an isdf_amd.engine.Engine (or anything with its sdf_metrics / nn_distance methods).
"""
import numpy as np
import torch

from . import _ffi


class GtVolume:
    """An axis-aligned ground-truth volume: values [nx, ny, nz] (fp32, on `device`), grid point (i, j, k) at
    origin + (i, j, k) * spacing.  The reference's grids are of this form (get_grid_pts, sdf_util.py:151-159, reads only
    transform[i, i] and transform[i, 3])."""

    def __init__(self, values, spacing, origin, device):
        v = torch.as_tensor(values)
        if v.dim() != 3 or min(v.shape) < 2:
            raise ValueError("GtVolume: values must be [nx, ny, nz] with every side >= 2 (got %s)" % (tuple(v.shape),))
        self.values = v.to(device=device, dtype=torch.float32).contiguous()
        self.spacing = tuple(float(x) for x in np.asarray(spacing, np.float64).reshape(3))
        self.origin = tuple(float(x) for x in np.asarray(origin, np.float64).reshape(3))
        if not all(np.isfinite(x) and x > 0 for x in self.spacing) or not all(np.isfinite(x) for x in self.origin):
            raise ValueError("GtVolume: spacing must be positive and finite, origin finite (got %s, %s)" % (self.spacing, self.origin))

    @classmethod
    def from_interpolator(cls, itp, device="cuda"):
        """From anything with scipy's RegularGridInterpolator attributes `.grid` (three ascending, evenly spaced coordinate
        arrays) and `.values` ([nx, ny, nz]); nothing else is read and scipy is not imported."""
        grid = [np.asarray(g, np.float64).reshape(-1) for g in itp.grid]
        if len(grid) != 3:
            raise ValueError("GtVolume: a 3-D interpolator is needed (%d axes)" % len(grid))
        spacing = []
        for g in grid:
            if g.size < 2:
                raise ValueError("GtVolume: every axis needs at least two grid points")
            h = (g[-1] - g[0]) / (g.size - 1)
            if not h > 0 or np.abs(np.diff(g) - h).max() > 1e-6 * h:
                raise ValueError("GtVolume: only ascending, evenly spaced (axis-aligned) grids are supported")
            spacing.append(h)
        values = np.asarray(itp.values)
        if values.shape != tuple(g.size for g in grid):
            raise ValueError("GtVolume: values %s do not match the grid %s" % (values.shape, tuple(g.size for g in grid)))
        return cls(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)), spacing, [g[0] for g in grid], device)

    def to_c(self):
        a = _ffi.GtVolumeArgs()
        a.values = self.values.data_ptr()
        a.nx, a.ny, a.nz = (int(d) for d in self.values.shape)
        for k in range(3):
            a.spacing[k], a.origin[k] = self.spacing[k], self.origin[k]
        return a


def _ratio(num, den):
    """num / den with the reference's 0 / 0 = NaN (an empty bin, no valid point)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(num, np.float64) / np.asarray(den, np.float64)


class SdfMetrics:
    """The evaluation record by name.  Means are over the valid points; an empty bin (or no valid point) is NaN."""

    def __init__(self, record):
        r = np.asarray(record, np.float64).reshape(-1)
        if r.size != _ffi.METRICS_RECORD:
            raise ValueError("SdfMetrics: a record of %d doubles is needed" % _ffi.METRICS_RECORD)
        self.record = r
        self.n_valid, self.n_in_bounds = int(r[0]), int(r[1])
        self.l1_sum = float(r[2])
        self.bin_sums, self.bin_counts = r[3:9].copy(), r[9:15].astype(np.int64)
        c = r[15:24].reshape(3, 3)
        self.chomp_diff_sums, self.pred_chomp_sums, self.gt_chomp_sums = c[:, 0].tolist(), c[:, 1].tolist(), c[:, 2].tolist()

    @property
    def av_l1(self):
        return float(_ratio(self.l1_sum, self.n_valid))

    @property
    def binned_l1(self):
        return _ratio(self.bin_sums, self.bin_counts).tolist()

    @property
    def l1_chomp_costs(self):
        return _ratio(self.chomp_diff_sums, self.n_valid).tolist()

    def as_dict(self):
        """what Trainer.eval_sdf returns (trainer.py:1860-1864)"""
        return {"av_l1": self.av_l1, "binned_l1": self.binned_l1, "l1_chomp_costs": self.l1_chomp_costs}


def sdf_metrics(engine, volume, pts, sdf, exclude_zero_gt=True):
    """SdfMetrics of predicted `sdf` [n] at `pts` [n, 3] against `volume`: one isdf_sdf_metrics call and ONE copy to the host."""
    record, _, _ = engine.sdf_metrics(volume, pts, sdf, exclude_zero_gt=exclude_zero_gt)
    return SdfMetrics(record.cpu().numpy())


class RegionMetrics:
    """One set (vis or vox) of an isdf_region_metrics record: `.sdf` is the SdfMetrics of its 24 leading fields, `.av_cossim` the
    mean cosine distance over its gradient points -- NaN when any selected ground-truth gradient is not finite (what the
    reference's .mean() gives) or when the set is empty."""

    def __init__(self, record):
        r = np.asarray(record, np.float64).reshape(-1)
        if r.size != _ffi.REGION_RECORD:
            raise ValueError("RegionMetrics: a record of %d doubles is needed" % _ffi.REGION_RECORD)
        self.record = r
        self.sdf = SdfMetrics(r[:_ffi.METRICS_RECORD])
        self.n_grad, self.cos_dist_sum, self.n_grad_nonfinite = int(r[24]), float(r[25]), int(r[26])

    @property
    def av_cossim(self):
        return float("nan") if self.n_grad_nonfinite else float(_ratio(self.cos_dist_sum, self.n_grad))

    def as_dict(self, cossim=False):
        """what eval_pts.sub_eval returns for the set; with `cossim` the av_cossim pair of eval_pts.py:189-190 (both entries are
        the one figure when the gradient comes from grad_fn)"""
        d = self.sdf.as_dict()
        if cossim:
            d["av_cossim"] = [self.av_cossim, self.av_cossim]
        return d


def region_metrics(engine, pts, sdf, volume=None, gt=None, sdf_grad=None, flags=None, delta=0.01):
    """(vis, vox) RegionMetrics: one isdf_region_metrics call and ONE copy to the host."""
    rec = engine.region_metrics(pts, sdf, volume=volume, gt=gt, sdf_grad=sdf_grad, flags=flags, delta=delta).cpu().numpy()
    return RegionMetrics(rec[0]), RegionMetrics(rec[1])


def accuracy_completion(engine, gt_points, rec_points):
    """(acc, comp): mean distance from every reconstructed point to its nearest ground-truth point and the other way round
    (metrics.accuracy, metrics.completion).  Two isdf_nn_distance calls, one copy of two doubles."""
    def points(p):
        p = p if torch.is_tensor(p) else torch.from_numpy(np.asarray(p, np.float32))
        return p.to(engine.device, torch.float32).reshape(-1, 3)
    gt, rec = points(gt_points), points(rec_points)
    _, _, acc_sum = engine.nn_distance(rec, gt)
    _, _, comp_sum = engine.nn_distance(gt, rec)
    sums = torch.cat([acc_sum.reshape(1), comp_sum.reshape(1)]).cpu().numpy()
    return float(_ratio(sums[0], rec.shape[0])), float(_ratio(sums[1], gt.shape[0]))
