"""Evaluation of the map against ground truth on the device (include/isdf_hip.h: isdf_sdf_metrics, isdf_region_metrics,
isdf_nn_distance, isdf_visible_points).

    GtVolume              the ground-truth SDF grid resident on the device (what the reference keeps behind a scipy
                          RegularGridInterpolator, sdf_util.py:174-180)
    sdf_metrics           av_l1, the six distance bins and the CHOMP cost figures of Trainer.eval_sdf / eval_object_sdf /
                          eval_traj_cost (trainer.py:1831-1866,1993-2003,2026-2050): one launch pair, one host copy
    region_metrics        the per-region figures of eval_pts.fixed_pts_eval (eval_pts.py:96-299): av_l1, bins, CHOMP, av_cossim for
                          the vis and vox sets in one launch pair, one host copy
    accuracy_completion   metrics.accuracy / completion (metrics.py:48-59): mean nearest-neighbour distance both ways
    visible_points        geometry.frustum.is_visible_torch (frustum.py:87-133): per point the number of posed depth frames that
                          see it -- in front of the frame, inside its image, no more than trunc behind the surface -- in one launch
                          over all frames, O(n) memory

`engine` is an isdf_amd.engine.Engine (or anything with its sdf_metrics / nn_distance / visible_points methods).
"""
import os
import types
import warnings

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


def visible_points(engine, pts, T_WC_batch, depth_batch, cam, trunc=0.2, want_mask=False):
    """(count i32 [n], mask u8 [F,n] or None, n_seen i64 [1]), all on the device: what frustum.is_visible_torch(pts, T_WC_batch,
    depth_batch, H, W, fx, fy, cx, cy, trunc) decides (frustum.py:87-133), as count = inside.sum(0), mask = inside (only with
    want_mask) and n_seen = (count > 0).sum().  The poses are inverted on the device with torch.linalg.inv, as the reference inverts
    them; then ONE isdf_visible_points call.  cam: anything with fx, fy, cx, cy; H and W are depth_batch's."""
    T_WC = torch.as_tensor(T_WC_batch).to(device=engine.device, dtype=torch.float32).reshape(-1, 4, 4)
    T_CW = torch.linalg.inv(T_WC) if T_WC.shape[0] else T_WC
    return engine.visible_points(pts, T_CW, depth_batch, cam, trunc=trunc, want_mask=want_mask)


class EvalMethods:
    """The trainer-level half (trainer.py:1819-2088): a base class of hot_path.HotPath; `self` is the grafted Trainer."""

    def _gt_volume(self):
        """`self.gt_sdf_interp`'s grid on the device (isdf_amd.metrics.GtVolume), uploaded once and re-made only if the attribute is
        replaced; the interpolator itself is never called"""
        hip, itp = self._hip, self.gt_sdf_interp
        if itp is None:
            raise _ffi.IsdfError("evaluation needs trainer.gt_sdf_interp (a ground-truth SDF grid)")
        c = hip.gt_volume
        if c is None or c[0] is not itp:
            c = hip.gt_volume = (itp, GtVolume.from_interpolator(itp, hip.device))
        return c[1]

    def _eval_frames(self, upto=None):
        """(depth_batch [F,H,W], T_WC_batch [F,4,4]) of the cached sequence up to the virtual clock, as eval_sdf_visible and
        eval_object_sdf build them (trainer.py:1869-1875,1968-1974) -- but RESIDENT: the reference converts and uploads the whole
        sequence on every call (2 GB at 600 frames of 680 x 1200); here only the frames not yet on the device are read from
        `self.cached_dataset` and copied.  Incremental runs ask for arange(int(tot_step_time * fps)), which only grows; the
        non-incremental get_all() is uploaded once.  The cache lives on self._hip (not in hip_state_dict); drop_eval_cache()
        releases it; a clock that went backwards or another dataset object starts it afresh.
        upto: the frames of cached_dataset[arange(upto)] instead of the clock's (eval_fixed: its timestamp is normally behind the
        clock, so this is a prefix of what is held; frames beyond what is held are uploaded, once)."""
        hip = self._hip
        ds = self.cached_dataset
        c = hip.eval_cache
        mode = "incremental" if self.incremental else "all"
        want = int(self.tot_step_time * self.fps) if self.incremental else 0
        if c is None or c.dataset is not ds or c.mode != mode or (upto is None and want < c.clock):
            c = hip.eval_cache = types.SimpleNamespace(dataset=ds, mode=mode, asked=0, clock=0, held=0, depth=None, T=None,
                                                       uploaded_frames=0, uploaded_bytes=0)
        if upto is None:
            c.clock = want
        else:
            want = int(upto)
        if mode == "all":
            if c.depth is None:
                sample = ds.get_all()
                self._eval_cache_append(c, sample["depth"], sample["T"])
        elif want > c.asked:
            sample = ds[np.arange(c.asked, want)]
            self._eval_cache_append(c, sample["depth"], sample["T"])
            c.asked = want
        if c.depth is None:                      # no frame yet: the reference's empty batch (its rays_per_frame then divides by 0)
            return (torch.zeros(0, self.H, self.W, device=hip.device), torch.zeros(0, 4, 4, device=hip.device))
        held = c.held
        if (mode == "all" and upto is not None) or (mode != "all" and want < c.asked):
            # a prefix: the frames with an index below `want` (SceneCache.__getitem__ keeps those in keep_ixs, dataset.py:251-257)
            keep = getattr(ds, "keep_ixs", None)
            k = int(np.searchsorted(np.asarray(keep), want)) if keep is not None else min(want, len(ds))
            held = min(k, c.held)
        return c.depth[:held], c.T[:held]

    def _eval_cache_append(self, c, depth, T):
        """new frames -> the resident buffers (capacity grows by half, never beyond the dataset's length when it has one)"""
        dev = self._hip.device
        depth = torch.as_tensor(np.asarray(depth, np.float32))
        T = torch.as_tensor(np.asarray(T, np.float32)).reshape(-1, 4, 4)
        k = int(depth.shape[0])
        if k == 0:
            return
        need = c.held + k
        if c.depth is None or need > c.depth.shape[0]:
            cap = need if c.mode == "all" else max(need, (c.held * 3) // 2, 32)
            try:
                cap = max(need, min(cap, len(c.dataset)))
            except TypeError:
                pass
            nd = torch.empty((cap,) + tuple(depth.shape[1:]), dtype=torch.float32, device=dev)
            nT = torch.empty(cap, 4, 4, dtype=torch.float32, device=dev)
            if c.held:
                nd[:c.held].copy_(c.depth[:c.held]); nT[:c.held].copy_(c.T[:c.held])
            c.depth, c.T = nd, nT
        c.depth[c.held:need].copy_(depth)
        c.T[c.held:need].copy_(T)
        c.held = need
        c.uploaded_frames += k
        c.uploaded_bytes += depth.numel() * 4 + T.numel() * 4

    def drop_eval_cache(self):
        """release the resident evaluation frames and the ground-truth volume (the next evaluation uploads them again)"""
        self._hip.eval_cache = None
        self._hip.gt_volume = None

    def eval_sdf(self, samples=200000, visible_region=True):
        """The reference's dict (av_l1, binned_l1 [6], l1_chomp_costs [3]; trainer.py:1819-1866).  The points come from
        eval_sdf_visible (bound below) or the reference's own eval_sdf_volume; ground-truth interpolation, mask, L1, the six bins
        and the CHOMP differences are ONE isdf_sdf_metrics pass and one copy of 24 doubles -- no point leaves the device."""
        if visible_region:
            sdf, eval_pts = self.eval_sdf_visible(samples)
        else:
            sdf, eval_pts = self.eval_sdf_volume(samples)
        return sdf_metrics(self.engine, self._gt_volume(), eval_pts, sdf, exclude_zero_gt=True).as_dict()

    def eval_sdf_visible(self, samples=20000):
        """(sdf [n], eval_pts [n,3]) of one sample per ray over the cached sequence (trainer.py:1868-1905): the same
        sample_points call and the same noise_std=0 forward, so the generators advance as in the reference; the frames come
        from the resident cache (_eval_frames).  The reference's ScanNet line (`dist_behind_surf == 0`, a comparison) has no effect."""
        depth_batch, T_WC_batch = self._eval_frames()
        rays_per_frame = samples // depth_batch.shape[0]
        sample_pts = self.sample_points(depth_batch, T_WC_batch, n_rays=rays_per_frame, dist_behind_surf=self.dist_behind_surf,
                                        n_strat_samples=1, n_surf_samples=0)
        pc = sample_pts["pc"]
        with torch.set_grad_enabled(False):
            sdf = self.sdf_map(pc, noise_std=0)
        return sdf.flatten(), pc.squeeze()

    def eval_object_sdf(self, samples=10000):
        """Per object the mean |sdf - gt| in a box around it, NaN while it is not visible (trainer.py:1955-2008).  The visibility
        test is the reference's (100 random offsets per object against every resident frame, frustum.is_visible_torch's predicate)
        as ONE isdf_visible_points launch whose 100 x n_objects counts are copied back -- an engine without visible_points gets the
        reference's own function; per visible object one isdf_sdf_metrics call that keeps zero-valued ground truth; the records
        come back in one copy."""
        errors = None
        if self.obj_bounds_file is not None:
            ref = self._hip.ref_module
            obj_bounds = ref.metrics.get_obj_eval_bounds(self.obj_bounds_file, self.up_ix)
            obj_bounds = torch.FloatTensor(obj_bounds).to(self.device)
            offsets = torch.rand(100, 3).to(self.device)
            extents = obj_bounds[:, 1] - obj_bounds[:, 0]
            pts = obj_bounds[:, 0] + offsets[:, None] * extents
            depth_batch, T_WC_batch = self._eval_frames()
            if getattr(self.engine, "visible_points", None) is not None:
                # one launch over the resident frames; the 100 x n_objects counts are all that comes back
                count, _, _ = visible_points(self.engine, pts.view(-1, 3), T_WC_batch, depth_batch, self, trunc=0.05)
                visible = count.cpu().numpy() > 0
            else:                                # an engine without the kernel: the reference's eager chain and its [F, N] mask
                visible = ref.geometry.frustum.is_visible_torch(pts.view(-1, 3), T_WC_batch, depth_batch, self.H, self.W, self.fx,
                                                                self.fy, self.cx, self.cy, trunc=0.05)
                visible = visible.detach().cpu().numpy().sum(axis=0) > 0
            visible = visible.reshape(100, len(obj_bounds))
            visible = visible.sum(axis=0) / 100 > 0.5
            vol, records = self._gt_volume(), []
            for i in range(len(obj_bounds)):
                if visible[i]:
                    offsets = torch.rand(samples, 3).to(self.device)
                    bounds = obj_bounds[i]
                    pts = bounds[0] + offsets * (bounds[1] - bounds[0])[None, :]
                    with torch.set_grad_enabled(False):
                        sdf = torch.squeeze(self.sdf_map(pts))
                    records.append(self.engine.sdf_metrics(vol, pts, sdf, exclude_zero_gt=False)[0])
            host = torch.stack(records).cpu().numpy() if records else np.zeros((0, _ffi.METRICS_RECORD))
            errors, k = [], 0
            for i in range(len(obj_bounds)):
                if visible[i]:
                    with np.errstate(divide="ignore", invalid="ignore"):
                        errors.append(np.float64(host[k, 2]) / np.float64(host[k, 0]))
                    k += 1
                else:
                    errors.append(np.nan)
        return errors

    def eval_traj_cost(self, t_ahead=5.):
        """(pred_chomp_costs [3], gt_chomp_costs [3]) summed along the next t_ahead seconds of the trajectory, or (nan, nan) when
        fewer than 90 % of its points have a valid non-zero ground truth or the section is shorter than 30 poses
        (trainer.py:2010-2052).  Network forward, then one isdf_sdf_metrics call: the validity count and both sets of sums
        are fields of its record."""
        if self.traj_file:
            traj = np.loadtxt(self.traj_file)
            traj_start_ix = self.tot_step_time * 30
            traj_end_ix = min(len(traj) - 1, (self.tot_step_time + t_ahead) * 30)
            traj_section = traj[int(traj_start_ix): int(traj_end_ix)]
            if len(traj_section) < 30:
                return np.nan, np.nan
            eval_pts = torch.from_numpy(np.ascontiguousarray(traj_section[:, [3, 7, 11]]))
            with torch.set_grad_enabled(False):
                sdf = self.sdf_map(eval_pts.float().to(self.device)).squeeze()
            m = sdf_metrics(self.engine, self._gt_volume(), eval_pts, sdf, exclude_zero_gt=True)
            if m.n_valid < 0.9 * len(traj_section):
                return np.nan, np.nan
            return m.pred_chomp_sums, m.gt_chomp_sums

    def eval_mesh(self, samples=200000):
        """(accuracy, completion) of the reconstructed mesh against the ground-truth scene mesh (trainer.py:2054-2064,
        metrics.py:62-73): mesh_rec() and the two trimesh surface samplings are the reference's; the two nearest-neighbour
        passes run on the device (isdf_nn_distance) instead of two host KD-trees."""
        ref = self._ref("eval_mesh", "trimesh")
        mesh_gt = ref.trimesh.load(self.scene_file)
        sdf_mesh = self.mesh_rec()
        rec_pc = ref.trimesh.sample.sample_surface(sdf_mesh, samples)
        gt_pc = ref.trimesh.sample.sample_surface(mesh_gt, samples)
        return accuracy_completion(self.engine, gt_pc[0], rec_pc[0])

    # ------------------------------------------------------------------ fixed-point evaluation (trainer.py:2080-2088)
    @staticmethod
    def _region_flags(valid_gt_sdf, valid_vox_sdf, valid_gt_grad=None):
        """flag byte per drawn point (_ffi.FLAG_*) from the mask files of one point set, eval_pts.py:130-152 written out:
        A = valid_gt_sdf [N] selects the vis sdf set, valid_vox_sdf [A.sum()] the vox subset of it; G = valid_gt_grad [N] the vis
        gradient set, and the vox gradient set is A & B & G with B scattered back to the N points."""
        A = np.asarray(valid_gt_sdf, bool).reshape(-1)
        B = np.zeros(A.shape[0], bool)
        B[A] = np.asarray(valid_vox_sdf, bool).reshape(-1)
        flags = A * np.uint8(_ffi.FLAG_VIS_SDF) + (A & B) * np.uint8(_ffi.FLAG_VOX_SDF)
        if valid_gt_grad is not None:
            G = np.asarray(valid_gt_grad, bool).reshape(-1)
            flags = flags + G * np.uint8(_ffi.FLAG_VIS_GRAD) + (A & B & G) * np.uint8(_ffi.FLAG_VOX_GRAD)
        return flags.astype(np.uint8)

    def eval_fixed(self):
        """The reference's nested dict (eval_pts.fixed_pts_eval, eval_pts.py:96-299) at the next timestamp of `self.eval_times`.
        Frames from the resident cache; the pixels and the one stratified draw on the torch CPU generator exactly as
        eval_pts.sample_rays draws them (the mask files are aligned index for index with these draws), whatever graft(rng=...)
        says; ONE sampler launch gives both point sets (column 0 of pc: sample_surface's, column 1: sample_visible_region's); one
        forward-with-gradient launch for the visible region, one forward for surface, objects and volume together; one
        isdf_region_metrics pass per leg into one records tensor, ONE copy back.  Two host synchronisations: the sampler's
        n_valid and that copy.  The Philox counter does not advance; afterwards the torch CPU generator and numpy's global one are
        where the reference leaves them.  Deviations: the visible region's sdf comes from the gradient-returning
        kernel; a mask-selected point outside the ground-truth grid is left out (the reference averages its 1e99 fill value in)
        with one warning; the object points are rounded to fp32 before the ground-truth lookup."""
        if self.dataset_format not in ("replicaCAD", "ScanNet"):       # the reference's own method (it fails there too)
            return super().eval_fixed()
        t = self.eval_times.pop(0)
        t_str = f"{t:.3f}"
        masks_dir = self.eval_pts_dir + t_str
        m = self._fixed_masks(masks_dir)
        eng, dev = self.engine, self._hip.device
        depth_batch, T_WC_batch = self._eval_frames(int(min(np.floor(t * 30), len(self.scene_dataset))))
        R, surf_pts, vis_pts = self._fixed_draws(t_str, depth_batch, T_WC_batch)
        sizes = (m["vis_valid_gt_sdf"].shape[0], m["vis_valid_gt_grad"].shape[0], m["surf_valid_gt_sdf"].shape[0])
        if sizes != (R, R, R):
            raise IndexError("eval_fixed: the mask files of %s hold %d / %d / %d entries for %d drawn points"
                             % ((masks_dir,) + sizes + (R,)))
        vis_flags = self._region_flags(m["vis_valid_gt_sdf"], m["vis_valid_vox_sdf"], m["vis_valid_gt_grad"])
        surf_flags = self._region_flags(m["surf_valid_gt_sdf"], m["surf_valid_vox_sdf"])
        obj_legs = self._fixed_object_legs(os.path.join(self.eval_pts_dir, t_str), masks_dir)
        vol_pts, vol_gt = self._fixed_volume_files()
        legs = obj_legs or []

        # network: one forward-with-gradient launch (visible region), one forward launch for everything else
        vis_sdf, vis_grad = eng.sdf_eval(vis_pts, want_grad=True)
        parts = [surf_pts] + [p.to(dev) for p, _ in legs] + [vol_pts.to(dev)]
        rest_pts = torch.cat(parts)
        rest_sdf = eng.sdf_eval(rest_pts)
        bounds_ix = np.cumsum([0] + [int(p.shape[0]) for p in parts])

        # metrics: one isdf_region_metrics call per leg into one records tensor, one copy back
        vol = self._gt_volume()
        records = torch.empty(3 + len(legs), 2, _ffi.REGION_RECORD, dtype=torch.float64, device=dev)
        eng.region_metrics(vis_pts, vis_sdf, volume=vol, sdf_grad=vis_grad, flags=torch.from_numpy(vis_flags), delta=0.01,
                           out=records[0])
        eng.region_metrics(surf_pts, rest_sdf[:R], volume=vol, flags=torch.from_numpy(surf_flags), out=records[1])
        selected = [[int((vis_flags & 1).sum()), int(((vis_flags >> 1) & 1).sum())],
                    [int((surf_flags & 1).sum()), int(((surf_flags >> 1) & 1).sum())]]
        for k, (p, fl) in enumerate(legs):
            a, b = bounds_ix[1 + k], bounds_ix[2 + k]
            eng.region_metrics(rest_pts[a:b], rest_sdf[a:b], volume=vol, flags=fl, out=records[2 + k])
            selected.append([int(p.shape[0]), int(((fl.numpy() >> 1) & 1).sum())])
        eng.region_metrics(rest_pts[bounds_ix[-2]:], rest_sdf[bounds_ix[-2]:], gt=vol_gt, out=records[2 + len(legs)])
        host = records.cpu().numpy()                                             # host synchronisation 2 of 2

        n_out = int(sum(sel[j] - host[k, j, 0] for k, sel in enumerate(selected) for j in (0, 1)))
        if n_out:
            warnings.warn("eval_fixed(t=%s): the mask files select %d points outside the ground-truth grid; they are left out "
                          "(the reference averages its 1e99 fill value into the result)" % (t_str, n_out))
        return self._fixed_result(t, host, len(legs), obj_legs is not None)

    @staticmethod
    def _fixed_masks(masks_dir):
        """the six mask files of one timestamp by name, read in the reference's order, with its three size checks"""
        m = {k: np.load(masks_dir + "/%s.npy" % k)
             for k in ("surf_valid_gt_sdf", "surf_valid_vox_sdf", "vis_valid_gt_sdf", "vis_valid_vox_sdf", "vis_valid_gt_grad",
                       "vis_valid_vox_grad")}
        assert m["surf_valid_gt_sdf"].sum() == m["surf_valid_vox_sdf"].shape[0]
        assert m["vis_valid_gt_sdf"].sum() == m["vis_valid_vox_sdf"].shape[0]
        assert m["vis_valid_gt_grad"].sum() == m["vis_valid_vox_grad"].shape[0]
        return m

    def _fixed_draws(self, t_str, depth_batch, T_WC_batch):
        """(R, surf_pts [R, 3], vis_pts [R, 3]): eval_pts.sample_rays' draws (eval_pts.py:354-393: seed, randint h, randint w,
        rand(n_valid, 1)) on the torch CPU generator and the one sampler launch over them"""
        dev = self._hip.device
        F, H, W = (int(v) for v in depth_batch.shape)
        torch.manual_seed(float(t_str) * 1e3)
        rays_per_frame = 200000 // F
        ih = torch.randint(0, H, (rays_per_frame * F,))
        iw = torch.randint(0, W, (rays_per_frame * F,))
        after_pixels = torch.get_rng_state()      # where sample_surface, the reference's last seeded call, leaves the generator
        ih_d, iw_d = ih.to(dev), iw.to(dev)
        ib_d = torch.arange(F, device=dev).repeat_interleave(rays_per_frame)
        R = int((depth_batch[ib_d, ih_d, iw_d] != 0).sum().item())           # host synchronisation 1 of 2
        U = torch.rand(R, 1)
        torch.set_rng_state(after_pixels)
        sc = self._sample_cfg(n_rays=rays_per_frame, dist_behind_surf=0. if self.dataset_format == "ScanNet" else 0.1,
                              n_strat=1, n_surf=1)
        sc.min_depth, sc.H, sc.W = 0.1, H, W
        s = self.engine.sample(depth_batch.contiguous(), T_WC_batch.contiguous(), None,
                               torch.arange(F, dtype=torch.int32, device=dev), None, sc,
                               draws=dict(indices_h=ih_d, indices_w=iw_d, U=U, N_off=torch.zeros(R, 0)), want_T=False)
        pc = s["pc"][:R]
        return R, pc[:, 0], pc[:, 1]

    def _fixed_object_legs(self, pts_dir, masks_dir):
        """[(points [n, 3] f32, flags [n] u8)] per object box that has files at this timestamp (eval_pts.py:204-258: 10000 seeded
        points per box), or None without an obj_bounds.txt"""
        obj_bounds_file = self.seq_dir + '/obj_bounds.txt'
        if not os.path.exists(obj_bounds_file):
            return None
        obj_bounds = np.loadtxt(obj_bounds_file).reshape(-1, 2, 3)          # eval_pts.load_obj_bounds
        obj_bounds[:, 1] += 0.08
        obj_bounds[:, 0, 0] -= 0.08
        obj_bounds[:, 0, 2] -= 0.08
        obj_legs = []
        listing = os.listdir(pts_dir)
        for i, bounds in enumerate(obj_bounds):
            if len([x for x in listing if f'obj{i}' in x]) == 0:
                continue
            valid_gt_sdf = np.load(masks_dir + f"/obj{i}_valid_gt_sdf.npy")
            valid_vox_sdf = np.load(masks_dir + f"/obj{i}_valid_vox_sdf.npy")
            np.random.seed(0)                                                # eval_pts.object_eval_pts
            offsets = np.random.rand(10000, 3)
            pts = (bounds[0] + offsets * (bounds[1] - bounds[0])[None, :])[valid_gt_sdf]
            fl = np.uint8(_ffi.FLAG_VIS_SDF) + np.asarray(valid_vox_sdf, bool) * np.uint8(_ffi.FLAG_VOX_SDF)
            obj_legs.append((torch.from_numpy(pts.astype(np.float32)), torch.from_numpy(fl.astype(np.uint8))))
        return obj_legs

    def _fixed_volume_files(self):
        """(points [n, 3] f32, ground truth [n] f64) of the full-volume leg (eval_pts.py:260-297), on the host"""
        seq = [x for x in self.seq_dir.split('/') if x != ""][-1]
        name = "replicaCAD" if self.dataset_format == "replicaCAD" else seq
        vol_pts = np.load(self.eval_pts_root + f"full_vol/{name}.npy").astype(np.float32)
        vol_gt = np.load(self.eval_pts_root + f"full_vol/gt_{seq}.npy").astype(np.float64)
        return torch.from_numpy(vol_pts).reshape(-1, 3), torch.from_numpy(vol_gt).reshape(-1)

    @staticmethod
    def _fixed_result(t, host, n_obj, with_objects):
        """the reference's nested dict from the records [3 + n_obj, 2, REGION_RECORD]: rays, visible_surf, objects.., vol"""
        pair = lambda k, **kw: {"vis": RegionMetrics(host[k, 0]).as_dict(**kw), "vox": RegionMetrics(host[k, 1]).as_dict(**kw)}
        res = {"time": t, "rays": pair(0, cossim=True), "visible_surf": pair(1)}
        if with_objects:
            res["objects"] = [{"vis": {"av_l1": RegionMetrics(host[2 + k, 0]).sdf.av_l1},
                               "vox": {"av_l1": RegionMetrics(host[2 + k, 1]).sdf.av_l1}} for k in range(n_obj)]
        res["vol"] = RegionMetrics(host[2 + n_obj, 0]).as_dict()
        return res
