"""SDF slice images on the device (include/isdf_hip.h: isdf_slice_images, isdf_plane_points).

    Colormap       a colour table with its under / over / bad colours and limits: what a matplotlib ScalarMappable holds
                   (sdf_util.get_colormap, sdf_util.py:276-299), packed for the kernel; matplotlib is never imported
    slice_images   the network on the points, then colours, ground truth and CHOMP cost fields of Trainer.compute_slices /
                   obj_slices_vis (trainer.py:1590-1639,1795-1807): ONE forward launch and one isdf_slice_images pass
    plane          the same on the points of a plane raster generated on the device

`engine` is an isdf_amd.engine.Engine (or anything with its sdf_eval / slice_images / plane_points methods).
"""
import numpy as np
import torch

from . import _ffi
from .engine import to_host


def _rgb_bytes(c):
    """colours as matplotlib's users make them bytes: (rgba * 255).astype(np.uint8)[..., :3] of floats in [0, 1]; uint8 is taken
    as it is"""
    c = np.asarray(c)
    if c.dtype != np.uint8:
        c = (np.asarray(c, np.float64) * 255).astype(np.uint8)
    return c[..., :3]


class Colormap:
    """table [N, 3 or 4] and the three colours outside it (floats in [0, 1] or uint8), and the limits of the linear norm:
    the colour of v is table[int((v - vmin) / (vmax - vmin) * N)], `under` below vmin, `over` above vmax, `bad` for NaN,
    table[N - 1] at vmax itself -- evaluated in float32 as matplotlib does on a float32 array."""

    def __init__(self, table, under, over, bad, vmin, vmax):
        t = _rgb_bytes(table).reshape(-1, 3)
        n = int(t.shape[0])
        if n < 1 or n > _ffi.COLORMAP_MAX_COLORS:
            raise ValueError("Colormap: 1 .. %d colours are supported (got %d)" % (_ffi.COLORMAP_MAX_COLORS, n))
        self.n_colors = n
        self.vmin, self.vmax = float(vmin), float(vmax)
        self.vmin32, self.range32 = np.float32(self.vmin), np.float32(self.vmax - self.vmin)
        if not (np.isfinite(self.vmin32) and np.isfinite(self.range32) and self.range32 > 0):
            raise ValueError("Colormap: vmin < vmax, both finite, are needed (got %r, %r)" % (vmin, vmax))
        rgb = np.concatenate([t] + [_rgb_bytes(c).reshape(1, 3) for c in (under, over, bad)]).astype(np.uint32)
        self.rgb = rgb.astype(np.uint8)                                         # [N + 3, 3]: the table, under, over, bad
        self.lut = (rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16)).astype(np.uint32)
        self._dev = {}

    @classmethod
    def from_scalar_mappable(cls, m):
        """From anything with matplotlib's ScalarMappable attributes: `m.cmap.N`, `m.cmap(indices)`, `m.cmap.get_under() /
        get_over() / get_bad()` and `m.norm.vmin / vmax` (a linear Normalize); nothing else is read."""
        n = int(m.cmap.N)
        table = np.asarray(m.cmap(np.arange(n)))
        return cls(table, m.cmap.get_under(), m.cmap.get_over(), m.cmap.get_bad(), m.norm.vmin, m.norm.vmax)

    def key(self):
        return (self.n_colors, self.vmin, self.vmax, self.lut.tobytes())

    def to_c(self, device):
        """isdf_colormap with the table on `device` (uploaded once per device and kept)"""
        device = torch.device(device)
        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = torch.from_numpy(self.lut.view(np.int32).copy()).to(device)
        a = _ffi.ColormapArgs()
        a.lut, a.n_colors, a.vmin, a.range = t.data_ptr(), self.n_colors, float(self.vmin32), float(self.range32)
        return a


class SliceImages:
    """device tensors with the leading shape of the points: sdf (fp32), pred_rgb (uint8 [..., 3]) and, where asked for, gt (fp32),
    gt_rgb (uint8 [..., 3]), pred_cost / gt_cost (fp32); `pts` where the points were generated"""

    def __init__(self, sdf, pred_rgb, gt, gt_rgb, pred_cost, gt_cost, pts=None):
        self.sdf, self.pred_rgb, self.gt, self.gt_rgb = sdf, pred_rgb, gt, gt_rgb
        self.pred_cost, self.gt_cost, self.pts = pred_cost, gt_cost, pts


def slice_images(engine, pts, cmap, gt_volume=None, chomp_eps=None, oob_fill=0.0):
    """SliceImages of pts [..., 3]: ONE engine.sdf_eval over all of them (however many slices they make), then one
    isdf_slice_images pass for the colours of the prediction and, with `gt_volume` (isdf_amd.metrics.GtVolume), the ground truth
    (`oob_fill` outside the volume) and its colours; with `chomp_eps` the CHOMP cost of both.  Nothing is copied to the host."""
    shp = tuple(pts.shape[:-1])
    with torch.no_grad():
        sdf = engine.sdf_eval(pts)
        pred_rgb, gt, gt_rgb, pred_cost, gt_cost = engine.slice_images(pts, sdf, cmap, gt_volume, chomp_eps, oob_fill)

    def view(t, *tail):
        return None if t is None else t.view(*shp, *tail)
    return SliceImages(sdf.view(*shp), view(pred_rgb, 3), view(gt), view(gt_rgb, 3), view(pred_cost), view(gt_cost))


def plane(engine, origin, du, dv, H, W, cmap, gt_volume=None, chomp_eps=None, oob_fill=0.0):
    """slice_images on the H x W raster p[i][j] = (origin + i * du) + j * dv, generated on the device (isdf_plane_points): a slice
    on any plane at any resolution, without a grid of points to select from.  The result carries the points as `.pts`."""
    pts = engine.plane_points(origin, du, dv, H, W)
    out = slice_images(engine, pts, cmap, gt_volume, chomp_eps, oob_fill)
    out.pts = pts
    return out


class SliceMethods:
    """The trainer-level half (trainer.py:1446-1481,1558-1815): a base class of hot_path.HotPath; `self` is the grafted Trainer."""

    def _slice_colormap(self, mappable):
        """the reference's ScalarMappable as an isdf_amd.slices.Colormap, made (and uploaded) once per distinct table"""
        cm = Colormap.from_scalar_mappable(mappable)
        return self._hip.slice_cmaps.setdefault(cm.key(), cm)

    def compute_slices(self, z_ixs=None, n_slices=6, include_gt=False, include_diff=False, include_chomp=False,
                       draw_cams=False, sdf_range=[-2, 2]):
        """The reference's dict of lists of uint8 images (pred_sdf, and gt_sdf / pred_cost / gt_cost / diff where asked for;
        trainer.py:1558-1707).  The slices are selected from grid_pc on the device as the reference selects them; ONE forward
        launch over all of them and ONE isdf_slice_images pass give the colours of the prediction and of the ground truth (the
        device copy of gt_sdf_interp's grid, fill 0 outside it) and both CHOMP cost fields; one copy to the host.  The colour map
        is the reference module's own sdf_util.get_colormap (which edits `sdf_range` in place, as there); cv2.resize,
        imgviz.depth2rgb and the camera markers are the reference module's own calls on the host.  `diff` is the all-white image
        the reference returns (it discards the difference it computes, trainer.py:1647-1671): nothing is computed for it."""
        ref = self._ref("compute_slices", "sdf_util", "sdf_util.get_colormap, cv2, imgviz")
        if z_ixs is None:
            z_ixs = torch.linspace(30, self.grid_dim - 30, n_slices)
            z_ixs = torch.round(z_ixs).long()
        z_ixs = z_ixs.to(self.device)
        pc = self.grid_pc.reshape(self.grid_dim, self.grid_dim, self.grid_dim, 3)
        pc = torch.index_select(pc, self.up_ix, z_ixs)
        if not self.up_aligned:
            indices = np.arange(len(z_ixs))[::-1]
            indices = torch.from_numpy(indices.copy()).to(self.device)
            pc = torch.index_select(pc, self.up_ix, indices)
        cmap = self._slice_colormap(ref.sdf_util.get_colormap(sdf_range=sdf_range))
        grid_shape = tuple(pc.shape[:-1])
        n_slices = grid_shape[self.up_ix]
        scales = torch.cat([self.scene_scale[:self.up_ix], self.scene_scale[self.up_ix + 1:]])
        im_size = 256 * scales / scales.min()
        im_size = im_size.int().cpu().numpy()

        res = slice_images(self.engine, pc, cmap, gt_volume=self._gt_volume() if include_gt else None,
                              chomp_eps=2. if include_chomp else None, oob_fill=0.)
        pred_rgb, gt_rgb, pred_cost, gt_cost = to_host(res.pred_rgb, res.gt_rgb, res.pred_cost, res.gt_cost)

        def resized(viz):
            return [ref.cv2.resize(np.take(viz, i, self.up_ix), im_size[::-1]) for i in range(n_slices)]

        def cost_images(cost):
            viz = ref.imgviz.depth2rgb(cost.reshape(self.grid_dim, -1), min_value=0., max_value=1.5)
            return resized(viz.reshape(*grid_shape, 3))
        slices = {"pred_sdf": resized(pred_rgb)}
        if include_chomp:
            slices["pred_cost"] = cost_images(pred_cost)
        if include_gt:
            slices["gt_sdf"] = resized(gt_rgb)
            if include_chomp:
                slices["gt_cost"] = cost_images(gt_cost.astype(np.float64))      # the reference's ground truth is float64
        if include_diff:
            if not include_gt:       # the reference reads its gt_sdf here, which only include_gt assigns (trainer.py:1643)
                raise UnboundLocalError("local variable 'gt_sdf' referenced before assignment")
            slices["diff"] = resized(np.full(grid_shape + (3,), 255, dtype=np.uint8))

        if draw_cams:       # the reference's markers (trainer.py:1673-1705), its own draw / cv2 calls
            cam_xyz = self.frames.T_WC_batch[:, :3, 3].cpu()
            cam_td = self.to_topdown(cam_xyz, im_size)
            cam_rots = self.frames.T_WC_batch[:, :3, :3].cpu().numpy()
            angs = [np.arctan2(rot[0, 2], rot[0, 0]) for rot in cam_rots]
            for i, im in enumerate(slices["pred_sdf"]):
                if self.incremental:
                    trajectory_gt = self.frames.T_WC_batch_np[:, :3, 3]
                    if self.frames.T_WC_gt is not None:
                        trajectory_gt = self.frames.T_WC_gt[:, :3, 3]
                    traj_td = self.to_topdown(trajectory_gt, im_size)
                    for j in range(len(traj_td) - 1):
                        if not (traj_td[j] == traj_td[j + 1]).all():
                            im = im.astype(np.uint8) / 255
                            im = ref.cv2.line(im, traj_td[j][::-1], traj_td[j + 1][::-1], [1., 0., 0.], 2)
                            im = (im * 255).astype(np.uint8)
                for (p, ang) in zip(cam_td, angs):
                    ref.draw.draw_agent(im, p, agent_rotation=ang, agent_radius_px=12)
                slices["pred_sdf"][i] = im
        return slices

    def obj_slices_vis(self, n_slices=6):
        """The reference's stacked image (per object the predicted slices over the ground-truth ones), or None without an
        obj_bounds_file (trainer.py:1775-1815): per object the reference's own 256 x n_slices x 256 points, one forward launch
        and one isdf_slice_images pass (colours of both, map [-0.5, 0.5]); the two images come back in one copy."""
        if self.obj_bounds_file is None:
            return None
        ref = self._ref("obj_slices_vis", "sdf_util", "sdf_util.get_colormap, metrics")
        up_ix = 1
        obj_bounds = ref.metrics.get_obj_eval_bounds(self.obj_bounds_file, up_ix)
        cmap = self._slice_colormap(ref.sdf_util.get_colormap(sdf_range=[-0.5, 0.5]))
        vol = self._gt_volume()
        all_slices = []
        for bounds in obj_bounds:
            dims = [256, 256, 256]
            dims[up_ix] = n_slices
            x = torch.linspace(bounds[0, 0], bounds[1, 0], dims[0])
            y = torch.linspace(bounds[0, 1], bounds[1, 1], dims[1])
            z = torch.linspace(bounds[0, 2], bounds[1, 2], dims[2])
            xx, yy, zz = torch.meshgrid(x, y, z, indexing="ij")
            pc = torch.cat((xx[..., None], yy[..., None], zz[..., None]), dim=3).to(self.device)
            res = slice_images(self.engine, pc, cmap, gt_volume=vol, oob_fill=0.)
            col, gt_col = to_host(res.pred_rgb, res.gt_rgb)
            col = np.hstack([col[:, i] for i in range(n_slices)])
            gt_col = np.hstack([gt_col[:, i] for i in range(n_slices)])
            all_slices.append(np.vstack((col, gt_col)))
        return np.vstack((all_slices))

    def get_sdf_grid_pc(self, include_gt=False, mask_near_pc=False):
        """(sdf_grid_pc, keep_mask) of the reference (trainer.py:1446-1481): grid_pc with the network's value as a float32
        [d, d, d, 4] array -- with include_gt (and a ground-truth grid) float64 [d, d, d, 5], the last column the ground truth with
        0 outside its volume, from the device lookup --, and with mask_near_pc the boolean [.., .., ..] mask of the grid points
        whose every-tenth representative lies within crop_dist of the keyframes' point cloud (Engine.nn_distance instead of a
        host KD-tree), repeated as the reference repeats it; else None.  One forward launch, one copy to the host."""
        d = self.grid_dim
        sdf_grid = self.get_sdf_grid()
        grid_pc = self.grid_pc.reshape(d, d, d, 3)
        sdf_grid_pc = torch.cat((grid_pc, sdf_grid[..., None]), dim=-1)
        with_gt = include_gt and self.gt_sdf_interp is not None
        if with_gt:
            gt = self.engine.slice_images(self.grid_pc, None, None, self._gt_volume(), None, oob_fill=0.)[1]
            sdf_grid_pc = torch.cat((sdf_grid_pc, gt.view(d, d, d, 1)), dim=-1)
            self.gt_sdf_interp.fill_value = 0.0           # the state the reference leaves its interpolator in (trainer.py:1454-1461)
            self.gt_sdf_interp.bounds_error = True
        near = None
        if mask_near_pc:
            pc = np.ascontiguousarray(self._vis_pointcloud(), dtype=np.float32)
            sparse = sdf_grid_pc[::10, ::10, ::10, :3]
            dist, _, _ = self.engine.nn_distance(sparse.reshape(-1, 3), torch.from_numpy(pc).reshape(-1, 3).to(self.device))
            near = (dist.double() < self.crop_dist).view(sparse.shape[:-1])
        sdf_grid_pc, keep_mask = to_host(sdf_grid_pc.detach(), near)
        if with_gt:
            sdf_grid_pc = sdf_grid_pc.astype(np.float64)
        if keep_mask is not None:
            keep_mask = keep_mask.repeat(10, axis=0).repeat(10, axis=1).repeat(10, axis=2)
        return sdf_grid_pc, keep_mask
