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
