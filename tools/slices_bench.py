#!/usr/bin/env python3
"""Slice timing on the trained default net (fixture `trained_default`) and a ground-truth volume sampled from
isdf_amd.synthetic.gt_sdf at 0.03 m: the route Trainer.compute_slices(include_gt=True) and Trainer.get_sdf_grid_pc(include_gt=True)
took around SDFMapHIP before they were bound (restated from trainer.py:1558-1626 and 1446-1461 -- chunks of 100 000 points through
the network, the field to the host, the colour map on the host (matplotlib's ScalarMappable if it imports, else the numpy model of
tests/slice_model.py), the points to the host, linear interpolation on the host (scipy's RegularGridInterpolator if it imports,
else the numpy model of tests/eval_model.py) and its colours) against the bound route (one forward launch, ONE isdf_slice_images
pass, one copy back).  cv2.resize is left out of both routes (the same host call on the same slabs either way).  The two routes
alternate within one process; device-synchronised wall time per call, medians over --reps.

    python tools/slices_bench.py [--reps 7] [--out profiles/slices_bench.json]"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from isdf_amd import modules, synthetic       # noqa: E402
from tests import eval_model as em             # noqa: E402
from tests import golden_util as gu            # noqa: E402
from tests import slice_model as sm            # noqa: E402

SPACING = 0.03
CHUNK = 100000          # trainer.py:63


class ModelMappable:
    """to_rgba by the numpy model, for hosts without matplotlib (a float table lookup, as matplotlib's)"""

    def __init__(self, rgb, vmin, vmax):
        self.rgb, self.vmin, self.vmax = rgb, vmin, vmax
        self.rgba = np.concatenate([np.minimum(rgb.astype(np.float64) / 255 + 1e-4, 1.0), np.ones((len(rgb), 1))], 1)

    def to_rgba(self, v, alpha=1., bytes=False):
        return self.rgba[sm.colour_index(np.asarray(v, np.float32), len(self.rgb) - 3, self.vmin, self.vmax)]


def host_colormap(g):
    """(ScalarMappable-like for the pre-change route, its name, the mappable graft() converts)"""
    rgb, lim = g["t2/rgb"], g["t2/lim"]
    duck = sm.TableMappable(rgb, lim[0], lim[1])
    try:
        from matplotlib import cm, colors
        table = np.concatenate([np.minimum(rgb[:-3] / 255 + 1e-4, 1.0), np.ones((len(rgb) - 3, 1))], 1)
        cmap = colors.ListedColormap(table)
        return cm.ScalarMappable(norm=colors.Normalize(lim[0], lim[1]), cmap=cmap), "matplotlib ScalarMappable.to_rgba", duck
    except ImportError:
        return ModelMappable(rgb, lim[0], lim[1]), "numpy colour model (matplotlib is not installed)", duck


def host_interpolator(ax, values):
    try:
        from scipy.interpolate import RegularGridInterpolator
        itp = RegularGridInterpolator(ax, values.astype(np.float64), bounds_error=False, fill_value=0.0)
        return (lambda p: itp(p)), "scipy RegularGridInterpolator (float64)"
    except ImportError:
        h, o = [a[1] - a[0] for a in ax], [a[0] for a in ax]
        return (lambda p: em.trilinear(values, h, o, p)[0].reshape(np.asarray(p).shape[:-1])), "numpy trilinear model (float64)"


def eager_compute_slices(tr, cmap, interp, n_slices):
    """trainer.py:1563-1626 with include_gt, as it ran around SDFMapHIP (cv2.resize left out)"""
    z_ixs = torch.round(torch.linspace(30, tr.grid_dim - 30, n_slices)).long().to(tr.device)
    pc = tr.grid_pc.reshape(tr.grid_dim, tr.grid_dim, tr.grid_dim, 3)
    pc = torch.index_select(pc, tr.up_ix, z_ixs)
    grid_shape = pc.shape[:-1]
    pc = pc.reshape(-1, 3)
    scales = torch.cat([tr.scene_scale[:tr.up_ix], tr.scene_scale[tr.up_ix + 1:]])
    im_size = (256 * scales / scales.min()).int().cpu().numpy()
    with torch.set_grad_enabled(False):
        sdf = modules.chunks(pc, CHUNK, tr.sdf_map)
        sdf = sdf.detach().cpu().numpy()
    sdf_viz = cmap.to_rgba(sdf.flatten(), alpha=1., bytes=False)
    sdf_viz = (sdf_viz * 255).astype(np.uint8)[..., :3].reshape(*grid_shape, 3)
    out = {"pred_sdf": [np.take(sdf_viz, i, tr.up_ix) for i in range(n_slices)]}
    pc = pc.reshape(*grid_shape, 3).detach().cpu().numpy()
    gt_sdf = interp(pc.reshape(-1, 3)).reshape(grid_shape)
    gt_viz = cmap.to_rgba(gt_sdf.flatten(), alpha=1., bytes=False).reshape(*grid_shape, 4)
    gt_viz = (gt_viz * 255).astype(np.uint8)[..., :3]
    out["gt_sdf"] = [np.take(gt_viz, i, tr.up_ix) for i in range(n_slices)]
    return out, im_size


def eager_get_sdf_grid_pc(tr, interp):
    """trainer.py:1426-1461 with include_gt, as it ran around SDFMapHIP"""
    d = tr.grid_dim
    with torch.set_grad_enabled(False):
        sdf_grid = modules.chunks(tr.grid_pc, CHUNK, tr.sdf_map).view(d, d, d)
    grid_pc = tr.grid_pc.reshape(d, d, d, 3)
    sdf_grid_pc = torch.cat((grid_pc, sdf_grid[..., None]), dim=-1).detach().cpu().numpy()
    gt_sdf = interp(tr.grid_pc.cpu().numpy()).reshape(d, d, d)
    return np.concatenate((sdf_grid_pc, gt_sdf[..., None]), axis=-1)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def alternate(fa, fb, reps):
    fa(); fb()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(fa)[0]); tb.append(timed(fb)[0])
    return float(np.median(ta)), float(np.median(tb))


def count_launches(fn):
    """kernel launches of one call (torch profiler, device activity)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as p:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in p.events() if e.device_type.name == "CUDA" and "Memcpy" not in e.name and "Memset" not in e.name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--grids", type=int, nargs="+", default=[200, 256])
    a = ap.parse_args()
    from bench_support.standin_trainer import HipTrainer
    from tests.accuracy_experiment import config
    g, t = sm.load_golden(), gu.load("trained_default")
    cam = dict(H=96, W=128, fx=100.0, fy=100.0, cx=63.5, cy=47.5)
    tr = HipTrainer("cuda", config(cam), inv_bounds_transform=synthetic.bounds_transform(), rng="philox", seed=1)
    tr.sdf_map.load_state_dict({k: torch.from_numpy(v) for k, v in gu.params_of(t).items()})
    sm.set_slice_geometry(tr, "A", "cuda")

    lo = synthetic.ROOM_LO - 0.3
    dims = tuple(int(round((hi - l) / SPACING)) + 1 for l, hi in zip(lo, synthetic.ROOM_HI + 0.3))
    ax = [np.arange(n) * SPACING + l for n, l in zip(dims, lo)]
    values = synthetic.gt_sdf(np.stack(np.meshgrid(*ax, indexing="ij"), -1)).astype(np.float32)
    tr.gt_sdf_interp = sm.GridInterp(values, [SPACING] * 3, lo)
    interp, interp_name = host_interpolator(ax, values)
    cmap, cmap_name, duck = host_colormap(g)
    tr._hip.ref_module = types.SimpleNamespace(sdf_util=types.SimpleNamespace(get_colormap=lambda sdf_range: duck),
                                               cv2=types.SimpleNamespace(resize=lambda img, dsize: img))
    rgb = g["t2/rgb"]
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, timing="device-synchronised wall time per call, median; the two "
               "routes alternate in one process; cv2.resize left out of both", host_colour_map=cmap_name,
               host_interpolation=interp_name, volume=list(dims), cases={})
    for d in a.grids:
        tr.grid_dim, tr.grid_pc = d, sm.grid_pc(d).cuda()
        fe = lambda: eager_compute_slices(tr, cmap, interp, 6)
        fb = lambda: tr.compute_slices(n_slices=6, include_gt=True)
        te, tb = alternate(fe, fb, a.reps)
        (e, _), b = fe(), fb()
        apart = [float(sm.index_distance(np.stack(b[k]), np.stack(e[k]), rgb).max()) for k in ("pred_sdf", "gt_sdf")]
        case = dict(grid=d, slices=6, points=6 * d * d, eager_ms=te, bound_ms=tb, speedup=te / tb,
                    launches_eager=count_launches(fe), launches_bound=count_launches(fb),
                    host_syncs_eager="3 (im_size, the field to the host, the points to the host)",
                    host_syncs_bound="2 (im_size, one copy of both colour images)",
                    max_index_distance_pred_gt=apart)
        res["cases"]["compute_slices_gt_grid%d" % d] = case
        print(json.dumps(case), flush=True)

    d = a.grids[0]
    tr.grid_dim, tr.grid_pc = d, sm.grid_pc(d).cuda()
    fe = lambda: eager_get_sdf_grid_pc(tr, interp)
    fb = lambda: tr.get_sdf_grid_pc(include_gt=True)[0]
    te, tb = alternate(fe, fb, min(a.reps, 5))
    e, b = fe(), fb()
    case = dict(grid=d, points=d ** 3, eager_ms=te, bound_ms=tb, speedup=te / tb, launches_eager=count_launches(fe),
                launches_bound=count_launches(fb), host_syncs_eager="2 (the field to the host, the points to the host)",
                host_syncs_bound="1 (one copy of the [d, d, d, 5] array)", shape=list(b.shape), dtype=str(b.dtype),
                pred_equal=bool(np.array_equal(e[..., :4], b[..., :4])), max_gt_diff=float(np.abs(e[..., 4] - b[..., 4]).max()))
    res["cases"]["get_sdf_grid_pc_gt_grid%d" % d] = case
    print(json.dumps(case), flush=True)
    res["bound_not_slower"] = all(c["speedup"] >= 1.0 for c in res["cases"].values())
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if not res["bound_not_slower"]:
        sys.exit("a bound call was slower than the pre-change route: %s" % {k: c["speedup"] for k, c in res["cases"].items()})


if __name__ == "__main__":
    main()
