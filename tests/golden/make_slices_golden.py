#!/usr/bin/env python3
"""Generate tests/golden/slices_small.npz by running the REFERENCE's slice code (imported read-only, as make_golden.py does,
with the same stubs for the packages that are absent) and matplotlib itself:

    sdf_util.get_colormap([-2, 2]) / ([-0.5, 0.5])      the two tables with their under / over / bad colours and limits
    ScalarMappable.to_rgba                              matplotlib's colours of ~20 000 float32 values (edge cases included)
    Trainer.compute_slices (grid 48, three slices)      the uint8 slabs as handed to cv2.resize, for both up_aligned cases,
                                                        with the points, the network's values and the ground truth behind them

Run in the build container only:
    python tests/golden/make_slices_golden.py

matplotlib >= 3.9 has no cm.get_cmap, which sdf_util.get_colormap calls: it is patched to matplotlib.colormaps[name].resampled(n),
which is what it was.  The network is the one of fixture trained_default (the synthetic room of isdf_amd.synthetic); the
ground-truth volume is that room's closed-form SDF on a 0.2 m grid.  Only data is written."""
import contextlib
import io
import os
import sys
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from tests import golden_util as gu  # noqa: E402
from tests import slice_model as sm  # noqa: E402

N_VALUES = 20000
VOL_SPACING = 0.2


def patch_get_cmap():
    import matplotlib
    from matplotlib import cm
    if not hasattr(cm, "get_cmap"):
        cm.get_cmap = lambda name, lut=None: matplotlib.colormaps[name].resampled(lut)


def test_values(rng):
    """uniform over +-2.5, a cluster around zero (the white band), multiples of the bin width, the ends of both ranges and their
    float32 neighbours, +-inf, NaN, +-0"""
    v = [rng.uniform(-2.5, 2.5, N_VALUES - 5000), rng.uniform(-0.03, 0.03, 3000), rng.uniform(-0.6, 0.6, 2000),
         np.arange(-250, 251) * 0.01]
    ends = np.array([-2.0, 2.0, -0.5, 0.5, 0.0, -0.0, 0.01, -0.01], np.float32)
    v += [ends, np.nextafter(ends, np.float32(np.inf)), np.nextafter(ends, np.float32(-np.inf)),
          np.array([np.inf, -np.inf, np.nan, 1e30, -1e30, 1e-30, -1e-30])]
    return np.concatenate([np.asarray(a, np.float32) for a in v])


def reference_trainer(mods):
    g = gu.load("trained_default")
    cam = dict(H=24, W=32, fx=30.0, fy=30.0, cx=15.5, cy=11.5)
    net = g["net"]
    netd = dict(H=int(net[0]), B=int(net[1]), n_freqs=int(net[2]), scale_input=float(net[3]), scale_output=float(net[4]))
    frames = gu.synth_frames(np.random.RandomState(5), 2, cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    with contextlib.redirect_stdout(io.StringIO()):
        return mg.build_trainer(mods, cam, netd, dict(mg.LOSS_DEFAULT), mg.SAMPLE_DEFAULT, frames, gu.params_of(g), g["bounds_T"], 0.0)


def gt_volume():
    from isdf_amd import synthetic
    lo = synthetic.ROOM_LO - VOL_SPACING
    dims = tuple(int(round((hi - l) / VOL_SPACING)) + 1 for l, hi in zip(lo, synthetic.ROOM_HI + VOL_SPACING))
    ax = [np.arange(n) * VOL_SPACING + l for n, l in zip(dims, lo)]
    values = synthetic.gt_sdf(np.stack(np.meshgrid(*ax, indexing="ij"), -1)).astype(np.float32)
    return values, np.array([VOL_SPACING] * 3), lo


def main():
    patch_get_cmap()
    mods = mg.import_reference()
    tmod = mods[0]
    from isdf.datasets import sdf_util
    rng = np.random.RandomState(20241017)
    out = {}

    values = test_values(rng)
    out["values"] = values
    for name, rng_ in (("t2", [-2, 2]), ("t05", [-0.5, 0.5])):
        m = sdf_util.get_colormap(sdf_range=list(rng_))
        n = m.cmap.N
        table = (np.asarray(m.cmap(np.arange(n))) * 255).astype(np.uint8)[:, :3]
        extra = [(np.asarray(c) * 255).astype(np.uint8)[:3] for c in (m.cmap.get_under(), m.cmap.get_over(), m.cmap.get_bad())]
        out[name + "/rgb"] = np.concatenate([table, np.stack(extra)])
        out[name + "/lim"] = np.array([m.norm.vmin, m.norm.vmax], np.float64)
        col = m.to_rgba(values, alpha=1., bytes=False)
        out[name + "/colours"] = (col * 255).astype(np.uint8)[..., :3]
        print(name, "N", n, "limits", out[name + "/lim"], "under/over/bad", extra)

    vol, spacing, origin = gt_volume()
    out["vol"], out["vol_spacing"], out["vol_origin"] = vol, spacing, origin
    T = np.eye(4)
    T[[0, 1, 2], [0, 1, 2]] = spacing
    T[:3, 3] = origin
    scale, Tb = sm.scene_geometry()
    out["scene_scale"], out["bounds_transform"], out["grid_dim"] = scale, Tb, np.array([sm.GRID_DIM])

    seen = []

    def resize(img, dsize):
        seen.append(np.asarray(img).copy())
        return np.zeros((int(dsize[1]), int(dsize[0])) + np.asarray(img).shape[2:], np.asarray(img).dtype)

    def depth2rgb(depth, min_value=None, max_value=None):       # imgviz is absent here; only the shape of its result is used
        return np.zeros(np.asarray(depth).shape + (3,), np.uint8)
    kept = {}
    real_interp = sdf_util.eval_sdf_interp

    def interp(itp, pc, handle_oob="except", oob_val=0.):
        kept["pts"] = np.asarray(pc).copy()
        kept["gt"] = real_interp(itp, pc, handle_oob=handle_oob, oob_val=oob_val)
        return kept["gt"]
    real_chunks = tmod.fc_map.chunks

    def chunks(pc, chunk_size, fn, **kw):
        kept["sdf"] = real_chunks(pc, chunk_size, fn, **kw)
        return kept["sdf"]
    for case in sm.CASES:
        tr = sm.set_slice_geometry(reference_trainer(mods), case)
        ref_grid = tmod.geometry.transform.make_3D_grid([-1.0, 1.0], sm.GRID_DIM, "cpu", transform=torch.from_numpy(Tb).float(),
                                                        scale=tr.scene_scale).view(-1, 3)
        assert torch.equal(ref_grid, tr.grid_pc), "tests/slice_model.grid_pc is not the reference's grid"
        tr.gt_sdf_interp = sdf_util.sdf_interpolator(vol.astype(np.float64), T)
        seen.clear()
        with mock.patch.object(tmod, "cv2", mock.MagicMock(resize=resize)), mock.patch.object(tmod, "imgviz", mock.MagicMock(depth2rgb=depth2rgb)), \
                mock.patch.object(sdf_util, "eval_sdf_interp", interp), mock.patch.object(tmod.fc_map, "chunks", chunks):
            slices = tr.compute_slices(n_slices=3, include_gt=True, include_diff=True)
        assert sorted(slices) == ["diff", "gt_sdf", "pred_sdf"] and len(seen) == 9
        out[case + "/pred_slabs"], out[case + "/gt_slabs"] = np.stack(seen[0:3]), np.stack(seen[3:6])
        assert all((s == 255).all() for s in seen[6:9])
        out[case + "/pts"] = kept["pts"].astype(np.float32)
        out[case + "/sdf"] = kept["sdf"].detach().numpy().reshape(kept["pts"].shape[:-1])
        out[case + "/gt"] = np.asarray(kept["gt"], np.float64)
        out[case + "/im_size"] = np.array(slices["pred_sdf"][0].shape[:2])
        oob = (kept["gt"] == 0).mean()
        print(case, "slab", seen[0].shape, "im_size", out[case + "/im_size"], "sdf range", float(kept["sdf"].min()),
              float(kept["sdf"].max()), "gt == 0 share %.3f" % oob)
        assert 0.02 < oob < 0.6

    path = os.path.join(HERE, "slices_small.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith(".npz") and f != "slices_small.npz")
    assert size < 1000000 and size <= largest


if __name__ == "__main__":
    main()
