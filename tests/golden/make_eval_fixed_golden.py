#!/usr/bin/env python3
"""Generate tests/golden/eval_fixed_small.npz by running the REFERENCE's fixed-point evaluation, eval_pts.fixed_pts_eval
(eval_pts.py:96-299; imported read-only, as make_eval_golden.py does), on a seeded toy set-up:

    12 frames of 96 x 128 behind a dataset with keep_ixs (every 5th frame of a 60-frame sequence), one pixel in 16 with a depth
    a volume in the style of make_eval_golden.py's `signed` / `zeroed` pair in one grid (tests/eval_fixed_model.scene_sdf:
    negative inside one sphere, ZERO inside the other)
    an analytic sdf_fn / grad_fn (eval_fixed_model.pred_sdf / pred_grad: a perturbed field and its gradient, rounded to float32)
    three object boxes, the middle one without files in the timestamp directory (skipped, as the reference skips it)
    a small full_vol point file

Run in the build container only:
    python tests/golden/make_eval_fixed_golden.py

The mask files are made as a real tool would make them -- in bounds, and for the gradient sets with a finite ground-truth
gradient -- and additionally exclude what another arithmetic could decide differently: points whose float64 ground truth lies
within 1e-5 m of a bin limit, of a CHOMP epsilon or of zero without being zero, and points whose grid coordinate, for any of the
seven lookups (the point and p +- 0.01 e_i), lies within 1e-4 voxel of a face of the grid.  Recorded: the inputs, the drawn
points, the masks, gt_grad_all and the result dict.  Only data is written."""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from tests import eval_fixed_model as fm  # noqa: E402

DIMS = (48, 36, 40)
SPACING = np.array([0.06, 0.07, 0.065])
ORIGIN = np.array([-1.4, -1.2, -1.3])
H, W, FX, FY, CX, CY = 96, 128, 64.0, 64.0, 63.5, 47.5
SEQ_LEN, KEEP_EVERY, T_EVAL = 60, 5, 1.5            # frames 0, 5, ..., 40 are what floor(1.5 * 30) = 45 selects: 9 of the 12 held
EDGES = (0.1, 0.2, 0.5, 1.0, 1.5, 2.0)
DELTA = 0.01
OBJ_BOUNDS_RAW = np.array([[[-0.55, -0.45, -0.6], [-0.1, -0.05, -0.25]],
                           [[0.6, -0.9, -0.9], [0.9, -0.6, -0.6]],
                           [[0.05, 0.15, 0.0], [0.5, 0.55, 0.35]]])
N_VOL = 3000


def frames():
    """depth [12, H, W] float32 (multiples of 1/1024; zero = no reading on 15 pixels of 16) and camera-to-world poses"""
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth, T = [], []
    for k in range(SEQ_LEN // KEEP_EVERY):
        d = 0.85 + 0.6 * ((hh * 7 + ww * 3 + k * 11) % 64) / 64.0
        d = np.where((hh + 2 * ww + k) % 16 == 0, np.round(d * 1024) / 1024, 0.0)
        depth.append(d.astype(np.float32))
        yaw, pitch = -0.33 + 0.06 * k, 0.12 - 0.02 * k
        Ry = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(pitch), -np.sin(pitch)], [0, np.sin(pitch), np.cos(pitch)]])
        M = np.eye(4)
        M[:3, :3] = Ry @ Rx
        M[:3, 3] = [-0.75 + 0.13 * k, -0.4 + 0.07 * k, -1.15]
        T.append(M.astype(np.float32).astype(np.float64))
    return np.stack(depth), np.stack(T)


def near_limits(gt, inb):
    near = np.zeros(len(gt), bool)
    for e in EDGES:
        near |= inb & (np.abs(gt - e) < 1e-5)
    return near | (inb & (gt != 0) & (np.abs(gt) < 1e-5))


def near_face(p64):
    """any of the seven lookups within 1e-4 voxel of a face of the grid"""
    out = np.zeros(len(p64), bool)
    offs = [np.zeros(3)] + [s * DELTA * np.eye(3)[i] for i in range(3) for s in (-1, 1)]
    for o in offs:
        u = (p64 + o - ORIGIN) / SPACING
        out |= np.any((np.abs(u) < 1e-4) | (np.abs(u - (np.array(DIMS) - 1)) < 1e-4), axis=1)
    return out


def vox_region(p64):
    """the part 'another mapper' covers: alternate 25 cm slabs across the scene"""
    return np.floor((p64[:, 0] + p64[:, 1] + p64[:, 2] + 10.0) * 4.0).astype(np.int64) % 2 == 0


def main():
    mods = mg.import_reference()
    transform = mods[5]
    from isdf.datasets import sdf_util
    from isdf.eval import eval_pts

    ax = [np.arange(n) * h + o for n, h, o in zip(DIMS, SPACING, ORIGIN)]
    volume = fm.scene_sdf(np.stack(np.meshgrid(*ax, indexing="ij"), -1)).astype(np.float32)
    tf = np.eye(4)
    tf[[0, 1, 2], [0, 1, 2]] = SPACING
    tf[:3, 3] = ORIGIN
    itp = sdf_util.sdf_interpolator(volume.astype(np.float64), tf)

    depth, T = frames()
    keep_ixs = np.arange(0, SEQ_LEN, KEEP_EVERY)
    ds = fm.KeepIxsDataset(depth, T, keep_ixs)
    dirs_C = transform.ray_dirs_C(1, H, W, FX, FY, CX, CY, "cpu", depth_type="z")
    t_str = f"{T_EVAL:.3f}"
    sample = ds[np.arange(0, min(np.floor(T_EVAL * 30), SEQ_LEN)).astype(int)]
    depth_batch, T_WC_batch = torch.FloatTensor(sample["depth"]), torch.FloatTensor(sample["T"])

    # the points the reference will draw, from its own functions
    vis_pts = eval_pts.sample_visible_region(t_str, depth_batch, T_WC_batch, "replicaCAD", dirs_C).numpy()
    surf_pts = eval_pts.sample_surface(t_str, depth_batch, T_WC_batch, dirs_C).numpy()
    assert vis_pts.dtype == np.float32 and vis_pts.shape == surf_pts.shape
    N = len(vis_pts)
    gt_grad_all, grad_valid = eval_pts.eval_grad(itp, torch.from_numpy(vis_pts), DELTA, is_gt_sdf=True)

    masks, n_drop, n_all = {}, 0, 0

    def sdf_masks(name, p64, extra_drop=None):
        nonlocal n_drop, n_all
        gt, inb = sdf_util.eval_sdf_interp(itp, p64, handle_oob="mask")
        drop = inb & (near_limits(gt, inb) | near_face(p64))
        n_drop, n_all = n_drop + drop.sum(), n_all + len(p64)
        valid = inb & ~drop
        vox = vox_region(p64)[valid]
        assert valid.mean() >= 0.5, (name, valid.mean())
        assert 0.3 <= vox.mean() <= 0.7, (name, vox.mean())
        masks[name + "_valid_gt_sdf"], masks[name + "_valid_vox_sdf"] = valid, vox
        return gt, valid, vox

    v64, s64 = vis_pts.astype(np.float64), surf_pts.astype(np.float64)
    gt_vis, A, B = sdf_masks("vis", v64)
    gt_surf, As, Bs = sdf_masks("surf", s64)
    G = grad_valid & ~near_face(v64)
    masks["vis_valid_gt_grad"] = G
    masks["vis_valid_vox_grad"] = vox_region(v64)[G]
    assert G.mean() >= 0.3 and (A & ~G).sum() > 100          # the gradient set is a proper part (zero-valued and edge lookups)
    sel = gt_vis[A]
    assert (sel < 0).sum() > 50 and (sel == 0).sum() > 50     # the first bin is populated, zero-valued ground truth is present
    assert (gt_surf[As] == 0).sum() > 10

    obj_ids = [0, 2]
    with tempfile.TemporaryDirectory() as root:
        b = fm.load_obj_bounds(OBJ_BOUNDS_RAW)
        for i in obj_ids:
            gt, valid, vox = sdf_masks("obj%d" % i, eval_pts.object_eval_pts(b[i]))
        assert n_drop < 0.01 * n_all, (n_drop, n_all)
        print("dropped %d of %d points near a limit or a face" % (n_drop, n_all))

        rng = np.random.RandomState(20241017)
        lo, hi = ORIGIN, ORIGIN + (np.array(DIMS) - 1) * SPACING
        vol_pts = (lo + rng.uniform(size=(N_VOL, 3)) * (hi - lo)).astype(np.float32)
        vol_gt, _ = sdf_util.eval_sdf_interp(itp, vol_pts.astype(np.float64), handle_oob="mask")
        eval_pts_dir, seq_dir, eval_pts_root = fm.write_tree(root, t_str, masks, OBJ_BOUNDS_RAW, vol_pts.astype(np.float64), vol_gt)
        assert np.array_equal(eval_pts.load_obj_bounds(seq_dir + "/obj_bounds.txt"), b)

        res = eval_pts.fixed_pts_eval(fm.pred_sdf, T_EVAL, eval_pts_dir, seq_dir, "replicaCAD", ds, dirs_C, itp, eval_pts_root,
                                      SEQ_LEN, grad_fn=fm.pred_grad)
    print(res)
    assert len(res["objects"]) == len(obj_ids)

    out = dict(volume=volume, spacing=SPACING, origin=ORIGIN, depth=depth, T=T, keep_ixs=keep_ixs, seq_len=np.array([SEQ_LEN]),
               cam=np.array([H, W, FX, FY, CX, CY]), t=np.array([T_EVAL]), vis_pts=vis_pts, surf_pts=surf_pts,
               gt_grad_all=gt_grad_all, obj_bounds_raw=OBJ_BOUNDS_RAW, obj_ids=np.array(obj_ids), vol_pts=vol_pts, vol_gt=vol_gt,
               n_dropped=np.array([n_drop, n_all]))
    out.update(masks)
    for k, v in fm.flatten(res).items():
        out["res/" + k] = v
    path = os.path.join(HERE, "eval_fixed_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", N, "drawn points")
    assert os.path.getsize(path) < 1048576


if __name__ == "__main__":
    main()
