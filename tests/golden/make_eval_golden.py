#!/usr/bin/env python3
"""Generate tests/golden/eval_metrics_small.npz by running the REFERENCE's evaluation code (imported read-only, as
make_golden.py does, with the same stubs for the packages that are absent) on small seeded inputs:

    sdf_util.sdf_interpolator, sdf_util.eval_sdf_interp(handle_oob='mask')      per-point ground truth and masks
    metrics.binned_losses, metrics.chomp_cost                                   bins, CHOMP costs
    Trainer.eval_sdf (its tail, on a given (sdf, eval_pts))                     the result dict
    metrics.accuracy, metrics.completion                                        mean nearest-neighbour distances

Run in the build container only:
    python tests/golden/make_eval_golden.py

Two volumes on one anisotropic grid: `signed` (negative inside two spheres, so the first bin is populated) and `zeroed`
(= max(signed, 0), as the replicaCAD grids store the inside of walls; rebuilt by the loader, not stored).  A float32 kernel can
put a point on the other side of a bin limit or of a face than float64 does, so points whose float64 ground truth lies within
1e-5 m of a bin limit, of a CHOMP epsilon or of zero without being zero, or whose grid coordinate lies within 1e-4 voxel of a
face plane, are dropped (under 1 % of them, asserted); with that, counts and masks compare with ==.  Only data is written."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

DIMS = (48, 36, 40)
SPACING = np.array([0.06, 0.07, 0.065])
ORIGIN = np.array([-1.4, -1.2, -1.3])
N_POINTS = 20000
EDGES = (0.1, 0.2, 0.5, 1.0, 1.5, 2.0)


def analytic(p):
    a = np.linalg.norm(p - np.array([-0.9, -0.7, -0.8]), axis=-1) - 0.55
    b = np.linalg.norm(p - np.array([0.2, 0.3, 0.1]), axis=-1) - 0.45
    return np.minimum(a, b)


def main():
    mods = mg.import_reference()
    trainer = mods[0]
    from isdf.datasets import sdf_util
    from isdf.eval import metrics
    rng = np.random.RandomState(20240607)

    ax = [np.arange(n) * h + o for n, h, o in zip(DIMS, SPACING, ORIGIN)]
    grid = np.stack(np.meshgrid(*ax, indexing="ij"), -1)
    signed = analytic(grid).astype(np.float32)                  # float32-representable: the kernel reads the same numbers
    zeroed = np.maximum(signed, 0)
    transform = np.eye(4)
    transform[[0, 1, 2], [0, 1, 2]] = SPACING
    transform[:3, 3] = ORIGIN

    lo, hi = ORIGIN, ORIGIN + (np.array(DIMS) - 1) * SPACING
    n_out = N_POINTS // 4
    inside = lo + rng.uniform(size=(N_POINTS - n_out, 3)) * (hi - lo)
    outside = []
    while len(outside) < n_out:
        c = (lo - 0.5) + rng.uniform(size=(n_out, 3)) * (hi - lo + 1.0)
        c = c[np.any((c < lo) | (c > hi), axis=1)]
        outside.extend(c[:n_out - len(outside)])
    pts = np.concatenate([inside, np.array(outside)])[rng.permutation(N_POINTS)].astype(np.float32)

    # drop what float32 could decide differently
    p64 = pts.astype(np.float64)
    u = (p64 - ORIGIN) / SPACING
    near_face = np.any((np.abs(u) < 1e-4) | (np.abs(u - (np.array(DIMS) - 1)) < 1e-4), axis=1)
    near_edge = np.zeros(len(pts), bool)
    for vol in (signed, zeroed):
        itp = sdf_util.sdf_interpolator(vol.astype(np.float64), transform)
        g, m = sdf_util.eval_sdf_interp(itp, p64, handle_oob="mask")
        for e in EDGES:
            near_edge |= m & (np.abs(g - e) < 1e-5)
        near_edge |= m & (g != 0) & (np.abs(g) < 1e-5)
    drop = near_face | near_edge
    print("dropped: %d near an edge, %d near a face, of %d" % (near_edge.sum(), near_face.sum(), len(pts)))
    assert drop.mean() < 0.01
    pts = pts[~drop]
    p64 = pts.astype(np.float64)
    itp_signed = sdf_util.sdf_interpolator(signed.astype(np.float64), transform)
    g_signed, m_signed = sdf_util.eval_sdf_interp(itp_signed, p64, handle_oob="mask")
    sdf = np.where(m_signed, g_signed, 0.3) + 0.05 * rng.standard_normal(len(pts))
    sdf = sdf.astype(np.float32)

    out = dict(signed=signed, spacing=SPACING, origin=ORIGIN, pts=pts, sdf=sdf, n_generated=np.array([N_POINTS]))
    for name, vol in (("signed", signed), ("zeroed", zeroed)):
        itp = sdf_util.sdf_interpolator(vol.astype(np.float64), transform)
        gt, inb = sdf_util.eval_sdf_interp(itp, p64, handle_oob="mask")
        assert inb.sum() > 0.7 * len(pts) and (~inb).sum() > 0.2 * len(pts)
        gt_store = np.where(inb, gt, 0.0)
        if name == "signed":
            out["signed/gt"] = gt_store
        else:                                # stored as its difference from the signed volume's (most points share the value)
            d = np.nonzero(gt_store != out["signed/gt"])[0]
            out["zeroed/gt_diff_index"], out["zeroed/gt_diff_value"] = d.astype(np.int32), gt_store[d]
        out[name + "/in_bounds"] = inb
        # the tail of Trainer.eval_sdf on the given (sdf, eval_pts): zero ground truth excluded
        tr = object.__new__(trainer.Trainer)
        tr.device, tr.gt_sdf_interp = "cpu", itp
        tr.eval_sdf_visible = lambda samples: (torch.from_numpy(sdf.copy()), torch.from_numpy(pts.copy()))
        res = tr.eval_sdf(visible_region=True)
        valid = np.logical_and(gt != 0., inb)
        out[name + "/valid"] = valid
        out[name + "/av_l1"] = np.array([res["av_l1"]])
        out[name + "/binned_l1"] = np.array(res["binned_l1"], np.float64)
        out[name + "/l1_chomp_costs"] = np.array(res["l1_chomp_costs"], np.float64)
        gv, sv = gt[valid], sdf[valid]
        lim = np.array([-1e99, 0., 0.1, 0.2, 0.5, 1., 1e99])
        out[name + "/bin_counts"] = np.array([((gv > lim[b]) & (gv < lim[b + 1])).sum() for b in range(6)])
        # the same through the numpy branch of metrics.binned_losses / chomp_cost, in float64 throughout
        d64 = np.abs(sv.astype(np.float64) - gv)
        out[name + "/binned_l1_np"] = np.array(metrics.binned_losses(d64, gv), np.float64)
        out[name + "/pred_chomp_sums"] = np.array([metrics.chomp_cost(sv.astype(np.float64), epsilon=e).sum() for e in (1., 1.5, 2.)])
        out[name + "/gt_chomp_sums"] = np.array([metrics.chomp_cost(gv.copy(), epsilon=e).sum() for e in (1., 1.5, 2.)])
        out[name + "/chomp_diff_means"] = np.array([np.abs(metrics.chomp_cost(sv.astype(np.float64), epsilon=e)
                                                           - metrics.chomp_cost(gv.copy(), epsilon=e)).mean() for e in (1., 1.5, 2.)])
        # eval_object_sdf's figure (trainer.py:1993-2003): zeros kept
        out[name + "/l1_keep_zero"] = np.array([np.abs(gt[inb] - sdf[inb]).mean()])
        print(name, res, "bin counts", out[name + "/bin_counts"], "zero gt", (inb & (gt == 0)).sum())
    assert out["signed/bin_counts"].min() > 0 and out["zeroed/bin_counts"][0] == 0 and out["zeroed/bin_counts"][1:].min() > 0

    # two point sets (a noisy reconstruction of a ground-truth surface) and the reference's accuracy / completion
    def sphere(n, r, noise):
        v = rng.standard_normal((n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        return (np.array([0.2, 0.3, 0.1]) + r * v + noise * rng.standard_normal((n, 3))).astype(np.float32)
    gt_points, rec_points = sphere(2500, 0.45, 0.0), sphere(3000, 0.46, 0.01)
    rec_points = rec_points[rec_points[:, 1] < 0.6]              # an incomplete reconstruction: completion > accuracy
    out["gt_points"], out["rec_points"] = gt_points, rec_points
    out["accuracy"] = np.array([metrics.accuracy(gt_points.astype(np.float64), rec_points.astype(np.float64))])
    out["completion"] = np.array([metrics.completion(gt_points.astype(np.float64), rec_points.astype(np.float64))])
    print("accuracy", out["accuracy"], "completion", out["completion"])

    path = os.path.join(HERE, "eval_metrics_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
