#!/usr/bin/env python3
"""Evaluation timing on the trained default net (fixture `trained_default`), a ground-truth volume sampled from
isdf_amd.synthetic.gt_sdf and 200 000 evaluation points: the route Trainer.eval_sdf took around SDFMapHIP before it was bound
(restated from trainer.py:1831-1866 -- forward, points to the host, linear interpolation on the host (scipy's
RegularGridInterpolator if it imports, else the numpy model of tests/eval_model.py), ground truth back to the device, torch ops
for the L1, the six bins and the CHOMP costs, with their .item() calls) against the bound route (forward + ONE isdf_sdf_metrics
call + one copy of 24 doubles).  The same for accuracy / completion at 200 000 x 200 000 points (scipy.spatial.cKDTree, if
present, against two isdf_nn_distance calls), and the bytes uploaded by the second of two eval_sdf_visible calls 30 frames apart
(the whole sequence so far before; the new frames after).  The two routes alternate within one process; device-synchronised wall
time per call, medians over --reps.

    python tools/eval_bench.py [--reps 7] [--out profiles/eval_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from isdf_amd import metrics, synthetic        # noqa: E402
from tests import eval_model as em             # noqa: E402
from tests import golden_util as gu            # noqa: E402

N_POINTS = 200000
SPACING = 0.03
LIMITS = np.array([-1e99, 0., 0.1, 0.2, 0.5, 1., 1e99])


def chomp_torch(sdf, epsilon):
    cost = -sdf + epsilon / 2.
    cost[sdf > 0] = 1 / (2 * epsilon) * (sdf[sdf > 0] - epsilon) ** 2
    cost[sdf > epsilon] = 0.
    return cost


def eager_eval_sdf(sdf_map, pts_dev, interp):
    """trainer.py:1831-1866 after eval_sdf_visible, as it ran around SDFMapHIP"""
    with torch.no_grad():
        sdf = sdf_map(pts_dev).flatten()
        gt, valid = interp(pts_dev.cpu().detach().numpy())
        valid = np.logical_and(gt != 0., valid)
        gt_sdf = torch.from_numpy(gt[valid]).to(pts_dev.device)
        sdf = sdf[valid]
        diff = torch.abs(sdf - gt_sdf)
        l1 = diff.mean()
        lb = torch.tensor(LIMITS[:-1]).to(gt_sdf.device)
        ub = torch.tensor(LIMITS[1:]).to(gt_sdf.device)
        masks = torch.logical_and(gt_sdf > lb[:, None], gt_sdf < ub[:, None])
        bins = ((diff * masks).sum(1) / masks.sum(1)).tolist()
        costs = [torch.abs(chomp_torch(sdf, e) - chomp_torch(gt_sdf, e)).mean().item() for e in (1., 1.5, 2.)]
        return {"av_l1": l1.item(), "binned_l1": bins, "l1_chomp_costs": costs}


def bound_eval_sdf(sdf_map, pts_dev, vol):
    with torch.no_grad():
        sdf = sdf_map(pts_dev).flatten()
    return metrics.sdf_metrics(sdf_map.engine, vol, pts_dev, sdf).as_dict()


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


def surface_points(n, rng):
    """points on the synthetic room's spheres and floor (two such sets stand in for the sampled meshes)"""
    k = n // 4
    out = []
    for c, r in synthetic.SPHERES:
        v = rng.standard_normal((k, 3))
        out.append(c + r * v / np.linalg.norm(v, axis=1, keepdims=True))
    f = rng.uniform(size=(n - 3 * k, 3)) * (synthetic.ROOM_HI - synthetic.ROOM_LO) + synthetic.ROOM_LO
    f[:, 1] = synthetic.ROOM_HI[1]
    out.append(f)
    return np.concatenate(out).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--nn-points", type=int, default=N_POINTS)
    a = ap.parse_args()
    from isdf_amd.modules import PositionalEncodingHIP, SDFMapHIP
    g = gu.load("trained_default")
    net = g["net"]
    pe = PositionalEncodingHIP(min_deg=0, max_deg=int(net[2]) - 1, scale=float(net[3]),
                               transform=torch.from_numpy(g["bounds_T"].astype(np.float32)))
    sdf_map = SDFMapHIP(pe, hidden_size=int(net[0]), hidden_layers_block=int(net[1]), scale_output=float(net[4]), device="cuda")
    sdf_map.load_state_dict({k: torch.from_numpy(v) for k, v in gu.params_of(g).items()})
    eng = sdf_map.engine
    rng = np.random.RandomState(0)

    dims = tuple(int(round((hi - lo) / SPACING)) + 1 for lo, hi in zip(synthetic.ROOM_LO, synthetic.ROOM_HI))
    ax = [np.arange(n) * SPACING + lo for n, lo in zip(dims, synthetic.ROOM_LO)]
    values = synthetic.gt_sdf(np.stack(np.meshgrid(*ax, indexing="ij"), -1)).astype(np.float32)
    vol = metrics.GtVolume(values, [SPACING] * 3, synthetic.ROOM_LO, "cuda")
    pts = (rng.uniform(size=(N_POINTS, 3)) * (synthetic.ROOM_HI - synthetic.ROOM_LO + 0.6) + synthetic.ROOM_LO - 0.3).astype(np.float32)
    pts_dev = torch.from_numpy(pts).cuda()
    try:
        from scipy.interpolate import RegularGridInterpolator
        itp = RegularGridInterpolator(ax, values.astype(np.float64), bounds_error=False, fill_value=1e99)
        host_name = "scipy RegularGridInterpolator (float64)"

        def interp(p):
            v = itp(p)
            return v, v != 1e99
    except ImportError:
        host_name = "numpy trilinear model (float64)"

        def interp(p):
            return em.trilinear(values, [SPACING] * 3, synthetic.ROOM_LO, p)

    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, timing="device-synchronised wall time per call, median; "
               "the two routes alternate in one process", cases={})
    fe = lambda: eager_eval_sdf(sdf_map, pts_dev, interp)
    fb = lambda: bound_eval_sdf(sdf_map, pts_dev, vol)
    te, tb = alternate(fe, fb, a.reps)
    re_, rb = fe(), fb()
    only = lambda: eng.sdf_metrics(vol, pts_dev, torch.zeros(N_POINTS, device="cuda"))
    t_kernel = float(np.median([timed(only)[0] for _ in range(a.reps)]))
    res["cases"]["eval_sdf_200k"] = dict(
        points=N_POINTS, volume=list(dims), host_interpolation=host_name, eager_ms=te, bound_ms=tb, speedup=te / tb,
        sdf_metrics_alone_ms=t_kernel, launches_eager=count_launches(fe), launches_bound=count_launches(fb),
        host_syncs_eager="9 (points to the host, ground truth up, l1.item(), bins.tolist(), 3 x mean().item(), 2 boolean-mask "
                         "compactions)", host_syncs_bound=1,
        av_l1_eager=re_["av_l1"], av_l1_bound=rb["av_l1"],
        max_abs_diff=float(np.nanmax(np.abs(np.array([re_["av_l1"]] + re_["binned_l1"] + re_["l1_chomp_costs"])
                                            - np.array([rb["av_l1"]] + rb["binned_l1"] + rb["l1_chomp_costs"])))))
    print(json.dumps(res["cases"]["eval_sdf_200k"]), flush=True)

    n = a.nn_points
    gt_pts, rec_pts = surface_points(n, rng), surface_points(n, rng) + (0.01 * rng.standard_normal((n, 3))).astype(np.float32)
    gt_dev, rec_dev = torch.from_numpy(gt_pts).cuda(), torch.from_numpy(rec_pts).cuda()
    fb = lambda: metrics.accuracy_completion(eng, gt_dev, rec_dev)
    fb()
    tb = float(np.median([timed(fb)[0] for _ in range(a.reps)]))
    one = lambda: eng.nn_distance(rec_dev, gt_dev)
    t_one = float(np.median([timed(one)[0] for _ in range(a.reps)]))
    case = dict(points=[n, n], bound_ms=tb, nn_distance_one_direction_ms=t_one, pairs_per_s=float(n) * n / (t_one * 1e-3),
                launches_bound=count_launches(fb), host_syncs_bound=1, bound=list(fb()))
    try:
        from scipy.spatial import cKDTree

        def host():
            acc = cKDTree(gt_pts).query(rec_pts)[0].mean()
            return acc, cKDTree(rec_pts).query(gt_pts)[0].mean()
        th = []
        for _ in range(min(a.reps, 3)):
            t0 = time.perf_counter()
            rh = host()
            th.append((time.perf_counter() - t0) * 1e3)
        case.update(host_ckdtree_ms=float(np.median(th)), speedup=float(np.median(th)) / tb, host=[float(v) for v in rh],
                    rel_diff=[abs(b - h) / h for b, h in zip(case["bound"], rh)])
    except ImportError:
        case.update(host_ckdtree_ms="not measured (scipy.spatial is not installed)")
    res["cases"]["accuracy_completion_%dk" % (n // 1000)] = case
    print(json.dumps(case), flush=True)

    # eval_sdf_visible twice, 30 frames apart, at the replicaCAD camera: bytes uploaded by the second call
    from bench_support.standin_trainer import HipTrainer
    from tests.accuracy_experiment import config
    cam = synthetic.REPLICA_CAM
    T = synthetic.trajectory(60)[::15]
    depth = np.stack([synthetic.render_depth(T[i], cam, np.random.RandomState(i)) for i in range(len(T))])
    ds = em.CountingDataset(depth, T, 60)
    tr = HipTrainer("cuda", config(cam), inv_bounds_transform=synthetic.bounds_transform(), rng="philox", seed=1)
    tr.cached_dataset, tr.tot_step_time = ds, 1.0

    def eager_upload(n_frames):      # trainer.py:1869-1875
        sample = ds[np.arange(n_frames)]
        d = torch.FloatTensor(sample["depth"]).to(tr.device)
        Tb = torch.FloatTensor(sample["T"]).to(tr.device)
        return d.numel() * 4 + Tb.numel() * 4
    t1, _ = timed(lambda: tr.eval_sdf_visible(N_POINTS))
    b1 = tr._hip.eval_cache.uploaded_bytes
    tr.tot_step_time = 2.0
    t2, _ = timed(lambda: tr.eval_sdf_visible(N_POINTS))
    b2 = tr._hip.eval_cache.uploaded_bytes - b1
    te2, be2 = timed(lambda: eager_upload(60))
    res["cases"]["eval_sdf_visible_second_call"] = dict(
        frames_so_far=60, new_frames=30, frame=[cam["H"], cam["W"]], bytes_uploaded_eager=int(be2), bytes_uploaded_bound=int(b2),
        eager_convert_and_upload_ms=te2, bound_first_call_ms=t1, bound_second_call_ms=t2,
        note="eager = the conversion and upload alone (torch.FloatTensor(sample['depth']).to(device) of every frame so far); "
             "the bound calls include reading the new frames from the dataset, sampling and the forward")
    print(json.dumps(res["cases"]["eval_sdf_visible_second_call"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
