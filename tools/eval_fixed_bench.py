#!/usr/bin/env python3
"""One Trainer.eval_fixed, two ways, on the trained default net (fixture `trained_default`), 120 cached frames of 680 x 1200
(every 5th frame of a 600-frame sequence, as eval_pts.get_cache_dataset keeps them) and a 201 x 101 x 168 ground-truth volume
sampled from isdf_amd.synthetic.gt_sdf:

    bound     HotPath.eval_fixed: resident frames, one sampler launch, one forward-with-gradient and one forward launch, one
              isdf_region_metrics pass per leg, one copy back
    pre-PR    the route the call took before it was bound -- eval_pts.fixed_pts_eval's arithmetic (eval_pts.py:96-299) restated
              with scipy / numpy around SDFMapHIP: the whole cached sequence from numpy to torch, three 200 000-ray draws on the
              host, scipy's float64 RegularGridInterpolator once per region and six times for the central-difference gradient,
              three batches through the network with a host round trip each, bins / CHOMP / cosine in numpy

The mask files are made by this tool from the pre-PR route's own points (in bounds; a finite ground-truth gradient), two object
boxes and a 100 000-point full-volume file.  The two routes alternate within one process; device-synchronised wall time per
call, median over --reps; launches from the torch profiler; host synchronisations counted with torch's sync debug mode.

    python tools/eval_fixed_bench.py [--reps 7] [--out profiles/eval_fixed_bench.json]"""
import argparse
import json
import os
import sys
import tempfile
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from isdf_amd import synthetic                     # noqa: E402
from tests import eval_fixed_model as fm          # noqa: E402
from tests import eval_model as em                # noqa: E402
from tests import golden_util as gu               # noqa: E402

SAMPLES = 200000
DIMS = (201, 101, 168)
SEQ_LEN, KEEP_EVERY, T_EVAL = 600, 5, 20.0
N_DISTINCT = 8
N_VOL = 100000


class TiledDataset(fm.KeepIxsDataset):
    """120 held frames, N_DISTINCT rendered ones repeated (rendering 120 frames of 680 x 1200 on the host would take minutes)"""

    def __getitem__(self, idx):
        idx = np.asarray(idx)
        held = np.searchsorted(self.keep_ixs, idx[np.isin(idx, self.keep_ixs)])
        self.reads.append(len(held))
        k = held % len(self.depth)
        return {"image": None, "depth": self.depth[k], "T": self.T[k]}

    def __len__(self):
        return len(self.keep_ixs)


def host_rays(t_str, depth_batch, T_WC_batch, dirs_C, dist_behind_surf, surface):
    """eval_pts.sample_rays (eval_pts.py:354-400) on host tensors"""
    torch.manual_seed(float(t_str) * 1e3)
    F, H, W = depth_batch.shape
    rpf = SAMPLES // F
    ih, iw = torch.randint(0, H, (rpf * F,)), torch.randint(0, W, (rpf * F,))
    ib = torch.arange(F).repeat_interleave(rpf)
    d = depth_batch[ib, ih, iw].view(-1)
    ok = d != 0
    d, ib, ih, iw = d[ok], ib[ok], ih[ok], iw[ok]
    Ts, dC = T_WC_batch[ib], dirs_C[ih, iw, :].view(-1, 3)
    origins = Ts[:, :3, -1]
    dirs_W = (Ts[:, :3, :3] * dC[:, None, :]).sum(dim=-1)
    if surface:
        z = d[:, None]
    else:
        z = torch.rand(d.shape[0], 1) * ((d + dist_behind_surf) - 0.1)[:, None] + 0.1
    return (origins[:, None, :] + dirs_W[:, None, :] * z[:, :, None]).squeeze()


def np_metrics(pred, gt, bins=True):
    diff = np.abs(pred - gt)
    out = {"av_l1": diff.mean().item()}
    if bins:
        lim = em.BIN_LIMITS
        out["binned_l1"] = [diff[(gt > lim[b]) & (gt < lim[b + 1])].mean().item() if ((gt > lim[b]) & (gt < lim[b + 1])).any()
                            else float("nan") for b in range(6)]
        out["l1_chomp_costs"] = [np.abs(em.chomp(pred, e) - em.chomp(gt, e)).mean().item() for e in em.EPSILONS]
    return out


def host_eval_fixed(tr, itp, dirs_C, t, masks_dir, obj_bounds, vol_pts, vol_gt):
    """eval_pts.fixed_pts_eval restated: every step on the host except the network"""
    def sdf_fn(pts):
        with torch.no_grad():
            return tr.sdf_map(torch.FloatTensor(pts).to(tr.device)).detach().cpu().numpy()

    def grad_fn(pts):
        _, g = tr.sdf_map.forward_with_grad(torch.FloatTensor(pts).to(tr.device))
        return g.detach().cpu().numpy()

    def lookup(p):
        v = itp(np.asarray(p, np.float64))
        return v, v != 1e99

    def sub_eval(pts, gt, vox):
        p = np.concatenate((pts[vox], pts[~vox]))
        g = np.concatenate((gt[vox], gt[~vox]))
        sdf = sdf_fn(p)
        n = int(vox.sum())
        return {"vis": np_metrics(sdf, g), "vox": np_metrics(sdf[:n], g[:n])}

    t_str = f"{t:.3f}"
    m = {k: np.load(os.path.join(masks_dir, k + ".npy")) for k in
         ("surf_valid_gt_sdf", "surf_valid_vox_sdf", "vis_valid_gt_sdf", "vis_valid_vox_sdf", "vis_valid_gt_grad", "vis_valid_vox_grad")}
    ds = tr.cached_dataset
    sample = ds[np.arange(0, min(np.floor(t * 30), SEQ_LEN)).astype(int)]
    ds.reads.pop()
    depth_batch, T_WC_batch = torch.FloatTensor(sample["depth"]), torch.FloatTensor(sample["T"])
    res = {"time": t}
    pts = host_rays(t_str, depth_batch, T_WC_batch, dirs_C, 0.1, False).numpy()[m["vis_valid_gt_sdf"]]
    res["rays"] = sub_eval(pts, lookup(pts)[0], m["vis_valid_vox_sdf"])
    pts_all = host_rays(t_str, depth_batch, T_WC_batch, dirs_C, 0.1, False).numpy().astype(np.float64)
    grad = np.zeros(pts_all.shape)
    for i in range(3):
        for dx in (-1, 1):
            off = np.zeros(3)
            off[i] = dx * 0.01
            v, ok = lookup(pts_all + off)
            v[~(ok & (v != 0))] = np.nan
            grad[:, i] += dx * v
    grad /= 0.02
    G, A, B = m["vis_valid_gt_grad"], m["vis_valid_gt_sdf"], m["vis_valid_vox_sdf"]
    sel = G[A][B]
    for name, p, gg in (("vis", pts_all[G], grad[G]), ("vox", pts_all[A][B][sel], grad[A][B][sel])):
        c = float(fm.cos_distance(grad_fn(p), gg).mean())
        res["rays"][name]["av_cossim"] = [c, c]
    pts = host_rays(t_str, depth_batch, T_WC_batch, dirs_C, 0., True).numpy()[m["surf_valid_gt_sdf"]]
    res["visible_surf"] = sub_eval(pts, lookup(pts)[0], m["surf_valid_vox_sdf"])
    res["objects"] = []
    for i, b in enumerate(obj_bounds):
        va, vx = np.load(os.path.join(masks_dir, "obj%d_valid_gt_sdf.npy" % i)), np.load(os.path.join(masks_dir, "obj%d_valid_vox_sdf.npy" % i))
        p = fm.object_points(b)[va]
        g = lookup(p)[0]
        p, g = np.concatenate((p[vx], p[~vx])), np.concatenate((g[vx], g[~vx]))
        sdf = sdf_fn(p)
        n = int(vx.sum())
        res["objects"].append({"vis": np_metrics(sdf, g, False), "vox": np_metrics(sdf[:n], g[:n], False)})
    res["vol"] = np_metrics(sdf_fn(vol_pts), vol_gt)
    return res


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as p:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in p.events() if e.device_type.name == "CUDA" and "Memcpy" not in e.name and "Memset" not in e.name)


def count_syncs(fn):
    """host synchronisations torch reports for one call (set_sync_debug_mode), or a reason"""
    try:
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
        return sum(1 for x in w if "synchroniz" in str(x.message))
    except Exception as e:                                                    # noqa: BLE001
        return "not measured (%s)" % type(e).__name__
    finally:
        torch.cuda.set_sync_debug_mode("default")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from scipy.interpolate import RegularGridInterpolator
    from bench_support.standin_trainer import HipTrainer
    from isdf_amd.hot_path import HotPath
    from tests.accuracy_experiment import config
    cam = synthetic.REPLICA_CAM
    tr = HipTrainer("cuda", config(cam), inv_bounds_transform=synthetic.bounds_transform(), rng="philox", seed=1)
    g = gu.load("trained_default")
    tr.sdf_map.load_state_dict({k: torch.from_numpy(v) for k, v in gu.params_of(g).items()})
    keep = np.arange(0, SEQ_LEN, KEEP_EVERY)
    T = synthetic.trajectory(SEQ_LEN)[keep][:: len(keep) // N_DISTINCT][:N_DISTINCT]
    depth = np.stack([synthetic.render_depth(T[i], cam, np.random.RandomState(i)) for i in range(N_DISTINCT)]).astype(np.float32)
    ds = TiledDataset(depth, T.astype(np.float32), keep)
    lo, hi = np.asarray(synthetic.ROOM_LO, np.float64), np.asarray(synthetic.ROOM_HI, np.float64)
    spacing = (hi - lo) / (np.array(DIMS) - 1)
    ax = [np.arange(n) * h + o for n, h, o in zip(DIMS, spacing, lo)]
    values = synthetic.gt_sdf(np.stack(np.meshgrid(*ax, indexing="ij"), -1)).astype(np.float32)
    itp = RegularGridInterpolator(ax, values.astype(np.float64), bounds_error=False, fill_value=1e99)
    H, W = cam["H"], cam["W"]
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    dirs_C = torch.from_numpy(np.stack([(jj - cam["cx"]) / cam["fx"], (ii - cam["cy"]) / cam["fy"], np.ones_like(jj, float)], -1)
                              .astype(np.float32))
    rng = np.random.RandomState(0)
    obj_raw = np.array([[[1.0, 1.0, 1.0], [1.6, 1.6, 1.6]], [[3.5, 0.8, 2.5], [4.2, 1.5, 3.2]]])
    vol_pts = (lo + rng.uniform(size=(N_VOL, 3)) * (hi - lo)).astype(np.float32).astype(np.float64)
    vol_gt = itp(vol_pts)

    with tempfile.TemporaryDirectory() as root:
        # masks from the pre-PR route's own points
        t_str = f"{T_EVAL:.3f}"
        sample = ds[np.arange(SEQ_LEN)]
        ds.reads.clear()
        db, Tb = torch.FloatTensor(sample["depth"]), torch.FloatTensor(sample["T"])
        masks = {}
        vis = host_rays(t_str, db, Tb, dirs_C, 0.1, False).numpy().astype(np.float64)
        surf = host_rays(t_str, db, Tb, dirs_C, 0., True).numpy().astype(np.float64)
        for name, p in (("vis", vis), ("surf", surf), ("obj0", fm.object_points(fm.load_obj_bounds(obj_raw)[0])),
                        ("obj1", fm.object_points(fm.load_obj_bounds(obj_raw)[1]))):
            A = itp(p) != 1e99
            masks[name + "_valid_gt_sdf"], masks[name + "_valid_vox_sdf"] = A, rng.uniform(size=A.sum()) > 0.5
        G = np.isfinite(fm.gt_gradient(values, spacing, lo, vis, 0.01)).all(axis=1)
        masks["vis_valid_gt_grad"], masks["vis_valid_vox_grad"] = G, rng.uniform(size=G.sum()) > 0.5
        del db, Tb, sample
        dirs = fm.write_tree(root, t_str, masks, obj_raw, vol_pts, vol_gt)
        tr.eval_pts_dir, tr.seq_dir, tr.eval_pts_root = dirs
        tr.scene_dataset, tr.dataset_format, tr.cached_dataset, tr.tot_step_time = range(SEQ_LEN), "replicaCAD", ds, T_EVAL

        class _Grid:
            grid, values = ax, itp.values
        tr.gt_sdf_interp = _Grid()
        masks_dir = dirs[0] + t_str
        bounds = fm.load_obj_bounds(obj_raw)

        def bound():
            tr.eval_times = [T_EVAL]
            return HotPath.eval_fixed(tr)

        def host():
            return host_eval_fixed(tr, itp, dirs_C, T_EVAL, masks_dir, bounds, vol_pts, vol_gt)

        t_first, rb = timed(bound)                       # uploads the 120 frames
        first_bytes = tr._hip.eval_cache.uploaded_bytes
        rh = host()
        tb, th = [], []
        for _ in range(a.reps):
            tb.append(timed(bound)[0]); th.append(timed(host)[0])
        fb, fh = fm.flatten(rb), fm.flatten(rh)
        diff = max(float(np.nanmax(np.abs(fb[k] - fh[k]))) for k in fb)
        n_pts = int(masks["vis_valid_gt_sdf"].shape[0])
        res = dict(device=torch.cuda.get_device_name(0), reps=a.reps,
                   timing="device-synchronised wall time per call, median; the two routes alternate in one process",
                   setup=dict(frames=len(keep), frame=[H, W], volume=list(DIMS), drawn_points=n_pts, full_vol_points=N_VOL,
                              objects=2, net="trained_default"),
                   bound_ms=float(np.median(tb)), pre_pr_ms=float(np.median(th)), speedup=float(np.median(th) / np.median(tb)),
                   bound_first_call_ms=t_first, bound_first_call_uploaded_bytes=int(first_bytes),
                   bound_later_call_uploaded_frame_bytes=int(tr._hip.eval_cache.uploaded_bytes - first_bytes),
                   pre_pr_converted_bytes_per_call=int(len(keep) * (H * W + 16) * 4),
                   launches_bound=count_launches(bound), launches_pre_pr=count_launches(host),
                   host_syncs_bound=count_syncs(bound), host_syncs_pre_pr=count_syncs(host),
                   max_abs_diff=diff, av_l1=[rb["rays"]["vis"]["av_l1"], rh["rays"]["vis"]["av_l1"]],
                   av_cossim=[rb["rays"]["vis"]["av_cossim"][0], rh["rays"]["vis"]["av_cossim"][0]])
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
