#!/usr/bin/env python3
"""The voxel baseline (isdf_amd.fusion, isdf_amd/csrc/fusion.hip): what the fusion and the distance transform cost, and how the
baseline scores beside the net on the synthetic room.

    python tools/fusion_bench.py [--reps 7] [--out profiles/fusion_bench.json]

Fusion: 100 frames of 480 x 640 into 256^3 voxels of 2 cm around the cameras (frames and poses generated ON the device from a seed,
as tools/visible_bench.py makes them), Engine.tsdf_integrate (one launch) against the same fusion written in torch ops on the same
GPU, frame by frame.  Distance transform: Engine.distance_transform and Engine.occupancy_sdf at 128^3, 256^3 and 512^3 (a ball,
a slab and 0.1 % scattered voxels) against scipy.ndimage.distance_transform_edt on the HOST (one transform, and the two that
sdf_from_occupancy makes); sqrt of the device's squared distances is compared with scipy's result bit for bit.

Timing, as tools/visible_bench.py measures: per arm two warm-up calls, then --reps windows of back-to-back calls (each window at
least --window-ms long), device-synchronised at both ends, the arms alternating; the figure is the median window divided by its
calls.  The host partner is a host clock around one call (--host-reps of them at 128^3 and 256^3, one at 512^3).

Scores: the stand-in trainer on the synthetic room's stream at 480 x 640 (12 keyframes, 150 steps each, 1 cm depth noise); the
net's eval_sdf and, on the very points it drew, baseline_metrics of full_sdf(fuse_frames(trainer, voxel)) at 5 cm and 2.5 cm.
A record, not a test bar: no threshold was set in advance."""
import argparse
import contextlib
import io
import json
import math
import os
import subprocess
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from isdf_amd import fusion, metrics, synthetic        # noqa: E402

H, W = 480, 640
CAM = types.SimpleNamespace(fx=577.87, fy=577.87, cx=319.5, cy=239.5)


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return os.environ.get("ISDF_COMMIT", "unknown")


def device_frames(F, gen, dev="cuda"):
    """depth [F,H,W] (smooth 1.3-3.7 m plus noise, ~4 % zeros) and T_WC [F,4,4] (cameras on a 1 m circle, turning about the up
    axis and nodding), built on the device"""
    v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    depth = torch.empty(F, H, W, device=dev)
    for f in range(F):
        d = 2.5 + 1.2 * torch.sin(0.011 * u + f) * torch.cos(0.007 * v - 0.5 * f) + 0.05 * torch.randn(H, W, device=dev, generator=gen)
        d[torch.rand(H, W, device=dev, generator=gen) < 0.04] = 0.0
        depth[f] = d
    f = torch.arange(F, device=dev, dtype=torch.float32)
    a, b = 0.37 * f, 0.3 * torch.sin(0.11 * f)
    one, zero = torch.ones_like(a), torch.zeros_like(a)
    Ry = torch.stack([torch.cos(a), zero, torch.sin(a), zero, one, zero, -torch.sin(a), zero, torch.cos(a)], 1).view(F, 3, 3)
    Rx = torch.stack([one, zero, zero, zero, torch.cos(b), -torch.sin(b), zero, torch.sin(b), torch.cos(b)], 1).view(F, 3, 3)
    T = torch.eye(4, device=dev).repeat(F, 1, 1)
    T[:, :3, :3] = Ry @ Rx
    T[:, :3, 3] = torch.stack([torch.cos(0.05 * f), 0.2 * torch.sin(0.03 * f), torch.sin(0.05 * f)], 1)
    return depth, T


def torch_integrate(tsdf, weight, depth, T_CW, cam, origin, spacing, trunc, max_weight=float("inf"), min_depth=0.0,
                    max_depth=float("inf")):
    """isdf_tsdf_integrate in torch ops, the sequence of include/isdf_hip.h frame by frame: the comparison partner"""
    dev = tsdf.device
    nx, ny, nz = tsdf.shape
    x = (origin[0] + torch.arange(nx, device=dev, dtype=torch.float32) * spacing[0]).view(nx, 1, 1)
    y = (origin[1] + torch.arange(ny, device=dev, dtype=torch.float32) * spacing[1]).view(1, ny, 1)
    z = (origin[2] + torch.arange(nz, device=dev, dtype=torch.float32) * spacing[2]).view(1, 1, nz)
    Fh, Fw = float(depth.shape[1]), float(depth.shape[2])
    for f in range(depth.shape[0]):
        a = T_CW[f]
        xc = ((a[0, 0] * x + a[0, 1] * y) + a[0, 2] * z) + a[0, 3]
        yc = ((a[1, 0] * x + a[1, 1] * y) + a[1, 2] * z) + a[1, 3]
        zc = ((a[2, 0] * x + a[2, 1] * y) + a[2, 2] * z) + a[2, 3]
        uc = (cam.fx * xc + cam.cx * zc) / zc + 0.5
        vc = (cam.fy * yc + cam.cy * zc) / zc + 0.5
        inside = (uc >= 0) & (uc < Fw) & (vc >= 0) & (vc < Fh) & (zc > 0)
        col = torch.where(inside, uc, torch.zeros_like(uc)).long()
        row = torch.where(inside, vc, torch.zeros_like(vc)).long()
        d = depth[f][row, col]
        s = d - zc
        ok = inside & (d > min_depth) & (d < max_depth) & (s >= -trunc)
        t = torch.clamp(s, max=trunc)
        w1 = weight + 1.0
        tsdf.copy_(torch.where(ok, (tsdf * weight + t) / w1, tsdf))
        weight.copy_(torch.where(ok, torch.clamp(w1, max=max_weight), weight))
    return tsdf, weight


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def measure(arms, reps, window_ms):
    """{name: (median ms, [min, max], calls per window)}"""
    calls, times = {}, {}
    for name, fn in arms:
        fn()
        first = window(fn, 1)
        calls[name] = max(1, int(math.ceil(window_ms / max(first, 1e-3))))
        times[name] = []
    for _ in range(reps):
        for name, fn in arms:
            times[name].append(window(fn, calls[name]))
    return {name: (float(np.median(t)), [float(min(t)), float(max(t))], calls[name]) for name, t in times.items()}


def fusion_case(eng, reps, window_ms, F=100, side=256, voxel=0.02):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    depth, T_WC = device_frames(F, gen)
    T_CW = torch.linalg.inv(T_WC)
    origin, spacing, trunc = (-0.5 * side * voxel,) * 3, (voxel,) * 3, 4 * voxel
    vols = {k: (torch.zeros(side, side, side, device="cuda"), torch.zeros(side, side, side, device="cuda")) for k in ("hip", "torch")}

    def run(name, fn):
        t, w = vols[name]
        t.zero_()
        w.zero_()
        fn(t, w, depth, T_CW, CAM, origin, spacing, trunc)
    arms = (("hip", lambda: run("hip", eng.tsdf_integrate)), ("torch", lambda: run("torch", torch_integrate)))
    m = measure(arms, reps, window_ms)
    (th, wh), (tt, wt) = vols["hip"], vols["torch"]
    row = dict(frames=F, frame=[H, W], volume=[side] * 3, voxel_m=voxel, trunc_m=trunc, pairs=F * side ** 3,
               hip_ms=m["hip"][0], torch_ms=m["torch"][0], hip_ms_spread=m["hip"][1], torch_ms_spread=m["torch"][1],
               calls_per_window={k: v[2] for k, v in m.items()}, torch_over_hip=m["torch"][0] / m["hip"][0],
               hip_gpair_per_s=F * side ** 3 / m["hip"][0] / 1e6, includes="zeroing both volumes (two fills of %d MB)" % (side ** 3 * 4 >> 20),
               observed_share=float((wh > 0).float().mean()), weight_max=float(wh.max()),
               voxels_whose_weight_differs=int((wh != wt).sum()), max_abs_tsdf_difference=float((th - tt).abs().max()))
    return row


def occupancy(side, gen):
    """u8 [side]^3 on the device: a ball, a slab and 0.1 % scattered voxels"""
    i = torch.arange(side, device="cuda", dtype=torch.float32)
    c = 0.5 * side
    r2 = (i.view(-1, 1, 1) - c) ** 2 + (i.view(1, -1, 1) - 0.8 * c) ** 2 + (i.view(1, 1, -1) - 1.1 * c) ** 2
    occ = (r2 < (0.3 * side) ** 2) | (i.view(1, -1, 1) > 0.93 * side) | (torch.rand(side, side, side, device="cuda", generator=gen) < 0.001)
    return occ.to(torch.uint8)


def edt_case(eng, side, reps, window_ms, host_reps):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(side)
    occ = occupancy(side, gen)
    m = measure((("transform", lambda: eng.distance_transform(occ)), ("occupancy_sdf", lambda: eng.occupancy_sdf(occ, 0.02))), reps, window_ms)
    row = dict(volume=[side] * 3, occupied_share=float(occ.float().mean()), transform_ms=m["transform"][0], occupancy_sdf_ms=m["occupancy_sdf"][0],
               transform_ms_spread=m["transform"][1], occupancy_sdf_ms_spread=m["occupancy_sdf"][1],
               calls_per_window={k: v[2] for k, v in m.items()}, gvoxel_per_s=side ** 3 / m["transform"][0] / 1e6)
    try:
        from scipy import ndimage
    except ImportError:
        row["scipy"] = None
        return row
    occ_h = occ.cpu().numpy()
    inv = 1 - occ_h
    one, two = [], []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        a = ndimage.distance_transform_edt(inv)
        t1 = time.perf_counter()
        b = ndimage.distance_transform_edt(occ_h)
        ref = ((a - b).astype(float) * 0.02)
        t2 = time.perf_counter()
        one.append((t1 - t0) * 1e3)
        two.append((t2 - t0) * 1e3)
    d2 = eng.distance_transform(occ).cpu().numpy()
    sdf = eng.occupancy_sdf(occ, 0.02).cpu().numpy()
    row.update(scipy_transform_ms=float(np.median(one)), scipy_sdf_from_occupancy_ms=float(np.median(two)), scipy_calls=host_reps,
               sqrt_dist2_equals_scipy=bool(np.sqrt(d2.astype(np.float64)).tobytes() == a.tobytes()),
               occupancy_sdf_equals_scipy_after_cast=bool(sdf.tobytes() == ref.astype(np.float32).tobytes()))
    row["scipy_over_hip_transform"] = row["scipy_transform_ms"] / row["transform_ms"]
    row["scipy_over_hip_occupancy_sdf"] = row["scipy_sdf_from_occupancy_ms"] / row["occupancy_sdf_ms"]
    return row


class Grid:
    """what graft() reads of trainer.gt_sdf_interp: `.grid` and `.values`"""

    def __init__(self, grid, values):
        self.grid, self.values = grid, values


def scores(n_kf, steps_per_kf, samples, voxels):
    from bench_support.standin_trainer import HipTrainer
    from tests import eval_model as em
    from tests.accuracy_experiment import config
    cam = dict(synthetic.SCANNET_CAM)
    np.random.seed(1)
    torch.manual_seed(1)
    tr = HipTrainer("cuda", config(cam), inv_bounds_transform=synthetic.bounds_transform(), rng="philox", seed=1)
    traj = synthetic.trajectory(48 * n_kf + 48)
    rng = np.random.RandomState(1)
    depths = []
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        for k in range(n_kf):
            depths.append(synthetic.render_depth(traj[48 * k], cam, rng, noise_std=0.01))
            tr.last_is_keyframe = True
            tr.add_frame(tr.make_frame(48 * k, depths[-1], traj[48 * k]))
            tr.noise_std = tr.noise_kf
            for _ in range(steps_per_kf):
                losses, _ = tr.step()
    torch.cuda.synchronize()
    train = dict(keyframes=n_kf, steps=n_kf * steps_per_kf, final_total_loss=float(losses["total_loss"]),
                 train_and_render_s=time.perf_counter() - t0)
    # the room's box as the trainer's grid, and its analytic field on a 5 cm grid as the ground truth
    extents = synthetic.ROOM_HI - synthetic.ROOM_LO
    Tb = np.eye(4)
    Tb[:3, 3] = 0.5 * (synthetic.ROOM_LO + synthetic.ROOM_HI)
    tr.grid_dim, tr.scene_scale_np, tr.bounds_transform_np = 128, 0.5 * extents, Tb
    ax = tuple(np.arange(n) * 0.05 - 0.5 for n in (141, 81, 121))
    values = synthetic.gt_sdf(np.stack(np.meshgrid(*ax, indexing="ij"), -1)).astype(np.float32)
    tr.gt_sdf_interp = Grid(ax, values)
    tr.cached_dataset, tr.tot_step_time = em.CountingDataset(np.stack(depths), traj[::48][:n_kf], n_kf), n_kf / tr.fps
    seen = {}
    inner = tr.eval_sdf_visible

    def spy(n):
        seen["out"] = inner(n)
        return seen["out"]
    tr.eval_sdf_visible = spy
    out = dict(training=train, samples=samples, net=tr.eval_sdf(samples=samples, visible_region=True), baseline={})
    _, pts = seen["out"]
    gt = metrics.GtVolume.from_interpolator(tr.gt_sdf_interp, "cuda")
    for voxel in voxels:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vol = fusion.fuse_frames(tr, voxel=voxel)
        field = fusion.full_sdf(tr, vol)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        for name, f in (("full_sdf", field), ("full_sdf_without_blend", fusion.full_sdf(tr, vol, blend=False))):
            m = fusion.baseline_metrics(tr, f, vol, gt, pts)
            out["baseline"].setdefault("%g m" % voxel, dict(dims=list(vol.dims), trunc_m=vol.trunc, fuse_and_full_sdf_wall_ms=ms,
                                                            observed_share=float((vol.weight > 0).float().mean())))[name] = \
                dict(m.as_dict(), n_valid=m.n_valid, points=int(pts.shape[0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sides", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--kf", type=int, default=12)
    ap.add_argument("--steps-per-kf", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fusion_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fusion_bench needs a HIP device: there is nothing to measure without one")
    from isdf_amd.engine import Engine, NetConfig
    eng = Engine(NetConfig(hidden=64, blocks=1), "cuda")
    res = dict(commit=commit(), device=torch.cuda.get_device_name(0), reps=a.reps, window_ms=a.window_ms,
               timing="device-synchronised wall time per call, median over windows of back-to-back calls; the arms alternate in one "
                      "process; scipy: a host clock around one call, median of scipy_calls")
    res["fusion"] = fusion_case(eng, a.reps, a.window_ms)
    print(json.dumps(dict(fusion=res["fusion"])), flush=True)
    res["distance_transform"] = {}
    for side in a.sides:
        row = edt_case(eng, side, a.reps, a.window_ms, a.host_reps if side < 512 else 1)
        res["distance_transform"]["%d^3" % side] = row
        print(json.dumps({"%d^3" % side: row}), flush=True)
    res["scores_on_the_synthetic_room"] = scores(a.kf, a.steps_per_kf, 200000, (0.05, 0.025))
    print(json.dumps(res["scores_on_the_synthetic_room"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
