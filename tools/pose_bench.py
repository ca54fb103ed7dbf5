#!/usr/bin/env python3
"""Frame-to-map pose alignment (isdf_amd.tracking, isdf_amd/csrc/pose.hip) on a TRAINED map: what an iteration costs and how
close to the true pose it gets.

    python tools/pose_bench.py [--reps 20] [--kf 12] [--steps-per-kf 150] [--out profiles/pose_bench.json]

The map: the stand-in trainer (bench_support/standin_trainer.py) on the synthetic room's stream at 480 x 640, a pinned schedule of
`--kf` keyframes 48 frames apart, `--steps-per-kf` steps each, 1 cm depth noise.

Timing (cases 680 x 1200 stride 8 and 480 x 640 stride 4, B = 1, 5 and 20 poses over five rendered frames, poses perturbed by
0.03 m / 2 degrees): HIP events on the launch stream around ten back-to-back calls each of the points launch, the field call
(Engine.sdf_eval with gradient) and the system launch of one iteration, per call; one warm-up per shape, `--reps` repeats, medians; the two arms alternate.  `iteration_wall_ms`
and `refine_ms` are host clocks around calls that end in the records' copy and the stream's end.  The comparison partner
(`torch`) is the same iteration written in torch ops on the same device around the same Engine.sdf_eval: the back-projection in
float32, weights, Jacobians and the two einsum contractions in float64.  There is no parent-commit figure: the parent has no
such call.

Accuracy: poses of the stream that were NOT keyframes (24 frames off the keyframe grid), their depth rendered with the same
noise, perturbed by 0.03 m / 2 degrees and 0.08 m / 5 degrees, refined with the defaults; error before and after against the true
pose.  A record, not a test bar."""
import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from isdf_amd import synthetic, tracking        # noqa: E402
from tests import pose_model as pm              # noqa: E402


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return os.environ.get("ISDF_COMMIT", "unknown")


class TorchOps:
    """Engine.pose_points / Engine.pose_system written in torch ops (any device): the comparison partner"""

    @staticmethod
    def _lattice(depth, T_WC, frame_of_pose, stride, min_depth, max_depth):
        dev = depth.device
        T = torch.as_tensor(np.asarray(T_WC, np.float32).reshape(-1, 4, 4)[:, :3, :]).to(dev)
        fop = torch.arange(T.shape[0], device=dev) if frame_of_pose is None else torch.as_tensor(np.asarray(frame_of_pose, np.int64)).to(dev)
        z = depth[fop][:, ::stride, ::stride]
        valid = torch.isfinite(z) & (z != 0) & (z >= min_depth) & (z <= max_depth)
        return T, z, valid

    def pose_points(self, depth, T_WC, cam, frame_of_pose=None, stride=4, min_depth=0.0, max_depth=float("inf")):
        T, z, valid = self._lattice(depth, T_WC, frame_of_pose, stride, min_depth, max_depth)
        H, W = depth.shape[1:]
        c = torch.arange(0, W, stride, device=depth.device, dtype=torch.float32)
        r = torch.arange(0, H, stride, device=depth.device, dtype=torch.float32)
        pc = torch.stack([z * (c - cam.cx) / cam.fx, z * (r[:, None] - cam.cy) / cam.fy, z], -1).reshape(T.shape[0], -1, 3)
        t = T[:, None, :, 3]
        pw = pc @ T[:, :, :3].transpose(1, 2) + t
        return torch.where(valid.reshape(T.shape[0], -1, 1), pw, t.expand_as(pw)).reshape(-1, 3)

    def pose_system(self, depth, T_WC, cam, pts, sdf, grad, frame_of_pose=None, stride=4, min_depth=0.0, max_depth=float("inf"),
                    huber=0.05, trunc=0.3, out=None, workspace=None):
        T, z, valid = self._lattice(depth, T_WC, frame_of_pose, stride, min_depth, max_depth)
        B = T.shape[0]
        hub, tr = float(np.float32(huber)), float(np.float32(trunc))
        r = sdf.reshape(B, -1).double()
        a = r.abs()
        valid = valid.reshape(B, -1)
        used = valid & (a <= tr)
        quad = a <= hub
        w = torch.where(quad, torch.ones_like(a), hub / a.clamp_min(1e-300)) * used
        g = grad.reshape(B, -1, 3).double()
        d = pts.reshape(B, -1, 3).double() - T[:, None, :, 3].double()
        J = torch.cat([g, torch.cross(d, g, dim=-1)], -1)
        r0 = torch.where(used, r, torch.zeros_like(r))                      # a NaN residual is not used and must not reach a sum
        Hm = torch.einsum("bn,bni,bnj->bij", w, J, J)
        rec = torch.zeros(B, 32, dtype=torch.float64, device=depth.device)
        rec[:, 0], rec[:, 1] = used.sum(1), valid.sum(1)
        rec[:, 2] = (w * r0 * r0).sum(1)
        rec[:, 3] = (torch.where(quad, 0.5 * r0 * r0, hub * (r0.abs() - 0.5 * hub)) * used).sum(1)
        rec[:, 4:10] = torch.einsum("bn,bni->bi", w * r0, J)
        iu = torch.triu_indices(6, 6, device=depth.device)
        rec[:, 10:31] = Hm[:, iu[0], iu[1]]
        rec[:, 31] = (r0.abs() * used).sum(1)
        return rec


def train_map(n_kf, steps_per_kf, cam, seed=1):
    from bench_support.standin_trainer import HipTrainer
    from tests.accuracy_experiment import config
    np.random.seed(seed)
    torch.manual_seed(seed)
    tr = HipTrainer("cuda", config(cam), inv_bounds_transform=synthetic.bounds_transform(), rng="philox", seed=seed)
    traj = synthetic.trajectory(48 * n_kf + 48)
    rng = np.random.RandomState(seed)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        for k in range(n_kf):
            fr = tr.make_frame(48 * k, synthetic.render_depth(traj[48 * k], cam, rng, noise_std=0.01), traj[48 * k])
            tr.last_is_keyframe = True
            tr.add_frame(fr)
            tr.noise_std = tr.noise_kf
            for _ in range(steps_per_kf):
                losses, _ = tr.step()
    torch.cuda.synchronize()
    return tr, traj, dict(keyframes=n_kf, steps=n_kf * steps_per_kf, final_total_loss=float(losses["total_loss"]),
                          train_and_render_s=time.perf_counter() - t0)


INNER = 10      # back-to-back calls between one pair of events


def iteration_events(ops, eng, depth, T, cam, fop, stride):
    """(points_ms, field_ms, system_ms) per call of one iteration's parts: HIP events around INNER back-to-back calls of each"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    kw = dict(frame_of_pose=fop, stride=stride)
    ev[0].record()
    for _ in range(INNER):
        pts = ops.pose_points(depth, T, cam, **kw)
    ev[1].record()
    with torch.no_grad():
        for _ in range(INNER):
            sdf, grad = eng.sdf_eval(pts, want_grad=True)
    ev[2].record()
    for _ in range(INNER):
        rec = ops.pose_system(depth, T, cam, pts, sdf, grad, **kw)
    ev[3].record()
    torch.cuda.synchronize()
    return [ev[k].elapsed_time(ev[k + 1]) / INNER for k in range(3)], rec


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def time_case(eng, cam, depth, T_true, B, stride, reps):
    fop = (np.arange(B) % depth.shape[0]).astype(np.int32)
    T0 = pm.perturb(T_true[fop], 0.03, 2.0, seed=B)
    arms = dict(hip=eng, torch=TorchOps())

    def field(pts):
        with torch.no_grad():
            return eng.sdf_eval(pts, want_grad=True)
    rows = {k: dict(points_ms=[], field_ms=[], system_ms=[], iteration_wall_ms=[], refine_ms=[]) for k in arms}
    out = {}
    for rep in range(reps + 1):                                              # rep 0: the warm-up of every shape, not recorded
        for name, ops in arms.items():
            (p, f, s), rec = iteration_events(ops, eng, depth, T0, cam, fop, stride)
            w1, _ = wall(lambda: tracking.refine_pose(ops, depth, T0, cam, frame_of_pose=fop, stride=stride, iters=1, field=field))
            w2, res = wall(lambda: tracking.refine_pose(ops, depth, T0, cam, frame_of_pose=fop, stride=stride, field=field))
            if rep:
                for k, v in zip(("points_ms", "field_ms", "system_ms", "iteration_wall_ms", "refine_ms"), (p, f, s, w1, w2)):
                    rows[name][k].append(v)
            out[name] = (rec, res)
    H, W = depth.shape[1:]
    n_pix = -(-H // stride) * -(-W // stride)
    row = dict(B=B, n_pix=n_pix, points=B * n_pix)
    for name in arms:
        rec, res = out[name]
        row[name] = {k: float(np.median(v)) for k, v in rows[name].items()}
        row[name]["iteration_ms"] = row[name]["points_ms"] + row[name]["field_ms"] + row[name]["system_ms"]
        row[name]["refine_iterations"] = res.iterations.tolist()
        row[name]["refine_reasons"] = sorted(set(res.reason))
    # each arm read its own points (torch's matmul fuses its multiply-adds), so the fields differ in the last bits: H against H,
    # relative to H's largest entry
    a, b = out["hip"][0].cpu().numpy()[:, 10:31], out["torch"][0].cpu().numpy()[:, 10:31]
    row["H_rel_diff_hip_vs_torch"] = float((np.abs(a - b).max(1) / np.abs(a).max(1)).max())
    row["speedup_points_plus_system"] = (row["torch"]["points_ms"] + row["torch"]["system_ms"]) / (row["hip"]["points_ms"] + row["hip"]["system_ms"])
    row["speedup_refine"] = row["torch"]["refine_ms"] / row["hip"]["refine_ms"]
    return row


def accuracy(eng, cam, traj, n_kf, n_held=8):
    c = types.SimpleNamespace(**cam)
    ids = [int(48 * k + 24) for k in np.linspace(0, n_kf - 1, n_held).astype(int)]
    T_true = traj[ids].astype(np.float64)
    rng = np.random.RandomState(99)
    depth = torch.from_numpy(np.stack([synthetic.render_depth(traj[i], cam, rng, noise_std=0.01) for i in ids])).cuda()
    at_truth = tracking.pose_system(eng, depth, T_true, c)
    res = dict(held_out_frames=ids, stride=4, depth_noise_m=0.01,
               mean_abs_sdf_at_true_pose=float((at_truth.abs_sum / np.maximum(at_truth.used, 1)).mean()),
               used_fraction_at_true_pose=float((at_truth.used / np.maximum(at_truth.valid, 1)).mean()), perturbations={})
    for metres, degrees in ((0.03, 2.0), (0.08, 5.0)):
        T0 = pm.perturb(T_true, metres, degrees, seed=int(degrees))
        r = tracking.refine_pose(eng, depth, T0, c)
        bt, br = pm.pose_error(T0, T_true)
        at, ar = pm.pose_error(r.T_WC, T_true)
        res["perturbations"]["%.2f m / %g deg" % (metres, degrees)] = dict(
            before_m=dict(mean=float(bt.mean()), max=float(bt.max())), before_deg=dict(mean=float(br.mean()), max=float(br.max())),
            after_m=dict(mean=float(at.mean()), median=float(np.median(at)), max=float(at.max()), per_pose=at.tolist()),
            after_deg=dict(mean=float(ar.mean()), median=float(np.median(ar)), max=float(ar.max()), per_pose=ar.tolist()),
            iterations=r.iterations.tolist(), reasons=r.reason, final_huber_cost=[h[-1][0] for h in r.history],
            final_used=[h[-1][1] for h in r.history])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kf", type=int, default=12)
    ap.add_argument("--steps-per-kf", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pose_bench needs a HIP device: there is nothing to measure without one")
    cam = dict(synthetic.SCANNET_CAM)
    tr, traj, train = train_map(a.kf, a.steps_per_kf, cam)
    eng = tr.engine
    res = dict(commit=commit(), device=torch.cuda.get_device_name(0), reps=a.reps, training=train,
               timing="HIP events on the launch stream around %d back-to-back calls of each part of one iteration, per call; host clock around calls that end in the stream's "
                      "end for iteration_wall_ms (refine_pose, iters=1) and refine_ms (refine_pose, defaults); medians; one warm-up "
                      "per shape; the hip and torch arms alternate" % INNER,
               settings=dict(huber=0.05, trunc=0.3, damping=1e-6, tol=1e-6, iters=10, min_points=64), cases={})
    print(json.dumps(dict(training=train)), flush=True)
    res["accuracy_on_trained_map"] = accuracy(eng, cam, traj, a.kf)
    print(json.dumps(res["accuracy_on_trained_map"]), flush=True)
    for name, c, stride in (("680x1200 stride 8", dict(synthetic.REPLICA_CAM), 8), ("480x640 stride 4", cam, 4)):
        ids = [48 * k + 24 for k in range(5)]
        rng = np.random.RandomState(7)
        depth = torch.from_numpy(np.stack([synthetic.render_depth(traj[i], c, rng, noise_std=0.01) for i in ids])).cuda()
        cn = types.SimpleNamespace(**c)
        res["cases"][name] = {}
        for B in (1, 5, 20):
            row = time_case(eng, cn, depth, traj[ids].astype(np.float64), B, stride, a.reps)
            res["cases"][name]["B=%d" % B] = row
            print(json.dumps({name: {"B=%d" % B: row}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
