#!/usr/bin/env python3
"""Planning against the map (isdf_amd.planning, isdf_amd/csrc/traj.hip): what an iteration costs.

    python tools/plan_bench.py [--reps 20] [--out profiles/plan_bench.json]

Cases: B in {1, 64, 1024} trajectories of T = 64 waypoints, S in {1, 8} body spheres, seeds of `seed_trajectories` through the
synthetic room, the default-shape network at its initial weights as the field (the cost of the field call does not depend on
the weights; nothing here says anything about plans through a trained map, which is unmeasured).

Timing: HIP events on the launch stream around ten back-to-back calls each of the field call (Engine.sdf_eval with gradient) and
of the step launch, per call; one warm-up per shape, `--reps` repeats, medians; the two arms alternate.  `loop_ms_per_iteration`
is a host clock around `optimise_trajectories(iters=50, check_every=50, tol=0)` (ends in the records' copy and the stream's
end), divided by 50.  The comparison partner (`torch`) is the same step written in eager torch ops on the same device around the
same Engine.sdf_eval, in float64, the tridiagonal solve by the same closed form through cumsum.  There is no parent-commit
figure: the parent has no such call.  A record, not a test bar."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from isdf_amd import planning        # noqa: E402


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return os.environ.get("ISDF_COMMIT", "unknown")


class TorchOps:
    """Engine.traj_points / Engine.traj_step written in torch ops: the comparison partner"""

    def __init__(self, eng):
        self.device = eng.device
        self.sdf_eval = eng.sdf_eval

    @staticmethod
    def traj_points(x, offsets, radii=0.0):
        off = torch.as_tensor(np.asarray(offsets, np.float32), device=x.device)
        return (x[:, :, None, :] + off[None, None]).reshape(-1, 3)

    def traj_step(self, x, state, offsets, radii, sdf, grad, eps=0.2, w_obs=8.0, w_smooth=1.0, eta=8.0, max_step=0.05, tol=1e-5,
                  out=None, q_out=None, want_grad=False):
        B, T = x.shape[:2]
        dev = x.device
        eps, w_obs, w_smooth, eta, max_step, tol = (float(np.float32(v)) for v in (eps, w_obs, w_smooth, eta, max_step, tol))
        rad = torch.as_tensor(np.broadcast_to(np.asarray(radii, np.float64).reshape(-1), (np.asarray(offsets).reshape(-1, 3).shape[0],)).copy(),
                              device=dev)
        S = rad.numel()
        xd, s, g = x.double(), sdf.reshape(B, T, S).double(), grad.reshape(B, T, S, 3).double()
        ok = torch.isfinite(s) & torch.isfinite(g).all(-1)
        n_bad = (~torch.isfinite(s)).sum((1, 2)) + (~torch.isfinite(g)).sum((1, 2, 3))
        d = torch.where(ok, s - rad, torch.full_like(s, float("inf")))
        u = d - eps
        c = torch.where(d < 0, -d + eps * 0.5, torch.where(d <= eps, u * u / (2 * eps), torch.zeros_like(d)))
        cp = torch.where(d < 0, -torch.ones_like(d), torch.where(d <= eps, u / eps, torch.zeros_like(d)))
        C = c.sum(-1)
        C[:, 0] = 0
        C[:, -1] = 0
        G = (cp[..., None] * torch.where(ok[..., None], g, torch.zeros_like(g))).sum(2)
        v = (xd[:, 2:] - xd[:, :-2]) * 0.5
        sigma = v.norm(dim=-1)
        vh = torch.where(sigma[..., None] > 0, v / sigma[..., None].clamp_min(1e-300), torch.zeros_like(v))
        cv = torch.zeros(B, T, 3, dtype=torch.float64, device=dev)
        cv[:, 1:-1] = C[:, 1:-1, None] * vh
        e = xd[:, 1:] - xd[:, :-1]
        seg2 = (e * e).sum(-1)
        gr = torch.zeros(B, T, 3, dtype=torch.float64, device=dev)
        gr[:, 1:-1] = w_obs * (sigma[..., None] * G[:, 1:-1] + (cv[:, :-2] - cv[:, 2:]) * 0.5) \
            + w_smooth * (T - 1) * (2 * xd[:, 1:-1] - xd[:, :-2] - xd[:, 2:])
        n = T - 2
        i = torch.arange(1, n + 1, dtype=torch.float64, device=dev)[None, :, None]
        w = (n + 1) - i
        gi = gr[:, 1:-1]
        P = torch.cumsum(i * gi, 1)
        tail = torch.flip(torch.cumsum(torch.flip(w * gi, [1]), 1), [1])
        Q = torch.cat([tail[:, 1:], torch.zeros_like(tail[:, :1])], 1)
        delta = -((w * P + i * Q) / (n + 1)) / (eta * (T - 1))
        m = delta.norm(dim=-1).max(1).values
        moving = state == 0
        st = torch.where(moving & (n_bad > 0), torch.full_like(state, 2), torch.where(moving & (m < tol), torch.ones_like(state), state))
        apply = moving & (st == 0)
        kappa = torch.where(m <= max_step, torch.ones_like(m), max_step / m.clamp_min(1e-300)) * apply
        x[:, 1:-1] = (xd[:, 1:-1] + kappa[:, None, None] * delta).float()
        state.copy_(st)
        rec = out if out is not None else torch.empty(B, 16, dtype=torch.float64, device=dev)
        rec.zero_()
        rec[:, 0], rec[:, 1] = (C[:, 1:-1] * sigma).sum(1), 0.5 * (T - 1) * seg2.sum(1)
        rec[:, 2], rec[:, 3], rec[:, 4] = d.reshape(B, -1).min(1).values, (d < 0).reshape(B, -1).sum(1), (d < eps).reshape(B, -1).sum(1)
        rec[:, 5], rec[:, 6], rec[:, 7] = (gr * gr).sum((1, 2)), m * moving, kappa
        rec[:, 8], rec[:, 9], rec[:, 10] = n_bad, st, seg2.sqrt().sum(1)
        if q_out is not None:
            q_out.copy_(self.traj_points(x, offsets).view_as(q_out))
        return (rec, gr) if want_grad else rec


INNER = 10      # back-to-back calls between one pair of events


def events(ops, eng, x0, off, rad):
    """(field_ms, step_ms) per call: HIP events around INNER back-to-back calls of each"""
    x = x0.clone()
    state = torch.zeros(x.shape[0], dtype=torch.int32, device=x.device)
    q = ops.traj_points(x, off, rad).contiguous()
    rec = torch.empty(x.shape[0], 16, dtype=torch.float64, device=x.device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    with torch.no_grad():
        for _ in range(INNER):
            sdf, grad = eng.sdf_eval(q, want_grad=True)
    ev[1].record()
    for _ in range(INNER):
        ops.traj_step(x, state, off, rad, sdf, grad, out=rec, q_out=q)
    ev[2].record()
    torch.cuda.synchronize()
    return [ev[k].elapsed_time(ev[k + 1]) / INNER for k in range(2)], rec.cpu().numpy()


def time_case(eng, B, S, reps):
    T = 64
    x0 = torch.from_numpy(planning.seed_trajectories((0.4, 2.2, 1.5), (2.8, 2.2, 1.7), T, B, seed=B)).cuda()
    off = np.zeros((S, 3), np.float32)
    off[:, 0] = 0.05 * np.arange(S)
    rad = np.full(S, 0.1, np.float32)
    arms = dict(hip=eng, torch=TorchOps(eng))
    rows = {k: dict(field_ms=[], step_ms=[], loop_ms_per_iteration=[]) for k in arms}
    recs = {}
    for rep in range(reps + 1):                                              # rep 0: the warm-up of every shape, not recorded
        for name, ops in arms.items():
            (f, s), recs[name] = events(ops, eng, x0, off, rad)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            planning.optimise_trajectories(ops, x0, offsets=off, radii=rad, iters=50, check_every=50, tol=0.0)
            torch.cuda.synchronize()
            loop = (time.perf_counter() - t0) * 1e3 / 50
            if rep:
                for k, v in zip(("field_ms", "step_ms", "loop_ms_per_iteration"), (f, s, loop)):
                    rows[name][k].append(v)
    row = dict(B=B, T=T, S=S, points=B * T * S)
    for name in arms:
        row[name] = {k: float(np.median(v)) for k, v in rows[name].items()}
    a, b = recs["hip"], recs["torch"]
    row["cost_rel_diff_hip_vs_torch"] = float((np.abs(a[:, :2] - b[:, :2]) / np.maximum(np.abs(a[:, :2]), 1e-300)).max())
    row["speedup_step"] = row["torch"]["step_ms"] / row["hip"]["step_ms"]
    row["speedup_loop"] = row["torch"]["loop_ms_per_iteration"] / row["hip"]["loop_ms_per_iteration"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("plan_bench needs a HIP device: there is nothing to measure without one")
    from isdf_amd.engine import Engine, NetConfig
    eng = Engine(NetConfig(), "cuda")
    res = dict(commit=commit(), device=torch.cuda.get_device_name(0), reps=a.reps,
               timing="HIP events on the launch stream around %d back-to-back calls of the field call and of the step launch, per call; "
                      "host clock around optimise_trajectories(iters=50, check_every=50, tol=0) divided by 50 for loop_ms_per_iteration; "
                      "medians; one warm-up per shape; the hip and torch arms alternate" % INNER,
               field="default-shape network at its initial weights", plans_on_a_trained_map="unmeasured",
               settings=dict(planning.DEFAULTS), cases={})
    for S in (1, 8):
        for B in (1, 64, 1024):
            row = time_case(eng, B, S, a.reps)
            res["cases"]["B=%d S=%d" % (B, S)] = row
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
