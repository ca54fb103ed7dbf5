#!/usr/bin/env python3
"""Exploration (isdf_amd.explore, isdf_amd/csrc/explore.hip): what frontiers, clusters and view gain cost, against
scipy.ndimage.label + numpy.bincount on the host and against the same voxel walk written in torch ops on the same GPU, and one
next_best_view end to end with its split.

    python tools/explore_bench.py [--sides 128 256] [--views 64 256] [--reps 5] [--out profiles/explore_bench.json]

Scene: the analytic room of isdf_amd.synthetic with the partition wall of the routing tests, on a side^3 grid of 6 / side metre
voxels; three 320 x 240 depth frames taken at the robot's place (tests/explore_model.room_first_views) are fused by
fusion.integrate, and explore.volume_states gives the state volume.  Timing: device-synchronised wall time, the median of --reps
windows after one warm-up; the HIP and torch arms of the view gain alternate inside every repetition.  The torch walk is the header's
sequence over all rays at once (one pass per step, left when no ray is active); whether its results equal the kernel's bit for bit is recorded
(`torch_equals_hip`).  A record, not a test bar."""
import argparse
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

from isdf_amd import explore, fusion, routing        # noqa: E402
from tests import explore_model as em                  # noqa: E402

CAM_FUSE = dict(H=240, W=320, fx=160.0, fy=160.0, cx=159.5, cy=119.5)
CAM_GAIN = types.SimpleNamespace(H=60, W=80, fx=40.0, fy=40.0, cx=39.5, cy=29.5)
T_MAX = 5.0


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return os.environ.get("ISDF_COMMIT", "unknown")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median(fn, reps):
    fn()
    t = [timed(fn)[0] for _ in range(reps)]
    return dict(ms=float(np.median(t)), spread=[float(min(t)), float(max(t))])


def room_state(eng, side):
    voxel = 6.0 / side
    vol = fusion.TsdfVolume((side,) * 3, voxel, (voxel / 2,) * 3, 4 * voxel, "cuda")
    T = em.room_first_views()
    depth = torch.from_numpy(np.stack([em.room_depth(t, CAM_FUSE) for t in T])).cuda()
    fusion.integrate(eng, vol, depth, torch.from_numpy(T).cuda(), types.SimpleNamespace(**CAM_FUSE))
    return vol, explore.volume_states(vol)


def torch_walk(state, grid, T, cam, H, W, t_min, t_max, distinct):
    """em.view_gain in torch ops on state's device: (unknown [B,H,W], depth [B,H,W], distinct [B] or None)"""
    dev = state.device
    dims = tuple(state.shape)
    flat = state.reshape(-1)
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    T = T.to(dev, torch.float32).reshape(-1, 4, 4)
    B = T.shape[0]
    rr, cc = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    x = ((cc.float() - cam.cx) / f(cam.fx))[None]      # tensor / tensor: torch turns a division by a Python scalar into a product
    y = ((rr.float() - cam.cy) / f(cam.fy))[None]
    g0, dg = [], []
    for a in range(3):
        dW = (T[:, a, 0, None, None] * x + T[:, a, 1, None, None] * y) + T[:, a, 2, None, None]
        g0.append(((T[:, a, 3] - grid.origin[a]) / f(grid.spacing[a]))[:, None, None].expand_as(dW).reshape(-1))
        dg.append((dW / f(grid.spacing[a])).reshape(-1))
    N = B * H * W
    view = torch.arange(B, device=dev).repeat_interleave(H * W)
    hit = torch.ones(N, dtype=torch.bool, device=dev)
    for v in g0 + dg:
        hit &= torch.isfinite(v)
    t0, t1 = torch.full((N,), t_min, device=dev), torch.full((N,), t_max, device=dev)
    for a in range(3):
        hi = float(dims[a]) - 0.5
        zero = dg[a] == 0
        hit &= ~(zero & ((g0[a] < -0.5) | (g0[a] >= hi)))
        ta, tb = (-0.5 - g0[a]) / dg[a], (hi - g0[a]) / dg[a]
        t0 = torch.where(zero | ~hit, t0, torch.maximum(t0, torch.minimum(ta, tb)))
        t1 = torch.where(zero | ~hit, t1, torch.minimum(t1, torch.maximum(ta, tb)))
    hit &= t0 < t1
    inf = f(float("inf"))
    cell, step, inv, tmax = [], [], [], []
    boundary = lambda a, c: torch.where(dg[a] == 0, inf, ((c.float() + 0.5 * step[a].float()) - g0[a]) * inv[a])
    for a in range(3):
        c = torch.clamp(torch.floor((g0[a] + t0 * dg[a]) + 0.5), 0.0, float(dims[a] - 1))
        cell.append(torch.where(hit, c, torch.zeros_like(c)).long())
        step.append(torch.where(dg[a] > 0, 1, -1))
        inv.append(1.0 / dg[a])
        tmax.append(boundary(a, cell[a]))
    count = torch.zeros(N, dtype=torch.int32, device=dev)
    depth = torch.zeros(N, device=dev)
    bits = torch.zeros(B, flat.numel(), dtype=torch.bool, device=dev) if distinct else None
    active, t_in = hit.clone(), t0.clone()
    for it in range(sum(dims)):
        if it % 8 == 0 and not bool(active.any()):
            break
        p = torch.where(active, (cell[0] * dims[1] + cell[1]) * dims[2] + cell[2], 0)
        v = flat[p]
        unk = active & (v == em.UNKNOWN)
        count += unk
        if distinct:
            bits[view[unk], p[unk]] = True
        occ = active & (v >= em.OCCUPIED)
        depth = torch.where(occ, t_in, depth)
        active &= ~occ
        ay = tmax[1] < tmax[0]
        mxy = torch.where(ay, tmax[1], tmax[0])
        az = tmax[2] < mxy
        t_in = torch.where(active, torch.where(az, tmax[2], mxy), t_in)
        active &= t_in < t1
        for a, sel in ((2, active & az), (1, active & ~az & ay), (0, active & ~az & ~ay)):
            cell[a] = torch.where(sel, cell[a] + step[a], cell[a])
            left = sel & ((cell[a] < 0) | (cell[a] >= dims[a]))
            active &= ~left
            cell[a] = torch.where(left, 0, cell[a])
            tmax[a] = torch.where(sel & ~left, boundary(a, cell[a]), tmax[a])
    return count.reshape(B, H, W), depth.reshape(B, H, W), bits.sum(1).int() if distinct else None


def side_case(eng, side, views, reps):
    vol, state = room_state(eng, side)
    host = state.cpu().numpy()
    row = dict(volume=[side] * 3, voxel_m=6.0 / side, states=[int((host == k).sum()) for k in range(3)])
    fr = explore.frontiers(eng, state)
    row.update(rounds=int(fr.rounds), converged=bool(fr.converged), frontiers=median(lambda: explore.frontiers(eng, state), reps))
    label = fr.label.clone()
    quiet = median(lambda: eng.frontier_relax(label, 8), reps)
    row["quiet_round_ms"] = quiet["ms"] / 8
    cl = explore.clusters(eng, fr)
    row.update(clusters=median(lambda: explore.clusters(eng, fr), reps), n_clusters=int(len(cl.root)), frontier_voxels=int(cl.size.sum()))
    # the host: scipy.ndimage.label with the 3 x 3 x 3 structure on the frontier mask + numpy.bincount
    from scipy import ndimage
    t0 = time.perf_counter()
    mask = em.frontier_mask(host)
    t1 = time.perf_counter()
    comp, m = ndimage.label(mask, structure=np.ones((3, 3, 3), int))
    sizes = np.bincount(comp[mask], minlength=m + 1)[1:]
    t2 = time.perf_counter()
    row["host"] = dict(mask_ms=(t1 - t0) * 1e3, label_bincount_ms=(t2 - t1) * 1e3, n_clusters=int(m),
                       sizes_equal=bool(np.array_equal(np.sort(sizes), np.sort(cl.size))))
    row["host_over_hip"] = (row["host"]["mask_ms"] + row["host"]["label_bincount_ms"]) / (row["frontiers"]["ms"] + row["clusters"]["ms"])
    # view gain: candidate poses of the room, tiled to the batch
    big = explore.clusters(eng, fr, min_size=20)
    cand = explore.candidate_views(host, vol, big, 16, 0.6, 0, em.ROOM_UP)
    row["gain"] = {}
    for B in views:
        T = torch.from_numpy(np.resize(cand.T_WC, (B, 4, 4)).astype(np.float32)).cuda()
        for distinct in (True, False):
            hip = lambda: explore.view_gain(eng, state, vol, T, CAM_GAIN, CAM_GAIN.H, CAM_GAIN.W, 0.0, T_MAX, distinct, ws_budget=1 << 40)
            ref = lambda: torch_walk(state, explore._grid(vol), T, CAM_GAIN, CAM_GAIN.H, CAM_GAIN.W, 0.0, T_MAX, distinct)
            a, b = hip(), ref()
            same = bool(torch.equal(a.unknown, b[0]) and torch.equal(a.depth, b[1]) and (not distinct or torch.equal(a.distinct, b[2])))
            th, tt = [], []
            for _ in range(reps):
                th.append(timed(hip)[0])
                tt.append(timed(ref)[0])
            steps = int(a.unknown.sum().item())
            row["gain"]["B%d_%s" % (B, "distinct" if distinct else "plain")] = dict(
                hip_ms=float(np.median(th)), hip_spread=[float(min(th)), float(max(th))], torch_ms=float(np.median(tt)),
                torch_spread=[float(min(tt)), float(max(tt))], torch_over_hip=float(np.median(tt) / np.median(th)),
                rays=B * CAM_GAIN.H * CAM_GAIN.W, unknown_voxels_passed=steps, torch_equals_hip=same)
            print(json.dumps({"side": side, "B": B, "distinct": distinct, **row["gain"]["B%d_%s" % (B, "distinct" if distinct else "plain")]}),
                  flush=True)
    # next_best_view end to end, and its stages one by one
    nbv_kw = dict(min_size=20, n_per_cluster=16, radius=0.6, up=em.ROOM_UP, t_max=T_MAX)
    # the robot stands where the first frames were taken: no frame measures the voxels round its own eye, the robot knows them free
    free = (state == explore.FREE).to(torch.uint8)
    r, c = int(np.ceil(0.2 / vol.spacing[0])), explore.voxel_of(vol, em.ROOM_ROBOT)[0]
    free[c[0] - r:c[0] + r + 1, c[1] - r:c[1] + r + 1, c[2] - r:c[2] + r + 1] = 1
    run = lambda: explore.next_best_view(eng, state, vol, em.ROOM_ROBOT, CAM_GAIN, CAM_GAIN.H, CAM_GAIN.W, free=free, **nbv_kw)
    nbv = run()
    split = {}
    split["frontiers_ms"], fr2 = timed(lambda: explore.frontiers(eng, state))
    split["clusters_ms"], cl2 = timed(lambda: explore.clusters(eng, fr2, min_size=20))
    split["candidates_ms"], cand2 = timed(lambda: explore.candidate_views(state, vol, cl2, 16, 0.6, 0, em.ROOM_UP))
    split["view_gain_ms"], _ = timed(lambda: explore.view_gain(eng, state, vol, cand2.T_WC, CAM_GAIN, CAM_GAIN.H, CAM_GAIN.W, 0.0, T_MAX))
    split["distance_field_ms"], field = timed(lambda: routing.distance_field(eng, free, explore.voxel_of(vol, em.ROOM_ROBOT)))
    split["route_rounds"] = int(field.rounds)
    row["next_best_view"] = dict(total=median(run, reps), split=split, candidates=None if nbv.table is None else int(len(nbv.table.cluster)),
                                 gain=nbv.gain, cost_m=nbv.cost, route_vertices=None if nbv.route is None else int(len(nbv.route)))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--views", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explore_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("explore_bench needs a HIP device: there is nothing to measure without one")
    from isdf_amd.engine import Engine, NetConfig
    eng = Engine(NetConfig(hidden=64, blocks=1), "cuda")
    res = dict(commit=commit(), device=torch.cuda.get_device_name(0), reps=a.reps, image=[CAM_GAIN.H, CAM_GAIN.W], t_max_m=T_MAX,
               timing="device-synchronised wall time, median of reps after one warm-up; HIP and torch arms alternate",
               not_measured="kernel trace, counters, a real sequence; tile cap, pixel tile and pointer jumping were not varied", sides={})
    for s in a.sides:
        res["sides"]["%d^3" % s] = side_case(eng, s, a.views, a.reps)
        print(json.dumps({k: v for k, v in res["sides"]["%d^3" % s].items() if k != "gain"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
