#!/usr/bin/env python3
"""Point visibility against posed depth frames: isdf_amd.metrics.visible_points (one isdf_visible_points launch over all frames)
against the route Trainer.eval_object_sdf took before it -- the predicate of geometry.frustum.is_visible_torch (frustum.py:87-133,
use_projection=True) as its eager torch chain, restated below because the tool runs where the reference is not installed -- on the
same GPU, at F in {60, 600} frames of 680 x 1200 and n in {1 000, 200 000} points.

Frames, poses and points are generated ON the device from a seed (600 frames are 1.96 GB).  Both arms start from T_WC, invert the
poses with torch.linalg.inv and end with the per-point count on the HOST (what eval_object_sdf consumes); the eager arm is also
timed as it literally ran, with the whole [F, n] mask copied to the host.  Per arm: two warm-up calls, then --reps windows of
back-to-back calls (each window at least --window-ms long), device-synchronised at both ends, the two arms alternating; the
figure is the median window divided by its calls.  Peak memory: torch's allocator high-water mark over one call, above what was
allocated before it.

    python tools/visible_bench.py [--reps 7] [--out profiles/visible_bench.json]"""
import argparse
import json
import math
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from isdf_amd import metrics        # noqa: E402

H, W = 680, 1200
CAM = types.SimpleNamespace(fx=600.0, fy=600.0, cx=599.5, cy=339.5)
TRUNC = 0.05                        # eval_object_sdf's


def device_frames(F, gen, dev="cuda"):
    """depth [F,H,W] (smooth 1.3-3.7 m plus noise, ~4 % zeros) and T_WC [F,4,4] (cameras on a 1 m circle, turning about the up
    axis and nodding), built on the device"""
    v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    depth = torch.empty(F, H, W, device=dev)
    for f in range(F):                                   # frame by frame: no [F,H,W] temporary beside the result
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


def eager_mask(pts, poses_WC, frames, cam, trunc):
    """The eager route, operation for operation what eval_object_sdf's former call cost: a batched inverse, the [F,4,n] and [F,3,n]
    matrix products, one division, four comparisons, the int64 pixel tensor, a boolean-mask compaction (a host synchronisation),
    the gather and the scatter back -- every intermediate of size F * n.  Returns the bool [F, n] mask."""
    dev = pts.device
    n_frames = frames.shape[0]
    intrinsics = torch.tensor([[cam.fx, 0.0, cam.cx], [0.0, cam.fy, cam.cy], [0.0, 0.0, 1.0]], dtype=torch.float32, device=dev)
    pts_h = torch.cat([pts, pts.new_ones(pts.shape[0], 1)], dim=1).t()                      # [4, n]
    cam_pts = (torch.linalg.inv(poses_WC) @ pts_h)[:, :3]                                    # [F, 3, n]
    proj = intrinsics @ cam_pts
    zc = proj[:, 2]
    pix = (proj[:, :2] / zc.unsqueeze(1)).permute(0, 2, 1)                                   # [F, n, 2] = (u, v)
    in_image = (pix[..., 0] > 0) & (pix[..., 0] < W) & (pix[..., 1] > 0) & (pix[..., 1] < H)
    hit = pix.long()[in_image]                                                               # the compaction
    which = torch.arange(n_frames, device=dev).repeat_interleave(in_image.sum(dim=1))
    limit = torch.full(in_image.shape, float("-inf"), device=dev)
    limit[in_image] = frames[which, hit[:, 1], hit[:, 0]] + trunc
    return in_image & (zc > 0) & (zc < limit)


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return int(torch.cuda.max_memory_allocated() - before)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--frames", type=int, nargs="+", default=[60, 600])
    ap.add_argument("--points", type=int, nargs="+", default=[1000, 200000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("visible_bench: no GPU visible -- nothing is measured without one")
    from isdf_amd.engine import Engine, NetConfig
    eng = Engine(NetConfig(hidden=64, blocks=1), "cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    depth_all, T_all = device_frames(max(a.frames), gen)
    res = dict(device=torch.cuda.get_device_name(0), frame=[H, W], trunc=TRUNC, reps=a.reps, window_ms=a.window_ms,
               timing="device-synchronised wall time per call (T_WC in, per-point count on the host out), median over windows of "
                      "back-to-back calls; the two arms alternate in one process", cases={})
    for F in a.frames:
        depth, T_WC = depth_all[:F], T_all[:F]
        for n in a.points:
            pts = (torch.rand(n, 3, device="cuda", generator=gen) - 0.5) * 8.0
            kernel = lambda: metrics.visible_points(eng, pts, T_WC, depth, CAM, trunc=TRUNC)[0].cpu()
            eager = lambda: eager_mask(pts, T_WC, depth, CAM, TRUNC).sum(0).cpu()
            literal = lambda: eager_mask(pts, T_WC, depth, CAM, TRUNC).detach().cpu().numpy().sum(axis=0) > 0
            T_CW = torch.linalg.inv(T_WC)
            launches = lambda: eng.visible_points(pts, T_CW, depth, CAM, trunc=TRUNC)     # the entry point alone: no inverse, no copy
            arms = (("kernel", kernel), ("eager", eager), ("literal", literal), ("launches", launches))
            times = {}
            calls = {}
            for name, fn in arms:
                fn()
                first = window(fn, 1)                                   # second warm-up call, and the size of a window
                calls[name] = max(1, int(math.ceil(a.window_ms / max(first, 1e-3))))
                times[name] = []
            for _ in range(a.reps):
                for name, fn in arms:
                    times[name].append(window(fn, calls[name]))
            ck, ce = kernel().numpy().astype(np.int64), eager().numpy().astype(np.int64)
            case = dict(frames=F, points=n, pairs=F * n,
                        kernel_ms=float(np.median(times["kernel"])), eager_ms=float(np.median(times["eager"])),
                        eager_mask_to_host_ms=float(np.median(times["literal"])),
                        entry_point_alone_ms=float(np.median(times["launches"])),
                        kernel_ms_spread=[float(min(times["kernel"])), float(max(times["kernel"]))],
                        eager_ms_spread=[float(min(times["eager"])), float(max(times["eager"]))],
                        calls_per_window=calls,
                        kernel_peak_bytes=peak_bytes(lambda: metrics.visible_points(eng, pts, T_WC, depth, CAM, trunc=TRUNC)),
                        eager_peak_bytes=peak_bytes(lambda: eager_mask(pts, T_WC, depth, CAM, TRUNC).sum(0)),
                        visible_pair_share=float(ck.sum()) / (F * n), points_seen=int((ck > 0).sum()),
                        points_whose_count_differs=int((ck != ce).sum()))
            case["eager_over_kernel"] = case["eager_ms"] / case["kernel_ms"]
            case["eager_over_kernel_peak_bytes"] = case["eager_peak_bytes"] / max(case["kernel_peak_bytes"], 1)
            res["cases"]["F%d_n%d" % (F, n)] = case
            print(json.dumps(case), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    # the eager chain multiplies through rocBLAS (its own summation order): a pair on a limit may fall the other way, no more
    bad = [k for k, c in res["cases"].items() if c["points_whose_count_differs"] > max(2, c["points"] // 100)]
    if bad:
        raise SystemExit("visible_bench: the two arms disagree on more than 1 %% of the points in %s" % bad)


if __name__ == "__main__":
    main()
