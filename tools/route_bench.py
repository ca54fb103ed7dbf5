#!/usr/bin/env python3
"""Routing (isdf_amd.routing, isdf_amd/csrc/route.hip): what the geodesic field costs, against the same relaxation written in torch
ops and against variants of the kernel, and plan_route end to end beside plan_path.

    python tools/route_bench.py [--sides 128 256] [--reps 5] [--variants name=path/to/lib.so ...] [--variant-reps 3] [--out profiles/route_bench.json]

Scene: the analytic room of isdf_amd.synthetic with the partition wall of tests/test_route_gpu.py (x in [2.85, 3.15], z > 1.2; the
door is z < 1.2), sampled at side^3 voxels of max(6, 3, 5) / side metres, robot radius 0.15 m plus the margin of
routing.free_space; the goal is (5.0, 1.5, 4.0).  Per side: rounds to convergence, the time of one round (a window of
back-to-back Engine.route_relax calls on a converged field, device-synchronised at both ends -- every launch then runs ONE sweep
per tile, the kernel's floor), the total time of routing.distance_field (init, rounds in groups of 8, one 32-byte copy per
group; median of --reps, after one warm-up), and the same Jacobi update in torch ops (26 shifted minima per sweep; the time of a
sweep, and the sweeps it needs, counted by running it to its fixed point once, which must equal the kernel's field bit for bit).

--variants: other builds of the library (tools/build_variants.py, e.g. inner4='sed:route.hip:s/ROUTE_INNER = 8;/ROUTE_INNER = 4;/'
or plain=@tools/variants/route_plain_sweep.patch, the one-voxel-per-thread sweep without LDS).  Each is measured in a fresh child
process with ISDF_HIP_LIB set, the set repeated --variant-reps times in turn so that the arms alternate; their fields are compared with
the shipped library's by checksum.

End to end: routing.plan_route and planning.plan_path on the 60 x 30 x 50 grid of the test, the closed-form field supplied as
`field=`: wall time (device-synchronised, median of --reps) and what each returns.  A record, not a test bar."""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from isdf_amd import planning, routing, synthetic        # noqa: E402

WALL_LO, WALL_HI = (2.85, 0.0, 1.2), (3.15, 3.0, 5.0)
START, GOAL, RADIUS = (1.0, 1.5, 4.0), (5.0, 1.5, 4.0), 0.15


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return os.environ.get("ISDF_COMMIT", "unknown")


def scene_field(pts):
    """(sdf, grad) float32 on pts' device: min(synthetic.gt_sdf, box SDF of the wall) in torch float64 and its gradient"""
    p = pts.detach().to(torch.float64).requires_grad_(True)
    t = lambda v: torch.tensor(np.asarray(v, np.float64), dtype=torch.float64, device=p.device)
    with torch.enable_grad():
        d = torch.minimum(p - t(synthetic.ROOM_LO), t(synthetic.ROOM_HI) - p).min(-1).values
        for c, r in synthetic.SPHERES:
            d = torch.minimum(d, torch.linalg.norm(p - t(c), dim=-1) - r)
        for lo, hi in list(synthetic.BOXES) + [(WALL_LO, WALL_HI)]:
            q = torch.maximum(t(lo) - p, p - t(hi))
            d = torch.minimum(d, torch.linalg.norm(torch.clamp(q, min=0.0), dim=-1) + torch.clamp(q.max(-1).values, max=0.0))
        g, = torch.autograd.grad(d.sum(), p)
    return d.detach().to(torch.float32), g.to(torch.float32)


def scene(dims, voxel):
    """(free u8 dims on the device, index_to_world [3,4]): voxel (i, j, k) centred at (i + 0.5, j + 0.5, k + 0.5) * voxel"""
    A = np.array([[voxel, 0, 0, voxel / 2], [0, voxel, 0, voxel / 2], [0, 0, voxel, voxel / 2]])
    ax = [torch.arange(n, device="cuda", dtype=torch.float32) * voxel + voxel / 2 for n in dims]
    pts = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    sdf = torch.cat([scene_field(c)[0] for c in pts.split(1 << 20)])
    return routing.free_space(sdf.reshape(dims), RADIUS, voxel=voxel).contiguous(), A


def torch_sweep(dist, free, none):
    """one Jacobi sweep of the header's update in torch ops: 26 shifted minima over a NONE-padded copy"""
    nx, ny, nz = dist.shape
    pad = torch.nn.functional.pad(dist, (1, 1, 1, 1, 1, 1), value=none)
    best = dist
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            for dk in (-1, 0, 1):
                if di or dj or dk:
                    w = 2 + (di != 0) + (dj != 0) + (dk != 0)
                    best = torch.minimum(best, pad[1 + di:1 + di + nx, 1 + dj:1 + dj + ny, 1 + dk:1 + dk + nz] + w)
    return torch.where(free != 0, best, dist)


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def field_case(eng, side, reps, with_torch):
    voxel = 6.0 / side
    free, A = scene((side,) * 3, voxel)
    goal = routing.snap(A, GOAL)
    f = routing.distance_field(eng, free, goal)                     # warm-up, and the field itself
    host = f.dist.cpu().numpy()
    row = dict(volume=[side] * 3, voxel_m=voxel, free_share=float(free.float().mean()), converged=bool(f.converged), rounds=int(f.rounds),
               launches=2 * int(f.rounds), reached_share=float((f.dist < routing.NONE).float().mean()),
               farthest_cost=int(host[host < routing.NONE].max()), crc32=zlib.crc32(host.tobytes()))
    total = [window(lambda: routing.distance_field(eng, free, goal), 1) for _ in range(reps)]
    row.update(total_ms=float(np.median(total)), total_ms_spread=[float(min(total)), float(max(total))])
    dist = f.dist.clone()
    quiet = [window(lambda: eng.route_relax(free, dist, 8), 4) / 8 for _ in range(reps)]
    row.update(quiet_round_ms=float(np.median(quiet)), mean_round_ms=row["total_ms"] / (8 * -(-f.rounds // 8)))
    if with_torch:
        none = routing.NONE
        d = eng.route_init(free, goal)
        sweeps = 0
        while True:
            new = torch_sweep(d, free, none)
            sweeps += 1
            if torch.equal(new, d):
                break
            d = new
        sweep = [window(lambda: torch_sweep(d, free, none), 4) for _ in range(reps)]
        row.update(torch_sweeps=sweeps, torch_sweep_ms=float(np.median(sweep)), torch_total_ms_estimate=sweeps * float(np.median(sweep)),
                   torch_field_equals_hip=bool(torch.equal(d, f.dist)))
        row["torch_over_hip_total"] = row["torch_total_ms_estimate"] / row["total_ms"]
    return row


def end_to_end(eng, reps):
    dims, voxel = (60, 30, 50), 0.1
    free, A = scene(dims, voxel)
    kw = dict(radii=RADIUS, field=scene_field)

    def route_arm():
        return routing.plan_route(eng, START, GOAL, free, A, **kw)

    def path_arm():
        return planning.plan_path(eng, START, GOAL, **kw)
    out = {}
    for name, fn in (("plan_route", route_arm), ("plan_path", path_arm)):
        fn()
        out[name] = dict(times=[])
    for _ in range(reps):
        for name, fn in (("plan_route", route_arm), ("plan_path", path_arm)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            out[name]["times"].append((time.perf_counter() - t0) * 1e3)
            out[name]["result"] = r
    rows = {}
    for name, o in out.items():
        res, best = o["result"][0], o["result"][1]
        rec = res.records
        rows[name] = dict(wall_ms=float(np.median(o["times"])), wall_ms_spread=[float(min(o["times"])), float(max(o["times"]))],
                          seeds=int(res.x.shape[0]), iterations=int(res.iterations), best=best,
                          seeds_free_of_collision=int((rec.in_collision == 0).sum()),
                          best_min_clearance_m=None if best is None else float(rec.min_clearance[best]),
                          best_length_m=None if best is None else float(rec.length[best]))
    t = [window(lambda: routing.route(eng, free, A, START, GOAL), 1) for _ in range(reps)]
    line = routing.route(eng, free, A, START, GOAL)
    rows["route_alone"] = dict(wall_ms=float(np.median(t)), vertices=int(len(line)),
                               length_m=float(np.linalg.norm(np.diff(line, axis=0), axis=1).sum()),
                               w_obs=routing.hold_weight(float(np.linalg.norm(np.diff(line, axis=0), axis=1).sum())))
    rows["grid"] = dict(dims=list(dims), voxel_m=voxel, radius_m=RADIUS, field="closed form, supplied as field=")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--variants", nargs="*", default=[])
    ap.add_argument("--variant-reps", type=int, default=3)
    ap.add_argument("--child", action="store_true", help="measure the fields with the loaded library and print one JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "route_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("route_bench needs a HIP device: there is nothing to measure without one")
    from isdf_amd.engine import Engine, NetConfig
    eng = Engine(NetConfig(hidden=64, blocks=1), "cuda")
    if a.child:
        print("ROUTE_BENCH_CHILD " + json.dumps({"%d^3" % s: field_case(eng, s, a.reps, False) for s in a.sides}), flush=True)
        return
    res = dict(commit=commit(), device=torch.cuda.get_device_name(0), reps=a.reps,
               timing="device-synchronised wall time, median of reps after one warm-up; variants: fresh child processes in turn")
    res["field"] = {}
    for s in a.sides:
        res["field"]["%d^3" % s] = field_case(eng, s, a.reps, True)
        print(json.dumps({"%d^3" % s: res["field"]["%d^3" % s]}), flush=True)
    res["end_to_end"] = end_to_end(eng, a.reps)
    print(json.dumps(res["end_to_end"]), flush=True)
    if a.variants:
        libs = [("shipped", os.path.join(ROOT, "isdf_amd", "libisdf_hip.so"))] + [tuple(v.split("=", 1)) for v in a.variants]
        runs = {name: [] for name, _ in libs}
        for _ in range(a.variant_reps):
            for name, lib in libs:
                env = dict(os.environ, ISDF_HIP_LIB=os.path.abspath(lib))
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", "3", "--sides"]
                                     + [str(s) for s in a.sides], env=env, capture_output=True, text=True, timeout=600)
                if out.returncode != 0:
                    sys.exit("variant %s failed (%d):\n%s" % (name, out.returncode, out.stderr[-2000:]))
                line = [ln for ln in out.stdout.splitlines() if ln.startswith("ROUTE_BENCH_CHILD ")][-1]
                runs[name].append(json.loads(line.split(" ", 1)[1]))
                print("variant %s: %s" % (name, {k: round(v["total_ms"], 2) for k, v in runs[name][-1].items()}), flush=True)
        res["variants"] = {}
        for name, rs in runs.items():
            res["variants"][name] = {}
            for key in rs[0]:
                tot = [r[key]["total_ms"] for r in rs]
                res["variants"][name][key] = dict(rounds=rs[0][key]["rounds"], total_ms=float(np.median(tot)),
                                                  total_ms_spread=[float(min(tot)), float(max(tot))],
                                                  quiet_round_ms=float(np.median([r[key]["quiet_round_ms"] for r in rs])),
                                                  field_equals_shipped=rs[0][key]["crc32"] == runs["shipped"][0][key]["crc32"])
        print(json.dumps(res["variants"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
