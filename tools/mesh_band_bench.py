#!/usr/bin/env python3
"""Narrow-band surface extraction against the dense path on the trained default net (fixture `trained_default`) over its
bounds box: what fraction of the grid the band evaluates per level, and where the time goes.

    python tools/mesh_band_bench.py [--dims 256 512 1024] [--reps 5] [--out profiles/mesh_band_bench.json]
    python tools/mesh_band_bench.py --scan [--out profiles/mesh_band_slack_scan.json]

Timing: HIP events on the launch stream, one warm-up of every shape, then `--reps` repeats with the two paths alternating;
medians.  band total = Engine.band_volume + Engine.marching_cubes, events around the whole call (it includes the host's
per-level count reads); network = the events around every field call inside it; selection = band_volume - network; the dense
path = Engine.sdf_eval over the cached full grid (as get_sdf_grid holds grid_pc; making the grid is not timed) +
Engine.marching_cubes.  The band's positions are made inside the selection and are part of its time.

--scan: the smallest slack, in steps of 0.25, at which the band mesh equals the dense mesh bit for bit, for `trained_default`
and `trained_franka` at dims 96 and 129 (DEFAULT_SLACK is 1.5 x the largest, at least 1.5)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import golden_util as gu            # noqa: E402


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return os.environ.get("ISDF_COMMIT", "unknown")


def engine_of(g):
    from isdf_amd.engine import Engine, NetConfig
    H, B, nf, si, so = g["net"]
    eng = Engine(NetConfig(hidden=int(H), blocks=int(B), n_freqs=int(nf), scale_input=float(si), scale_output=float(so),
                           transform=g["bounds_T"]), "cuda")
    eng.load_params(gu.params_of(g))
    return eng


def bounds_affine(g, dim):
    """the index -> world affine of a dim^3 grid over the fixture's bounds box (set_scene_properties' extents / 0.9)"""
    from isdf_amd.mesh import grid_index_to_world
    T_bounds = np.linalg.inv(g["bounds_T"].astype(np.float64))
    pc = g["eval/pc"].reshape(-1, 3).astype(np.float64)
    local = (pc - T_bounds[:3, 3]) @ T_bounds[:3, :3]
    scale = 2 * np.abs(local).max(0) / (2 * 0.9)
    return grid_index_to_world(dim, scale, T_bounds)


class Events:
    def __init__(self):
        self.pairs = []

    def span(self):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.pairs.append((a, b))
        return a, b

    def ms(self):
        return sum(a.elapsed_time(b) for a, b in self.pairs)


def run_band(eng, dim, A, slack, coarse):
    net, whole, mc = Events(), Events(), Events()

    def field(p):
        a, b = net.span()
        a.record()
        out = eng.sdf_eval(p)
        b.record()
        return out
    a, b = whole.span()
    a.record()
    vol, st = eng.band_volume(dim, A, slack=slack, coarse=coarse, field=field)
    b.record()
    a, b = mc.span()
    a.record()
    mesh = eng.marching_cubes(vol, 0.0, A)
    b.record()
    torch.cuda.synchronize()
    t = dict(selection_ms=whole.ms() - net.ms(), network_ms=net.ms(), mc_ms=mc.ms(), total_ms=whole.ms() + mc.ms())
    return t, st, mesh


def run_dense(eng, dim, A, pts):
    net, mc = Events(), Events()
    a, b = net.span()
    a.record()
    vol = eng.sdf_eval(pts).view(dim, dim, dim)
    b.record()
    a, b = mc.span()
    a.record()
    mesh = eng.marching_cubes(vol, 0.0, A)
    b.record()
    torch.cuda.synchronize()
    return dict(network_ms=net.ms(), mc_ms=mc.ms(), total_ms=net.ms() + mc.ms()), mesh


def median(rows):
    return {k: float(np.median([r[k] for r in rows])) for k in rows[0]}


def bench(a):
    from isdf_amd.mesh import DEFAULT_SLACK, grid_points
    g = gu.load("trained_default")
    eng = engine_of(g)
    slack = DEFAULT_SLACK if a.slack is None else a.slack
    res = dict(commit=commit(), device=torch.cuda.get_device_name(0), reps=a.reps, slack=slack, coarse=a.coarse,
               timing="HIP events on the launch stream, medians; one warm-up per shape; band and dense alternate", dims={})
    for dim in a.dims:
        A = bounds_affine(g, dim)
        row = dict(points=dim ** 3)
        dense_ok = dim <= a.dense_max
        pts = grid_points(dim, A, "cuda") if dense_ok else None
        run_band(eng, dim, A, slack, a.coarse)
        if dense_ok:
            run_dense(eng, dim, A, pts)
        tb, td = [], []
        for _ in range(a.reps):
            t, st, mb = run_band(eng, dim, A, slack, a.coarse)
            tb.append(t)
            if dense_ok:
                t, md = run_dense(eng, dim, A, pts)
                td.append(t)
        row["band"] = dict(median(tb), fraction=st["fraction"], evaluated=st["evaluated"], leaks=st["leaks"],
                           levels=[dict(l, fraction=l["evaluated"] / dim ** 3) for l in st["levels"]],
                           vertices=int(mb[0].shape[0]), faces=int(mb[1].shape[0]))
        if dense_ok:
            same = all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(mb, md))
            row["dense"] = dict(median(td), vertices=int(md[0].shape[0]), faces=int(md[1].shape[0]))
            row["band_equals_dense_bitwise"] = bool(same)
            row["speedup_total"] = row["dense"]["total_ms"] / row["band"]["total_ms"]
        else:
            row["dense"] = "not measured (--dense-max %d)" % a.dense_max
        res["dims"][str(dim)] = row
        print(json.dumps({str(dim): row}), flush=True)
        del pts
        torch.cuda.empty_cache()
    return res


def scan(a):
    from isdf_amd.mesh import extract_surface, grid_points
    res = dict(commit=commit(), device=torch.cuda.get_device_name(0), step=0.25, nets={})
    for name in ("trained_default", "trained_franka"):
        try:
            g = gu.load(name)
            eng = engine_of(g)
        except Exception as e:                                          # the weights did not load: say so in the record
            res["nets"][name] = "not measured: %s" % e
            continue
        res["nets"][name] = {}
        for dim in (96, 129):
            A = bounds_affine(g, dim)
            dense = eng.marching_cubes(eng.sdf_eval(grid_points(dim, A, "cuda")).view(dim, dim, dim), 0.0, A)
            rows, smallest = [], None
            for q in range(1, 17):
                slack = 0.25 * q
                v, f, n, st = extract_surface(eng, dim, A, slack=slack, widen=False)
                same = all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip((v, f, n), dense))
                rows.append(dict(slack=slack, complete=bool(same), leaks=st["leaks"], fraction=st["fraction"],
                                 faces=int(f.shape[0]), dense_faces=int(dense[1].shape[0])))
                if same and smallest is None:
                    smallest = slack
            res["nets"][name][str(dim)] = dict(smallest_complete_slack=smallest, rows=rows)
            print(json.dumps({name: {str(dim): dict(smallest_complete_slack=smallest,
                                                    rows=[(r["slack"], r["complete"], r["leaks"], round(r["fraction"], 4)) for r in rows])}}),
                  flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slack", type=float, default=None)
    ap.add_argument("--coarse", type=int, default=8)
    ap.add_argument("--dense-max", type=int, default=1024, help="largest dim the dense path is run at")
    ap.add_argument("--scan", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mesh_band_bench needs a HIP device: there is nothing to measure without one")
    res = scan(a) if a.scan else bench(a)
    out = a.out or os.path.join(ROOT, "profiles", "mesh_band_slack_scan.json" if a.scan else "mesh_band_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
