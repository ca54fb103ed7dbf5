#!/usr/bin/env python3
"""Ground truth from a mesh through the tile index (isdf_amd.mesh_sdf accel="tiles", isdf_amd/csrc/tri_tiles.hip) against the brute
force it must equal (accel=None, isdf_amd/csrc/tri.hip), the same calls on the same machine.

    python tools/mesh_sdf_tiles_bench.py [--reps 5] [--out profiles/mesh_sdf_tiles_bench.json]

  * surface_distance and mesh_sdf at --points x --triangles (about 1 M x 100 k: tools/mesh_sdf_bench.py's icosphere soup);
  * mesh_volume at --volume^3 on the synthetic room at k = 3 (3 876 faces) and k = 6 (245 796 faces);
  * mesh_accuracy_completion at --samples samples, the room at k = 6 against the room at k = 3;
  * per workload the share of tiles x blocks staged for the distance and as near (the call's stats), the one-off cost of building the
    index, that distance bits and indices agree, and the largest winding difference to brute force on --check of the points and on all;
  * for the first workload, where the culled call's time goes (`balance`).

Timing as tools/mesh_sdf_bench.py: warm-up calls (two; one where a call takes more than five seconds), then --reps calls, each
between device synchronisations; the figure is the median.  A record, not a test bar: no ratio was promised in advance."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from isdf_amd import mesh_sdf, synthetic        # noqa: E402
from isdf_amd.engine import morton_order        # noqa: E402
from mesh_sdf_bench import commit, soup         # noqa: E402


def timed(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    if time.perf_counter() - t <= 5.0:
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return float(np.median(out)), out


def both(res, key, fn, reps):
    """fn(accel) timed through accel=None and accel="tiles" """
    res[key] = {}
    for name, accel in (("brute", None), ("tiles", "tiles")):
        t, all_t = timed(lambda: fn(accel), reps)
        res[key][name] = {"seconds": t, "all_seconds": all_t}
    res[key]["speedup"] = res[key]["brute"]["seconds"] / res[key]["tiles"]["seconds"]
    print("%s: brute %.4f s, tiles %.4f s (x%.2f)" % (key, res[key]["brute"]["seconds"], res[key]["tiles"]["seconds"],
                                                      res[key]["speedup"]), flush=True)


def shares(eng, mesh, pts, beta):
    """the call's stats as shares of non-empty tiles x blocks"""
    tiles, clean = mesh.tiles()
    s = eng.tri_distance_tiles(mesh.packed, mesh.n_faces, tiles, clean, pts, beta=beta, want_winding=True, want_stats=True)[5].tolist()
    full = float((tiles[:, 14] > 0).sum()) * s[2]
    return {"tiles": int((tiles[:, 14] > 0).sum()), "blocks": s[2], "staged_for_distance": s[0] / full, "staged_as_near": s[1] / full}


def check(eng, mesh, pts, beta, free_winding, count):
    """both paths on all of `pts` (the blocks are those of the timed call); the winding difference on `count` seeded ones and on all"""
    brute = eng.tri_distance(mesh.packed, mesh.n_faces, pts, want_index=True, want_winding=True)
    tiles, clean = mesh.tiles()
    got = eng.tri_distance_tiles(mesh.packed, mesh.n_faces, tiles, clean, pts, beta=beta, want_index=True, want_winding=True)
    sel = torch.randperm(pts.shape[0], device=pts.device, generator=torch.Generator("cuda").manual_seed(1))[:count]
    free = lambda w: (w - free_winding).abs() < 0.5
    diff = (got[3] - brute[3]).abs()
    return {"points": int(pts.shape[0]), "dist_bits_equal": bool(torch.equal(got[0].view(torch.int32), brute[0].view(torch.int32))),
            "index_equal": bool(torch.equal(got[1], brute[1])), "subset": int(sel.numel()), "max_winding_diff_subset": float(diff[sel].max()),
            "max_winding_diff_all": float(diff.max()), "signs_differ": int((free(got[3]) != free(brute[3])).sum()),
            "signs_differ_off_surface": int(((free(got[3]) != free(brute[3])) & (brute[0] > 1e-3)).sum())}


def balance(eng, mesh, pts, reps):
    """where the time of the culled call goes: the same call with every tile staged (an identity qperm of scattered points: every
    block spans the scene), the tiles staged per block (every eighth block of the Morton order, each run as a call of its own),
    and the call on a quarter of the points -- a quarter of the blocks"""
    tiles, clean = mesh.tiles()
    n = int(pts.shape[0])
    call = lambda p, q: eng.tri_distance_tiles(mesh.packed, mesh.n_faces, tiles, clean, p, q, want_stats=True)
    qp = morton_order(pts)
    ident = torch.arange(n, dtype=torch.int32, device=pts.device)
    out = {"morton_qperm_seconds": timed(lambda: call(pts, qp), reps)[0], "identity_qperm_seconds": timed(lambda: call(pts, ident), reps)[0]}
    full = float((tiles[:, 14] > 0).sum())
    out["identity_qperm_staged"] = call(pts, ident)[5].tolist()[0] / (full * -(-n // 1024))
    sp, one = pts[qp.long()], ident[:1024].contiguous()
    per = torch.stack([call(sp[b:b + 1024].contiguous(), one)[5][0] for b in range(0, n - 1023, 8192)]).cpu().numpy()
    out["staged_per_block"] = {"blocks_sampled": len(per), "tiles": int(full), "mean": float(per.mean()), "median": float(np.median(per)),
                               "p90": float(np.percentile(per, 90)), "max": int(per.max())}
    q = n // 4
    out["quarter_of_the_points_seconds"] = timed(lambda: call(pts[:q], morton_order(pts[:q])), reps)[0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--triangles", type=int, default=100000)
    ap.add_argument("--volume", type=int, default=256)
    ap.add_argument("--samples", type=int, default=200000)
    ap.add_argument("--check", type=int, default=4096)
    ap.add_argument("--beta", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_sdf_tiles_bench.json"))
    a = ap.parse_args()
    from isdf_amd.engine import Engine, NetConfig
    eng = Engine(NetConfig(hidden=64, blocks=1), "cuda")
    res = {"commit": commit(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "beta": a.beta}

    v, f = soup(a.triangles, 0)
    mesh = mesh_sdf.PackedMesh(eng, v, f)
    torch.cuda.synchronize()
    t = time.perf_counter()
    mesh.tiles()
    torch.cuda.synchronize()
    res["soup"] = {"points": a.points, "triangles": mesh.n_faces, "first_index_build_seconds": time.perf_counter() - t}
    pts = torch.rand(a.points, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 10.0
    both(res["soup"], "surface_distance", lambda accel: mesh_sdf.surface_distance(eng, mesh, pts, accel=accel), a.reps)
    both(res["soup"], "mesh_sdf", lambda accel: mesh_sdf.mesh_sdf(eng, mesh, pts, accel=accel, beta=a.beta), a.reps)
    res["soup"]["shares"] = shares(eng, mesh, pts, a.beta)
    res["soup"]["check"] = check(eng, mesh, pts, a.beta, 0.0, a.check)
    res["soup"]["balance"] = balance(eng, mesh, pts, a.reps)
    print(json.dumps(res["soup"]["shares"]), json.dumps(res["soup"]["check"]), json.dumps(res["soup"]["balance"]), flush=True)

    n = a.volume
    spacing = (synthetic.ROOM_HI - synthetic.ROOM_LO) / (n - 1)
    rooms = {}
    for k in (3, 6):
        rv, rf = synthetic.room_mesh(k)
        room = rooms[k] = mesh_sdf.PackedMesh(eng, rv, rf)
        torch.cuda.synchronize()
        t = time.perf_counter()
        room.tiles()
        torch.cuda.synchronize()
        key = "mesh_volume_k%d" % k
        res[key] = {"dims": n, "triangles": room.n_faces, "index_build_seconds": time.perf_counter() - t}
        both(res, key + "_timing", lambda accel: mesh_sdf.mesh_volume(eng, room, spacing, synthetic.ROOM_LO, n, free_winding=-1,
                                                                       accel=accel, beta=a.beta), a.reps)
        res[key].update(res.pop(key + "_timing"))
        nodes = mesh_sdf.grid_nodes(tuple(synthetic.ROOM_LO), tuple(spacing), (n, n, n), 0, min(n ** 3, 1 << 20), eng.device)
        res[key]["shares_first_chunk"] = shares(eng, room, nodes, a.beta)
        res[key]["check"] = check(eng, room, nodes, a.beta, -1.0, a.check)
        print(json.dumps(res[key]["shares_first_chunk"]), json.dumps(res[key]["check"]), flush=True)

    def acc_comp(accel):
        return mesh_sdf.mesh_accuracy_completion(eng, rooms[6], rooms[3], a.samples, torch.Generator("cuda").manual_seed(0), accel=accel)
    res["mesh_accuracy_completion"] = {"samples": a.samples, "triangles": [rooms[6].n_faces, rooms[3].n_faces],
                                       "same_floats": acc_comp(None) == acc_comp("tiles")}
    both(res, "acc_timing", acc_comp, a.reps)
    res["mesh_accuracy_completion"].update(res.pop("acc_timing"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
