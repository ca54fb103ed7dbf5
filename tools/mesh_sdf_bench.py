#!/usr/bin/env python3
"""Ground truth from a mesh (isdf_amd.mesh_sdf, isdf_amd/csrc/tri.hip): the brute-force rate of isdf_tri_distance.

    python tools/mesh_sdf_bench.py [--reps 5] [--out profiles/mesh_sdf_bench.json]

  * pairs/s for distance only and for distance + winding number at --points x --triangles (about 1 M x 100 k: an icosphere soup
    generated from a seed), one Engine.tri_distance call per figure;
  * the same work in chunked torch ops on the same GPU (the float32 sequence of include/isdf_hip.h written with torch, --torch-points
    points at a time against all triangles), on a subset of the points: the baseline, as pairs/s;
  * a 256^3 mesh_volume of the synthetic room mesh (k = 3);
  * VALU instructions per pair, counted in the disassembly of the kernels' inner loops (one division per pair marks the pairs), and
    the fraction of the VALU issue rate (256 CUs x 4 SIMDs, one wave64 instruction per 2 cycles, at the nominal 2.4 GHz) that the
    measured rate implies.

Timing: two warm-up calls, then --reps calls, each between device synchronisations; the figure is the median.  A record, not a
test bar: no rate was promised in advance."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from isdf_amd import _ffi, isa_lint, mesh_sdf, synthetic        # noqa: E402

PEAK_LANE_INSTR = 256 * 4 * 64 * 2.4e9 / 2       # lane-instructions per second at the nominal clock


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return os.environ.get("ISDF_COMMIT", "unknown")


def timed(fn, reps):
    for _ in range(2):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return float(np.median(out)), out


def soup(m, seed):
    """about m triangles: unit icospheres (k = 3, 1 280 faces each) scattered in a 10 m cube"""
    v0, f0 = synthetic._icosphere(np.zeros(3), 0.3, 3)
    rng = np.random.RandomState(seed)
    count = max(1, round(m / len(f0)))
    centres = rng.uniform(0.0, 10.0, (count, 3))
    v = (v0[None] + centres[:, None]).reshape(-1, 3)
    f = (f0[None] + (np.arange(count) * len(v0))[:, None, None]).reshape(-1, 3)
    return v, f.astype(np.int32)


def torch_distance(packed, pts, winding, chunk):
    """the header's float32 sequence in torch ops, `chunk` points at a time against every slot"""
    t = [packed[None, :, k] for k in range(23)]
    valid = packed[None, :, 15] != 0
    dist = torch.empty(pts.shape[0], device=pts.device)
    wn = torch.empty(pts.shape[0], device=pts.device) if winding else None
    for i in range(0, pts.shape[0], chunk):
        q = pts[i:i + chunk]
        ap = [q[:, k, None] - t[k] for k in range(3)]
        d1 = (t[4] * ap[0] + t[5] * ap[1]) + t[6] * ap[2]
        d2 = (t[8] * ap[0] + t[9] * ap[1]) + t[10] * ap[2]
        d3, d4, d5, d6 = d1 - t[3], d2 - t[7], d1 - t[7], d2 - t[11]
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        zero, unit = torch.zeros_like(d1), torch.ones_like(d1)
        den, nv, nw = (va + vb) + vc, vb, vc
        face = torch.ones_like(d1, dtype=torch.bool)
        for cond, (cd, cv, cw) in (((va < 0) & (e43 >= 0) & (e56 >= 0), (e43 + e56, e56, e43)),
                                   ((vb < 0) & (d2 >= 0) & (d6 <= 0), (d2 - d6, zero, d2)),
                                   ((d6 >= 0) & (d5 <= d6), (unit, zero, unit)),
                                   ((vc < 0) & (d1 >= 0) & (d3 <= 0), (d1 - d3, d1, zero)),
                                   ((d3 >= 0) & (d4 <= d3), (unit, unit, zero)),
                                   ((d1 <= 0) & (d2 <= 0), (unit, zero, zero))):
            den, nv, nw, face = torch.where(cond, cd, den), torch.where(cond, cv, nv), torch.where(cond, cw, nw), face & ~cond
        r = 1.0 / den
        v, w = nv * r, nw * r
        d = [ap[k] - (t[4 + k] * v + t[8 + k] * w) for k in range(3)]
        dn = (t[20] * ap[0] + t[21] * ap[1]) + t[22] * ap[2]
        dd = torch.where(face, dn * dn, (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        dd = torch.where(valid & ~torch.isnan(dd), dd, torch.full_like(dd, float("inf")))
        dist[i:i + chunk] = dd.min(1).values.sqrt()
        if winding:
            a = [-x for x in ap]
            b = [t[12 + k] - q[:, k, None] for k in range(3)]
            c = [t[16 + k] - q[:, k, None] for k in range(3)]
            la, lb, lc = (torch.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) for x in (a, b, c))
            det = (a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2])) + a[2] * (b[0] * c[1] - b[1] * c[0])
            dot = lambda x, y: (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]
            om = 2.0 * torch.atan2(det, ((la * lb * lc + dot(a, b) * lc) + dot(b, c) * la) + dot(c, a) * lb)
            wn[i:i + chunk] = (torch.where(valid, om, zero).double().sum(1) / (4.0 * np.pi)).float()
    return dist, wn


def valu_per_pair():
    """{kernel instance: (VALU instructions, pairs) of its innermost hot loop}: the innermost loop (a backward branch with no
    other backward branch inside) holding the most VALU instructions; one v_div_fixup_f32 per pair"""
    out = {}
    with tempfile.TemporaryDirectory(prefix="isdf_bench_") as wd:
        for obj in isa_lint.code_objects(_ffi.LIB_PATH, wd):
            text = isa_lint.disassemble(obj)
            if "tri_distance_kernel" not in text:
                continue
            name, body = None, {}
            for line in text.split("\n"):
                if line.endswith(">:") and "<" in line:
                    name = line[line.index("<") + 1:-2]
                    body[name] = []
                elif name and "//" in line and line.startswith("\t"):
                    ins, rest = line.split("//", 1)
                    addr = int(rest.split(":")[0].strip(), 16)
                    target = int(rest.rsplit("+0x", 1)[1].rstrip(">"), 16) if ins.split()[0].startswith(("s_cbranch", "s_branch")) and "+0x" in rest else None
                    body[name].append((addr, ins.split()[0], target))
            for name, ins in body.items():
                if "tri_distance_kernel" not in name or not ins:
                    continue
                base = ins[0][0]
                loops = [(base + t, a) for a, _, t in ins if t is not None and base + t <= a]
                inner = [l for l in loops if not any(o != l and l[0] <= o[0] and o[1] <= l[1] for o in loops)]
                best = (0, 0)
                for lo, hi in inner:
                    ops = [op for a, op, _ in ins if lo <= a <= hi]
                    valu = sum(op.startswith("v_") for op in ops)
                    if valu > best[0]:
                        best = (valu, sum(op == "v_div_fixup_f32" for op in ops))
                out["winding" if "ILb1" in name else "distance"] = best
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--triangles", type=int, default=100000)
    ap.add_argument("--torch-points", type=int, default=256)
    ap.add_argument("--torch-subset", type=int, default=4096)
    ap.add_argument("--volume", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_sdf_bench.json"))
    a = ap.parse_args()
    from isdf_amd.engine import Engine, NetConfig
    eng = Engine(NetConfig(hidden=64, blocks=1), "cuda")
    v, f = soup(a.triangles, 0)
    mesh = mesh_sdf.PackedMesh(eng, v, f)
    m = mesh.n_faces
    gen = torch.Generator("cuda").manual_seed(0)
    pts = torch.rand(a.points, 3, device="cuda", generator=gen) * 10.0
    res = {"commit": commit(), "device": torch.cuda.get_device_name(0), "points": a.points, "triangles": m, "reps": a.reps,
           "chunks": int((eng.lib.isdf_tri_ws_bytes(a.points, m) - 32 * ((a.points + 255) // 256) - 256) // (8 * a.points) - 1)}
    pairs = float(a.points) * m
    for key, wind in (("distance", False), ("winding", True)):
        t, all_t = timed(lambda: eng.tri_distance(mesh.packed, m, pts, want_winding=wind), a.reps)
        res[key] = {"seconds": t, "all_seconds": all_t, "pairs_per_s": pairs / t}
        print("%s: %.3f s, %.3e pairs/s" % (key, t, pairs / t), flush=True)
    sub = pts[:a.torch_subset]
    for key, wind in (("distance", False), ("winding", True)):
        t, all_t = timed(lambda: torch_distance(mesh.packed, sub, wind, a.torch_points), max(2, a.reps // 2))
        rate = float(sub.shape[0]) * m / t
        res[key]["torch"] = {"points": int(sub.shape[0]), "chunk": a.torch_points, "seconds": t, "pairs_per_s": rate,
                             "speedup": res[key]["pairs_per_s"] / rate}
        print("torch %s: %.3f s for %d points, %.3e pairs/s" % (key, t, sub.shape[0], rate), flush=True)
    # the two agree: the torch sequence is the kernel's (the divisions and square roots may differ in the last place)
    d_hip, _, _, w_hip, _ = eng.tri_distance(mesh.packed, m, sub, want_winding=True)
    d_t, w_t = torch_distance(mesh.packed, sub, True, a.torch_points)
    res["max_abs_diff_vs_torch"] = {"dist": float((d_hip - d_t).abs().max()), "winding": float((w_hip - w_t).abs().max())}
    rv, rf = synthetic.room_mesh(3)
    room = mesh_sdf.PackedMesh(eng, rv, rf)
    n = a.volume
    spacing = (synthetic.ROOM_HI - synthetic.ROOM_LO) / (n - 1)
    t, all_t = timed(lambda: mesh_sdf.mesh_volume(eng, room, spacing, synthetic.ROOM_LO, n, free_winding=-1), max(2, a.reps // 2))
    res["mesh_volume"] = {"dims": n, "triangles": room.n_faces, "seconds": t, "all_seconds": all_t,
                          "pairs_per_s": float(n) ** 3 * room.n_faces / t}
    print("mesh_volume %d^3 x %d triangles: %.3f s" % (n, room.n_faces, t), flush=True)
    try:
        for key, (valu, npairs) in valu_per_pair().items():
            per = valu / npairs if npairs else float("nan")
            res[key]["valu_per_pair"] = per
            res[key]["loop"] = {"valu_instructions": valu, "pairs": npairs}
            res[key]["valu_issue_fraction"] = res[key]["pairs_per_s"] * per / PEAK_LANE_INSTR
    except (OSError, subprocess.CalledProcessError, RuntimeError) as e:
        res["valu_per_pair_error"] = str(e)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: res[k] for k in ("distance", "winding", "mesh_volume")}, indent=1))


if __name__ == "__main__":
    main()
