#!/usr/bin/env python3
"""Mesh reconstruction timing for the trained default net (fixture `trained_default`) on the grid the grafted mesh_rec evaluates:

    python tools/mesh_bench.py [--dims 200 256] [--reps 20] [--out profiles/mesh_bench.json]

Per grid_dim: get_sdf_grid's single forward launch over dim^3 points; marching cubes (the four launches of isdf_marching_cubes at a
capacity that fits, device events); the one device -> host copy of the mesh mesh_rec makes; vertex / triangle counts; and the
bytes marching cubes has to move -- the volume read once, the mesh written, plus the per-point vertex-id array of its workspace
written and read -- over its kernel time, against the 6.3 TB/s an MI355X streams in practice.  Medians over --reps."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12


def bounds_grid(g, dim):
    """make_3D_grid over the fixture's bounds box (as set_scene_properties would derive it from the scene)"""
    T_bounds = np.linalg.inv(g["bounds_T"].astype(np.float64))
    pc = g["eval/pc"].reshape(-1, 3).astype(np.float64)
    local = (pc - T_bounds[:3, 3]) @ T_bounds[:3, :3]
    scale = 2 * np.abs(local).max(0) / (2 * 0.9)
    t = torch.linspace(-1.0, 1.0, dim, dtype=torch.float32, device="cuda")
    G = torch.stack(torch.meshgrid(t, t, t, indexing="ij"), -1) * torch.tensor(scale, dtype=torch.float32, device="cuda")
    Tt = torch.tensor(T_bounds, dtype=torch.float32, device="cuda")
    return (G @ Tt[:3, :3].T + Tt[:3, 3]).reshape(-1, 3).contiguous(), scale, T_bounds


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(np.min(out))


def run(dim, reps):
    from isdf_amd import _ffi
    from isdf_amd.engine import Engine, NetConfig, _stream
    from isdf_amd.mesh import grid_index_to_world
    from tests import golden_util as gu
    g = gu.load("trained_default")
    H, B, nf, si, so = g["net"]
    eng = Engine(NetConfig(hidden=int(H), blocks=int(B), n_freqs=int(nf), scale_input=float(si), scale_output=float(so),
                           transform=g["bounds_T"]), "cuda")
    eng.load_params(gu.params_of(g))
    pts, scale, T_bounds = bounds_grid(g, dim)
    A = grid_index_to_world(dim, scale, T_bounds)
    vol = eng.sdf_eval(pts).view(dim, dim, dim)
    verts, faces, normals = eng.marching_cubes(vol, 0.0, A)          # sizes the outputs
    V, F = verts.shape[0], faces.shape[0]
    t_eval = timed(lambda: eng.sdf_eval(pts), reps)

    # marching cubes alone: the entry point's four launches into buffers that fit
    lib, m = eng.lib, eng._mesher
    args = _ffi.McArgs()
    args.volume, args.D0, args.D1, args.D2, args.level, args.has_transform = vol.data_ptr(), dim, dim, dim, 0.0, 1
    args.index_to_world[:] = [float(x) for x in A.reshape(-1)]
    vb = torch.empty(V, 3, device="cuda"); nb = torch.empty(V, 3, device="cuda")
    fb = torch.empty(F, 3, dtype=torch.int32, device="cuda")
    st = _stream(eng.device)

    def mc():
        _ffi.check(lib.isdf_marching_cubes(C.byref(args), _ffi.ptr(m.counts), _ffi.ptr(vb), _ffi.ptr(nb), V, _ffi.ptr(fb), F,
                                           _ffi.ptr(m._ws), m._ws.numel(), st), "isdf_marching_cubes")
    t_mc = timed(mc, reps)
    assert m.counts.tolist() == [V, F]
    assert torch.equal(fb, faces)

    # the one device -> host copy of mesh_rec (vertices, normals, faces in one buffer)
    def d2h():
        torch.cat([verts.reshape(-1), normals.reshape(-1), faces.reshape(-1).view(torch.float32)]).cpu()
    t_copy = timed(d2h, reps)

    # the whole device part of mesh_rec: grid evaluation + Engine.marching_cubes (its count read-back included) + the copy
    def chain():
        v, f, n = eng.marching_cubes(eng.sdf_eval(pts).view(dim, dim, dim), 0.0, A)
        torch.cat([v.reshape(-1), n.reshape(-1), f.reshape(-1).view(torch.float32)]).cpu()
    t_chain = timed(chain, reps)

    P = dim ** 3
    mesh_bytes = 24 * V + 12 * F
    moved = 4 * P + mesh_bytes + 8 * P
    return dict(grid_dim=dim, points=P, vertices=V, triangles=F,
                grid_eval_ms=t_eval[0], grid_eval_ms_min=t_eval[1],
                marching_cubes_ms=t_mc[0], marching_cubes_ms_min=t_mc[1],
                host_copy_ms=t_copy[0], host_copy_MB=mesh_bytes / 1e6,
                eval_mc_copy_ms=t_chain[0],
                mc_bytes_moved_MB=moved / 1e6,
                mc_bytes_note="volume read once (4 B/point) + mesh written (24 B/vertex + 12 B/triangle) + workspace vertex ids "
                              "written and read (8 B/point)",
                mc_achieved_TBps=moved / (t_mc[0] * 1e-3) / 1e12,
                mc_fraction_of_6p3TBps=moved / (t_mc[0] * 1e-3) / HBM_ACHIEVABLE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs="+", default=[200, 256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from isdf_amd import build
    build.build(verbose=False)
    rows = [run(d, a.reps) for d in a.dims]
    rec = dict(tool="tools/mesh_bench.py", device=torch.cuda.get_device_name(0), net="trained_default (256 x 2 blocks, 6 octaves)",
               rows=rows)
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
