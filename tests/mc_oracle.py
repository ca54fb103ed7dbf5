"""Plain numpy marching cubes written from the contract of include/isdf_hip.h (`isdf_marching_cubes`), with the tables the
library exports (`isdf_mc_tables`): the reference the HIP kernels (tests/test_mesh_gpu.py) and the CPU tests of the grafted
`mesh_rec` (tests/test_mesh_cpu.py) are held to.  fp32 arithmetic in the kernels' formula order; vertex and face ORDER identical."""
import ctypes as C

import numpy as np


def library_tables():
    """(edge_corners int32 [12, 2], tri_table int8 [256, 3 * ISDF_MC_MAX_TRIS]) as the library ships them (host call only)"""
    from isdf_amd import _ffi
    ec = np.zeros((12, 2), np.int32)
    tt = np.zeros((256, 3 * _ffi.MC_MAX_TRIS), np.int8)
    _ffi.check(_ffi.lib().isdf_mc_tables(ec.ctypes.data_as(C.c_void_p), tt.ctypes.data_as(C.c_void_p)), "isdf_mc_tables")
    return ec, tt


def corner_offset(c):
    return np.array([c & 1, c >> 1 & 1, c >> 2 & 1])


def gradient(vol):
    """central differences inside, one-sided at the borders, in fp32 (np.gradient with unit spacing)"""
    return np.stack(np.gradient(vol.astype(np.float32)), axis=-1).astype(np.float32)


def edge_flags(vol, level):
    """[D0, D1, D2, 3] bool: the +axis edge of each point carries a vertex"""
    v = vol.astype(np.float32)
    fin = np.isfinite(v)
    ins = v < np.float32(level)
    out = np.zeros(v.shape + (3,), bool)
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        out[lo + (a,)] = fin[lo] & fin[hi] & (ins[lo] != ins[hi])
    return out


def marching_cubes(vol, level=0.0, tables=None, index_to_world=None):
    """-> verts [V, 3] f32, faces [F, 3] int32, normals [V, 3] f32 (index coordinates unless index_to_world, a [3, 4] affine)"""
    ec, tt = library_tables() if tables is None else tables
    v = np.ascontiguousarray(vol, dtype=np.float32)
    D = v.shape
    lev = np.float32(level)
    flags = edge_flags(v, lev)
    vid = np.cumsum(flags.reshape(-1)) - 1                # vertex id of every (point, axis), valid where flagged
    vid = vid.reshape(flags.shape).astype(np.int64)
    pts, axes = np.nonzero(flags.reshape(-1, 3))          # ordered by point, then axis
    ijk = np.stack(np.unravel_index(pts, D), axis=1)
    nb = ijk + np.eye(3, dtype=np.int64)[axes]
    fa = v[tuple(ijk.T)]
    fb = v[tuple(nb.T)]
    t = (lev - fa) / (fb - fa)
    p = ijk.astype(np.float32)
    p[np.arange(len(axes)), axes] += t
    g = gradient(v)
    ga, gb = g[tuple(ijk.T)], g[tuple(nb.T)]
    n = ga + t[:, None] * (gb - ga)
    n = n / np.sqrt((n * n).sum(1, keepdims=True))
    if index_to_world is not None:
        A = np.asarray(index_to_world, np.float32).reshape(3, 4)
        p = (p @ A[:, :3].T + A[:, 3]).astype(np.float32)
        Nm = np.linalg.inv(A[:, :3].astype(np.float64)).T.astype(np.float32)
        n = n @ Nm.T
        n = (n / np.sqrt((n * n).sum(1, keepdims=True))).astype(np.float32)
    # faces: cells in linear order, each case's triangles in table order
    C0, C1, C2 = D[0] - 1, D[1] - 1, D[2] - 1
    case = np.zeros((C0, C1, C2), np.int64)
    ok = np.ones((C0, C1, C2), bool)
    for c in range(8):
        o = corner_offset(c)
        cv = v[o[0]:o[0] + C0, o[1]:o[1] + C1, o[2]:o[2] + C2]
        ok &= np.isfinite(cv)
        case |= (cv < lev).astype(np.int64) << c
    cells = np.nonzero(ok.reshape(-1))[0]
    cc = case.reshape(-1)[cells]
    cijk = np.stack(np.unravel_index(cells, (C0, C1, C2)), axis=1)
    tri = tt[cc].astype(np.int64).reshape(len(cells), -1, 3)          # [cells, max_tris, 3] edge ids, -1 padded
    keep = tri[:, :, 0] >= 0
    e = tri[keep]                                                      # row-major: cell, then table order
    cell_of = np.broadcast_to(np.arange(len(cells))[:, None], keep.shape)[keep]
    lower = ec[:, 0]
    off = np.stack([corner_offset(c) for c in range(8)])
    owner = cijk[cell_of][:, None, :] + off[lower[e]]                  # [F, 3, 3]
    faces = vid[owner[..., 0], owner[..., 1], owner[..., 2], e // 4]
    return p.astype(np.float32), faces.astype(np.int32), n.astype(np.float32)


def edge_use(faces):
    """{undirected edge: number of faces using it}"""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    e = np.sort(e, axis=1)
    u, cnt = np.unique(e, axis=0, return_counts=True)
    return u, cnt


def euler_characteristic(verts, faces):
    u, _ = edge_use(faces)
    used = np.unique(faces)
    return len(used) - len(u) + len(faces)


def signed_volume(verts, faces):
    v = verts.astype(np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
