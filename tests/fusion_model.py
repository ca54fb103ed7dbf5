"""Numpy models of the voxel-baseline kernels, written from the op-by-op statements in include/isdf_hip.h (isdf_tsdf_integrate,
isdf_distance_transform, isdf_occupancy_sdf) -- TEST INFRASTRUCTURE -- and the loader of tests/golden/fusion_small.npz
(tests/golden/make_fusion_golden.py: the reference's sdf_util.sdf_from_occupancy on the CPU).

`integrate32` follows the fusion's sequence in np.float32, frame by frame, and is what the kernel must equal bit for bit;
`integrate64` is the same sequence in float64 (a sanity bound, nothing is asserted equal to it).  `dist2_brute` is the exact integer
minimum over all feature voxels; `sdf_from_dist2` the float64 square roots and the cast."""
import os

import numpy as np
import torch

EDT_NONE = 1 << 30
GRIDS = [((12, 9, 7), 0.05, 0.05), ((33, 17, 5), 0.3, 0.07), ((8, 8, 8), 0.9, 0.05), ((20, 3, 2), 0.01, 0.07)]   # dims, density, voxel


def _integrate(dtype, tsdf, weight, depth, T_CW, cam, origin, spacing, trunc, max_weight, min_depth, max_depth):
    f = dtype
    tsdf, w = np.array(tsdf, f), np.array(weight, f)
    nx, ny, nz = tsdf.shape
    d = np.asarray(depth, f)
    F, H, W = d.shape
    A = np.asarray(T_CW, f).reshape(-1, 4, 4)
    assert A.shape[0] == F
    o, s = np.asarray(origin, f), np.asarray(spacing, f)
    fx, fy, cx, cy = (f(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    trunc, max_weight, min_depth, max_depth = f(trunc), f(max_weight), f(min_depth), f(max_depth)
    x = (o[0] + np.arange(nx).astype(f) * s[0])[:, None, None]
    y = (o[1] + np.arange(ny).astype(f) * s[1])[None, :, None]
    z = (o[2] + np.arange(nz).astype(f) * s[2])[None, None, :]
    with np.errstate(all="ignore"):
        for k in range(F):
            a = A[k]
            xc = ((a[0, 0] * x + a[0, 1] * y) + a[0, 2] * z) + a[0, 3]
            yc = ((a[1, 0] * x + a[1, 1] * y) + a[1, 2] * z) + a[1, 3]
            zc = ((a[2, 0] * x + a[2, 1] * y) + a[2, 2] * z) + a[2, 3]
            u = (fx * xc + cx * zc) / zc
            v = (fy * yc + cy * zc) / zc
            uc, vc = u + f(0.5), v + f(0.5)
            assert uc.dtype == f and uc.shape == tsdf.shape
            inside = (uc >= 0) & (uc < f(W)) & (vc >= 0) & (vc < f(H)) & (zc > 0)
            col = np.where(inside, uc, 0).astype(np.int64)
            row = np.where(inside, vc, 0).astype(np.int64)
            dv = d[k][row, col]
            ok = inside & (dv > min_depth) & (dv < max_depth)
            sd = dv - zc
            ok &= sd >= -trunc
            t = np.where(sd < trunc, sd, trunc)
            w1 = w + f(1.0)
            nt = (tsdf * w + t) / w1
            assert nt.dtype == f
            tsdf = np.where(ok, nt, tsdf)
            w = np.where(ok, np.minimum(w1, max_weight), w)
    return tsdf, w


def integrate32(tsdf, weight, depth, T_CW, cam, origin, spacing, trunc, max_weight=np.inf, min_depth=0.0, max_depth=np.inf):
    """(tsdf, weight) float32 after the F frames, in index order; the inputs are not modified"""
    return _integrate(np.float32, tsdf, weight, depth, T_CW, cam, origin, spacing, trunc, max_weight, min_depth, max_depth)


def integrate64(tsdf, weight, depth, T_CW, cam, origin, spacing, trunc, max_weight=np.inf, min_depth=0.0, max_depth=np.inf):
    return _integrate(np.float64, tsdf, weight, depth, T_CW, cam, origin, spacing, trunc, max_weight, min_depth, max_depth)


def dist2_brute(feature, invert=False, chunk=1 << 22):
    """int32 [nx,ny,nz]: min over the voxels q with (feature[q] != 0) != invert of |p - q|^2, EDT_NONE without one"""
    feat = (np.asarray(feature) != 0) != bool(invert)
    q = np.argwhere(feat).astype(np.int64)
    p = np.argwhere(np.ones(feat.shape, bool)).astype(np.int64)
    out = np.full(len(p), EDT_NONE, np.int64)
    if len(q):
        rows = max(1, chunk // len(q))
        for s in range(0, len(p), rows):
            df = p[s:s + rows, None, :] - q[None, :, :]
            out[s:s + rows] = (df * df).sum(-1).min(axis=1)
    return out.reshape(feat.shape).astype(np.int32)


def dist2_passes(feature, invert=False):
    """the same minimum by the three separable min-plus passes the header states (z, y, x; saturated at EDT_NONE): for grids too
    large for `dist2_brute`; tests/test_fusion_cpu.py holds the two equal"""
    d = np.where((np.asarray(feature) != 0) != bool(invert), 0, EDT_NONE).astype(np.int64)
    for axis in (2, 1, 0):
        L = d.shape[axis]
        v = np.moveaxis(d, axis, 0).reshape(L, -1)
        q = np.arange(L, dtype=np.int64)
        cost = (q[:, None] - q[None, :]) ** 2                                   # [p, q]
        out = np.minimum((v[None, :, :] + cost[:, :, None]).min(axis=1), EDT_NONE)
        d = np.moveaxis(out.reshape((L,) + tuple(np.delete(d.shape, axis))), 0, axis)
    return d.astype(np.int32)


def sdf_from_dist2(a2, b2, voxel, dtype=np.float32):
    """(sqrt(a2) - sqrt(b2)) * voxel in float64, then the cast; +inf where a2 is EDT_NONE, -inf where b2 is"""
    a2, b2 = np.asarray(a2, np.int64), np.asarray(b2, np.int64)
    out = (np.sqrt(a2.astype(np.float64)) - np.sqrt(b2.astype(np.float64))) * np.float64(voxel)
    out = np.where(a2 == EDT_NONE, np.inf, np.where(b2 == EDT_NONE, -np.inf, out))
    return out.astype(dtype)


def occupancy_sdf(occ, voxel, dtype=np.float32):
    occ = np.asarray(occ) != 0
    return sdf_from_dist2(dist2_brute(occ), dist2_brute(occ, invert=True), voxel, dtype)


def load_golden():
    """[dict(dims, voxel, occ u8 [nx,ny,nz], sdf float64 [nx,ny,nz])] in the order of GRIDS"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fusion_small.npz"))
    out = []
    for k, (dims, _, voxel) in enumerate(GRIDS):
        n = int(np.prod(dims))
        assert float(g["g%d/voxel" % k]) == voxel and tuple(g["g%d/dims" % k]) == dims
        out.append(dict(dims=dims, voxel=voxel, occ=np.unpackbits(g["g%d/occ" % k])[:n].reshape(dims), sdf=g["g%d/sdf" % k]))
    return out


class StubEngine:
    """the tensor-level calls of isdf_amd.engine.Engine that isdf_amd.fusion uses, computed by these models on the host (CPU
    tensors in and out)"""

    def __init__(self):
        self.device = torch.device("cpu")
        self.calls = []

    def tsdf_integrate(self, tsdf, weight, depth, T_CW, cam, origin, spacing, trunc, max_weight=np.inf, min_depth=0.0,
                       max_depth=np.inf):
        c = dict(fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy)
        t, w = integrate32(tsdf.numpy(), weight.numpy(), depth.numpy(), T_CW.numpy(), c, origin, spacing, trunc, max_weight,
                           min_depth, max_depth)
        tsdf.copy_(torch.from_numpy(t))
        weight.copy_(torch.from_numpy(w))
        self.calls.append(("integrate", int(depth.shape[0])))
        return tsdf, weight

    def distance_transform(self, feature, invert=False):
        self.calls.append(("edt", bool(invert)))
        return torch.from_numpy(dist2_brute(feature.numpy(), invert))

    def occupancy_sdf(self, occ, voxel):
        self.calls.append(("occupancy_sdf", float(voxel)))
        return torch.from_numpy(occupancy_sdf(occ.numpy(), voxel))
