"""A numpy float32 model of isdf_visible_points, written from the op-by-op statement in include/isdf_hip.h (every operation
rounded to float32, nothing fused, IEEE division), and the loader of its fixture tests/golden/visible_small.npz
(tests/golden/make_visible_golden.py: the reference's frustum.is_visible_torch on the CPU)."""
import os

import numpy as np

CAM = dict(H=48, W=64, fx=60.0, fy=60.0, cx=31.5, cy=23.5)
CASES = [(1, 257), (3, 4099), (70, 3000)]          # (frames, points)
TRUNCS = [0.05, 0.2]


class Cam:
    """anything with fx, fy, cx, cy"""

    def __init__(self, fx, fy, cx, cy, **_):
        self.fx, self.fy, self.cx, self.cy = fx, fy, cx, cy


def visible32(pts, T_CW, depth, fx, fy, cx, cy, trunc):
    """bool [F, n]: frame f sees point i.  pts [n,3], T_CW [F,4,4] camera-from-world, depth [F,H,W], all float32."""
    f32 = np.float32
    p = np.asarray(pts, f32).reshape(-1, 3)
    A = np.asarray(T_CW, f32).reshape(-1, 4, 4)
    d = np.asarray(depth, f32)
    F, H, W = d.shape
    assert A.shape[0] == F
    fx, fy, cx, cy, trunc = f32(fx), f32(fy), f32(cx), f32(cy), f32(trunc)
    x, y, z = p[None, :, 0], p[None, :, 1], p[None, :, 2]
    with np.errstate(all="ignore"):
        def row(r):
            a = A[:, r, :, None]
            return ((a[:, 0] * x + a[:, 1] * y) + a[:, 2] * z) + a[:, 3]
        xc, yc, zc = row(0), row(1), row(2)
        assert xc.dtype == f32
        u = (fx * xc + cx * zc) / zc
        v = (fy * yc + cy * zc) / zc
        inside = (u > 0) & (u < f32(W)) & (v > 0) & (v < f32(H))
        col = np.where(inside, u, 0).astype(np.int64)           # truncation, as .long()
        rw = np.where(inside, v, 0).astype(np.int64)
        dv = d[np.arange(F)[:, None], rw, col]
        lim = dv + trunc
        assert lim.dtype == f32
        return inside & (zc > 0) & (zc < lim)


def _bits(packed, F, n):
    return np.unpackbits(packed)[:F * n].reshape(F, n).astype(bool)


def load_golden():
    """{"depth", "T_WC", "T_CW" (all 70 frames; a case uses the first F), "cases": [dict(F, n, trunc, pts, mask, border)]}"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "visible_small.npz"))
    out = dict(depth=g["depth"], T_WC=g["T_WC"], T_CW=g["T_CW"], cases=[])
    assert [float(v) for v in g["cam"]] == [CAM[k] for k in ("H", "W", "fx", "fy", "cx", "cy")]
    for F, n in CASES:
        for trunc in TRUNCS:
            key = "F%d_n%d" % (F, n)
            tk = key + "/trunc%g" % trunc
            out["cases"].append(dict(F=F, n=n, trunc=trunc, pts=g[key + "/pts"], mask=_bits(g[tk + "/mask"], F, n),
                                     border=_bits(g[tk + "/border"], F, n)))
    return out
