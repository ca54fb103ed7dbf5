#!/usr/bin/env python3
"""Generate tests/golden/visible_small.npz by running the REFERENCE's geometry.frustum.is_visible_torch (imported read-only, as
make_eval_golden.py does) on the CPU, on small seeded inputs.

Run in the build container only:
    python tests/golden/make_visible_golden.py

Frames: golden_util.synth_frames at 48 x 64 (70 of them; a case uses the first F).  Cases (F, n) = (1, 257), (3, 4099), (70, 3000):
257 and 4099 sit just past a block of 256 points, 70 is one more than a 64-frame stage (the launcher splits so few points into rows of
8 frames, so a block that stages twice is tests/test_visible_gpu.py's own large case); each at trunc 0.05 and 0.2.  Half of a case's
points are back-projected pixels of random frames, pushed from 0.6 m in front of the surface to 0.3 m behind it; the other half are
uniform in [-5, 5]^3 (points behind cameras, outside images, on zero-depth pixels).

A float32 kernel can decide a pair differently from wherever the reference's arithmetic lands when the pair sits on a limit, so the
file also stores a `border` mask per case, from the same predicate in float64: u or v within 1e-3 px of an integer (the image edges
are integers too), |z| < 1e-4, or inside the image with |z - (depth + trunc)| < 1e-4.  Under 1 % of the pairs (asserted; in the 257-pair case one
pair is 0.39 %, and the seed is one at which that case has one border pair and no more than two).  Stored:
pts, depth, T_WC, the CPU's torch.linalg.inv(T_WC) as T_CW, the reference's [F, n] mask and the border mask, both bit-packed.  Only
data is written."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from tests import visible_model as vm  # noqa: E402
from tests.golden_util import synth_frames  # noqa: E402


def border64(pts, T_CW, depth, cam, trunc):
    p = np.concatenate([pts.astype(np.float64), np.ones((len(pts), 1))], axis=1)
    pc = np.einsum("frc,nc->frn", T_CW.astype(np.float64), p)
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    with np.errstate(all="ignore"):
        u = (cam["fx"] * x + cam["cx"] * z) / z
        v = (cam["fy"] * y + cam["cy"] * z) / z
        near_int = (np.abs(u - np.round(u)) < 1e-3) | (np.abs(v - np.round(v)) < 1e-3)
        inside = (u > 0) & (u < cam["W"]) & (v > 0) & (v < cam["H"])
        col, row = np.where(inside, u, 0).astype(np.int64), np.where(inside, v, 0).astype(np.int64)
        lim = depth.astype(np.float64)[np.arange(len(depth))[:, None], row, col] + np.float64(np.float32(trunc))
        return near_int | (np.abs(z) < 1e-4) | (inside & (np.abs(z - lim) < 1e-4))


def main():
    mg.import_reference()
    from isdf.geometry import frustum
    cam = vm.CAM
    rng = np.random.RandomState(2)
    F_all = max(F for F, _ in vm.CASES)
    depth, _, T_WC = synth_frames(rng, F_all, cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    T_CW = torch.linalg.inv(torch.from_numpy(T_WC)).numpy()
    out = dict(depth=depth, T_WC=T_WC, T_CW=T_CW, cam=np.array([cam[k] for k in ("H", "W", "fx", "fy", "cx", "cy")], np.float64))
    for F, n in vm.CASES:
        half = n // 2
        f = rng.randint(0, F, half)
        u, v = rng.uniform(0, cam["W"], half), rng.uniform(0, cam["H"], half)
        zc = depth[f, v.astype(int), u.astype(int)].astype(np.float64) + rng.uniform(-0.6, 0.3, half)
        pc = np.stack([(u - cam["cx"]) / cam["fx"] * zc, (v - cam["cy"]) / cam["fy"] * zc, zc, np.ones(half)], axis=1)
        near = np.einsum("nrc,nc->nr", T_WC[f].astype(np.float64), pc)[:, :3]
        pts = np.concatenate([near, rng.uniform(-5, 5, (n - half, 3))])[rng.permutation(n)].astype(np.float32)
        key = "F%d_n%d" % (F, n)
        out[key + "/pts"] = pts
        for trunc in vm.TRUNCS:
            with torch.no_grad():
                ref = frustum.is_visible_torch(torch.from_numpy(pts), torch.from_numpy(T_WC[:F]), torch.from_numpy(depth[:F]),
                                               cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], trunc=trunc).numpy()
            assert ref.shape == (F, n) and ref.dtype == bool
            border = border64(pts, T_CW[:F], depth[:F], cam, trunc)
            model = vm.visible32(pts, T_CW[:F], depth[:F], cam["fx"], cam["fy"], cam["cx"], cam["cy"], trunc)
            print("%s trunc %g: visible %.2f %%, border %.3f %%, model != reference on %d pairs (%d outside the border)"
                  % (key, trunc, 100 * ref.mean(), 100 * border.mean(), (model != ref).sum(), ((model != ref) & ~border).sum()))
            assert border.mean() < 0.01 and 0.01 < ref.mean() < 0.60
            tk = key + "/trunc%g" % trunc
            out[tk + "/mask"], out[tk + "/border"] = np.packbits(ref), np.packbits(border)
    path = os.path.join(HERE, "visible_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
