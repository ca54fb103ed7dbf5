"""Numpy models of the evaluation kernels (include/isdf_hip.h: isdf_sdf_metrics, isdf_nn_distance) -- TEST INFRASTRUCTURE.

float64 is the yardstick: `trilinear` restates what scipy's linear RegularGridInterpolator computes on an evenly spaced grid
(faces inclusive), `sdf_metrics` the tail of Trainer.eval_sdf (trainer.py:1831-1866: mask, L1, metrics.binned_losses,
metrics.chomp_cost).  float32 exists for the nearest-neighbour model only: `nn_sq_dist32` forms (dx*dx + dy*dy) + dz*dz with
every operation rounded to float32, which the kernel must reproduce bit for bit.  `trilinear32` restates the kernel's own
float32 order of operations (no fused multiply-add: an emulation, used to size error bounds, not to assert against)."""
import numpy as np

BIN_LIMITS = np.array([-np.inf, 0.0, 0.1, 0.2, 0.5, 1.0, np.inf])
EPSILONS = (1.0, 1.5, 2.0)
RECORD = 24


def trilinear(values, spacing, origin, pts, dtype=np.float64):
    """(gt [n], in_bounds [n]): gt is undefined (0) where the point is out of bounds"""
    v = np.asarray(values, dtype)
    p = np.asarray(pts, dtype).reshape(-1, 3)
    h, o = np.asarray(spacing, dtype), np.asarray(origin, dtype)
    u = (p - o) / h
    hi = np.asarray(v.shape, dtype) - 1
    with np.errstate(invalid="ignore"):
        inb = np.all((u >= 0) & (u <= hi), axis=1)
    uc = np.where(inb[:, None], u, 0)
    i = np.minimum(uc.astype(np.int64), np.asarray(v.shape) - 2)
    t = (uc - i).astype(dtype)
    ix, iy, iz = i[:, 0], i[:, 1], i[:, 2]
    tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]

    def lerp(a, b, w):
        return a + w * (b - a)
    c00 = lerp(v[ix, iy, iz], v[ix, iy, iz + 1], tz)
    c01 = lerp(v[ix, iy + 1, iz], v[ix, iy + 1, iz + 1], tz)
    c10 = lerp(v[ix + 1, iy, iz], v[ix + 1, iy, iz + 1], tz)
    c11 = lerp(v[ix + 1, iy + 1, iz], v[ix + 1, iy + 1, iz + 1], tz)
    gt = lerp(lerp(c00, c01, ty), lerp(c10, c11, ty), tx)
    return np.where(inb, gt, 0).astype(dtype), inb


def trilinear32(values, spacing, origin, pts):
    return trilinear(np.asarray(values, np.float32), np.asarray(spacing, np.float32), np.asarray(origin, np.float32),
                     np.asarray(pts, np.float32), np.float32)


def chomp(sdf, epsilon):
    """metrics.chomp_cost (metrics.py:95-104), the three assignments in its order"""
    s = np.asarray(sdf, np.float64)
    cost = -s + epsilon / 2.0
    pos = s > 0
    cost[pos] = 1.0 / (2.0 * epsilon) * (s[pos] - epsilon) ** 2
    cost[s > epsilon] = 0.0
    return cost


def sdf_metrics(values, spacing, origin, pts, sdf, exclude_zero_gt=True):
    """(record [24] float64 in the kernel's layout, gt [n], valid [n] bool)"""
    gt, inb = trilinear(values, spacing, origin, pts)
    valid = inb & ((gt != 0) | (not exclude_zero_gt))
    s, g = np.asarray(sdf, np.float64).reshape(-1)[valid], gt[valid]
    d = np.abs(s - g)
    rec = np.zeros(RECORD)
    rec[0], rec[1], rec[2] = valid.sum(), inb.sum(), d.sum()
    for b in range(6):
        m = (g > BIN_LIMITS[b]) & (g < BIN_LIMITS[b + 1])
        rec[3 + b], rec[9 + b] = d[m].sum(), m.sum()
    for e, eps in enumerate(EPSILONS):
        cp, cg = chomp(s, eps), chomp(g, eps)
        rec[15 + 3 * e: 18 + 3 * e] = np.abs(cp - cg).sum(), cp.sum(), cg.sum()
    return rec, gt, valid


def result_dict(rec):
    """Trainer.eval_sdf's dict from a record (0 / 0 = NaN as in the reference)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"av_l1": float(rec[2] / rec[0]), "binned_l1": (rec[3:9] / rec[9:15]).tolist(),
                "l1_chomp_costs": (rec[15:24:3] / rec[0]).tolist()}


def nn_sq_dist32(query, target, chunk=2048):
    """(d2 [n] float32, index [n] int64): the minimum over the targets of (dx*dx + dy*dy) + dz*dz in float32, the lowest index on
    ties (np.argmin returns the first minimum)"""
    q = np.asarray(query, np.float32).reshape(-1, 3)
    t = np.asarray(target, np.float32).reshape(-1, 3)
    d2 = np.empty(len(q), np.float32)
    idx = np.empty(len(q), np.int64)
    for s in range(0, len(q), chunk):
        a = q[s:s + chunk, None, :] - t[None, :, :]
        assert a.dtype == np.float32
        a = a * a
        m = (a[..., 0] + a[..., 1]) + a[..., 2]
        j = np.argmin(m, axis=1)
        idx[s:s + chunk] = j
        d2[s:s + chunk] = m[np.arange(len(j)), j]
    return d2, idx


def nn_dist64(query, target, chunk=1024):
    q = np.asarray(query, np.float64).reshape(-1, 3)
    t = np.asarray(target, np.float64).reshape(-1, 3)
    out = np.empty(len(q))
    for s in range(0, len(q), chunk):
        a = q[s:s + chunk, None, :] - t[None, :, :]
        out[s:s + chunk] = np.sqrt((a * a).sum(-1).min(axis=1))
    return out


def load_golden():
    """tests/golden/eval_metrics_small.npz (make_eval_golden.py) as a dict, with what the generator left out to save space put
    back: the zeroed volume (= max(signed, 0)) and its per-point ground truth (stored as its difference from the signed one's)"""
    import os
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_metrics_small.npz")))
    g["zeroed"] = np.maximum(g["signed"], 0)
    gt = g["signed/gt"].copy()
    gt[g["zeroed/gt_diff_index"]] = g["zeroed/gt_diff_value"]
    g["zeroed/gt"] = gt
    return g


class CountingDataset:
    """stands in for datasets.SceneCache: frame i of the sequence is fixture frame i % K; counts what is read"""

    def __init__(self, depth, T, n):
        self.depth, self.T, self.n, self.reads = depth, T, n, []

    def __len__(self):
        return self.n

    def __getitem__(self, idx):
        idx = np.asarray(idx)
        self.reads.append(len(idx))
        k = idx % len(self.depth)
        return {"depth": self.depth[k], "T": self.T[k], "image": None}

    def get_all(self):
        return self[np.arange(self.n)]
