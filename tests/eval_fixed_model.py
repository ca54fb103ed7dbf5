"""Numpy float64 model of isdf_region_metrics (include/isdf_hip.h) and of the result eval_pts.fixed_pts_eval assembles from it
-- TEST INFRASTRUCTURE.  The trilinear lookup, the bins and the CHOMP cost are tests/eval_model.py's; new here are the region
flags, the central-difference ground-truth gradient (eval_pts.eval_grad(..., is_gt_sdf=True), eval_pts.py:68-93) and the cosine
distance (torch.nn.CosineSimilarity(dim=1, eps=1e-6): x.y / (max(|x|, eps) * max(|y|, eps)))."""
import os

import numpy as np

from tests import eval_model as em

RECORD = 27
VIS_SDF, VOX_SDF, VIS_GRAD, VOX_GRAD = 1, 2, 4, 8


def gt_gradient(values, spacing, origin, pts, delta):
    """[n, 3] float64: (f(p + d e_i) - f(p - d e_i)) / (2 d) with f NaN out of bounds or where it is == 0"""
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    grad = np.zeros(p.shape)
    for i in range(3):
        for dx in (-1, 1):
            q = p.copy()
            q[:, i] += dx * delta
            f, inb = em.trilinear(values, spacing, origin, q)
            f = np.where(inb & (f != 0), f, np.nan)
            grad[:, i] += dx * f
    return grad / (2 * delta)


def cos_distance(x, y, eps=1e-6):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    nx, ny = np.sqrt((x * x).sum(1)), np.sqrt((y * y).sum(1))
    return 1.0 - (x * y).sum(1) / (np.maximum(nx, eps) * np.maximum(ny, eps))


def cos_distance_reference(x32, y64, eps=1e-6):
    """1 - cos as the REFERENCE gets it (eval_pts.py:175-187): torch.nn.CosineSimilarity on a float32 predicted gradient and a
    float64 ground-truth gradient divides each operand by its own clamped norm in the operand's OWN precision before the
    product is promoted to float64 -- the predicted gradient is normalised in float32.  Restated with torch's primitives (its
    float32 norm is not numpy's to the last bit).  isdf_region_metrics widens the predicted gradient first (cos_distance); the
    two differ by the float32 roundings of that normalisation: the norm (three squares, two sums, a root) and one division per
    component, under 4 * eps32 per point."""
    import torch
    x, y = torch.from_numpy(np.ascontiguousarray(x32, np.float32)), torch.from_numpy(np.ascontiguousarray(y64, np.float64))
    xn = x / torch.linalg.vector_norm(x, 2, dim=1, keepdim=True).clamp_min(eps)
    yn = y / torch.linalg.vector_norm(y, 2, dim=1, keepdim=True).clamp_min(eps)
    return (1 - (xn * yn).sum(1)).numpy()


def _sdf_fields(sdf, gt):
    """the 24 leading fields over points that all count (s, g float64)"""
    rec = np.zeros(24)
    d = np.abs(sdf - gt)
    rec[0] = rec[1] = len(gt)
    rec[2] = d.sum()
    for b in range(6):
        m = (gt > em.BIN_LIMITS[b]) & (gt < em.BIN_LIMITS[b + 1])
        rec[3 + b], rec[9 + b] = d[m].sum(), m.sum()
    for e, eps in enumerate(em.EPSILONS):
        cp, cg = em.chomp(sdf, eps), em.chomp(gt, eps)
        rec[15 + 3 * e: 18 + 3 * e] = np.abs(cp - cg).sum(), cp.sum(), cg.sum()
    return rec


def region_records(pts, sdf, values=None, spacing=None, origin=None, gt=None, sdf_grad=None, flags=None, delta=0.01,
                   cos_fn=None):
    """records [2, 27] float64 (vis, vox) in the kernel's layout.  Ground truth from the volume (values, spacing, origin) or from
    `gt` [n] (every point in bounds).  cos_fn: cos_distance_reference to get the reference's own figure.  float64 `pts` are used as they are: the reference looks the OBJECT points up in float64,
    the kernel takes them rounded to float32."""
    p = np.asarray(pts).astype(np.float64).reshape(-1, 3)       # float32 points widen (the kernel's input); float64 ones stay
    s = np.asarray(sdf, np.float32).astype(np.float64).reshape(-1)
    n = len(p)
    f = np.full(n, 3, np.uint8) if flags is None else np.asarray(flags, np.uint8).reshape(-1)
    if sdf_grad is None:
        f = f & 3
    if gt is None:
        g, inb = em.trilinear(values, spacing, origin, p)
    else:
        g, inb = np.asarray(gt, np.float64).reshape(-1), np.ones(n, bool)
    out = np.zeros((2, RECORD))
    gg = None
    if (f & 12).any():
        sel = (f & 12) != 0
        gg = np.full((n, 3), np.nan)
        gg[sel] = gt_gradient(values, spacing, origin, p[sel], delta)
    for k in range(2):
        m = ((f >> k) & 1).astype(bool) & inb
        out[k, :24] = _sdf_fields(s[m], g[m])
        m = ((f >> (2 + k)) & 1).astype(bool)
        if m.any():
            fin = np.isfinite(gg[m]).all(axis=1)
            x = np.asarray(sdf_grad, np.float32).reshape(-1, 3)[m]
            out[k, 24], out[k, 26] = m.sum(), (~fin).sum()
            out[k, 25] = (cos_fn or cos_distance)(x[fin], gg[m][fin]).sum()     # (cos_distance widens the float32 gradient)
    return out


def set_dict(rec, cossim=False, only_l1=False):
    """the dict of one set as eval_pts.sub_eval / fixed_pts_eval report it (0 / 0 = NaN)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        if only_l1:
            return {"av_l1": float(rec[2] / rec[0])}
        d = em.result_dict(rec[:24])
        if cossim:
            c = float("nan") if rec[26] else float(np.float64(rec[25]) / np.float64(rec[24]))
            d["av_cossim"] = [c, c]
    return d


def load_golden():
    """tests/golden/eval_fixed_small.npz (make_eval_fixed_golden.py) as a dict, with what the generator left out to save space
    recomputed: the toy map's predictions at the stored points, the seeded object points, the flag bytes of every leg"""
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_fixed_small.npz")))
    g["vis_sdf"], g["vis_grad"], g["surf_sdf"] = pred_sdf(g["vis_pts"]), pred_grad(g["vis_pts"]), pred_sdf(g["surf_pts"])
    g["vis_flags"] = chained_flags(g["vis_valid_gt_sdf"], g["vis_valid_vox_sdf"], g["vis_valid_gt_grad"])
    g["surf_flags"] = chained_flags(g["surf_valid_gt_sdf"], g["surf_valid_vox_sdf"])
    state = np.random.get_state()
    bounds = load_obj_bounds(g["obj_bounds_raw"])
    for k, i in enumerate(g["obj_ids"]):
        pts = object_points(bounds[i])[g["obj%d_valid_gt_sdf" % i]]
        g["obj_leg%d_pts" % k], g["obj_leg%d_sdf" % k] = pts, pred_sdf(pts)
        g["obj_leg%d_flags" % k] = (VIS_SDF + VOX_SDF * g["obj%d_valid_vox_sdf" % i].astype(np.uint8)).astype(np.uint8)
    np.random.set_state(state)
    g["vol_sdf"] = pred_sdf(g["vol_pts"])
    return g


def result_from_fixture(g, records_fn=region_records):
    """the nested dict of eval_pts.fixed_pts_eval from the fixture's inputs; records_fn(pts, sdf, **kw) -> [2, 27]"""
    vol = dict(values=g["volume"], spacing=g["spacing"], origin=g["origin"])
    res = {"time": float(g["t"][0])}
    r = records_fn(g["vis_pts"], g["vis_sdf"], sdf_grad=g["vis_grad"], flags=g["vis_flags"], delta=0.01, **vol)
    res["rays"] = {"vis": set_dict(r[0], cossim=True), "vox": set_dict(r[1], cossim=True)}
    r = records_fn(g["surf_pts"], g["surf_sdf"], flags=g["surf_flags"], **vol)
    res["visible_surf"] = {"vis": set_dict(r[0]), "vox": set_dict(r[1])}
    res["objects"] = []
    for k in range(len(g["obj_ids"])):
        r = records_fn(g["obj_leg%d_pts" % k], g["obj_leg%d_sdf" % k], flags=g["obj_leg%d_flags" % k], **vol)
        res["objects"].append({"vis": set_dict(r[0], only_l1=True), "vox": set_dict(r[1], only_l1=True)})
    r = records_fn(g["vol_pts"], g["vol_sdf"], gt=g["vol_gt"])
    res["vol"] = set_dict(r[0])
    return res


def flatten(res, prefix=""):
    """{dotted key: float64 array} of a nested result dict"""
    out = {}
    if isinstance(res, dict):
        for k, v in res.items():
            out.update(flatten(v, prefix + str(k) + "."))
    elif isinstance(res, list) and res and isinstance(res[0], dict):
        for i, v in enumerate(res):
            out.update(flatten(v, prefix + "%d." % i))
    else:
        out[prefix[:-1]] = np.asarray(res, np.float64).reshape(-1)
    return out


# ---- the toy set-up of tests/golden/make_eval_fixed_golden.py: an analytic scene and an analytic "network" ----------------
# Only +, -, *, / and sqrt (all correctly rounded), so every machine recomputes the same float32 predictions from the stored points.
_CA, _RA = np.array([-0.9, -0.7, -0.8]), 0.55
_CB, _RB = np.array([0.2, 0.3, 0.1]), 0.45


def _dist(p, c):
    d = p - c
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])


def scene_sdf(p):
    """the ground-truth field of the fixture's volume: negative inside sphere A (the first bin is populated), ZERO inside
    sphere B (as the replicaCAD grids store the inside of walls)"""
    p = np.asarray(p, np.float64)
    return np.minimum(_dist(p, _CA) - _RA, np.maximum(_dist(p, _CB) - _RB, 0.0))


def _as32(pts):
    return np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 3)          # Trainer.sdf_fn: torch.FloatTensor(pts)


def pred_sdf(pts):
    """the toy map: the signed two-sphere field plus a smooth perturbation, float32 [n] (what Trainer.sdf_fn returns)"""
    p = _as32(pts)
    a, b = _dist(p, _CA) - _RA, _dist(p, _CB) - _RB
    return (np.minimum(a, b) + 0.03 * (p[:, 0] * p[:, 1] - 0.5 * p[:, 2] * p[:, 2]) + 0.02).astype(np.float32)


def pred_grad(pts):
    """its gradient, float32 [n, 3] (what Trainer.grad_fn returns)"""
    p = _as32(pts)
    da, db = _dist(p, _CA), _dist(p, _CB)
    use_a = (da - _RA) <= (db - _RB)
    g = np.where(use_a[:, None], (p - _CA) / da[:, None], (p - _CB) / db[:, None])
    g = g + 0.03 * np.stack([p[:, 1], p[:, 0], -p[:, 2]], axis=1)
    return g.astype(np.float32)


def load_obj_bounds(raw):
    """eval_pts.load_obj_bounds on the numbers of obj_bounds.txt"""
    b = np.asarray(raw, np.float64).reshape(-1, 2, 3).copy()
    b[:, 1] += 0.08
    b[:, 0, 0] -= 0.08
    b[:, 0, 2] -= 0.08
    return b


def object_points(bounds):
    """eval_pts.object_eval_pts; sets numpy's global generator as the reference does"""
    np.random.seed(0)
    offsets = np.random.rand(10000, 3)
    return bounds[0] + offsets * (bounds[1] - bounds[0])[None, :]


def chained_flags(valid_gt_sdf, valid_vox_sdf, valid_gt_grad=None):
    """the flag byte per drawn point from the index sets the reference's chained boolean indexing selects (eval_pts.py:130-152),
    built from index arrays -- independently of HotPath._region_flags"""
    n = len(valid_gt_sdf)
    ix = np.arange(n)
    vis = ix[valid_gt_sdf]
    vox = vis[valid_vox_sdf]
    f = np.zeros(n, np.uint8)
    f[vis] |= VIS_SDF
    f[vox] |= VOX_SDF
    if valid_gt_grad is not None:
        f[ix[valid_gt_grad]] |= VIS_GRAD
        vox_region_gt_valid_grad = valid_gt_grad[valid_gt_sdf][valid_vox_sdf]
        f[ix[valid_gt_sdf][valid_vox_sdf][vox_region_gt_valid_grad]] |= VOX_GRAD
    return f


class KeepIxsDataset:
    """stands in for datasets.SceneCache with keep_ixs (dataset.py:251-257): holds the frames of the sequence whose index is in
    keep_ixs; indexing with a list of sequence indices returns those that are held.  Counts the frames it hands out."""

    def __init__(self, depth, T, keep_ixs):
        self.depth, self.T, self.keep_ixs, self.reads = depth, T, np.asarray(keep_ixs), []

    def __len__(self):
        return len(self.depth)

    def __getitem__(self, idx):
        idx = [x for x in np.asarray(idx).tolist() if x in self.keep_ixs]
        idx = np.array([np.where(self.keep_ixs == x)[0][0] for x in idx], dtype=np.int64)
        self.reads.append(len(idx))
        return {"image": None, "depth": self.depth[idx], "T": self.T[idx]}

    def get_all(self):
        self.reads.append(len(self.depth))
        return {"image": None, "depth": self.depth, "T": self.T}


def write_tree(root, t_str, masks, obj_bounds_raw=None, vol_pts=None, vol_gt=None, seq="seq0", fmt="replicaCAD"):
    """the directory tree eval_pts.fixed_pts_eval reads, under `root`: (eval_pts_dir, seq_dir, eval_pts_root), each ending in '/'.
    masks: {file stem: array}; an existing tree gets the new timestamp added."""
    eval_pts_root = os.path.join(str(root), "eval_pts") + "/"
    seq_dir = os.path.join(str(root), "seqs", seq) + "/"
    eval_pts_dir = eval_pts_root + "vox/0.055/" + seq + "/eval_pts/"
    os.makedirs(os.path.join(eval_pts_dir, t_str), exist_ok=True)
    os.makedirs(seq_dir, exist_ok=True)
    os.makedirs(eval_pts_root + "full_vol", exist_ok=True)
    for stem, m in masks.items():
        np.save(os.path.join(eval_pts_dir, t_str, stem + ".npy"), m)
    if obj_bounds_raw is not None:
        np.savetxt(seq_dir + "obj_bounds.txt", np.asarray(obj_bounds_raw).reshape(-1, 6))
    if vol_pts is not None:
        np.save(eval_pts_root + "full_vol/" + ("replicaCAD" if fmt == "replicaCAD" else seq) + ".npy", vol_pts)
        np.save(eval_pts_root + "full_vol/gt_%s.npy" % seq, vol_gt)
    return eval_pts_dir, seq_dir, eval_pts_root
