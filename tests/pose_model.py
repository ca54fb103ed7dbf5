"""Host model of the pose-alignment kernels (include/isdf_hip.h: isdf_pose_points, isdf_pose_system) and of the loop around them:
the point chain in numpy float32 exactly as the header states it, the record in float64 from the float32 arrays (with the sum of
|term| per entry, the scale of the reordering bound), an analytic field, and a stub engine whose two calls are this model, so
that isdf_amd.tracking's host loop runs without a device."""
import types

import numpy as np
import torch

from isdf_amd import synthetic

REC = 32
TRIU = np.triu_indices(6)


def cam_of(H, W, f):
    """the test cameras: fx = fy = f, principal point at the image centre"""
    return types.SimpleNamespace(H=H, W=W, fx=float(f), fy=float(f), cx=(W - 1) / 2.0, cy=(H - 1) / 2.0)


def as_dict(cam):
    return dict(H=cam.H, W=cam.W, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy)


def lattice(H, W, stride):
    """(rows, cols) of the lattice pixels, row-major: every stride-th row and column from 0"""
    r, c = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    return r.reshape(-1), c.reshape(-1)


def valid32(z, min_depth, max_depth):
    z = np.asarray(z, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z != 0) & (z >= np.float32(min_depth)) & (z <= np.float32(max_depth))


def _poses12(T_WC):
    T = np.asarray(T_WC)
    if T.shape[-2:] == (4, 4):
        T = T.reshape(-1, 4, 4)[:, :3, :]
    return np.ascontiguousarray(T.reshape(-1, 12), dtype=np.float32)


def points32(depth, T_WC, cam, frame_of_pose=None, stride=4, min_depth=0.0, max_depth=np.inf):
    """(pts [B * n_pix, 3] float32, valid [B * n_pix] bool): every operation in float32, rounded on its own"""
    depth = np.asarray(depth, np.float32)
    T = _poses12(T_WC)
    B = T.shape[0]
    fop = np.arange(B) if frame_of_pose is None else np.asarray(frame_of_pose).reshape(-1)
    r, c = lattice(depth.shape[1], depth.shape[2], stride)
    fx, fy, cx, cy = (np.float32(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy))
    out, ok = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            z = depth[fop[b], r, c]
            v = valid32(z, min_depth, max_depth)
            xc = (z * (c.astype(np.float32) - cx)) / fx
            yc = (z * (r.astype(np.float32) - cy)) / fy
            t = T[b]
            w = np.stack([((t[4 * k] * xc + t[4 * k + 1] * yc) + t[4 * k + 2] * z) + t[4 * k + 3] for k in range(3)], -1)
            w[~v] = t[[3, 7, 11]]
            out.append(w.astype(np.float32))
            ok.append(v)
    return np.concatenate(out), np.concatenate(ok)


def _pose_terms(pts, sdf, grad, valid, T, b, n, hub, tr):
    """(terms [used points, 32], used [n] bool, ok [n] bool) of pose b: every product in the kernel's order"""
    s = slice(b * n, (b + 1) * n)
    r = np.asarray(sdf[s], np.float32).astype(np.float64)
    a = np.abs(r)
    ok = np.asarray(valid[s], bool)
    with np.errstate(invalid="ignore"):
        used = ok & (a <= tr)
    r, a = r[used], a[used]
    g = np.asarray(grad[s], np.float32).astype(np.float64)[used]
    d = np.asarray(pts[s], np.float32).astype(np.float64)[used] - T[b, [3, 7, 11]]
    quad = a <= hub
    w = np.where(quad, 1.0, hub / np.where(quad, 1.0, a))
    J = np.concatenate([g, np.stack([d[:, 1] * g[:, 2] - d[:, 2] * g[:, 1], d[:, 2] * g[:, 0] - d[:, 0] * g[:, 2],
                                     d[:, 0] * g[:, 1] - d[:, 1] * g[:, 0]], -1)], -1)
    wr = w * r
    terms = np.zeros((len(r), REC))
    terms[:, 0] = 1.0
    terms[:, 2] = wr * r
    terms[:, 3] = np.where(quad, 0.5 * (r * r), hub * (a - 0.5 * hub))
    terms[:, 4:10] = wr[:, None] * J
    terms[:, 10:31] = (w[:, None] * J)[:, TRIU[0]] * J[:, TRIU[1]]
    terms[:, 31] = a
    return terms, used, ok


def records64(pts, sdf, grad, valid, T_WC, huber=0.05, trunc=0.3):
    """(records [B, 32], scale [B, 32]) in float64 from the float32 arrays: the header's record, and per entry the sum of |term|
    (the counts' scale is the count).  huber and trunc are rounded to float32 first, as the ABI takes them."""
    T = _poses12(T_WC).astype(np.float64)
    B = T.shape[0]
    n = len(sdf) // B
    hub, tr = float(np.float32(huber)), float(np.float32(trunc))
    rec, scale = np.zeros((B, REC)), np.zeros((B, REC))
    for b in range(B):
        terms, _, ok = _pose_terms(pts, sdf, grad, valid, T, b, n, hub, tr)
        rec[b], scale[b] = terms.sum(0), np.abs(terms).sum(0)
        rec[b, 1] = scale[b, 1] = ok.sum()
    return rec, scale


def terms64(pts, sdf, grad, valid, T_WC, huber=0.05, trunc=0.3):
    """[B, n_pix, 32]: what every lattice pixel adds to its pose's record (zero where it is not used; column 1 counts the valid
    pixels), for the exact-order model of tests/reduce_model.py"""
    T = _poses12(T_WC).astype(np.float64)
    B = T.shape[0]
    n = len(sdf) // B
    out = np.zeros((B, n, REC))
    for b in range(B):
        terms, used, ok = _pose_terms(pts, sdf, grad, valid, T, b, n, float(np.float32(huber)), float(np.float32(trunc)))
        out[b, used] = terms
        out[b, :, 1] = ok
    return out


# ---- analytic fields: float64 value, central-difference gradient (h = 1e-4), both rounded to float32 ---------------------
H_FD = 1e-4


def room_field(pts):
    """(sdf, grad) float32 of synthetic.gt_sdf at pts [N, 3]"""
    p = np.asarray(pts, np.float64)
    g = np.stack([(synthetic.gt_sdf(p + H_FD * e) - synthetic.gt_sdf(p - H_FD * e)) / (2 * H_FD) for e in np.eye(3)], -1)
    return synthetic.gt_sdf(p).astype(np.float32), g.astype(np.float32)


def plane_field(pts, axis=1, offset=3.0):
    """a single infinite plane (the room's floor y = 3): sdf = offset - p[axis], gradient -e_axis everywhere"""
    p = np.asarray(pts, np.float64)
    g = np.zeros(p.shape, np.float32)
    g[:, axis] = -1.0
    return (offset - p[:, axis]).astype(np.float32), g


def room_field_torch(pts):
    """room_field restated in torch float64 on pts' device: (sdf, grad) float32 tensors"""
    def sdf(p):
        lo = torch.tensor(synthetic.ROOM_LO, dtype=torch.float64, device=p.device)
        hi = torch.tensor(synthetic.ROOM_HI, dtype=torch.float64, device=p.device)
        d = torch.minimum(p - lo, hi - p).min(-1).values
        for c, r in synthetic.SPHERES:
            d = torch.minimum(d, torch.linalg.norm(p - torch.tensor(c, dtype=torch.float64, device=p.device), dim=-1) - r)
        for blo, bhi in synthetic.BOXES:
            blo = torch.tensor(blo, dtype=torch.float64, device=p.device)
            bhi = torch.tensor(bhi, dtype=torch.float64, device=p.device)
            q = torch.maximum(blo - p, p - bhi)
            outside = torch.linalg.norm(torch.clamp(q, min=0.0), dim=-1)
            inside = torch.clamp(q.max(-1).values, max=0.0)
            d = torch.minimum(d, outside + inside)
        return d
    p = pts.detach().to(torch.float64)
    eye = torch.eye(3, dtype=torch.float64, device=p.device)
    g = torch.stack([(sdf(p + H_FD * eye[k]) - sdf(p - H_FD * eye[k])) / (2 * H_FD) for k in range(3)], -1)
    return sdf(p).to(torch.float32), g.to(torch.float32)


# ---- the test scene: eight poses of the synthetic trajectory ----------------------------------------------------------------------------------------
def poses8():
    return synthetic.trajectory(600)[::75].astype(np.float64)


def render(T_WC, cam, seed=0, invalid_frac=0.02, noise_std=0.0):
    """depth [B, H, W] float32 of the analytic room from the poses, `invalid_frac` of the pixels set to 0"""
    return np.stack([synthetic.render_depth(np.asarray(T, np.float32), as_dict(cam), np.random.RandomState(seed + i),
                                            invalid_frac=invalid_frac, noise_std=noise_std) for i, T in enumerate(T_WC)])


def so3_exp(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / th ** 2 * (K @ K)


def perturb(T_WC, metres, degrees, seed=0):
    """every pose moved by `metres` along a random direction and turned by `degrees` about a random axis (about its centre)"""
    rng = np.random.RandomState(seed)
    out = np.array(T_WC, np.float64)
    for T in out:
        v, w = rng.standard_normal(3), rng.standard_normal(3)
        T[:3, :3] = so3_exp(w / np.linalg.norm(w) * np.deg2rad(degrees)) @ T[:3, :3]
        T[:3, 3] += v / np.linalg.norm(v) * metres
    return out


def pose_error(T, T_true):
    """(metres, degrees) between poses [.., 4, 4]; the angle as asin(|dR - dR^T|_F / sqrt 8), exact for small angles where
    arccos of the trace loses half the digits"""
    T, T_true = np.asarray(T, np.float64).reshape(-1, 4, 4), np.asarray(T_true, np.float64).reshape(-1, 4, 4)
    dt = np.linalg.norm(T[:, :3, 3] - T_true[:, :3, 3], axis=-1)
    dR = T[:, :3, :3] @ np.transpose(T_true[:, :3, :3], (0, 2, 1))
    s = np.linalg.norm(dR - np.transpose(dR, (0, 2, 1)), axis=(1, 2)) / np.sqrt(8.0)
    return dt, np.rad2deg(np.arcsin(np.clip(s, 0.0, 1.0)))


def gauss_newton(depth, T_WC, cam, field, frame_of_pose=None, stride=4, huber=0.05, trunc=0.3, iters=10, damping=1e-6, tol=1e-6,
                 min_points=64):
    """the damped Gauss-Newton loop of isdf_amd.tracking.refine_pose, written out on its own: (T [B,4,4] float64, iterations [B], converged [B]); field: numpy
    pts -> (sdf, grad)"""
    T = np.array(T_WC, np.float64).reshape(-1, 4, 4)
    B = T.shape[0]
    fop = np.arange(B) if frame_of_pose is None else np.asarray(frame_of_pose)
    its, done = np.zeros(B, int), np.zeros(B, bool)
    for b in range(B):
        for _ in range(iters):
            pts, valid = points32(depth, T[b:b + 1], cam, fop[b:b + 1], stride)
            sdf, grad = field(pts)
            rec = records64(pts, sdf, grad, valid, T[b:b + 1], huber, trunc)[0][0]
            its[b] += 1
            if rec[0] < min_points:
                break
            Hm = np.zeros((6, 6))
            Hm[TRIU] = rec[10:31]
            Hm = Hm + np.triu(Hm, 1).T
            try:
                L = np.linalg.cholesky(Hm + damping * np.diag(np.diag(Hm)))
            except np.linalg.LinAlgError:
                break
            xi = -np.linalg.solve(L.T, np.linalg.solve(L, rec[4:10]))
            T[b, :3, :3] = so3_exp(xi[3:]) @ T[b, :3, :3]
            T[b, :3, 3] += xi[:3]
            if np.linalg.norm(xi) < tol:
                done[b] = True
                break
    return T, its, done


class StubEngine:
    """the two tensor-level calls of isdf_amd.engine.Engine, computed by this model on the host (CPU tensors in and out)"""

    def __init__(self):
        self.device = torch.device("cpu")
        self.calls = []

    def pose_points(self, depth, T_WC, cam, frame_of_pose=None, stride=4, min_depth=0.0, max_depth=float("inf")):
        pts, _ = points32(depth.numpy(), T_WC, cam, frame_of_pose, stride, min_depth, max_depth)
        self.calls.append(("points", len(np.asarray(T_WC).reshape(-1, 4, 4)), None if frame_of_pose is None else list(frame_of_pose)))
        return torch.from_numpy(pts)

    def pose_system(self, depth, T_WC, cam, pts, sdf, grad, frame_of_pose=None, stride=4, min_depth=0.0, max_depth=float("inf"),
                    huber=0.05, trunc=0.3, out=None, workspace=None):
        _, valid = points32(depth.numpy(), T_WC, cam, frame_of_pose, stride, min_depth, max_depth)
        rec, _ = records64(pts.numpy(), sdf.numpy(), grad.numpy(), valid, T_WC, huber, trunc)
        self.calls.append(("system", rec.shape[0], None if frame_of_pose is None else list(frame_of_pose)))
        return torch.from_numpy(rec)


def host_field(fn):
    """a numpy field (pts -> (sdf, grad)) as the tensor callable isdf_amd.tracking takes"""
    def field(pts):
        s, g = fn(pts.numpy())
        return torch.from_numpy(s), torch.from_numpy(g)
    return field
