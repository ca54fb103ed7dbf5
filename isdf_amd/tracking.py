"""Frame-to-map pose alignment on the device (include/isdf_hip.h: isdf_pose_points, isdf_pose_system).

"Here is a depth frame and roughly where it was taken; where was it really?" -- damped Gauss-Newton on the point-to-SDF residual:
the frame's pixels are back-projected under the pose guess, the map is asked for sdf and d sdf / dx there, and the pose moves so
that the points land on the zero set.  The reference has no counterpart: it takes T_WC from a tracker or from robot kinematics.

    pose_system     one linearisation of B poses: H [B,6,6], b [B,6] and the scalar sums, float64 on the host
    refine_pose     the loop; per iteration one points launch, one field call over all B * n_pix points, one system launch, ONE copy
                    of B x 32 doubles to pinned host memory, a float64 solve per pose on the host
    refine_frames   refine_pose over the stored keyframes of a grafted trainer; it RETURNS the result and writes nothing back

Conventions.  Twist xi = (v, omega) about the camera centre, update R <- exp(omega^) R, t <- t + v; residual r = sdf(x); Jacobian
J = [g, (x - t) x g]; Huber weights (`huber`), residuals beyond `trunc` are dropped; the step solves (H + damping diag(H)) xi = -b.
Plain damped Gauss-Newton: no step rejection.  Module-level functions only: nothing is added to HotPath or HipState.
"""
import collections

import numpy as np
import torch

from . import _ffi
from .engine import host_array

REC = _ffi.POSE_RECORD
_TRIU = np.triu_indices(6)

PoseSystem = collections.namedtuple("PoseSystem", "H b used valid wr2 cost abs_sum records")
PoseSystem.__doc__ = """One linearisation, float64 numpy: H [B,6,6] = sum w J J^T, b [B,6] = sum w r J, used [B] points, valid [B]
pixels, wr2 [B] = sum w r^2, cost [B] = the Huber cost, abs_sum [B] = sum |r| over the used points, records [B,32] as the kernel
wrote them."""

PoseResult = collections.namedtuple("PoseResult", "T_WC converged reason iterations history")
PoseResult.__doc__ = """T_WC [B,4,4] float64; per pose converged (bool [B]), reason (list of str: "converged", "max_iters",
"no_valid_pixels", "too_few_points", "not_positive_definite"), iterations (int [B]: linearisations evaluated); history: per pose
the list of (huber_cost, used, |xi|) of its iterations (|xi| is NaN where no step was taken)."""


class _Scratch:
    """per-device workspace of isdf_pose_system and the pinned host mirror of its records"""

    def __init__(self, device):
        self.device = device
        self.ws = None
        self.records = None
        self.pinned = None

    def reserve(self, engine, B):
        need = int(engine.lib.isdf_pose_ws_bytes(B)) if hasattr(engine, "lib") else 0
        if need > 0 and (self.ws is None or self.ws.numel() < need):
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        if self.records is None or self.records.shape[0] < B:
            self.records = torch.empty(B, REC, dtype=torch.float64, device=self.device)
            self.pinned = torch.empty(B, REC, dtype=torch.float64, pin_memory=self.device.type == "cuda")
        return self.ws, self.records[:B]

    def fetch(self, records):
        """the records on the host: ONE copy into the pinned buffer, then the stream's end"""
        B = int(records.shape[0])
        if records.device.type != "cuda":
            return records.detach().numpy().astype(np.float64).reshape(B, REC)
        host = self.pinned[:B]
        host.copy_(records, non_blocking=True)
        torch.cuda.current_stream(records.device).synchronize()
        return host.numpy().copy()


_SCRATCH = {}


def _scratch(device):
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None or device.type != "cuda" else torch.cuda.current_device())
    s = _SCRATCH.get(key)
    if s is None:
        s = _SCRATCH[key] = _Scratch(device)
    return s


def _engine(obj):
    """an Engine, or anything that has one as `.engine` (SDFMapHIP, a grafted trainer)"""
    return getattr(obj, "engine", obj)


def unpack_records(records):
    """PoseSystem of records [B, 32] (float64, host)"""
    r = np.asarray(records, np.float64).reshape(-1, REC)
    H = np.zeros((r.shape[0], 6, 6))
    H[:, _TRIU[0], _TRIU[1]] = r[:, 10:31]
    H[:, _TRIU[1], _TRIU[0]] = r[:, 10:31]
    return PoseSystem(H, r[:, 4:10].copy(), r[:, 0].copy(), r[:, 1].copy(), r[:, 2].copy(), r[:, 3].copy(), r[:, 31].copy(), r)


def _linearise(eng, scratch, depth, T, cam, fop, field, kw):
    """records [B, 32] on the host for the poses T [B,4,4] (float64; uploaded as float32)"""
    ws, out = scratch.reserve(eng, T.shape[0])
    pts = eng.pose_points(depth, T, cam, frame_of_pose=fop, stride=kw["stride"], min_depth=kw["min_depth"], max_depth=kw["max_depth"])
    sdf, grad = field(pts)
    rec = eng.pose_system(depth, T, cam, pts, sdf, grad, frame_of_pose=fop, huber=kw["huber"], trunc=kw["trunc"], out=out,
                          workspace=ws, stride=kw["stride"], min_depth=kw["min_depth"], max_depth=kw["max_depth"])
    return scratch.fetch(rec)


def _setup(obj, depth, T_WC, frame_of_pose, field):
    eng = _engine(obj)
    T = np.array(T_WC.detach().cpu() if torch.is_tensor(T_WC) else T_WC, dtype=np.float64).reshape(-1, 4, 4)
    fop = None
    if frame_of_pose is not None:
        fop = host_array(frame_of_pose, np.int32).reshape(-1)
        if fop.size != T.shape[0]:
            raise ValueError("%d poses but %d frame indices" % (T.shape[0], fop.size))
    if field is None:
        def field(pts):
            with torch.no_grad():
                return eng.sdf_eval(pts, want_grad=True)
    return eng, _scratch(depth.device), T, fop, field


def pose_system(engine, depth, T_WC, cam, frame_of_pose=None, stride=4, min_depth=0.0, max_depth=float("inf"), huber=0.05, trunc=0.3,
                field=None):
    """PoseSystem of ONE linearisation at the B poses T_WC [B,4,4] against depth [F,H,W] (device): pose b reads frame
    frame_of_pose[b] (None: frame b).  cam: anything with fx, fy, cx, cy.  field: callable, device points [N,3] -> (sdf [N],
    grad [N,3]) on the device; default `engine.sdf_eval(pts, want_grad=True)`."""
    eng, scratch, T, fop, field = _setup(engine, depth, T_WC, frame_of_pose, field)
    kw = dict(stride=stride, min_depth=min_depth, max_depth=max_depth, huber=huber, trunc=trunc)
    return unpack_records(_linearise(eng, scratch, depth, T, cam, fop, field, kw))


def so3_exp(w):
    """exp(w^) [3,3], float64 (Rodrigues; the series near 0)"""
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / (th * th)) * (K @ K)


def apply_twist(T, xi):
    """T [4,4] under the update R <- exp(omega^) R, t <- t + v with xi = (v, omega), float64"""
    out = np.array(T, np.float64)
    out[:3, :3] = so3_exp(xi[3:]) @ out[:3, :3]
    out[:3, 3] = out[:3, 3] + xi[:3]
    return out


def solve_step(H, b, damping):
    """xi of (H + damping diag(H)) xi = -b by Cholesky, or None where the damped matrix is not positive definite (or not finite)"""
    A = H + damping * np.diag(np.diag(H))
    if not (np.isfinite(A).all() and np.isfinite(b).all()):
        return None
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    return -np.linalg.solve(L.T, np.linalg.solve(L, b))


def refine_pose(engine_or_sdf_map_or_trainer, depth, T_WC, cam, frame_of_pose=None, stride=4, min_depth=0.0, max_depth=float("inf"),
                huber=0.05, trunc=0.3, iters=10, damping=1e-6, tol=1e-6, min_points=64, field=None):
    """PoseResult: the B poses T_WC [B,4,4] aligned to the map, each against its depth frame (see `pose_system` for the arguments).

    Per iteration, over the poses still moving: one points launch, one field call, one system launch, one copy of their records,
    then per pose xi from `solve_step` and the update of `apply_twist`, in float64 on the host.  A pose stops when |xi| < tol
    ("converged"), after `iters` linearisations ("max_iters"), when fewer than `min_points` points are used ("too_few_points";
    "no_valid_pixels" when the frame has none) or when the damped matrix is not positive definite ("not_positive_definite"); in
    the last three cases it is left as it was at that point.  No step is ever rejected."""
    eng, scratch, T, fop, field = _setup(engine_or_sdf_map_or_trainer, depth, T_WC, frame_of_pose, field)
    B = T.shape[0]
    kw = dict(stride=stride, min_depth=min_depth, max_depth=max_depth, huber=huber, trunc=trunc)
    frames = np.arange(B, dtype=np.int32) if fop is None else fop
    reason = ["max_iters"] * B
    converged, iterations = np.zeros(B, bool), np.zeros(B, np.int64)
    history = [[] for _ in range(B)]
    active = np.arange(B)
    for _ in range(int(iters)):
        if active.size == 0:
            break
        s = unpack_records(_linearise(eng, scratch, depth, T[active], cam, frames[active], field, kw))
        moving = []
        for k, p in enumerate(active):
            iterations[p] += 1
            xi, stop = None, None
            if s.used[k] < min_points:
                stop = "no_valid_pixels" if s.valid[k] == 0 else "too_few_points"
            else:
                xi = solve_step(s.H[k], s.b[k], damping)
                if xi is None:
                    stop = "not_positive_definite"
            step = float("nan") if xi is None else float(np.linalg.norm(xi))
            history[p].append((float(s.cost[k]), int(s.used[k]), step))
            if stop is None:
                T[p] = apply_twist(T[p], xi)
                if step < tol:
                    stop, converged[p] = "converged", True
            if stop is None:
                moving.append(p)
            else:
                reason[p] = stop
        active = np.asarray(moving, dtype=np.int64)
    return PoseResult(T, converged, reason, iterations, history)


def refine_frames(trainer, idxs=None, **kw):
    """`refine_pose` over the stored keyframes of a grafted trainer: its `frames.depth_batch` and `frames.T_WC_batch` (idxs: which
    keyframes; None = all) with the trainer's intrinsics.  Returns the PoseResult -- result.T_WC[k] belongs to keyframe idxs[k];
    the keyframe store is not written: what to do with a refined pose is the caller's decision."""
    n = int(trainer.frames.depth_batch.shape[0])
    idxs = np.arange(n, dtype=np.int32) if idxs is None else np.asarray(idxs, np.int32).reshape(-1)
    T = trainer.frames.T_WC_batch.detach().cpu().numpy().astype(np.float64)[idxs]
    return refine_pose(trainer, trainer.frames.depth_batch, T, trainer, frame_of_pose=idxs, **kw)
