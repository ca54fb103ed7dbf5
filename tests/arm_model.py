"""Host model of the joint-space planning kernels (include/isdf_hip.h: isdf_arm_points, isdf_arm_step) and of the loop around them:
the frames, the functional, its gradient, the solve, the projection and the record in float64 numpy, written operation by operation
in the header's order and summed in the kernel's order (tests/reduce_model.py), so that every term that holds no sin or cos has the
device's bits; with each sum the sum of |term|, the scale of the bounds.  Also the scenes the CPU and GPU tests share."""
import numpy as np

from isdf_amd import kinematics as kin
from tests import reduce_model as rm
from tests import traj_model as tm

REC = 16
DEFAULTS = dict(kin.DEFAULTS)


def dot(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def cross_abs(a, b):
    """the sum of |term| of each component of a x b"""
    a, b = [np.abs(v) for v in a], [np.abs(v) for v in b]
    return [a[1] * b[2] + a[2] * b[1], a[2] * b[0] + a[0] * b[2], a[0] * b[1] + a[1] * b[0]]


def frames(chain, theta):
    """theta [..., J] (widened) -> (q [..., S, 3] float64 BEFORE the rounding to float32, a [..., J, 3], p [..., J, 3])"""
    th = np.asarray(theta, np.float64)
    lead = th.shape[:-1]
    base = chain.base.astype(np.float64)
    R = [[np.full(lead, base[r, c]) for c in range(3)] for r in range(3)]
    t = [np.full(lead, base[r, 3]) for r in range(3)]
    per_link = [(R, t)]
    a_all, p_all = [], []
    for j in range(chain.J):
        X, u = chain.X[j].astype(np.float64), chain.axes[j].astype(np.float64)
        A = [[dot(R[r][0], R[r][1], R[r][2], X[0, c], X[1, c], X[2, c]) for c in range(3)] for r in range(3)]
        p = [dot(R[r][0], R[r][1], R[r][2], X[0, 3], X[1, 3], X[2, 3]) + t[r] for r in range(3)]
        a = [dot(A[r][0], A[r][1], A[r][2], u[0], u[1], u[2]) for r in range(3)]
        a_all.append(np.stack(a, -1))
        p_all.append(np.stack(p, -1))
        if chain.kinds[j] == 0:
            sn, cs = np.sin(th[..., j]), np.cos(th[..., j])
            k = 1.0 - cs
            M = [[cs + k * (u[0] * u[0]), k * (u[0] * u[1]) - sn * u[2], k * (u[0] * u[2]) + sn * u[1]],
                 [k * (u[1] * u[0]) + sn * u[2], cs + k * (u[1] * u[1]), k * (u[1] * u[2]) - sn * u[0]],
                 [k * (u[2] * u[0]) - sn * u[1], k * (u[2] * u[1]) + sn * u[0], cs + k * (u[2] * u[2])]]
            R = [[dot(A[r][0], A[r][1], A[r][2], M[0][c], M[1][c], M[2][c]) for c in range(3)] for r in range(3)]
            t = p
        else:
            R, t = A, [p[r] + th[..., j] * a[r] for r in range(3)]
        per_link.append((R, t))
    q = []
    for s in range(chain.S):
        R, t = per_link[int(chain.links[s])]
        o = chain.centres[s].astype(np.float64)
        q.append(np.stack([dot(R[r][0], R[r][1], R[r][2], o[0], o[1], o[2]) + t[r] for r in range(3)], -1))
    return np.stack(q, -2), np.stack(a_all, -2), np.stack(p_all, -2)


def points32(chain, theta):
    """q [B * T * S, 3] float32 of theta [B, T, J] float32"""
    return frames(chain, np.asarray(theta, np.float32))[0].astype(np.float32).reshape(-1, 3)


def tsum(terms):
    """[B, T] -> [B]: thread k adds waypoints k, k + 256, .. ascending, then the block's order (a waypoint without a term holds 0)"""
    return rm.block_sum(rm._strided(np.asarray(terms, np.float64).T, 256))


def linearise(chain, theta, q, sdf, grad, eps, w_obs, w_smooth):
    """costs and gradient of B trajectories, float64 throughout: theta [B,T,J], q [B,T,S,3], sdf [B,T,S], grad [B,T,S,3] (any float
    dtype, widened).  Returns a dict of the record's entries, `scale` (sum of |term| of the four sums), grad [B,T,J] and
    grad_scale [B,T,J]."""
    th, q = np.asarray(theta, np.float64), np.asarray(q, np.float64)
    sdf, grad = np.asarray(sdf, np.float64), np.asarray(grad, np.float64)
    B, T, S = sdf.shape
    J = chain.J
    rad = chain.radii.astype(np.float64)
    eps, w_obs, ws = float(eps), float(w_obs), float(w_smooth) * float(T - 1)
    n_bad = (~np.isfinite(sdf)).sum(-1) + (~np.isfinite(grad)).sum((-1, -2))          # [B,T] values
    ok = np.isfinite(sdf) & np.isfinite(grad).all(-1)
    interior = np.zeros(T, bool)
    interior[1:-1] = True
    live = ok & interior[None, :, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = np.where(ok, sdf - rad[None, None, :], np.inf)
        c, cp = tm.cost(d, eps)
        c, cp = np.where(live, c, 0.0), np.where(live, cp, 0.0)
        v = np.zeros((B, T, S, 3))
        v[:, 1:-1] = (q[:, 2:] - q[:, :-2]) * 0.5
        sigma = np.where(live, tm.norm3(v), 0.0)
        h = np.where((sigma > 0)[..., None], v / sigma[..., None], 0.0)
        ch = c[..., None] * h
        prev, nxt = np.zeros_like(ch), np.zeros_like(ch)
        prev[:, 1:], nxt[:, :-1] = ch[:, :-1], ch[:, 1:]
        e = sigma * cp
        g = np.where(live[..., None], grad, 0.0)
        r = np.where(live[..., None], e[..., None] * g + (prev - nxt) * 0.5, 0.0)
        r_abs = np.where(live[..., None], np.abs(e[..., None] * g) + (np.abs(prev) + np.abs(nxt)) * 0.5, 0.0)
    x = np.stack(cross([q[..., k] for k in range(3)], [r[..., k] for k in range(3)]), -1)
    x_abs = np.stack(cross_abs([q[..., k] for k in range(3)], [r_abs[..., k] for k in range(3)]), -1)
    fo, fo_abs = np.zeros((B, T)), np.zeros((B, T))
    Rl, Ml = np.zeros((J, B, T, 3)), np.zeros((J, B, T, 3))
    Rl_abs, Ml_abs = np.zeros((J, B, T, 3)), np.zeros((J, B, T, 3))
    for s in range(S):                                                                # s ascending, as the kernel adds them
        fo = np.where(live[:, :, s], fo + c[:, :, s] * sigma[:, :, s], fo)
        fo_abs = fo_abs + np.abs(c[:, :, s] * sigma[:, :, s])
        link = int(chain.links[s])
        if link >= 1:
            m = live[:, :, s, None]
            Rl[link - 1] = np.where(m, Rl[link - 1] + r[:, :, s], Rl[link - 1])
            Ml[link - 1] = np.where(m, Ml[link - 1] + x[:, :, s], Ml[link - 1])
            Rl_abs[link - 1] += r_abs[:, :, s]
            Ml_abs[link - 1] += x_abs[:, :, s]
    for j in range(J - 2, -1, -1):                                                    # suffix sums over the links
        Rl[j], Ml[j] = Rl[j + 1] + Rl[j], Ml[j + 1] + Ml[j]
        Rl_abs[j], Ml_abs[j] = Rl_abs[j + 1] + Rl_abs[j], Ml_abs[j + 1] + Ml_abs[j]
    _, a, p = frames(chain, th)
    sm, sm_abs = np.zeros((B, T, J)), np.zeros((B, T, J))
    sm[:, 1:-1] = (2.0 * th[:, 1:-1] - th[:, :-2]) - th[:, 2:]
    sm_abs[:, 1:-1] = 2.0 * np.abs(th[:, 1:-1]) + np.abs(th[:, :-2]) + np.abs(th[:, 2:])
    gt, gs = np.zeros((B, T, J)), np.zeros((B, T, J))
    for j in range(J):
        aj, pj = [a[..., j, k] for k in range(3)], [p[..., j, k] for k in range(3)]
        Rs, Ms = [Rl[j][..., k] for k in range(3)], [Ml[j][..., k] for k in range(3)]
        Ra, Ma = [Rl_abs[j][..., k] for k in range(3)], [Ml_abs[j][..., k] for k in range(3)]
        if chain.kinds[j] == 0:
            pxr, pxr_abs = cross(pj, Rs), cross_abs(pj, Ra)
            w = [Ms[k] - pxr[k] for k in range(3)]
            o = dot(aj[0], aj[1], aj[2], w[0], w[1], w[2])
            o_abs = sum(np.abs(aj[k]) * (Ma[k] + pxr_abs[k]) for k in range(3))
        else:
            o = dot(aj[0], aj[1], aj[2], Rs[0], Rs[1], Rs[2])
            o_abs = sum(np.abs(aj[k]) * Ra[k] for k in range(3))
        gt[:, 1:-1, j] = (w_obs * o + ws * sm[..., j])[:, 1:-1]
        gs[:, 1:-1, j] = (w_obs * o_abs + ws * sm_abs[..., j])[:, 1:-1]
    g2, qd = np.zeros((B, T)), np.zeros((B, T - 1))
    dth = th[:, 1:] - th[:, :-1]
    for j in range(J):                                                                # j ascending
        g2 = g2 + gt[..., j] * gt[..., j]
        qd = qd + dth[..., j] * dth[..., j]
    seg = np.zeros((B, T))
    seg[:, :-1] = qd
    f_terms = np.where(interior[None], fo, 0.0)
    half = 0.5 * float(T - 1)
    out = dict(f_obs=tsum(f_terms), f_smooth=half * tsum(seg), grad_sq=tsum(g2), length=tsum(np.sqrt(seg)),
               min_d=np.where(ok, d, np.inf).reshape(B, -1).min(-1), n_neg=(ok & (d < 0)).reshape(B, -1).sum(-1),
               n_act=(ok & (d < eps)).reshape(B, -1).sum(-1), n_bad=n_bad.sum(-1), grad=gt, grad_scale=gs)
    out["scale"] = dict(f_obs=np.where(interior[None], fo_abs, 0.0).sum(-1), f_smooth=half * seg.sum(-1), grad_sq=g2.sum(-1),
                        length=np.sqrt(seg).sum(-1))
    return out


def objective(chain, theta, field, eps, w_obs, w_smooth):
    """(w_obs F_obs + w_smooth F_smooth [B], linearise's dict) of float64 trajectories theta [B,T,J] under field: float64 points
    [N,3] -> (sdf, grad); the query points stay float64"""
    th = np.asarray(theta, np.float64)
    B, T = th.shape[:2]
    q = frames(chain, th)[0]
    sdf, grad = field(q.reshape(-1, 3))
    lin = linearise(chain, th, q, sdf.reshape(B, T, -1), grad.reshape(B, T, -1, 3), eps, w_obs, w_smooth)
    return float(w_obs) * lin["f_obs"] + float(w_smooth) * lin["f_smooth"], lin


def limits(chain):
    lo = np.full(chain.J, -np.inf) if chain.lo is None else chain.lo.astype(np.float64)
    hi = np.full(chain.J, np.inf) if chain.hi is None else chain.hi.astype(np.float64)
    return lo, hi


def step64(chain, theta, state, q, sdf, grad, eps=0.2, w_obs=8.0, w_smooth=1.0, eta=32.0, max_step=0.05, tol=1e-5):
    """one isdf_arm_step on the host: (records [B,16], scale [B,16], grad [B,T,J], theta_new float32 [B,T,J], state_new int32 [B],
    grad_scale [B,T,J]).  theta float32 [B,T,J], state [B]; q [B*T*S,3], sdf [B*T*S], grad [B*T*S,3] float32; the scalar
    parameters are rounded to float32 first, as the ABI takes them."""
    th32 = np.asarray(theta, np.float32)
    B, T, J = th32.shape
    S = chain.S
    eps, w_obs, w_smooth, eta, max_step, tol = (float(np.float32(v)) for v in (eps, w_obs, w_smooth, eta, max_step, tol))
    lin = linearise(chain, th32, np.asarray(q, np.float32).reshape(B, T, S, 3), np.asarray(sdf, np.float32).reshape(B, T, S),
                    np.asarray(grad, np.float32).reshape(B, T, S, 3), eps, w_obs, w_smooth)
    lo, hi = limits(chain)
    th = th32.astype(np.float64)

    def step(b, y):
        z0 = th[b, 1:-1] + -(y / (eta * float(T - 1)))
        z = np.minimum(np.maximum(z0, lo[None]), hi[None])
        dp = z - th[b, 1:-1]
        return dp, float(np.abs(dp).max()), float((z != z0).sum())
    return tm.close64(lin, th32, state, max_step, tol, step)


def loop64(chain, theta0, field, iters=400, **params):
    """the loop of kinematics.optimise_joint_trajectories on the host, theta stored in float32 between iterations: (theta float32
    [B,T,J], records [B,16] of the last step, iterations).  field: float64 points [N,3] -> (sdf, grad), rounded to float32."""
    p = dict(DEFAULTS, **params)
    th = np.asarray(theta0, np.float32).copy()
    state = np.zeros(th.shape[0], np.int32)
    rec, done = np.zeros((th.shape[0], REC)), 0
    while done < iters and (state == 0).any():
        q = points32(chain, th)
        sdf, grad = field(q.astype(np.float64))
        rec, _, _, th, state, _ = step64(chain, th, state, q, np.asarray(sdf, np.float32), np.asarray(grad, np.float32), **p)
        done += 1
    return th, rec, done


def sphere_field(centre=(1.5, 2.5, 1.5), radius=0.5):
    """the single analytic sphere of the gradient test: float64 distance and its exact gradient v / |v|"""
    return tm.sphere_field(centre, radius)


class StubEngine(tm.StubEngine):
    """arm_points and arm_step, computed by this model"""

    def __init__(self):
        super().__init__("arm", lambda th, chain: points32(chain, th),
                         lambda th, state, chain, q, sdf, grad, **kw: step64(chain, th, state, q.numpy(), sdf, grad, **kw))


# ---- scenes ------------------------------------------------------------------------------------------------------------
def _trans_z(z):
    X = np.hstack([np.eye(3), np.zeros((3, 1))])
    X[2, 3] = z
    return X


def arm_a():
    """four revolute joints on a base at (2.6, 3.0, 1.5) whose z axis points up from the floor (the room's y axis points down):
    16 spheres of radius 0.06 every 0.1 m along links 2, 3 and 4"""
    base = np.array([[1.0, 0.0, 0.0, 2.6], [0.0, 0.0, -1.0, 3.0], [0.0, 1.0, 0.0, 1.5]])
    X = np.stack([_trans_z(z) for z in (0.1, 0.2, 0.6, 0.5)])
    axes = [[0, 0, 1], [1, 0, 0], [1, 0, 0], [1, 0, 0]]
    links, centres = [], []
    for link, n in ((2, 7), (3, 6), (4, 3)):
        for i in range(n):
            links.append(link)
            centres.append([0.0, 0.0, 0.1 * i])
    return kin.Chain(base, X, [0, 0, 0, 0], axes, links, centres, 0.06)


def free_body():
    """Chain.free_body with five spheres of radius 0.08 at local x = -0.4 .. 0.4"""
    return kin.Chain.free_body([[x, 0.0, 0.0] for x in np.linspace(-0.4, 0.4, 5)], 0.08)


def line(start, goal, T):
    """theta [1, T, J] float32: the straight line in joint space"""
    return kin.seed_joint_trajectories(start, goal, T, 1)


# name -> (chain factory, start, goal): the end-to-end scenarios on the exact room, T = 32
SCENARIOS = {
    "arm_a": (arm_a, (-0.2, 1.1, 0.5, 0.2), (-2.9, 1.1, 0.5, 0.2)),
    "arm_a_high": (arm_a, (-0.2, 0.7, 0.6, 0.2), (-2.9, 0.7, 0.6, 0.2)),
    "free_body": (free_body, (3.3, 2.5, 0.5, 0.0, 0.0, 0.0), (5.5, 2.0, 2.3, 1.5, 0.0, 0.0)),
}
