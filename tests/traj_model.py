"""Host model of the planning kernels (include/isdf_hip.h: isdf_traj_points, isdf_traj_step) and of the loop around them: the query
points in numpy float32, one iteration in float64 written operation by operation in the header's order (so that every TERM of a
sum has the device's bits and only the order of summation differs; with it the sum of |term| per entry, the scale of the
reordering bound), both tridiagonal solves, and a stub engine whose two calls are this model, so that isdf_amd.planning's host
loop runs without a device."""
import numpy as np
import torch

REC = 16
DEFAULTS = dict(eps=0.2, w_obs=8.0, w_smooth=1.0, eta=8.0, max_step=0.05, tol=1e-5)


def body(offsets, radii):
    off = np.zeros((1, 3), np.float32) if offsets is None else np.ascontiguousarray(np.asarray(offsets, np.float32)).reshape(-1, 3)
    rad = np.asarray(radii, np.float32).reshape(-1)
    return off, np.ascontiguousarray(np.broadcast_to(rad, (off.shape[0],)) if rad.size == 1 else rad)


def points32(x, offsets):
    """q [B * T * S, 3] float32: x[b][t] + o_s, one float32 add per coordinate"""
    x, off = np.asarray(x, np.float32), np.asarray(offsets, np.float32).reshape(-1, 3)
    return (x[:, :, None, :] + off[None, None, :, :]).astype(np.float32).reshape(-1, 3)


def cost(d, eps):
    """(c, c') of the clearance d, float64"""
    u = d - eps
    c = np.where(d < 0, -d + eps * 0.5, np.where(d <= eps, (u * u) / (2.0 * eps), 0.0))
    cp = np.where(d < 0, -1.0, np.where(d <= eps, u / eps, 0.0))
    return c, cp


def norm3(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def solve_closed(g):
    """A^-1 g for A = tridiag(-1, 2, -1) of order n, g [n, ...]: the closed-form inverse min(i,j) (n+1-max(i,j)) / (n+1) through
    two ordered prefix sums, in the kernel's order"""
    g = np.asarray(g, np.float64)
    n = g.shape[0]
    shape = (n,) + (1,) * (g.ndim - 1)
    i = np.arange(1, n + 1, dtype=np.float64).reshape(shape)
    w = (n + 1) - i
    P = np.cumsum(i * g, axis=0)                                        # sequential, j ascending
    tail = np.cumsum((w * g)[::-1], axis=0)[::-1]                       # sequential, j descending: sum_{j >= i}
    Q = np.concatenate([tail[1:], np.zeros_like(tail[:1])], 0)          # sum_{j > i}
    return (w * P + i * Q) / float(n + 1)


def solve_thomas(g):
    """A^-1 g by the Thomas algorithm with the pivots of this matrix in closed form, (i+1)/i"""
    g = np.asarray(g, np.float64)
    n = g.shape[0]
    d = np.array(g, np.float64)
    for i in range(2, n + 1):
        d[i - 1] = g[i - 1] + d[i - 2] * (i - 1) / i
    y = np.empty_like(d)
    y[n - 1] = d[n - 1] * n / (n + 1)
    for i in range(n - 1, 0, -1):
        y[i - 1] = (d[i - 1] + y[i]) * i / (i + 1)
    return y


def linearise(x, sdf, grad, radii, eps, w_obs, w_smooth):
    """costs and gradient of B trajectories, float64 throughout: x [B,T,3], sdf [B,T,S], grad [B,T,S,3] (any float dtype, widened).
    Returns a dict of the record's entries, `scale` (sum of |term| of the four sums), and grad [B,T,3]."""
    x, sdf, grad = np.asarray(x, np.float64), np.asarray(sdf, np.float64), np.asarray(grad, np.float64)
    B, T, S = sdf.shape
    rad = np.asarray(radii, np.float64).reshape(-1)
    eps, w_obs, ws = float(eps), float(w_obs), float(w_smooth) * float(T - 1)
    n_bad = (~np.isfinite(sdf)).sum(-1) + (~np.isfinite(grad)).sum((-1, -2))          # [B,T] values
    ok = np.isfinite(sdf) & np.isfinite(grad).all(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(ok, sdf - rad[None, None, :], np.inf)
        c, cp = cost(d, eps)
        C, G = np.zeros((B, T)), np.zeros((B, T, 3))
        for s in range(S):                                                            # s ascending, as the kernel adds them
            C = C + np.where(ok[:, :, s], c[:, :, s], 0.0)
            G = G + np.where(ok[:, :, s, None], cp[:, :, s, None] * grad[:, :, s, :], 0.0)
    C[:, 0] = C[:, -1] = 0.0
    v = (x[:, 2:] - x[:, :-2]) * 0.5
    sigma = norm3(v)
    with np.errstate(invalid="ignore", divide="ignore"):
        vh = np.where(sigma[..., None] > 0, v / sigma[..., None], 0.0)
    cv = np.zeros((B, T, 3))
    cv[:, 1:-1] = C[:, 1:-1, None] * vh
    f_terms = C[:, 1:-1] * sigma
    e = x[:, 1:] - x[:, :-1]
    seg2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    obs = sigma[..., None] * G[:, 1:-1] + (cv[:, :-2] - cv[:, 2:]) * 0.5
    sm = (2.0 * x[:, 1:-1] - x[:, :-2]) - x[:, 2:]
    g = np.zeros((B, T, 3))
    g[:, 1:-1] = w_obs * obs + ws * sm
    gsq = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
    half = 0.5 * float(T - 1)
    out = dict(f_obs=f_terms.sum(-1), f_smooth=half * seg2.sum(-1), grad_sq=gsq.sum(-1), length=np.sqrt(seg2).sum(-1),
               min_d=np.where(ok, d, np.inf).reshape(B, -1).min(-1), n_neg=(ok & (d < 0)).reshape(B, -1).sum(-1),
               n_act=(ok & (d < eps)).reshape(B, -1).sum(-1), n_bad=n_bad.sum(-1), grad=g)
    out["scale"] = dict(f_obs=np.abs(f_terms).sum(-1), f_smooth=half * seg2.sum(-1), grad_sq=gsq.sum(-1), length=np.sqrt(seg2).sum(-1))
    # per component of grad_t the sum of |term|: the S products of sigma G, the two neighbours' C vh, the three of the smoothness
    absG = np.zeros((B, T, 3))
    with np.errstate(invalid="ignore"):
        for s in range(S):
            absG = absG + np.where(ok[:, :, s, None], np.abs(cp[:, :, s, None] * grad[:, :, s, :]), 0.0)
    gs = np.zeros((B, T, 3))
    gs[:, 1:-1] = w_obs * (sigma[..., None] * absG[:, 1:-1] + (np.abs(cv[:, :-2]) + np.abs(cv[:, 2:])) * 0.5) \
        + ws * (2.0 * np.abs(x[:, 1:-1]) + np.abs(x[:, :-2]) + np.abs(x[:, 2:]))
    out["grad_scale"] = gs
    return out


def objective(x, field, offsets, radii, eps, w_obs, w_smooth):
    """w_obs F_obs + w_smooth F_smooth [B] of float64 trajectories x [B,T,3] under field: float64 points [N,3] -> (sdf, grad)"""
    x = np.asarray(x, np.float64)
    B, T = x.shape[:2]
    off = np.asarray(offsets, np.float64).reshape(-1, 3)
    q = x[:, :, None, :] + off[None, None]
    sdf, grad = field(q.reshape(-1, 3))
    lin = linearise(x, sdf.reshape(B, T, -1), grad.reshape(B, T, -1, 3), radii, eps, w_obs, w_smooth)
    return float(w_obs) * lin["f_obs"] + float(w_smooth) * lin["f_smooth"], lin


def step64(x, state, offsets, radii, sdf, grad, eps=0.2, w_obs=8.0, w_smooth=1.0, eta=8.0, max_step=0.05, tol=1e-5, solve=solve_closed):
    """one isdf_traj_step on the host: (records [B,16], scale [B,16], grad [B,T,3], x_new float32 [B,T,3], state_new int32 [B],
    grad_scale [B,T,3]).  x float32 [B,T,3], state [B]; sdf [B*T*S], grad [B*T*S,3] float32; the scalar parameters are rounded
    to float32 first, as the ABI takes them."""
    x = np.asarray(x, np.float32)
    B, T = x.shape[:2]
    off, rad = body(offsets, radii)
    S = off.shape[0]
    eps, w_obs, w_smooth, eta, max_step, tol = (float(np.float32(v)) for v in (eps, w_obs, w_smooth, eta, max_step, tol))
    lin = linearise(x, np.asarray(sdf, np.float32).reshape(B, T, S), np.asarray(grad, np.float32).reshape(B, T, S, 3), rad, eps,
                    w_obs, w_smooth)

    def step(b, y):
        delta = -(y / (eta * float(T - 1)))
        return delta, float(norm3(delta).max()), 0.0
    return close64(lin, x, state, max_step, tol, step, solve)


def close64(lin, var, state, max_step, tol, step, solve=solve_closed):
    """a step after its linearisation `lin`, for isdf_traj_step and isdf_arm_step alike: the record, the state rule, the clamp
    factor and the new float32 trajectory.  var float32 [B,T,K]; step(b, y) turns y = solve(grad[b, 1:-1]) into (the step
    Delta [T-2,K] of the interior rows, its length m, the entries a limit cut).  Returns step64's tuple."""
    B = var.shape[0]
    state = np.asarray(state, np.int32).reshape(B)
    rec, scale = np.zeros((B, REC)), np.zeros((B, REC))
    new, state_new = var.copy(), state.copy()
    for k, name in ((0, "f_obs"), (1, "f_smooth"), (5, "grad_sq"), (10, "length")):
        rec[:, k], scale[:, k] = lin[name], lin["scale"][name]
    rec[:, 2], rec[:, 3], rec[:, 4], rec[:, 8] = lin["min_d"], lin["n_neg"], lin["n_act"], lin["n_bad"]
    for b in range(B):
        if state[b] == 0:
            delta, m, rec[b, 11] = step(b, solve(lin["grad"][b, 1:-1]))
            rec[b, 6] = m
            if lin["n_bad"][b] > 0:
                state_new[b] = 2
            elif m < tol:
                state_new[b] = 1
            else:
                kappa = 1.0 if m <= max_step else max_step / m
                rec[b, 7] = kappa
                new[b, 1:-1] = (var[b, 1:-1].astype(np.float64) + kappa * delta).astype(np.float32)
        rec[b, 9] = state_new[b]
    return rec, scale, lin["grad"], new, state_new, lin["grad_scale"]


def sphere_field(centre, radius):
    """a smooth field (away from the centre): the distance to a sphere, float64 value and exact gradient"""
    centre = np.asarray(centre, np.float64)

    def field(p):
        p = np.asarray(p, np.float64)
        r = np.linalg.norm(p - centre, axis=-1)
        return r - radius, (p - centre) / r[:, None]
    return field


def free_field(pts):
    """free space: 10 m from anything, a unit gradient"""
    n = len(pts)
    g = np.zeros((n, 3), np.float32)
    g[:, 2] = 1.0
    return np.full(n, 10.0, np.float32), g


def host_field(fn):
    """a numpy field (pts -> (sdf, grad)) as the tensor callable isdf_amd.planning takes; the values are rounded to float32"""
    def field(pts):
        s, g = fn(pts.numpy())
        return torch.from_numpy(np.asarray(s, np.float32)), torch.from_numpy(np.asarray(g, np.float32))
    return field


class StubEngine:
    """the two tensor-level calls of isdf_amd.engine.Engine, `<prefix>_points(var, *body)` and `<prefix>_step(var, state, *body, sdf,
    grad, ..)`, on the host (CPU tensors, var and state in place): points(var, body[0]) and step, by default this model's step64"""

    def __init__(self, prefix="traj", points=points32, step=None):
        self.device, self.calls = torch.device("cpu"), []
        self._points, self._step64 = points, step or step64
        setattr(self, prefix + "_points", self._points_call)
        setattr(self, prefix + "_step", self._step_call)

    def _points_call(self, var, *body):
        self.calls.append(("points", int(var.shape[0])))
        return torch.from_numpy(self._points(var.numpy(), body[0]))

    def _step_call(self, var, state, b0, b1, sdf, grad, out=None, q_out=None, want_grad=False, **params):
        rec, _, g, new, state_new, _ = self._step64(var.numpy(), state.numpy(), b0, b1, sdf.numpy(), grad.numpy(), **params)
        self.calls.append(("step", int(var.shape[0])))
        var.copy_(torch.from_numpy(new))
        state.copy_(torch.from_numpy(state_new))
        if q_out is not None:
            q_out.copy_(torch.from_numpy(self._points(new, b0)).view_as(q_out))
        rec = torch.from_numpy(rec) if out is None else out.copy_(torch.from_numpy(rec))
        return (rec, torch.from_numpy(g)) if want_grad else rec
