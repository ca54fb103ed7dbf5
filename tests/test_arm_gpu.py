"""Joint-space planning on the device: isdf_arm_points / isdf_arm_step through Engine.arm_points, Engine.arm_step and
isdf_amd.kinematics.  Reference: tests/arm_model.py, written operation by operation in the header's order and summed in the
kernel's order; the model's step is fed the DEVICE's query points, so that the only difference left between the two is the last
bit of sin and cos in a_j and p_j.  Bounds (derived, not measured; u = 2^-53):
  query points               one float32 ulp of the model's: device and host sin / cos may differ by an ulp of double, 8 orders
                             below half a float32 ulp, so only a rounding tie can flip
  [2] [3] [4] [8] [9] [11]   exact
  sums [0] [1] [5] [10]      2 (N - 1) u sum|term| as in test_traj_gpu.py (N = T-2, T, T-2, T-1), plus 1e-12 sum|term| for the
                             trigonometric ulps in a_j and p_j
  [6]                        1e-9 relative (the solve's cond(A) u = 5.6e4 x 1.1e-16 at T = 384, with a wide factor)
  [7]                        1, or max_step / [6] of the device's own [6], exactly (IEEE division)
  grad_out                   1e-12 sum|term| per component
  new theta                  one float32 ulp of the model's"""
import numpy as np
import pytest
import torch

from isdf_amd import _ffi, kinematics as kin
from tests import arm_model as am
from tests import pose_model as pm
from tests import traj_model as tm

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SHAPES = [(1, 3, 1, 1), (3, 65, 4, 16), (40, 16, 6, 5), (2, 257, 8, 64), (1, _ffi.ARM_MAX_WAYPOINTS, 8, 64)]
PARAMS = dict(am.DEFAULTS)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def eng():
    from isdf_amd.engine import Engine, NetConfig
    return Engine(NetConfig(hidden=64, blocks=1), "cuda")


def _rotation(rng, angle):
    w = rng.standard_normal(3)
    return pm.so3_exp(angle * w / np.linalg.norm(w))


def _chain(J, S, seed, lo=None, hi=None):
    """a random chain: kinds alternate from revolute, bases and joint transforms are rotated and offset, sphere 0 sits on link 0
    (S > 1), the others on links 1 .. J with one on the last"""
    rng = np.random.RandomState(1000 + seed)
    base = np.hstack([_rotation(rng, 1.0), rng.uniform(-0.5, 0.5, (3, 1))])
    X = np.stack([np.hstack([_rotation(rng, 0.7), rng.uniform(-0.3, 0.3, (3, 1))]) for _ in range(J)])
    axes = rng.standard_normal((J, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    links = rng.randint(1, J + 1, S)
    links[-1] = J
    if S > 1:
        links[0] = 0
    return kin.Chain(base, X, np.arange(J) % 2, axes, links, rng.uniform(-0.2, 0.2, (S, 3)), rng.uniform(0.0, 0.1, S), lo, hi)


def _inputs(B, T, J, S, seed):
    """theta: a noisy line in joint space per trajectory; hand-made sdf over all three branches of the cost (eps = 0.2) and random
    gradients"""
    rng = np.random.RandomState(seed)
    s = np.linspace(0.0, 1.0, T)[None, :, None]
    a, b = rng.uniform(-1.2, 1.2, (B, 1, J)), rng.uniform(-1.2, 1.2, (B, 1, J))
    theta = (a + s * (b - a) + 0.02 * rng.standard_normal((B, T, J))).astype(np.float32)
    sdf = rng.uniform(-0.1, 0.5, B * T * S).astype(np.float32)
    grad = rng.standard_normal((B * T * S, 3)).astype(np.float32)
    return dict(chain=_chain(J, S, seed), theta=theta, sdf=sdf, grad=grad, state=np.zeros(B, np.int32))


def _run(eng, c, state=None, chain=None, in_place=False, **kw):
    """one device step on copies: dict(rec, grad, theta, state, q_in, q)"""
    p = dict(PARAMS, **kw)
    chain = c["chain"] if chain is None else chain
    th, st = _cuda(c["theta"]), _cuda(c["state"] if state is None else np.asarray(state, np.int32))
    q = eng.arm_points(th, chain)
    q_in = q.cpu().numpy()
    q_out = q if in_place else torch.empty_like(q)
    rec, g = eng.arm_step(th, st, chain, q, _cuda(c["sdf"]), _cuda(c["grad"]), q_out=q_out, want_grad=True, **p)
    return dict(rec=rec.cpu().numpy(), grad=g.cpu().numpy(), theta=th.cpu().numpy(), state=st.cpu().numpy(), q_in=q_in, q=q_out.cpu().numpy(),
                theta_dev=th)


def _model(c, dev, state=None, chain=None, **kw):
    return am.step64(c["chain"] if chain is None else chain, c["theta"], c["state"] if state is None else state, dev["q_in"], c["sdf"],
                     c["grad"], **dict(PARAMS, **kw))


@pytest.fixture(scope="module")
def cases(eng):
    """shape -> inputs, the device's step (run once) and the model's on the device's query points, shared by the tests below"""
    out = {}
    for k, (B, T, J, S) in enumerate(SHAPES):
        c = _inputs(B, T, J, S, seed=k)
        c["dev"] = _run(eng, c)
        c["model"] = _model(c, c["dev"])
        out[(B, T, J, S)] = c
    return out


def _ulp32(a, b):
    return np.maximum(np.spacing(np.abs(a).astype(np.float32)), np.spacing(np.abs(b).astype(np.float32))).astype(np.float64)


@pytest.mark.parametrize("shape", SHAPES)
def test_query_points_are_within_one_ulp_of_the_model_and_the_step_s_are_arm_points_of_the_theta_it_leaves(eng, cases, shape):
    c = cases[shape]
    B, T, J, S = shape
    q = c["dev"]["q_in"]
    model = am.points32(c["chain"], c["theta"])
    assert q.shape == model.shape == (B * T * S, 3) and q.dtype == np.float32
    off_by = np.abs(q.astype(np.float64) - model.astype(np.float64))
    print("%s: %d of %d query coordinates differ from the model's (a rounding tie flipped)" % (shape, (off_by > 0).sum(), off_by.size))
    assert (off_by <= _ulp32(q, model)).all()
    again = eng.arm_points(c["dev"]["theta_dev"], c["chain"]).cpu().numpy()
    assert c["dev"]["q"].tobytes() == again.tobytes()
    assert (c["dev"]["q"] != q).any()


def _assert_records(name, rec, model, scale, T):
    N = {0: T - 2, 1: T, 5: T - 2, 10: T - 1}                 # [1]: T-1 terms and the scaling product
    for k in (2, 3, 4, 8, 9, 11):
        assert np.array_equal(rec[:, k], model[:, k]), (name, k, rec[:, k], model[:, k])
    for k, n in N.items():
        err, bound = np.abs(rec[:, k] - model[:, k]), (2.0 * (n - 1) * U + 1e-12) * scale[:, k]
        print("%s [%d]: worst |record - model| = %.3g, bound %.3g (sum|term| %.3g)" % (name, k, err.max(), bound[err.argmax()], scale[:, k].max()))
        assert (err <= bound).all(), (name, k)
    assert (np.abs(rec[:, 6] - model[:, 6]) <= 1e-9 * model[:, 6]).all(), (name, rec[:, 6], model[:, 6])
    assert np.array_equal(rec[:, 12:], np.zeros((len(rec), 4)))


@pytest.mark.parametrize("shape", SHAPES)
def test_records_gradient_and_new_theta_against_the_float64_model(cases, shape):
    c = cases[shape]
    B, T, J, S = shape
    dev = c["dev"]
    rec, scale, grad, th_new, state_new, grad_scale = c["model"]
    assert dev["rec"].shape == (B, 16) and dev["rec"].dtype == np.float64 and dev["grad"].shape == (B, T, J)
    if T * S >= 9:
        assert rec[:, 3].sum() > 0 and (rec[:, 4] > rec[:, 3]).all() and (rec[:, 4] < T * S).all()       # all three branches of c
    if S > 1:
        assert c["chain"].links[0] == 0 and set(c["chain"].kinds.tolist()) == {0, 1}
    _assert_records(str(shape), dev["rec"], rec, scale, T)
    ms = float(np.float32(PARAMS["max_step"]))
    moving = dev["rec"][:, 9] == 0
    assert moving.all() and np.array_equal(dev["state"], state_new)
    assert np.array_equal(dev["rec"][:, 7], np.where(dev["rec"][:, 6] <= ms, 1.0, ms / dev["rec"][:, 6]))
    gerr = np.abs(dev["grad"] - grad)
    print("%s: worst |grad_out - model| / sum|term| = %.3g" % (shape, (gerr / np.where(grad_scale > 0, grad_scale, 1.0)).max()))
    assert (gerr <= 1e-12 * grad_scale).all() and np.abs(grad).max() > 0
    assert np.array_equal(dev["grad"][:, [0, -1]], np.zeros((B, 2, J)))
    off_by = np.abs(dev["theta"].astype(np.float64) - th_new.astype(np.float64))
    print("%s: %d of %d joint values differ from the model's new theta (by one ulp at most)" % (shape, (off_by > 0).sum(), off_by.size))
    assert (off_by <= _ulp32(dev["theta"], th_new)).all()
    assert dev["theta"][:, [0, -1]].tobytes() == c["theta"][:, [0, -1]].tobytes()
    assert (dev["theta"][:, 1:-1] != c["theta"][:, 1:-1]).any()


def test_a_prismatic_chain_is_traj_step(eng):
    """x, y, z prismatic joints in an identity frame and spheres on link 3 are planning's robot: theta = x, centres = offsets.
    Counts and the least clearance are exact.  Each q is within half a float32 ulp of x + o, so a body point's velocity is within
    dv = sqrt(3) / 2 ulp(max|q|) of the waypoint's; hence |sigma_{t,s} - sigma_t| <= dv and |h_{t,s} - vh_t| <= 2 dv / sigma_t, and
      |F_obs - F_obs'| <= dv sum c,
      |grad - grad'|   <= w_obs (dv sum_s |c' g| + dv (C_{t-1} / sigma_{t-1} + C_{t+1} / sigma_{t+1}))  per component,
    each plus 1e-12 of the sum of |term| for the different orders of summation."""
    B, T, S = 40, 16, 5
    rng = np.random.RandomState(77)
    c = _inputs(B, T, 3, S, seed=7)
    off = (0.2 * rng.uniform(-1, 1, (S, 3))).astype(np.float32)
    eye = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (3, 1, 1))
    c["chain"] = kin.Chain(eye[0], eye, [1, 1, 1], np.eye(3), [3] * S, off, c["chain"].radii)
    rad = c["chain"].radii
    p = dict(PARAMS, eta=8.0)
    arm = _run(eng, c, **p)
    x, st = _cuda(c["theta"]), _cuda(c["state"])
    rec, g = eng.traj_step(x, st, off, rad, _cuda(c["sdf"]), _cuda(c["grad"]), want_grad=True, **p)
    rec, g = rec.cpu().numpy(), g.cpu().numpy()
    for k in (2, 3, 4, 8, 9):
        assert np.array_equal(arm["rec"][:, k], rec[:, k]), k
    assert np.abs(arm["q_in"].astype(np.float64) - tm.points32(c["theta"], off).astype(np.float64)).max() <= 0.5 * np.spacing(np.abs(arm["q_in"]).max())
    dv = np.sqrt(3.0) / 2 * float(np.spacing(np.float32(np.abs(arm["q_in"]).max())))
    x64 = c["theta"].astype(np.float64)
    d = c["sdf"].astype(np.float64).reshape(B, T, S) - rad.astype(np.float64)
    cc, cp = tm.cost(d, float(np.float32(p["eps"])))
    cc[:, [0, -1]], cp[:, [0, -1]] = 0.0, 0.0
    sigma = np.ones((B, T))
    sigma[:, 1:-1] = tm.norm3((x64[:, 2:] - x64[:, :-2]) * 0.5)
    assert sigma.min() > 1e-3
    C = cc.sum(-1)
    f_bound = dv * C.sum(-1) + 1e-12 * rec[:, 0]
    f_err = np.abs(arm["rec"][:, 0] - rec[:, 0])
    print("pure translation: worst |F_obs - traj_step's| = %.3g, bound %.3g" % (f_err.max(), f_bound[f_err.argmax()]))
    assert (f_err <= f_bound).all() and (rec[:, 0] > 0).all()
    absG = (np.abs(cp)[..., None] * np.abs(c["grad"].astype(np.float64).reshape(B, T, S, 3))).sum(2)
    Cs = C / sigma
    nb = np.zeros((B, T))
    nb[:, 1:-1] = Cs[:, :-2] + Cs[:, 2:]
    w_obs, ws = float(np.float32(p["w_obs"])), float(np.float32(p["w_smooth"])) * (T - 1)
    scale = w_obs * (sigma[..., None] * absG + nb[..., None]) + ws * 4.0 * np.abs(x64).max()
    g_bound = w_obs * dv * (absG + nb[..., None]) + 1e-12 * scale
    g_err = np.abs(arm["grad"] - g)
    print("pure translation: worst |grad - traj_step's| = %.3g, bound there %.3g" % (g_err.max(), g_bound.reshape(-1)[g_err.argmax()]))
    assert (g_err[:, 1:-1] <= g_bound[:, 1:-1]).all() and np.abs(g).max() > 1.0
    # the same functional, the same smoothness term: F_smooth and the path length have the same terms
    assert (np.abs(arm["rec"][:, [1, 10]] - rec[:, [1, 10]]) <= 2.0 * T * U * rec[:, [1, 10]]).all()


def test_limits_cut_the_step_and_infinite_limits_are_no_limits(eng):
    """eta = 4 and no step cap make the unprojected step long enough to leave the range theta covers; limits half way between that
    range and where the free step ends cut part of it.  theta starts inside the limits, so it must end inside them."""
    c = _inputs(3, 65, 4, 16, seed=41)
    rng = np.random.RandomState(41)                                 # every trajectory hovers about one configuration
    c["theta"] = (rng.uniform(-1.2, 1.2, (1, 1, 4)) + 0.02 * rng.standard_normal((3, 65, 4))).astype(np.float32)
    p = dict(max_step=float("inf"), eta=4.0)
    free = _run(eng, c, **p)
    print("limits: the free step's length %s" % free["rec"][:, 6])
    t_lo, t_hi, f_lo, f_hi = c["theta"].min((0, 1)), c["theta"].max((0, 1)), free["theta"].min((0, 1)), free["theta"].max((0, 1))
    assert (f_lo < t_lo).any() and (f_hi > t_hi).any()              # the free step leaves the range theta covers
    lo = np.where(f_lo < t_lo, 0.5 * (f_lo + t_lo), t_lo).astype(np.float32)     # half way to where it would go
    hi = np.where(f_hi > t_hi, 0.5 * (f_hi + t_hi), t_hi).astype(np.float32)
    assert (lo <= t_lo).all() and (hi >= t_hi).all()
    ch = c["chain"]
    lim = kin.Chain(ch.base, ch.X, ch.kinds, ch.axes, ch.links, ch.centres, ch.radii, lo, hi)
    dev = _run(eng, c, chain=lim, **p)
    rec, scale, grad, th_new, state_new, _ = _model(c, dev, chain=lim, **p)
    print("limits: cut entries per trajectory %s of %d" % (rec[:, 11], 63 * 4))
    assert np.array_equal(free["rec"][:, 11], np.zeros(3)) and rec[:, 11].sum() > 0 and (rec[:, 11] < 63 * 4).all()
    _assert_records("limits", dev["rec"], rec, scale, 65)
    assert (dev["theta"] >= lo).all() and (dev["theta"] <= hi).all()
    assert not ((free["theta"] >= lo).all() and (free["theta"] <= hi).all())
    assert np.array_equal(dev["rec"][:, 7], np.ones(3)) and (dev["rec"][:, 6] <= free["rec"][:, 6]).all()
    # m is the projected maximum: the longest move of a joint value, to the rounding of the new theta
    moved = np.abs(dev["theta"].astype(np.float64) - c["theta"]).max((1, 2))
    assert (np.abs(moved - dev["rec"][:, 6]) <= np.spacing(np.float32(np.abs(dev["theta"]).max()))).all()
    assert (np.abs(dev["theta"].astype(np.float64) - th_new) <= _ulp32(dev["theta"], th_new)).all()
    # every limit infinite: byte for byte the call without limits
    inf = kin.Chain(ch.base, ch.X, ch.kinds, ch.axes, ch.links, ch.centres, ch.radii, np.full(4, -np.inf), np.full(4, np.inf))
    same, none = _run(eng, c, chain=inf), _run(eng, c)
    for k in ("rec", "grad", "theta", "q"):
        assert same[k].tobytes() == none[k].tobytes(), k


def test_states_frozen_invalid_and_converged(eng):
    B, T, J, S = 5, 16, 6, 5
    c = _inputs(B, T, J, S, seed=31)
    n = T * S
    c["sdf"][3 * n + 7] = np.nan                  # trajectory 3: three non-finite values in two samples
    c["grad"][3 * n + 7, 1] = np.inf
    c["grad"][3 * n + 20, 2] = -np.inf
    c["sdf"][4 * n + S + 3] = np.inf              # trajectory 4: one at waypoint 1 ...
    c["sdf"][4 * n + 1] = -np.inf                 # ... and one at the FIXED waypoint 0 (sample index = t * S + s)
    dev = _run(eng, c, state=[0, 1, 2, 0, 0])
    rec = dev["rec"]
    assert dev["state"].tolist() == [0, 1, 2, 2, 2] and rec[:, 9].tolist() == [0, 1, 2, 2, 2]
    assert rec[:, 8].tolist() == [0, 0, 0, 3, 2]
    assert dev["theta"][1:].tobytes() == c["theta"][1:].tobytes() and (dev["theta"][0] != c["theta"][0]).any()
    assert np.array_equal(rec[1:3, 6:8], np.zeros((2, 2))) and rec[0, 7] > 0 and np.array_equal(rec[3:, 7], np.zeros(2))
    model = _model(c, dev, state=[0, 1, 2, 0, 0])
    _assert_records("states", rec, model[0], model[1], T)
    assert np.isfinite(rec).all() and np.isfinite(dev["grad"]).all()
    # the frozen trajectories' records still describe them
    assert (rec[1:3, 0] > 0).all() and (rec[1:3, 5] > 0).all() and (rec[1:3, 10] > 0).all()
    again = eng.arm_points(dev["theta_dev"], c["chain"]).cpu().numpy()
    assert dev["q"].tobytes() == again.tobytes()                                  # moving and frozen alike
    assert dev["q"].reshape(B, -1)[1:].tobytes() == dev["q_in"].reshape(B, -1)[1:].tobytes()
    # a step below tol: converged, theta untouched, the record keeps the step length
    c2 = _inputs(2, 16, 6, 5, seed=32)
    dev2 = _run(eng, c2, tol=100.0)
    assert dev2["state"].tolist() == [1, 1] and dev2["theta"].tobytes() == c2["theta"].tobytes()
    assert (dev2["rec"][:, 6] > 0).all() and (dev2["rec"][:, 6] < 100).all() and np.array_equal(dev2["rec"][:, 7], np.zeros(2))


def test_two_runs_are_bit_identical_in_place_or_not_and_a_trajectory_alone_equals_itself_in_a_batch(eng, cases):
    c = cases[(3, 65, 4, 16)]
    a = c["dev"]
    for b in (_run(eng, c), _run(eng, c, in_place=True)):           # q_out a buffer of its own, then q itself
        for k in ("rec", "grad", "theta", "q"):
            assert a[k].tobytes() == b[k].tobytes(), k
    n = 65 * 16
    for k in range(3):
        one = dict(c, theta=c["theta"][k:k + 1], sdf=c["sdf"][k * n:(k + 1) * n], grad=c["grad"][k * n:(k + 1) * n], state=c["state"][k:k + 1])
        alone = _run(eng, one)
        for name in ("rec", "grad", "theta"):
            assert alone[name].tobytes() == a[name][k:k + 1].tobytes(), (k, name)


@pytest.mark.parametrize("name", sorted(am.SCENARIOS))
def test_plans_through_the_exact_room_leave_the_obstacles_and_converge(eng, name):
    """defaults (eta = 32), T = 32, the straight line in joint space as the start, at most 400 iterations; beside it the model's
    loop on the host (float32 theta between iterations).  A float64 host prototype converged after 133 (arm A), 107 (arm A high)
    and 239 (free body) iterations at clearances of 0.173, 0.180 and 0.074 m."""
    make, start, goal = am.SCENARIOS[name]
    chain = make()
    th0 = am.line(start, goal, 32)
    first = kin.joint_step(eng, chain, th0, field=pm.room_field_torch)
    assert first.in_collision[0] > 0                                  # the straight line crosses an obstacle
    res = kin.optimise_joint_trajectories(eng, chain, th0, iters=400, field=pm.room_field_torch)
    r = res.records
    _, mrec, miters = am.loop64(chain, th0, pm.room_field, iters=400)
    print("%s: %d samples in collision at first; device %s after %d iterations, clearance %.4f m, F_obs %.5f, F_smooth %.5f | model "
          "state %d after %d iterations, clearance %.4f m" % (name, first.in_collision[0], res.reason[0], res.iterations, r.min_clearance[0],
                                                               r.cost_obs[0], r.cost_smooth[0], mrec[0, 9], miters, mrec[0, 2]))
    assert res.reason == ["converged"] and r.in_collision[0] == 0 and r.min_clearance[0] > 0
    th = res.x.cpu().numpy()
    assert th[0, 0].tobytes() == th0[0, 0].tobytes() and th[0, -1].tobytes() == th0[0, -1].tobytes()


def test_the_loop_through_the_real_field_returns_records_of_the_theta_it_returns(eng):
    """plumbing only (the net is randomly initialised): the default field is the engine's own sdf_eval"""
    chain = am.arm_a()
    th0 = kin.seed_joint_trajectories((-0.2, 1.1, 0.5, 0.2), (-2.9, 1.1, 0.5, 0.2), 16, 3, seed=1)
    moved = kin.optimise_joint_trajectories(eng, chain, th0, iters=3, check_every=2)
    th = moved.x.cpu().numpy()
    assert moved.iterations <= 3 and np.isfinite(th).all() and np.isfinite(moved.records.records).all()
    assert th[:, [0, -1]].tobytes() == th0[:, [0, -1]].tobytes()
    # tol above every possible step: the loop stops at its first linearisation, whose record is that of the theta it returns
    res = kin.optimise_joint_trajectories(eng, chain, moved.x, tol=100.0, check_every=1)
    assert res.reason == ["converged"] * 3 and res.iterations == 1 and torch.equal(res.x, moved.x)
    fresh = kin.joint_step(eng, chain, res.x, tol=100.0)
    assert fresh.records.tobytes() == res.records.records.tobytes()
    _, best = kin.plan_joint_path(eng, chain, (-0.2, 1.1, 0.5, 0.2), (-2.9, 1.1, 0.5, 0.2), T=16, n_seeds=4, iters=2)
    assert best is None or 0 <= best < 4
