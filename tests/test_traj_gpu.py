"""Planning on the device: isdf_traj_points / isdf_traj_step through Engine.traj_points, Engine.traj_step and isdf_amd.planning.
Reference: tests/traj_model.py, written operation by operation in the header's order, so that every term of a sum has the
device's bits and only the order of summation differs.  Bounds (derived, not measured; u = 2^-53):
  query points               bit-equal to the float32 model
  [2] [3] [4] [8] [9]        exact
  sums [0] [5] [10]          2 (N - 1) u sum|term|, N the number of terms (T-2, T-2, T-1): twice the worst-case reordering bound
  [1]                        2 N u sum|term|, N = T-1: the sum is scaled by (T-1)/2 afterwards, one more rounding on either side
  [6]                        1e-9 relative: the solve's cond(A) u = 4e5 x 1.1e-16 = 5e-11 at T = 1024, with a factor 20
  [7]                        1, or max_step / [6] of the device's own [6], exactly (IEEE division)
  grad_out                   1e-12 sum|term| per component (at most S + 5 terms of about ten roundings)
  new x                      one float32 ulp of the model's"""
import numpy as np
import pytest
import torch

from isdf_amd import planning
from tests import pose_model as pm
from tests import traj_model as tm

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SHAPES = [(1, 3, 1), (3, 65, 3), (2, 257, 32), (40, 16, 2), (1, 1024, 32)]
POINT_SHAPES = SHAPES[:4]
PARAMS = dict(tm.DEFAULTS)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def eng():
    from isdf_amd.engine import Engine, NetConfig
    return Engine(NetConfig(hidden=64, blocks=1), "cuda")


def _inputs(B, T, S, seed, box=1.0):
    """x: a noisy line per trajectory; hand-made sdf over all three branches of the cost (eps = 0.2) and random gradients"""
    rng = np.random.RandomState(seed)
    s = np.linspace(0.0, 1.0, T)[None, :, None]
    a, b = rng.uniform(-box, box, (B, 1, 3)), rng.uniform(-box, box, (B, 1, 3))
    x = (a + s * (b - a) + 0.02 * box * rng.standard_normal((B, T, 3))).astype(np.float32)
    off = (0.2 * box * rng.uniform(-1, 1, (S, 3))).astype(np.float32)
    off[0] = 0.0
    rad = rng.uniform(0.0, 0.1, S).astype(np.float32)
    sdf = rng.uniform(-0.1, 0.5, B * T * S).astype(np.float32)
    grad = rng.standard_normal((B * T * S, 3)).astype(np.float32)
    return dict(x=x, off=off, rad=rad, sdf=sdf, grad=grad, state=np.zeros(B, np.int32))


def _run(eng, c, state=None, **kw):
    """one device step on copies: dict(rec, grad, x, state, q)"""
    p = dict(PARAMS, **kw)
    x, st = _cuda(c["x"]), _cuda(c["state"] if state is None else np.asarray(state, np.int32))
    q = torch.empty(c["sdf"].size, 3, dtype=torch.float32, device="cuda")
    rec, g = eng.traj_step(x, st, c["off"], c["rad"], _cuda(c["sdf"]), _cuda(c["grad"]), q_out=q, want_grad=True, **p)
    return dict(rec=rec.cpu().numpy(), grad=g.cpu().numpy(), x=x.cpu().numpy(), state=st.cpu().numpy(), q=q.cpu().numpy())


@pytest.fixture(scope="module")
def cases(eng):
    """shape -> inputs, the device's step (run once) and the model's, shared by the tests below"""
    out = {}
    for k, (B, T, S) in enumerate(SHAPES):
        c = _inputs(B, T, S, seed=k)
        c["dev"] = _run(eng, c)
        c["model"] = tm.step64(c["x"], c["state"], c["off"], c["rad"], c["sdf"], c["grad"], **PARAMS)
        out[(B, T, S)] = c
    return out


@pytest.mark.parametrize("shape", POINT_SHAPES)
def test_query_points_equal_the_float32_model_bit_for_bit(eng, cases, shape):
    c = cases[shape]
    q = eng.traj_points(_cuda(c["x"]), c["off"], c["rad"]).cpu().numpy()
    model = tm.points32(c["x"], c["off"])
    assert q.shape == model.shape == (np.prod(shape), 3) and q.dtype == np.float32
    assert q.tobytes() == model.tobytes()


def _assert_records(name, rec, model, scale, T):
    N = {0: T - 2, 1: T, 5: T - 2, 10: T - 1}                 # [1]: T-1 terms and the scaling product
    for k in (2, 3, 4, 8, 9):
        assert np.array_equal(rec[:, k], model[:, k]), (name, k, rec[:, k], model[:, k])
    for k, n in N.items():
        err, bound = np.abs(rec[:, k] - model[:, k]), 2.0 * (n - 1) * U * scale[:, k]
        print("%s [%d]: worst |record - model| = %.3g, bound %.3g (sum|term| %.3g)" % (name, k, err.max(), bound[err.argmax()], scale[:, k].max()))
        assert (err <= bound).all(), (name, k)
    assert (np.abs(rec[:, 6] - model[:, 6]) <= 1e-9 * model[:, 6]).all(), (name, rec[:, 6], model[:, 6])
    assert np.array_equal(rec[:, 11:], np.zeros((len(rec), 5)))


@pytest.mark.parametrize("shape", SHAPES)
def test_records_gradient_and_new_x_against_the_float64_model(cases, shape):
    c = cases[shape]
    B, T, S = shape
    dev = c["dev"]
    rec, scale, grad, x_new, state_new, grad_scale = c["model"]
    assert dev["rec"].shape == (B, 16) and dev["rec"].dtype == np.float64 and dev["grad"].shape == (B, T, 3)
    if T * S >= 9:
        assert rec[:, 3].sum() > 0 and (rec[:, 4] > rec[:, 3]).all() and (rec[:, 4] < T * S).all()       # all three branches of c
    _assert_records(str(shape), dev["rec"], rec, scale, T)
    # the clamp factor, from the device's own step length
    ms = float(np.float32(PARAMS["max_step"]))
    moving = dev["rec"][:, 9] == 0
    assert moving.all() and np.array_equal(dev["state"], state_new)
    assert np.array_equal(dev["rec"][:, 7], np.where(dev["rec"][:, 6] <= ms, 1.0, ms / dev["rec"][:, 6]))
    gerr = np.abs(dev["grad"] - grad)
    print("%s: worst |grad_out - model| / sum|term| = %.3g" % (shape, (gerr / np.where(grad_scale > 0, grad_scale, 1.0)).max()))
    assert (gerr <= 1e-12 * grad_scale).all()
    assert np.array_equal(dev["grad"][:, [0, -1]], np.zeros((B, 2, 3)))
    ulp = np.maximum(np.spacing(np.abs(x_new)), np.spacing(np.abs(dev["x"])))
    off_by = np.abs(dev["x"].astype(np.float64) - x_new.astype(np.float64))
    print("%s: %d of %d coordinates differ from the model's new x (by one ulp at most)" % (shape, (off_by > 0).sum(), off_by.size))
    assert (off_by <= ulp).all()
    assert dev["x"][:, [0, -1]].tobytes() == c["x"][:, [0, -1]].tobytes()
    assert (dev["x"][:, 1:-1] != c["x"][:, 1:-1]).any()
    assert dev["q"].tobytes() == tm.points32(dev["x"], c["off"]).tobytes()


def test_the_clamp_binds_at_max_step_and_is_off_at_infinity(eng):
    """the trajectories lie inside |x| < 2^-4, where a float32 ulp is below 4e-9: the rounding of the new x (half an ulp per
    coordinate) stays inside the 1e-6 x max_step = 1e-8 the displacement bound allows; eta = 0.8 makes every trajectory's
    step longer than max_step in so small a box"""
    c = _inputs(3, 65, 3, seed=11, box=0.04)
    assert np.abs(c["x"]).max() < 2.0 ** -4
    ms = float(np.float32(0.01))
    dev = _run(eng, c, max_step=0.01, eta=0.8)
    rec = dev["rec"]
    assert (rec[:, 6] > ms).all() and np.array_equal(rec[:, 7], ms / rec[:, 6]) and (rec[:, 7] < 1).all()
    moved = np.linalg.norm(dev["x"].astype(np.float64) - c["x"].astype(np.float64), axis=-1).max(-1)
    print("clamped: step %s, factor %s, longest displacement / max_step - 1 = %s" % (rec[:, 6], rec[:, 7], moved / ms - 1))
    assert (moved <= ms * (1 + 1e-6)).all() and (moved >= ms * (1 - 1e-6)).all()
    free = _run(eng, c, max_step=float("inf"), eta=0.8)
    assert np.array_equal(free["rec"][:, 7], np.ones(3)) and np.array_equal(free["rec"][:, 6], rec[:, 6])
    model = tm.step64(c["x"], c["state"], c["off"], c["rad"], c["sdf"], c["grad"], **dict(PARAMS, max_step=float("inf"), eta=0.8))
    assert (np.abs(free["x"].astype(np.float64) - model[3].astype(np.float64)) <= np.spacing(np.abs(model[3]))).all()


def test_cost_borders(eng):
    """T = 3, S = 1, radius 0 (so d = sdf), one trajectory per d in {-ulp, 0, +ulp, eps - ulp, eps, eps + ulp} with float32
    ulps: every record is a single term"""
    f = np.float32
    eps = f(PARAMS["eps"])
    d = np.array([np.nextafter(f(0), f(-1)), f(0), np.nextafter(f(0), f(1)), np.nextafter(eps, f(0)), eps, np.nextafter(eps, f(1))], f)
    c = _inputs(6, 3, 1, seed=21)
    c["rad"][:] = 0.0
    sdf = np.full((6, 3), 10.0, f)               # the fixed waypoints far from everything: they count nowhere
    sdf[:, 1] = d
    c["sdf"] = sdf.reshape(-1)
    dev = _run(eng, c)["rec"]
    rec, scale = tm.step64(c["x"], c["state"], c["off"], c["rad"], c["sdf"], c["grad"], **PARAMS)[:2]
    print("borders: F_obs %s\n  model %s" % (dev[:, 0], rec[:, 0]))
    assert np.array_equal(dev[:, 3], [1, 0, 0, 0, 0, 0])                 # d < 0
    assert np.array_equal(dev[:, 4], [1, 1, 1, 1, 0, 0])                 # d < eps
    assert np.array_equal(dev[:, 2], d.astype(np.float64))
    assert (rec[:4, 0] > 0).all() and (np.abs(dev[:, 0] - rec[:, 0]) <= 1e-14 * rec[:, 0]).all()
    assert dev[4, 0] == 0 and dev[5, 0] == 0                              # c is exactly 0 at eps and one ulp above it
    assert (np.abs(dev[:, 5] - rec[:, 5]) <= 1e-14 * rec[:, 5]).all()


def test_states_frozen_invalid_and_converged(eng):
    c = _inputs(5, 16, 2, seed=31)
    n = 16 * 2
    c["sdf"][3 * n + 7] = np.nan                  # trajectory 3: three non-finite values in two samples
    c["grad"][3 * n + 7, 1] = np.inf
    c["grad"][3 * n + 20, 2] = -np.inf
    c["sdf"][4 * n + 3] = np.inf                  # trajectory 4: one at waypoint 1 ...
    c["sdf"][4 * n + 1] = -np.inf                 # ... and one at the FIXED waypoint 0 (sample index = t * S + s)
    dev = _run(eng, c, state=[0, 1, 2, 0, 0])
    rec = dev["rec"]
    assert dev["state"].tolist() == [0, 1, 2, 2, 2] and rec[:, 9].tolist() == [0, 1, 2, 2, 2]
    assert rec[:, 8].tolist() == [0, 0, 0, 3, 2]
    assert dev["x"][1:].tobytes() == c["x"][1:].tobytes() and (dev["x"][0] != c["x"][0]).any()
    assert np.array_equal(rec[1:3, 6:8], np.zeros((2, 2))) and rec[0, 7] > 0 and np.array_equal(rec[3:, 7], np.zeros(2))
    model = tm.step64(c["x"], [0, 1, 2, 0, 0], c["off"], c["rad"], c["sdf"], c["grad"], **PARAMS)
    _assert_records("states", rec, model[0], model[1], 16)
    assert np.isfinite(rec).all()
    # the frozen trajectories' records still describe them
    assert (rec[1:3, 0] > 0).all() and (rec[1:3, 5] > 0).all() and (rec[1:3, 10] > 0).all()
    assert dev["q"].tobytes() == tm.points32(dev["x"], c["off"]).tobytes()      # moving and frozen alike
    # a step below tol: converged, x untouched, the record keeps the step length
    c2 = _inputs(2, 16, 2, seed=32)
    dev2 = _run(eng, c2, tol=100.0)
    assert dev2["state"].tolist() == [1, 1] and dev2["x"].tobytes() == c2["x"].tobytes()
    assert (dev2["rec"][:, 6] > 0).all() and (dev2["rec"][:, 6] < 100).all() and np.array_equal(dev2["rec"][:, 7], np.zeros(2))


def test_two_runs_are_bit_identical_and_a_trajectory_alone_equals_itself_in_a_batch(eng, cases):
    c = cases[(3, 65, 3)]
    a, b = c["dev"], _run(eng, c)
    for k in ("rec", "grad", "x", "q"):
        assert a[k].tobytes() == b[k].tobytes(), k
    n = 65 * 3
    for k in range(3):
        one = dict(c, x=c["x"][k:k + 1], sdf=c["sdf"][k * n:(k + 1) * n], grad=c["grad"][k * n:(k + 1) * n], state=c["state"][k:k + 1])
        alone = _run(eng, one)
        for name in ("rec", "grad", "x"):
            assert alone[name].tobytes() == a[name][k:k + 1].tobytes(), (k, name)


E2E = [((0.4, 2.2, 1.5), (2.8, 2.2, 1.7), 32), ((0.3, 2.7, 3.0), (2.4, 2.0, 4.7), 48), ((3.2, 2.3, 2.6), (5.4, 2.6, 4.4), 48)]


@pytest.mark.parametrize("start,goal,T", E2E)
def test_paths_through_the_exact_room_leave_the_obstacles_and_converge(eng, start, goal, T):
    """defaults, one sphere of radius 0.1 m, the straight line as the start; a float64 host prototype of the loop ended at
    clearances of 0.131, 0.055 and 0.116 m after 60 to 70 iterations"""
    x0 = planning.seed_trajectories(start, goal, T, 1)
    first = planning.trajectory_step(eng, x0, radii=0.1, field=pm.room_field_torch)
    assert first.in_collision[0] > 0                                  # the straight line crosses an obstacle
    res = planning.optimise_trajectories(eng, x0, radii=0.1, field=pm.room_field_torch)
    r = res.records
    print("T = %d: %s after %d iterations, clearance %.4f m, F_obs %.5f, F_smooth %.5f, length %.4f m"
          % (T, res.reason[0], res.iterations, r.min_clearance[0], r.cost_obs[0], r.cost_smooth[0], r.length[0]))
    assert r.in_collision[0] == 0 and r.min_clearance[0] > 0
    assert res.reason == ["converged"] and res.iterations <= 150
    x = res.x.cpu().numpy()
    assert x[0, 0].tobytes() == x0[0, 0].tobytes() and x[0, -1].tobytes() == x0[0, -1].tobytes()


def test_the_loop_through_the_real_field_returns_records_of_the_x_it_returns(eng):
    """plumbing only (the net is randomly initialised): the default field is the engine's own sdf_eval"""
    x0 = planning.seed_trajectories((0.4, 2.2, 1.5), (2.8, 2.2, 1.7), 16, 3, seed=1)
    off = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0]], np.float32)
    moved = planning.optimise_trajectories(eng, x0, offsets=off, radii=0.05, iters=3, check_every=2)
    x = moved.x.cpu().numpy()
    assert moved.iterations <= 3 and np.isfinite(x).all() and np.isfinite(moved.records.records).all()
    assert x[:, [0, -1]].tobytes() == x0[:, [0, -1]].tobytes()
    # tol above every possible step: the loop stops at its first linearisation, whose record is that of the x it returns
    res = planning.optimise_trajectories(eng, moved.x, offsets=off, radii=0.05, tol=100.0, check_every=1)
    assert res.reason == ["converged"] * 3 and res.iterations == 1 and torch.equal(res.x, moved.x)
    fresh = planning.trajectory_step(eng, res.x, offsets=off, radii=0.05, tol=100.0)
    assert fresh.records.tobytes() == res.records.records.tobytes()
    _, best = planning.plan_path(eng, (0.4, 2.2, 1.5), (2.8, 2.2, 1.7), T=16, n_seeds=4, iters=2)
    assert best is None or 0 <= best < 4
