"""The host half of planning without a device: tests/traj_model.py (gradient, solves, state machine) and isdf_amd.planning's loop
driven through a stub engine whose two calls are that model."""
import numpy as np
import pytest
import torch

from isdf_amd import planning
from tests import traj_model as tm

OFFSETS3 = np.array([[0.0, 0.0, 0.0], [0.15, 0.0, 0.05], [-0.1, 0.12, 0.0]])
RADII3 = np.array([0.1, 0.05, 0.08])


def _bent_path(T, seed=0):
    """a path past the sphere of `tm.sphere_field((0, 0, 0), 0.5)`: clearances on all three branches of the cost"""
    rng = np.random.RandomState(seed)
    s = np.linspace(0.0, 1.0, T)
    x = np.stack([-1.0 + 2.0 * s, 0.35 + 0.5 * s, 0.1 * s], -1)
    return (x + 0.02 * rng.standard_normal(x.shape))[None]


def test_gradient_is_the_central_difference_of_the_discrete_cost():
    """T = 9, S = 3 with offsets, float64 throughout, h = 1e-6, every interior coordinate to 1e-6"""
    field = tm.sphere_field((0.0, 0.0, 0.0), 0.5)
    x = _bent_path(9)
    eps, w_obs, w_smooth = 0.2, 8.0, 1.0
    f0, lin = tm.objective(x, field, OFFSETS3, RADII3, eps, w_obs, w_smooth)
    assert lin["n_neg"][0] > 0 and lin["n_act"][0] > lin["n_neg"][0] and lin["n_act"][0] < 27       # all three branches
    h, worst = 1e-6, 0.0
    for t in range(1, 8):
        for k in range(3):
            xp, xm = x.copy(), x.copy()
            xp[0, t, k] += h
            xm[0, t, k] -= h
            fd = (tm.objective(xp, field, OFFSETS3, RADII3, eps, w_obs, w_smooth)[0][0]
                  - tm.objective(xm, field, OFFSETS3, RADII3, eps, w_obs, w_smooth)[0][0]) / (2 * h)
            worst = max(worst, abs(fd - lin["grad"][0, t, k]))
    print("worst |central difference - gradient| = %.3g" % worst)
    assert worst < 1e-6
    assert np.array_equal(lin["grad"][0, [0, -1]], np.zeros((2, 3)))


@pytest.mark.parametrize("T", [3, 4, 65, 1024])
def test_both_solves_agree_with_numpy_on_K(T):
    n = T - 2
    K = (T - 1) * (2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1))
    g = np.random.RandomState(T).standard_normal((n, 3))
    ref = np.linalg.solve(K, g)
    tol = 1e-10 * np.abs(ref).max()           # cond(K) ~ 4e5 at T = 1024: 4e5 x 2^-53 = 5e-11
    for solve in (tm.solve_closed, tm.solve_thomas):
        got = solve(g) / (T - 1)
        assert np.abs(got - ref).max() <= tol, solve.__name__


def test_a_zero_speed_waypoint_gives_a_finite_gradient():
    x = _bent_path(9)
    x[0, 5] = x[0, 3]                          # x_{t+1} == x_{t-1} at t = 4
    _, lin = tm.objective(x, tm.sphere_field((0.0, 0.0, 0.0), 0.5), OFFSETS3, RADII3, 0.2, 8.0, 1.0)
    assert np.isfinite(lin["grad"]).all() and np.isfinite(lin["f_obs"]).all()
    off, rad = tm.body(OFFSETS3, RADII3)
    s, g = tm.sphere_field((0.0, 0.0, 0.0), 0.5)(tm.points32(x, off).astype(np.float64))
    rec, _, grad, x_new, state, _ = tm.step64(x, [0], off, rad, s, g)
    assert np.isfinite(rec).all() and np.isfinite(grad).all() and np.isfinite(x_new).all() and state[0] == 0


def _line(a, b, T):
    return planning.seed_trajectories(a, b, T, 1)


def test_a_trajectory_in_free_space_converges_at_once_and_is_returned_unchanged():
    x0 = _line((0.0, 0.0, 0.0), (1.0, 2.0, 0.5), 16)
    x0 = np.concatenate([x0, x0 + np.float32(0.25)])
    eng = tm.StubEngine()
    res = planning.optimise_trajectories(eng, x0, radii=0.1, field=tm.host_field(tm.free_field), check_every=1)
    assert res.reason == ["converged"] * 2 and res.iterations == 1 and res.state.tolist() == [1, 1]
    # the straight line is the smoothness term's minimum up to the rounding of its float32 waypoints: the step is far below tol
    assert (res.records.step < 1e-6).all() and (res.records.scale == 0).all()
    assert res.x.numpy().tobytes() == x0.tobytes()
    assert eng.calls == [("points", 2), ("step", 2)]


def test_a_nan_in_the_field_is_invalid_field_and_leaves_x():
    x0 = np.concatenate([_bent_path(12, 1), _bent_path(12, 2)]).astype(np.float32)
    sphere = tm.sphere_field((0.0, 0.0, 0.0), 0.5)

    def field(pts):
        s, g = sphere(pts.astype(np.float64))
        s = s.astype(np.float32)
        s[12 + 5] = np.nan                     # trajectory 1, waypoint 5
        return s, g
    res = planning.optimise_trajectories(tm.StubEngine(), x0, radii=0.1, field=tm.host_field(field), iters=6, check_every=2)
    assert res.reason[1] == "invalid_field" and res.state[1] == 2 and res.records.bad[1] == 1
    assert res.x[1].numpy().tobytes() == x0[1].tobytes()
    assert res.reason[0] in ("max_iters", "converged") and res.x[0].numpy().tobytes() != x0[0].tobytes()


def test_check_every_changes_the_number_of_copies_not_the_result(monkeypatch):
    x0 = np.concatenate([_bent_path(12, 1), _line((0.0, 2.0, 0.0), (1.0, 2.0, 0.0), 12)]).astype(np.float32)
    field = tm.host_field(lambda p: tm.sphere_field((0.0, 0.0, 0.0), 0.5)(p.astype(np.float64)))
    copies, results = [], []
    fetch = planning._Scratch.fetch
    for every in (1, 4, 7):
        count = [0]

        def counted(self, records, count=count):
            count[0] += 1
            return fetch(self, records)
        monkeypatch.setattr(planning._Scratch, "fetch", counted)
        results.append(planning.optimise_trajectories(tm.StubEngine(), x0, radii=0.1, field=field, iters=12, check_every=every))
        copies.append(count[0])
    assert copies == [12, 3, 2]
    for r in results[1:]:
        assert r.x.numpy().tobytes() == results[0].x.numpy().tobytes() and r.state.tolist() == results[0].state.tolist()
        assert r.reason == results[0].reason
    assert results[0].state[1] == 1               # the line in free space stopped at iteration 1 and was left alone afterwards


def test_seed_trajectories_is_deterministic_and_keeps_line_and_endpoints():
    a, b = (0.4, 2.2, 1.5), (2.8, 2.2, 1.7)
    x = planning.seed_trajectories(a, b, 17, 6, spread=0.5, seed=3)
    assert x.shape == (6, 17, 3) and x.dtype == np.float32
    assert x.tobytes() == planning.seed_trajectories(a, b, 17, 6, spread=0.5, seed=3).tobytes()
    assert x.tobytes() != planning.seed_trajectories(a, b, 17, 6, spread=0.5, seed=4).tobytes()
    line = (np.asarray(a)[None] + np.linspace(0, 1, 17)[:, None] * (np.asarray(b) - np.asarray(a))[None]).astype(np.float32)
    assert np.array_equal(x[0], line)
    assert (x[:, 0] == np.float32(a)).all() and (x[:, -1] == np.float32(b)).all()
    dev = x[1:].astype(np.float64) - line[None]
    assert np.abs(dev @ (np.asarray(b) - np.asarray(a))).max() < 1e-5          # perpendicular to the line
    amp = np.linalg.norm(dev[:, 8], axis=-1)                                    # sin(pi / 2) = 1 at the middle waypoint
    assert (amp <= 0.5 + 1e-6).all() and amp.max() > 0.05


def test_plan_path_returns_none_when_every_seed_ends_in_collision():
    def inside(pts):
        g = np.zeros((len(pts), 3), np.float32)
        g[:, 0] = 1.0
        return np.full(len(pts), -0.3, np.float32), g
    res, best = planning.plan_path(tm.StubEngine(), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), T=8, n_seeds=4, iters=3, field=tm.host_field(inside))
    assert best is None and (res.records.in_collision > 0).all()
    res, best = planning.plan_path(tm.StubEngine(), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), T=8, n_seeds=4, iters=3,
                                   field=tm.host_field(tm.free_field))
    assert best == 0                              # in free space the straight line is the cheapest
    assert planning.plan_path(tm.StubEngine(), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), T=8, n_seeds=4, iters=3, clearance=20.0,
                              field=tm.host_field(tm.free_field))[1] is None


def test_trajectory_step_names_the_fields_of_the_record_and_leaves_x():
    x0 = _bent_path(12, 1).astype(np.float32)
    xt = torch.from_numpy(x0.copy())
    field = tm.host_field(lambda p: tm.sphere_field((0.0, 0.0, 0.0), 0.5)(p.astype(np.float64)))
    step, g = planning.trajectory_step(tm.StubEngine(), xt, offsets=OFFSETS3, radii=RADII3, field=field, want_grad=True)
    assert xt.numpy().tobytes() == x0.tobytes()
    assert g.shape == (1, 12, 3) and step.records.shape == (1, 16)
    assert step.state[0] == 0 and step.scale[0] > 0 and step.step[0] * step.scale[0] <= float(np.float32(0.05)) * (1 + 1e-12)
    assert step.active[0] >= step.in_collision[0] > 0 and step.min_clearance[0] < 0 and step.bad[0] == 0
    assert np.isclose(step.grad_sq[0], (g ** 2).sum()) and step.length[0] > 2.0
