"""The host half of joint-space planning without a device: tests/arm_model.py (frames, gradient, projection), Chain.forward, and
isdf_amd.kinematics' loop driven through a stub engine whose two calls are that model."""
import numpy as np
import pytest

from isdf_amd import kinematics as kin
from tests import arm_model as am
from tests import pose_model as pm
from tests import traj_model as tm

EPS, W_OBS, W_SMOOTH = 0.2, 8.0, 1.0


def _noisy_line(start, goal, T=12, seed=0):
    rng = np.random.RandomState(seed)
    th = am.line(start, goal, T).astype(np.float64)
    th[:, 1:-1] += 0.03 * rng.standard_normal(th[:, 1:-1].shape)
    return th


GRADIENT_SCENES = {
    # arm A sweeps its forearm through the sphere at (1.5, 2.5, 1.5); the free body flies through it while it turns
    "arm_a": (am.arm_a, (-0.2, 1.1, 0.5, 0.2), (-2.9, 1.1, 0.5, 0.2)),
    "free_body": (am.free_body, (0.6, 2.45, 1.4, 0.0, 0.0, 0.0), (2.4, 2.6, 1.65, 1.0, 0.5, 0.3)),
}


@pytest.mark.parametrize("scene", sorted(GRADIENT_SCENES))
def test_gradient_is_the_central_difference_of_the_discrete_functional(scene):
    """12 waypoints, float64 throughout, the analytic sphere (exact gradient), h = 1e-6; the bar is 1e-6 max|grad|: the round-off
    floor of the difference quotient is about 1e-16 F / h = 2e-9, a missing or mis-signed term is O(1)"""
    make, start, goal = GRADIENT_SCENES[scene]
    chain, field = make(), am.sphere_field()
    th = _noisy_line(start, goal)
    f0, lin = am.objective(chain, th, field, EPS, W_OBS, W_SMOOTH)
    n = th.shape[1] * chain.S
    assert lin["n_neg"][0] > 0 and lin["n_act"][0] > lin["n_neg"][0] and lin["n_act"][0] < n          # all three branches of c
    h, worst = 1e-6, 0.0
    for t in range(1, th.shape[1] - 1):
        for j in range(chain.J):
            tp, tn = th.copy(), th.copy()
            tp[0, t, j] += h
            tn[0, t, j] -= h
            fd = (am.objective(chain, tp, field, EPS, W_OBS, W_SMOOTH)[0][0] - am.objective(chain, tn, field, EPS, W_OBS, W_SMOOTH)[0][0]) / (2 * h)
            worst = max(worst, abs(fd - lin["grad"][0, t, j]))
    big = np.abs(lin["grad"]).max()
    print("%s: worst |central difference - gradient| = %.3g at max|grad| = %.3g (F = %.4g)" % (scene, worst, big, f0[0]))
    assert big > 1.0 and worst < 1e-6 * big
    assert np.array_equal(lin["grad"][0, [0, -1]], np.zeros((2, chain.J)))


def _rot_chain(kind, axis, X=None):
    X = np.hstack([np.eye(3), np.zeros((3, 1))]) if X is None else X
    return kin.Chain(np.hstack([np.eye(3), np.zeros((3, 1))]), [X], [kind], [axis], [0, 1], [[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]], 0.1)


def test_forward_a_revolute_joint_at_zero_leaves_the_frame_and_a_quarter_turn_moves_the_axes():
    X = np.array([[0.0, -1.0, 0.0, 0.5], [1.0, 0.0, 0.0, -0.25], [0.0, 0.0, 1.0, 2.0]])
    c = _rot_chain(0, [0.0, 0.0, 1.0], X)
    q, F = c.forward([0.0], frames=True)
    assert np.array_equal(F[0], np.hstack([np.eye(3), np.zeros((3, 1))])) and np.array_equal(F[1], X)
    assert np.array_equal(q[0], [0.0, 0.0, 0.0]) and np.allclose(q[1], X[:, :3] @ [1.0, 2.0, 3.0] + X[:, 3], atol=1e-15)
    # a quarter turn about z takes x to y and y to -x; about x it takes y to z and z to -y
    for axis, want in (([0.0, 0.0, 1.0], [[0, -1, 0], [1, 0, 0], [0, 0, 1]]), ([1.0, 0.0, 0.0], [[1, 0, 0], [0, 0, -1], [0, 1, 0]]),
                       ([0.0, 1.0, 0.0], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]])):
        q, F = _rot_chain(0, axis).forward([np.pi / 2], frames=True)
        assert np.allclose(F[1][:, :3], want, atol=1e-15) and np.array_equal(F[1][:, 3], np.zeros(3)), axis
        assert np.allclose(q[1], np.array(want, float) @ [1.0, 2.0, 3.0], atol=1e-15)
        assert np.allclose(_rot_chain(0, axis).forward([-np.pi / 2], frames=True)[1][1][:, :3], np.array(want).T, atol=1e-15)


def test_forward_a_prismatic_chain_is_a_translation_and_the_factories_place_their_bodies():
    off = np.array([[0.0, 0.0, 0.0], [0.1, -0.2, 0.3], [-0.4, 0.0, 0.05]])
    eye = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (3, 1, 1))
    c = kin.Chain(eye[0], eye, [1, 1, 1], np.eye(3), [3, 3, 3], off, 0.1)
    x = np.random.RandomState(0).uniform(-2, 2, (4, 5, 3))
    assert np.allclose(c.forward(x), x[..., None, :] + off.astype(np.float32).astype(np.float64), atol=1e-15)
    fb = kin.Chain.free_body(off, [0.1, 0.2, 0.3])
    th = np.concatenate([x, np.zeros_like(x)], -1)
    assert np.allclose(fb.forward(th), c.forward(x), atol=1e-15)                       # no rotation: the same translation
    th[..., 3] = np.pi / 2                                                             # a quarter turn about y: x -> -z, z -> x
    o = off.astype(np.float32).astype(np.float64)
    assert np.allclose(fb.forward(th), x[..., None, :] + np.stack([o[:, 2], o[:, 1], -o[:, 0]], -1), atol=1e-15)
    pb = kin.Chain.planar_base(off, 0.1)
    q = pb.forward([1.0, 2.0, np.pi / 2])
    assert np.allclose(q, np.array([1.0, 2.0, 0.0]) + np.stack([-o[:, 1], o[:, 0], o[:, 2]], -1), atol=1e-15)
    assert (fb.J, fb.S, pb.J, pb.S) == (6, 3, 3, 3) and fb.links.tolist() == [6] * 3 and pb.kinds.tolist() == [1, 1, 0]


def test_the_model_s_frames_are_chain_forward_and_its_points_round_them_once():
    rng = np.random.RandomState(3)
    for chain in (am.arm_a(), am.free_body()):
        th = rng.uniform(-2.0, 2.0, (2, 7, chain.J)).astype(np.float32)
        q64 = am.frames(chain, th)[0]
        assert np.abs(q64 - chain.forward(th)).max() < 1e-13
        assert am.points32(chain, th).tobytes() == q64.astype(np.float32).reshape(-1, 3).tobytes()


@pytest.mark.parametrize("bad", [dict(kinds=[0, 2]), dict(axes=[[0, 0, 1], [0, 0, 1.1]]), dict(links=[0, 3]), dict(links=[-1, 1]),
                                 dict(radii=[-0.1, 0.1]), dict(radii=[np.nan, 0.1]), dict(centres=[[0, 0, 0], [np.inf, 0, 0]]),
                                 dict(lo=[0.5, 0.0], hi=[0.0, 1.0]), dict(lo=[np.nan, 0.0])])
def test_chain_refuses_on_the_host_what_the_call_would_refuse(bad):
    eye = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (2, 1, 1))
    kw = dict(base=eye[0], X=eye, kinds=[0, 1], axes=[[0, 0, 1], [1, 0, 0]], links=[0, 2], centres=np.zeros((2, 3)), radii=[0.1, 0.1])
    kin.Chain(**kw)
    with pytest.raises(ValueError):
        kin.Chain(**dict(kw, **bad))
    with pytest.raises(ValueError):
        kin.Chain(eye[0], np.tile(eye[:1], (9, 1, 1)), [0] * 9, [[0, 0, 1]] * 9, [0], [[0, 0, 0]], 0.1)


def test_projection_counts_the_cut_entries_and_keeps_theta_inside_the_limits():
    """the model's step with limits: a limit that binds cuts some entries, the step length is the projected maximum"""
    rng = np.random.RandomState(5)
    free = am.free_body()
    th = am.line((0.6, 2.45, 1.4, 0.0, 0.0, 0.0), (2.4, 2.6, 1.65, 1.0, 0.5, 0.3), 12)
    q = am.points32(free, th)
    sdf, grad = am.sphere_field()(q.astype(np.float64))
    sdf, grad = sdf.astype(np.float32), (grad + 0.3 * rng.standard_normal(grad.shape)).astype(np.float32)
    p = dict(am.DEFAULTS, max_step=float("inf"), eta=4.0)
    rec0, _, _, th0, _, _ = am.step64(free, th, [0], q, sdf, grad, **p)
    moved = th0[0].astype(np.float64) - th[0].astype(np.float64)
    lo = (th[0].min(0) - 0.25 * np.abs(moved).max(0)).astype(np.float32)
    hi = (th[0].max(0) + 0.25 * np.abs(moved).max(0)).astype(np.float32)
    lim = kin.Chain(free.base, free.X, free.kinds, free.axes, free.links, free.centres, free.radii, lo, hi)
    rec, _, _, th1, state, _ = am.step64(lim, th, [0], q, sdf, grad, **p)
    assert rec0[0, 11] == 0 and 0 < rec[0, 11] < 60 and state[0] == 0
    assert (th1 >= lo).all() and (th1 <= hi).all() and not ((th0 >= lo).all() and (th0 <= hi).all())
    assert rec[0, 6] < rec0[0, 6] and rec[0, 7] == 1.0
    assert abs(np.abs(th1[0].astype(np.float64) - th[0]).max() - rec[0, 6]) <= np.spacing(np.float32(np.abs(th1).max()))


@pytest.mark.parametrize("name", sorted(am.SCENARIOS))
def test_the_model_s_loop_converges_free_of_collision_on_the_exact_room(name):
    """float32 storage of theta between iterations, the room's field rounded to float32, the defaults (eta = 32), T = 32, the
    straight line in joint space as the start"""
    make, start, goal = am.SCENARIOS[name]
    chain, th0 = make(), am.line(start, goal, 32)
    q = am.points32(chain, th0)
    first = am.step64(chain, th0, [0], q, *pm.room_field(q))[0]
    th, rec, iters = am.loop64(chain, th0, pm.room_field, iters=400)
    print("%s: %d samples in collision (least clearance %.3f m) -> state %d after %d iterations, clearance %.4f m"
          % (name, first[0, 3], first[0, 2], rec[0, 9], iters, rec[0, 2]))
    assert first[0, 3] > 0
    assert rec[0, 9] == 1 and iters < 400 and rec[0, 3] == 0 and rec[0, 2] > 0
    assert th[0, [0, -1]].tobytes() == th0[0, [0, -1]].tobytes()


def test_the_loop_does_not_depend_on_check_every_and_freezes_what_has_stopped():
    """two free bodies, one in free space (converges at its first linearisation) and one through the sphere; the host loop of
    kinematics.optimise_joint_trajectories through the stub engine"""
    chain = am.free_body()
    th0 = np.concatenate([am.line((0.6, 0.3, 1.4, 0, 0, 0), (2.4, 0.3, 1.65, 0, 0, 0), 12),
                          am.line((0.6, 2.45, 1.4, 0, 0, 0), (2.4, 2.6, 1.65, 1.0, 0.5, 0.3), 12)])
    field = tm.host_field(am.sphere_field())
    runs = []
    for every in (1, 7):
        eng = am.StubEngine()
        res = kin.optimise_joint_trajectories(eng, chain, th0, iters=21, check_every=every, field=field)
        runs.append(res)
        assert eng.calls[0] == ("points", 2) and eng.calls.count(("points", 2)) == 1 and res.iterations == 21
    a, b = runs
    assert a.x.numpy().tobytes() == b.x.numpy().tobytes() and a.records.records.tobytes() == b.records.records.tobytes()
    assert a.reason == ["converged", "max_iters"] and a.state.tolist() == [1, 0]
    assert a.x.numpy()[0].tobytes() == th0[0].tobytes() and (a.x.numpy()[1, 1:-1] != th0[1, 1:-1]).any()
    assert a.x.numpy()[:, [0, -1]].tobytes() == th0[:, [0, -1]].tobytes()
    step, g = kin.joint_step(am.StubEngine(), chain, th0, field=field, want_grad=True)
    assert step.in_collision.tolist()[0] == 0 and step.in_collision[1] > 0 and g.shape == (2, 12, 6)
    res, best = kin.plan_joint_path(am.StubEngine(), chain, th0[1, 0], th0[1, -1], T=12, n_seeds=3, iters=2, field=field)
    assert res.x.shape == (3, 12, 6) and (best is None or 0 <= best < 3)


def test_seeds_start_and_end_exactly_and_respect_the_limits():
    a, b = np.array([0.1, -0.4, 0.3, 1.0]), np.array([1.1, 0.2, -0.3, 0.5])
    th = kin.seed_joint_trajectories(a, b, 9, 5, spread=0.8, seed=2)
    assert th.shape == (5, 9, 4) and th.dtype == np.float32
    assert np.array_equal(th[:, 0], np.tile(a.astype(np.float32), (5, 1))) and np.array_equal(th[:, -1], np.tile(b.astype(np.float32), (5, 1)))
    assert np.allclose(th[0], a + np.linspace(0, 1, 9)[:, None] * (b - a), atol=1e-6)
    assert (np.abs(th[1:] - th[0]).reshape(4, -1).max(-1) > 0).all()
    lo, hi = np.minimum(a, b) - 0.05, np.maximum(a, b) + 0.05
    cl = kin.seed_joint_trajectories(a, b, 9, 5, spread=0.8, seed=2, lo=lo, hi=hi)
    assert (cl >= lo.astype(np.float32) - 1e-6).all() and (cl <= hi.astype(np.float32) + 1e-6).all() and (cl != th).any()
