"""The host half of pose alignment without a device: tests/pose_model.py (points, record, fields) and isdf_amd.tracking's loop
driven through a stub engine whose two calls are that model."""
import numpy as np
import pytest
import torch

from isdf_amd import tracking
from tests import pose_model as pm

CAM = pm.cam_of(48, 64, 60.0)


@pytest.fixture(scope="module")
def scene():
    T = pm.poses8()
    return dict(T=T, depth=pm.render(T, CAM, seed=0, invalid_frac=0.02))


def _refine(depth, T0, field=pm.room_field, **kw):
    eng = pm.StubEngine()
    res = tracking.refine_pose(eng, torch.from_numpy(depth), T0, CAM, field=pm.host_field(field), **kw)
    return res, eng


def test_jacobian_is_the_finite_difference_of_the_residual_under_the_stated_update():
    """smooth field: the distance to a sphere.  r(xi) = sdf(c' + exp(omega^)(x - c)) with c' = c + v; central differences in
    float64 against J = [g, (x - c) x g]"""
    centre, radius = np.array([0.3, -0.2, 2.0]), 1.1
    sdf = lambda p: np.linalg.norm(p - centre, axis=-1) - radius
    rng = np.random.RandomState(0)
    x = rng.uniform(-1, 1, (50, 3)) + np.array([0.0, 0.0, 2.0])
    c = np.array([0.1, 0.2, -0.3])
    g = (x - centre) / np.linalg.norm(x - centre, axis=-1, keepdims=True)
    J = np.concatenate([g, np.cross(x - c, g)], -1)
    h = 1e-6
    for k in range(6):
        xi = np.zeros(6)
        xi[k] = h
        moved = lambda s: (c + s * xi[:3]) + (x - c) @ tracking.so3_exp(s * xi[3:]).T
        fd = (sdf(moved(1.0)) - sdf(moved(-1.0))) / (2 * h)
        assert np.abs(fd - J[:, k]).max() < 1e-8, k
    # ... and the record's b and H are those Jacobians summed (weights 1: every |r| below huber)
    T = np.eye(4)
    T[:3, 3] = c
    r32, g32, x32 = sdf(x).astype(np.float32), g.astype(np.float32), x.astype(np.float32)
    rec, _ = pm.records64(x32, r32, g32, np.ones(50, bool), T[None], huber=10.0, trunc=20.0)
    s = tracking.unpack_records(rec)
    J32 = np.concatenate([g32.astype(np.float64), np.cross(x32.astype(np.float64) - np.float32(c).astype(np.float64), g32.astype(np.float64))], -1)
    assert np.allclose(s.H[0], J32.T @ J32, rtol=1e-12, atol=1e-12) and np.allclose(s.b[0], J32.T @ r32.astype(np.float64), rtol=1e-12, atol=1e-12)
    assert s.used[0] == s.valid[0] == 50 and np.array_equal(s.H[0], s.H[0].T)


def test_a_frame_without_valid_pixels_keeps_its_pose(scene):
    depth = scene["depth"][:2].copy()
    depth[1] = 0.0
    T0 = pm.perturb(scene["T"][:2], 0.03, 2.0, seed=1)
    res, _ = _refine(depth, T0)
    assert res.reason[1] == "no_valid_pixels" and not res.converged[1] and res.iterations[1] == 1
    assert np.array_equal(res.T_WC[1], T0[1])
    assert res.converged[0] and res.reason[0] == "converged"


def test_a_frame_with_too_few_used_points_keeps_its_pose(scene):
    depth = scene["depth"][:1].copy()
    keep = np.zeros(depth.shape, bool)
    keep[0, ::4, ::4][2:5, 3:9] = True                      # 18 lattice pixels survive
    depth[~keep] = 0.0
    T0 = pm.perturb(scene["T"][:1], 0.03, 2.0, seed=2)
    res, _ = _refine(depth, T0, min_points=64)
    assert res.reason[0] == "too_few_points" and not res.converged[0]
    assert 0 < res.history[0][0][1] < 64 and np.isnan(res.history[0][0][2])
    assert np.array_equal(res.T_WC[0], T0[0])


def test_a_rank_deficient_system_keeps_its_pose(scene):
    """a single infinite plane (y = 3, the room's floor) fixes one translation and two rotations: diag(H) has exact zeros, the
    relative damping leaves them zero, Cholesky refuses"""
    T0 = scene["T"][:1].copy()
    res, _ = _refine(scene["depth"][:1], T0, field=pm.plane_field, trunc=10.0)
    assert res.reason[0] == "not_positive_definite" and not res.converged[0] and res.iterations[0] == 1
    assert np.array_equal(res.T_WC[0], T0[0]) and res.history[0][0][1] >= 64


def test_frame_of_pose_maps_several_hypotheses_onto_one_frame(scene):
    T_true = scene["T"][2]
    T0 = np.concatenate([pm.perturb(T_true[None], 0.03, 2.0, seed=s) for s in (3, 4, 5)])
    eng = pm.StubEngine()
    res = tracking.refine_pose(eng, torch.from_numpy(scene["depth"]), T0, CAM, frame_of_pose=[2, 2, 2],
                               field=pm.host_field(pm.room_field))
    assert eng.calls[0] == ("points", 3, [2, 2, 2]) and eng.calls[1] == ("system", 3, [2, 2, 2])
    dt, dr = pm.pose_error(res.T_WC, np.repeat(T_true[None], 3, 0))
    assert res.converged.all() and dt.max() <= 1e-5 and dr.max() <= 1e-4
    with pytest.raises(ValueError):
        tracking.refine_pose(eng, torch.from_numpy(scene["depth"]), T0, CAM, frame_of_pose=[2, 2], field=pm.host_field(pm.room_field))


@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("metres,degrees", [(0.03, 2.0), (0.15, 8.0)])
def test_eight_poses_converge_to_the_true_pose_on_the_exact_field(scene, stride, metres, degrees):
    """eight poses, 48 x 64, 2 % invalid pixels: every pose within 10 iterations to at most 1e-5 m and 1e-4 degrees
    (a float64 host prototype of the loop reached 2.7e-7 m and 5.3e-6 degrees; the bar leaves 20 - 40 x for a differently
    rounded but equivalent field)"""
    T0 = pm.perturb(scene["T"], metres, degrees, seed=7)
    res, eng = _refine(scene["depth"], T0, stride=stride, iters=10)
    dt, dr = pm.pose_error(res.T_WC, scene["T"])
    print("stride %d, %.2f m / %g deg: iterations %s, worst error %.3g m %.3g deg" % (stride, metres, degrees, res.iterations.tolist(),
                                                                                 dt.max(), dr.max()))
    assert res.converged.all() and res.reason == ["converged"] * 8 and res.iterations.max() <= 10
    assert dt.max() <= 1e-5 and dr.max() <= 1e-4
    # the batch shrinks as poses converge: the last call carries no more poses than the first
    assert eng.calls[0][1] == 8 and eng.calls[-1][1] <= 8


def test_the_loop_equals_the_model_loop_written_on_its_own(scene):
    T0 = pm.perturb(scene["T"][:3], 0.08, 5.0, seed=9)
    res, _ = _refine(scene["depth"][:3], T0)
    T, its, done = pm.gauss_newton(scene["depth"][:3], T0, CAM, pm.room_field)
    assert done.all() and res.converged.all() and np.array_equal(its, res.iterations)
    assert np.abs(T - res.T_WC).max() < 1e-12


def test_pose_system_names_the_fields_of_the_record(scene):
    s = tracking.pose_system(pm.StubEngine(), torch.from_numpy(scene["depth"][:2]), scene["T"][:2], CAM, field=pm.host_field(pm.room_field))
    assert s.H.shape == (2, 6, 6) and s.b.shape == (2, 6) and s.H.dtype == s.b.dtype == np.float64
    n_pix = 12 * 16
    assert (s.valid <= n_pix).all() and (s.used <= s.valid).all() and (s.used > 0.9 * 0.98 * n_pix).all()
    assert np.allclose(s.records[:, 0], s.used) and (s.cost >= 0.5 * s.wr2 * (1 - 1e-12)).all()
