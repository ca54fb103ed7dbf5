"""Host-side checks of routing: the Dijkstra model against the closed form of the empty grid, the grids the GPU tests use, and
the parts of isdf_amd.routing that run on the host (free_space, snap, resample, seed_routes)."""
import math

import numpy as np
import pytest
import torch

from isdf_amd import _ffi, planning, routing
from tests import route_model as rm


@pytest.mark.parametrize("shape,goal", [((9, 10, 11), (3, 4, 5)), ((1, 1, 40), (0, 0, 7)), ((7, 1, 5), (6, 0, 0)), ((1, 1, 1), (0, 0, 0))])
def test_model_equals_the_closed_form_on_an_empty_grid(shape, goal):
    dist = rm.dijkstra(np.ones(shape, np.uint8), [goal])
    assert dist.dtype == np.int32 and np.array_equal(dist, rm.closed_form(shape, goal))
    # 3 a + b + c by hand: offsets (5, 2, 1) -> one corner move, one edge move, three face moves
    if shape == (9, 10, 11):
        assert dist[8, 6, 4] == 5 * 1 + 4 * 1 + 3 * 3 == 3 * 5 + 2 + 1
    far = np.unravel_index(np.argmax(dist), shape)
    path, n = rm.trace(dist, far)
    assert n == len(path) and path[-1] == np.ravel_multi_index(goal, shape) and n == np.abs(np.array(far) - goal).max() + 1


def test_model_neighbour_order_and_weights():
    assert len(rm.NEIGHBOURS) == 26 and rm.NEIGHBOURS == sorted(rm.NEIGHBOURS)
    assert rm.NEIGHBOURS[0] == (-1, -1, -1) and rm.NEIGHBOURS[12] == (0, 0, -1) and rm.NEIGHBOURS[13] == (0, 0, 1)
    assert sorted(set(rm.WEIGHTS)) == [3, 4, 5] and [rm.WEIGHTS.count(w) for w in (3, 4, 5)] == [6, 12, 8]
    assert rm.NONE == _ffi.ROUTE_NONE


def test_model_ignores_bad_goals_and_reports_trace_failures():
    free = np.ones((3, 3, 3), np.uint8)
    free[1, 1, 1] = 0
    assert (rm.dijkstra(free, [[1, 1, 1], [5, 0, 0], [-1, 0, 0]]) == rm.NONE).all()
    assert (rm.dijkstra(free, np.zeros((0, 3), np.int64)) == rm.NONE).all()
    dist = rm.dijkstra(free, [[0, 0, 0]])
    assert dist[1, 1, 1] == rm.NONE and dist[2, 2, 2] == 12                 # round the blocked centre: 4 + 5 + 3 instead of 5 + 5
    assert rm.trace(dist, (1, 1, 1)) == ([], 0) and rm.trace(dist, (3, 0, 0)) == ([], 0)
    path, n = rm.trace(dist, (2, 2, 2))
    assert n == 4 and rm.trace(dist, (2, 2, 2), max_len=2) == (path[:2], -1)
    broken = dist.copy()
    broken[2, 2, 2] += 1                                                     # no neighbour explains it
    assert rm.trace(broken, (2, 2, 2)) == ([26], -1)


def test_the_test_grids_have_what_the_gpu_tests_rely_on():
    free, goals = rm.random_obstacles()
    assert free.shape == (20, 17, 23) and abs(free.mean() - 0.35) < 0.02
    assert free[tuple(goals.T)].tolist() == [1, 1, 0]
    dist = rm.dijkstra(free, goals)
    open_ = free != 0
    assert ((dist < rm.NONE) & open_).sum() > 2000 and 0 < ((dist == rm.NONE) & open_).sum() < 50       # reachable and walled-in
    assert (dist[~open_] == rm.NONE).all()
    maze, goal = rm.serpentine()
    d = rm.dijkstra(maze, goal)
    assert maze.shape == (24, 8, 24) and (d[maze != 0] < rm.NONE).all()
    path, n = rm.trace(d, (22, 0, 0))
    assert n > 1000 > 20 * max(maze.shape) // 2                              # many times the diameter
    T = _ffi.ROUTE_TILE
    for edge_only in (False, True):
        free, goal = rm.diagonal_corridor(T, edge_only)
        d = rm.dijkstra(free, goal)
        i = np.arange(2 * T + 1)
        assert np.array_equal(d[i, i, 0 if edge_only else i], (4 if edge_only else 5) * i) and free.sum() == 2 * T + 1


def test_free_space_thresholds_nan_and_margin():
    v = torch.tensor([[-1.0, 0.0, 0.2], [0.2000001, float("nan"), float("inf")], [float("-inf"), 0.3, 1.0]])
    m = routing.free_space(v, 0.2)
    assert m.dtype == torch.uint8 and m.shape == v.shape
    assert m.tolist() == [[0, 0, 0], [1, 0, 1], [0, 1, 1]]                   # strictly above; NaN is blocked
    assert routing.free_space(v.numpy(), 0.2).tolist() == m.tolist()
    assert routing.margin(0.1) == 0.5 * math.sqrt(3.0) * 0.1
    c = 0.15 + routing.margin(0.1)                                           # 0.2366...
    assert abs(c - 0.2366025) < 1e-7
    w = torch.tensor([0.2366, 0.2367, 0.16, 0.5], dtype=torch.float32)
    assert routing.free_space(w, 0.15, voxel=0.1).tolist() == [0, 1, 0, 1]
    assert routing.free_space(w, 0.15).tolist() == [1, 1, 1, 1]


def test_snap_rounds_through_the_inverse_affine():
    A = np.array([[0.1, 0, 0, 0.05], [0, 0.1, 0, 0.05], [0, 0, 0.1, 0.05]])
    assert routing.snap(A, [[1.02, 1.53, 3.97], [0.05, 0.05, 0.05], [-0.12, 6.0, 0.149]]).tolist() == [[10, 15, 39], [0, 0, 0], [-2, 60, 1]]
    R = np.array([[0.0, 0.2, 0.0, 1.0], [0.2, 0.0, 0.0, -1.0], [0.0, 0.0, 0.5, 0.0]])          # axes swapped, anisotropic
    assert routing.snap(R, [[1.41, -0.38, 1.1]]).tolist() == [[3, 2, 2]]


def test_resample_end_points_and_spacing():
    line = np.array([[0, 0, 0], [0, 0, 0], [3, 0, 0], [3, 4, 0], [3, 4, 0], [3, 4, 5]], np.float64)      # 12 m, repeated points
    x = routing.resample(line, 25)
    assert x.shape == (25, 3) and x.dtype == np.float32
    assert x[0].tolist() == [0, 0, 0] and x[-1].tolist() == [3, 4, 5]
    step = np.abs(np.diff(x.astype(np.float64), axis=0)).sum(1)             # along axis-parallel legs the L1 step is the arc step
    assert np.allclose(step, 0.5, atol=1e-6)
    assert np.allclose(x[6], [3, 0, 0]) and np.allclose(x[14], [3, 4, 0])   # the corners fall on samples 6 and 14
    y = routing.resample(line, 2)
    assert y.tolist() == [[0, 0, 0], [3, 4, 5]]
    assert routing.resample([[1, 2, 3]], 4).tolist() == [[1, 2, 3]] * 4
    with pytest.raises(ValueError):
        routing.resample(line, 1)


def test_seed_routes_use_the_draws_of_seed_trajectories():
    start, goal = np.array([1.0, 1.5, 4.0]), np.array([5.0, 1.5, 4.0])
    straight = np.stack([start, goal])
    ours = routing.seed_routes(straight, 16, 5, spread=0.3, seed=3)
    theirs = planning.seed_trajectories(start, goal, 16, 5, spread=0.3, seed=3)
    assert ours.shape == theirs.shape == (5, 16, 3) and ours.dtype == np.float32
    assert np.allclose(ours, theirs, atol=1e-6)                              # on a straight route the two constructions coincide
    bent = np.array([[1.0, 1.5, 4.0], [1.0, 1.5, 0.7], [5.0, 1.5, 0.7], [5.0, 1.5, 4.0]])
    x = routing.seed_routes(bent, 32, 4, spread=0.3, seed=0)
    assert np.array_equal(x[0], routing.resample(bent, 32))
    assert (x[:, 0] == x[0, 0]).all() and (x[:, -1] == x[0, -1]).all()
    off = x[1:].astype(np.float64) - x[0]
    assert (np.abs(off @ (goal - start)) < 1e-5).all()                       # bulges are perpendicular to goal - start
    peak = np.linalg.norm(off, axis=-1).max(1)
    assert (peak > 0).all() and (peak < 0.3).all()


def test_hold_weight_grows_with_the_route_and_never_falls_below_the_default():
    assert routing.hold_weight(0.5) == planning.DEFAULTS["w_obs"] == 8.0
    assert routing.hold_weight(9.6) == 2.0 * 1.0 * 9.6 / 0.2 and routing.hold_weight(9.6, w_smooth=0.5, eps=0.4) == pytest.approx(24.0)
