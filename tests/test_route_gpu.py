"""Routing on the device: isdf_route_init / isdf_route_relax / isdf_route_trace through Engine.route_* and isdf_amd.routing.
Reference: tests/route_model.py -- Dijkstra on the same graph and the trace with the header's neighbour order.  Everything is
int32: fields and paths are compared bit for bit, no tolerance anywhere.  End to end the field is the closed-form room of
isdf_amd.synthetic with a partition wall, supplied as `field=` (as tests/test_traj_gpu.py does)."""
import numpy as np
import pytest
import torch

from isdf_amd import _ffi, planning, routing, synthetic
from tests import route_model as rm

pytestmark = pytest.mark.gpu

TILE = _ffi.ROUTE_TILE
NONE = _ffi.ROUTE_NONE


@pytest.fixture(scope="module")
def eng():
    from isdf_amd.engine import Engine, NetConfig
    return Engine(NetConfig(hidden=64, blocks=1), "cuda")


def _blocked_goals():
    free, _ = rm.random_obstacles()
    return free, np.argwhere(free == 0)[[0, 100, 2000]]


GRIDS = {
    "one_voxel": lambda: (np.ones((1, 1, 1), np.uint8), np.array([[0, 0, 0]])),
    "thin": lambda: (np.ones((1, 1, 40), np.uint8), np.array([[0, 0, 33]])),
    "empty": lambda: (np.ones((9, 10, 11), np.uint8), np.array([[3, 4, 5]])),          # no side a multiple of the tile
    "corner_corridor": lambda: rm.diagonal_corridor(TILE),
    "edge_corridor": lambda: rm.diagonal_corridor(TILE, edge_only=True),
    "random": rm.random_obstacles,
    "maze": rm.serpentine,
    "goals_blocked": _blocked_goals,
    "no_goals": lambda: (rm.random_obstacles()[0], np.zeros((0, 3), np.int64)),
}


@pytest.fixture(scope="module")
def cases(eng):
    """name -> dict(free, goals, model, field): the model's field and the device's (relaxed once), shared by the tests below"""
    out = {}
    for name, make in GRIDS.items():
        free, goals = make()
        out[name] = dict(free=free, goals=goals, model=rm.dijkstra(free, goals),
                         field=routing.distance_field(eng, torch.from_numpy(free).cuda(), goals))
    return out


@pytest.mark.parametrize("name", list(GRIDS))
def test_the_field_equals_dijkstra_bit_for_bit(cases, name):
    c = cases[name]
    dev = c["field"].dist.cpu().numpy()
    print("%s %s: converged %s after %d rounds; %d voxels reached, farthest %d" % (
        name, c["free"].shape, c["field"].converged, c["field"].rounds, (c["model"] < NONE).sum(),
        c["model"][c["model"] < NONE].max() if (c["model"] < NONE).any() else -1))
    assert c["field"].converged and dev.dtype == np.int32 and dev.shape == c["free"].shape
    assert dev.tobytes() == c["model"].tobytes()
    assert (dev[c["free"] == 0] == NONE).all()


def test_the_empty_grid_is_the_closed_form_and_the_corridors_cross_tile_corners_and_edges(cases):
    assert np.array_equal(cases["empty"]["field"].dist.cpu().numpy(), rm.closed_form((9, 10, 11), (3, 4, 5)))
    assert np.array_equal(cases["thin"]["field"].dist.cpu().numpy()[0, 0], 3 * np.abs(np.arange(40) - 33))
    assert cases["one_voxel"]["field"].dist.item() == 0
    i = np.arange(2 * TILE + 1)
    assert np.array_equal(cases["corner_corridor"]["field"].dist.cpu().numpy()[i, i, i], 5 * i)      # two moves across tile corners
    assert np.array_equal(cases["edge_corridor"]["field"].dist.cpu().numpy()[i, i, 0], 4 * i)        # two across tile edges


def test_unreachable_pockets_and_fields_without_a_goal_stay_none(cases):
    c = cases["random"]
    dev, open_ = c["field"].dist.cpu().numpy(), c["free"] != 0
    pockets = open_ & (c["model"] == NONE)
    assert pockets.any() and (dev[pockets] == NONE).all() and (dev[open_ & ~pockets] < NONE).all()
    for name in ("goals_blocked", "no_goals"):
        f = cases[name]["field"]
        assert (f.dist == NONE).all() and f.converged and f.rounds == 1                 # the first round already changes nothing


def test_maze_convergence_does_not_depend_on_how_often_the_host_looks(eng, cases):
    c = cases["maze"]
    free = torch.from_numpy(c["free"]).cuda()
    ref = c["field"]
    assert ref.converged and ref.rounds > 8, ref.rounds                                # many rounds: several groups of the default 8
    want = c["model"].tobytes()
    # one more round leaves the bytes alone and reports no change
    dist = ref.dist.clone()
    changed = eng.route_relax(free, dist, 1)
    assert changed.tolist() == [0] and dist.cpu().numpy().tobytes() == want
    for every in (1, 3, 8):
        f = routing.distance_field(eng, free, c["goals"], check_every=every)
        assert f.converged and f.rounds == ref.rounds and f.dist.cpu().numpy().tobytes() == want, every
    # cut short: not converged, every value an upper bound that is the cost of a real path, NONE or >= the true distance
    short = routing.distance_field(eng, free, c["goals"], check_every=2, max_rounds=4)
    d = short.dist.cpu().numpy()
    assert not short.converged and short.rounds == 4 and (d >= c["model"]).all() and (d > c["model"]).any()
    # the flags of a group: 1 while the front moves, 0 from the first quiet round on
    dist = eng.route_init(free, c["goals"])
    flags = eng.route_relax(free, dist, ref.rounds + 2).tolist()
    assert flags == [1] * (ref.rounds - 1) + [0] * 3 and dist.cpu().numpy().tobytes() == want


def _device_paths(eng, field, starts, max_len):
    path, length = eng.route_trace(field.dist, torch.as_tensor(np.asarray(starts, np.int32)), max_len)
    return path.cpu().numpy(), length.cpu().numpy()


@pytest.mark.parametrize("name", ["random", "maze"])
def test_traced_paths_equal_the_model_index_for_index(eng, cases, name):
    c = cases[name]
    free, model = c["free"], c["model"]
    reach = np.argwhere(model < NONE)
    rng = np.random.RandomState(7)
    starts = np.concatenate([reach[rng.choice(len(reach), 12, replace=False)], reach[[np.argmax(model[tuple(reach.T)])]],
                             np.asarray(c["goals"][:1])])
    paths = routing.trace(eng, c["field"], starts)
    dims = np.array(free.shape)
    for s, vox in zip(starts, paths):
        want, n = rm.trace(model, s)
        lin = (vox[:, 0] * dims[1] + vox[:, 1]) * dims[2] + vox[:, 2]
        assert n == len(vox) >= 1 and lin.tolist() == want, s
        assert (vox[0] == s).all() and model[tuple(vox[-1])] == 0
        assert (free[tuple(vox.T)] != 0).all()
        step = np.abs(np.diff(vox, axis=0))
        assert (step.max(1) == 1).all() if len(vox) > 1 else True                      # every step a neighbour move
        d = model[tuple(vox.T)].astype(np.int64)
        assert np.array_equal(d[:-1] - d[1:], 2 + (step != 0).sum(1))                  # dist drops by exactly the move's weight
    assert len(paths[-1]) == 1                                                         # a start on a goal: the goal alone


def test_trace_reports_unreachable_starts_and_a_max_len_that_is_too_small(eng, cases):
    c = cases["random"]
    free, model = c["free"], c["model"]
    pocket = np.argwhere((free != 0) & (model == NONE))[0]
    blocked = np.argwhere(free == 0)[0]
    far = np.array(np.unravel_index(np.argmax(np.where(model < NONE, model, -1)), model.shape))
    want, n = rm.trace(model, far)
    starts = np.stack([pocket, blocked, [-1, 0, 0], [0, 17, 0], far])
    path, length = _device_paths(eng, c["field"], starts, n)
    assert length.tolist() == [0, 0, 0, 0, n] and path[4].tolist() == want
    assert [len(p) for p in routing.trace(eng, c["field"], starts)] == [0, 0, 0, 0, n]
    # one short: -1, the first n - 1 voxels, and not a word past them (a sentinel-filled buffer handed to the entry point itself)
    buf = torch.full((n + 7,), -7, dtype=torch.int32, device="cuda")
    ln = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    st = torch.as_tensor(far.astype(np.int32)).cuda()
    rc = _ffi.lib().isdf_route_trace(_ffi.ptr(c["field"].dist), *free.shape, _ffi.ptr(st), 1, n - 1, _ffi.ptr(buf), _ffi.ptr(ln), None)
    torch.cuda.synchronize()
    assert rc == 0 and ln.item() == -1
    assert buf[:n - 1].tolist() == want[:n - 1] and (buf[n - 1:] == -7).all()
    # a field that is not a fixed point: no neighbour explains the start's value
    broken = c["field"].dist.clone()
    broken[tuple(far)] += 1
    path, length = eng.route_trace(broken, torch.as_tensor(far.astype(np.int32)), n)
    assert length.tolist() == [-1] and path[0, 0].item() == want[0]


# ---- end to end: the analytic room with a partition wall; the door is z < 1.2 -------------------------------------------------
WALL_LO, WALL_HI = (2.85, 0.0, 1.2), (3.15, 3.0, 5.0)
START, GOAL, RADIUS, VOXEL, DIMS = (1.0, 1.5, 4.0), (5.0, 1.5, 4.0), 0.15, 0.1, (60, 30, 50)
GRID = np.array([[VOXEL, 0, 0, VOXEL / 2], [0, VOXEL, 0, VOXEL / 2], [0, 0, VOXEL, VOXEL / 2]])      # voxel (i, j, k) -> its centre


def scene_sdf(p):
    """float64 numpy: min(synthetic.gt_sdf, the box SDF of the wall)"""
    p = np.asarray(p, np.float64)
    q = np.maximum(np.array(WALL_LO) - p, p - np.array(WALL_HI))
    box = np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)
    return np.minimum(synthetic.gt_sdf(p), box)


def scene_field(pts):
    """(sdf, grad) float32 on pts' device: scene_sdf restated in torch float64, its gradient by differentiating the closed form"""
    p = pts.detach().to(torch.float64).requires_grad_(True)
    t = lambda v: torch.tensor(np.asarray(v, np.float64), dtype=torch.float64, device=p.device)
    with torch.enable_grad():
        d = torch.minimum(p - t(synthetic.ROOM_LO), t(synthetic.ROOM_HI) - p).min(-1).values
        for c, r in synthetic.SPHERES:
            d = torch.minimum(d, torch.linalg.norm(p - t(c), dim=-1) - r)
        for lo, hi in list(synthetic.BOXES) + [(WALL_LO, WALL_HI)]:
            q = torch.maximum(t(lo) - p, p - t(hi))
            d = torch.minimum(d, torch.linalg.norm(torch.clamp(q, min=0.0), dim=-1) + torch.clamp(q.max(-1).values, max=0.0))
        g, = torch.autograd.grad(d.sum(), p)
    return d.detach().to(torch.float32), g.to(torch.float32)


@pytest.fixture(scope="module")
def scene_free():
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in DIMS], indexing="ij"), -1).reshape(-1, 3)
    centres = idx @ GRID[:, :3].T + GRID[:, 3]
    return routing.free_space(torch.from_numpy(scene_sdf(centres).reshape(DIMS)), RADIUS, voxel=VOXEL).cuda()


def test_scene_field_is_the_numpy_closed_form():
    rng = np.random.RandomState(0)
    p = rng.uniform(synthetic.ROOM_LO, synthetic.ROOM_HI, (4096, 3))
    sdf, grad = scene_field(torch.from_numpy(p).cuda())
    assert np.allclose(sdf.cpu().numpy(), scene_sdf(p), atol=1e-6)
    norm = np.linalg.norm(grad.cpu().numpy(), axis=-1)
    assert (np.abs(norm - 1) < 1e-5).mean() > 0.99                                     # a distance field: unit gradient off its creases


def test_plan_path_alone_finds_no_way_round_the_wall(eng):
    """the gap this feature closes: every default seed of plan_path crosses the wall and stays in collision"""
    res, best = planning.plan_path(eng, START, GOAL, radii=RADIUS, field=scene_field)
    print("plan_path: in_collision per seed %s" % res.records.in_collision.astype(int).tolist())
    assert best is None and (res.records.in_collision > 0).all()


def test_the_route_clears_the_radius_on_the_exact_field(eng, scene_free):
    line = routing.route(eng, scene_free, GRID, START, GOAL)
    assert line is not None and line[0].tolist() == list(START) and line[-1].tolist() == list(GOAL)
    mid = 0.5 * (line[1:] + line[:-1])
    d = scene_sdf(np.concatenate([line, mid]))
    length = np.linalg.norm(np.diff(line, axis=0), axis=1).sum()
    print("route: %d vertices, %.2f m, least clearance %.4f m (radius %.2f), lowest z %.2f" % (len(line), length, d.min(), RADIUS,
                                                                                            line[:, 2].min()))
    assert (d > RADIUS).all()
    assert line[:, 2].min() < 1.2 and (np.linalg.norm(np.diff(line[1:-1], axis=0), axis=1) <= VOXEL * 3 ** 0.5 + 1e-9).all()
    # one field, several starts: the second lies inside the wall
    both = routing.routes(eng, scene_free, GRID, [START, (3.0, 1.5, 3.0)], GOAL)
    assert np.array_equal(both[0], line) and both[1] is None


def test_plan_route_returns_a_collision_free_trajectory_through_the_door(eng, scene_free):
    res, best, line = routing.plan_route(eng, START, GOAL, scene_free, GRID, radii=RADIUS, field=scene_field)
    assert best is not None and line is not None and res.x.shape == (8, 64, 3)
    r = res.records
    print("plan_route: best %d of 8 (%s after %d iterations): clearance %.4f m, length %.2f m; in_collision per seed %s" % (
        best, res.reason[best], res.iterations, r.min_clearance[best], r.length[best], r.in_collision.astype(int).tolist()))
    assert r.in_collision[best] == 0 and r.min_clearance[best] >= 0.0 and res.state[best] != planning.INVALID
    x = res.x[best].cpu().numpy()
    assert x[0].tolist() == list(np.float32(START)) and x[-1].tolist() == list(np.float32(GOAL)) and x[:, 2].min() < 1.2


def test_a_sealed_goal_has_no_route(eng, scene_free):
    g = routing.snap(GRID, GOAL)[0]
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in DIMS], indexing="ij"), -1)
    shell = torch.from_numpy(np.abs(idx - g).max(-1) == 3).cuda()                       # a closed box of blocked voxels round the goal
    sealed = torch.where(shell, torch.zeros_like(scene_free), scene_free)
    assert sealed[tuple(g)] == 1
    assert routing.plan_route(eng, START, GOAL, sealed, GRID, radii=RADIUS, field=scene_field) == (None, None, None)
    assert routing.route(eng, sealed, GRID, START, GOAL) is None


def test_masks_from_the_net_and_from_the_voxel_baseline(eng):
    """plumbing (the net is randomly initialised, the volume holds two hand-set voxels): the masks are free_space of the fields"""
    from isdf_amd import fusion, mesh
    dims, A = (5, 6, 7), np.array([[0.5, 0, 0, 0.3], [0, 0.5, 0, 0.2], [0, 0, 0.5, 0.1]], np.float32)
    m = routing.map_free_space(eng, dims, A, 0.01)
    sdf = eng.sdf_eval(mesh.grid_points(dims, A, "cuda")).reshape(dims)
    assert m.dtype == torch.uint8 and tuple(m.shape) == dims and m.is_contiguous() and torch.equal(m, (sdf > 0.01).to(torch.uint8))
    assert torch.equal(routing.map_free_space(eng, dims, A, 0.01, voxel=0.5), (sdf > 0.01 + routing.margin(0.5)).to(torch.uint8))
    vol = fusion.TsdfVolume((6, 5, 4), 0.1, (0.0, 0.0, 0.0), 0.4, "cuda")
    assert not routing.volume_free_space(eng, vol, 0.0).any()                  # nothing was measured: everything is blocked ...
    assert routing.volume_free_space(eng, vol, 0.0, unknown_free=True).all()    # ... unless the caller says otherwise
    vol.weight[1:5, 1:4, 1:3] = 1.0
    vol.tsdf[1:5, 1:4, 1:3] = 0.4
    vol.tsdf[2, 2, 1] = -0.05                                                   # one occupied voxel
    free = routing.volume_free_space(eng, vol, 0.05)
    want = (fusion.full_sdf(eng, vol) > 0.05) & (vol.weight > 0)
    assert torch.equal(free, want.to(torch.uint8)) and free[2, 2, 1] == 0 and free[4, 3, 2] == 1 and free[0, 0, 0] == 0
    assert free.sum() < (vol.weight > 0).sum()
