"""Host-side checks of exploration: the label model against scipy.ndimage.label, the walk model against densely sampled float64
rays, the batched walk model against the per-ray one on the views of the GPU tests, and the parts of isdf_amd.explore that run on
the host, over a stand-in Engine backed by the models (tests/explore_model.StubEngine)."""
import types

import numpy as np
import pytest
import torch

from isdf_amd import _ffi, explore, fusion, synthetic
from tests import explore_model as em

CAM = types.SimpleNamespace(**em.VIEW_CAM)


def test_constants_are_the_binding_s():
    assert (em.UNKNOWN, em.FREE, em.OCCUPIED) == (_ffi.VOXEL_UNKNOWN, _ffi.VOXEL_FREE, _ffi.VOXEL_OCCUPIED) == (0, 1, 2)
    assert em.NONE == _ffi.FRONTIER_NONE == explore.NONE and em.RECORD == _ffi.FRONTIER_RECORD


@pytest.mark.parametrize("name", ["thin", "random", "corner_chain", "edge_chain", "corner_touch", "corner_apart", "serpentine",
                                  "no_frontier", "face_voxel"])
def test_model_labels_equal_scipy_components_with_least_index_labels(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    state = em.label_grids()[name]
    mask, lab = em.frontier_mask(state), em.labels(state)
    comp, m = ndimage.label(mask, structure=np.ones((3, 3, 3), int))
    assert (lab[~mask] == em.NONE).all()
    index = np.arange(mask.size).reshape(mask.shape)
    for c in range(1, m + 1):
        assert (lab[comp == c] == index[comp == c].min()).all()
    counts, rec = em.cluster_records(lab)
    assert counts.tolist() == [m, mask.sum(), 0] and len(rec) == m
    assert np.array_equal(rec[:, 1], np.bincount(comp[mask], minlength=m + 1)[1:][np.argsort([index[comp == c].min() for c in range(1, m + 1)])])


def test_the_grids_have_what_the_gpu_tests_rely_on():
    g = em.label_grids()
    count = lambda name: em.cluster_records(em.labels(g[name]))[0].tolist()
    assert count("one_unknown") == count("one_free") == count("one_occupied") == [0, 0, 0]
    assert count("no_frontier") == count("face_voxel") == [0, 0, 0]
    assert count("corner_chain") == count("edge_chain") == [1, 17, 0]
    assert count("corner_touch") == [1, 2, 0] and count("corner_apart") == [2, 2, 0]
    assert count("serpentine")[0] == 1 and count("serpentine")[1] == (g["serpentine"] == em.FREE).sum() > 1000
    assert count("thin") == [6, 6, 0]                       # 1, 6, 9, 19, 21, 38: no two adjacent; 29 and 31 touch the occupied one only
    r = count("random")
    assert r[0] > 1 and r[1] > 100
    # a label that is not a root: an orphan, and it joins no record
    lab = em.labels(g["corner_apart"])
    roots = np.flatnonzero(lab.reshape(-1) < em.NONE)
    lab.reshape(-1)[roots[1]] = roots[1] - 1
    counts, rec = em.cluster_records(lab)
    assert counts.tolist() == [1, 2, 1] and rec[:, 1].tolist() == [1]
    assert em.cluster_records(em.labels(g["random"]), max_clusters=r[0] - 1)[1] is None


def test_walk_model_visits_every_cell_a_dense_float64_ray_spends_time_in():
    """the header's sequence on random rays, with zero components and origins on cell boundaries and centres: consecutive cells
    differ by one unit step, and every cell a float64 ray sampled at 5e-4 spends more than 2e-3 of parameter in is visited"""
    rng = np.random.RandomState(0)
    dims = (9, 10, 11)
    f32 = np.float32
    for n in range(300):
        g0 = rng.uniform(-4, 14, 3).astype(f32)
        d = rng.standard_normal(3).astype(f32) * f32(rng.choice([0.5, 3.0, 20.0]))
        kind = rng.randint(0, 6)
        if kind == 0:
            d[rng.randint(3)] = 0
        elif kind == 1:
            d[rng.choice(3, 2, replace=False)] = 0
        elif kind == 2:
            g0 = (np.round(g0) + f32(0.5)).astype(f32)
        elif kind == 3:
            g0 = np.round(g0).astype(f32)
            d[rng.randint(3)] = 0
        t_min, t_max = f32(rng.choice([0.0, 0.3])), f32(rng.choice([np.inf, 5.0, 0.8]))
        visited = [c for c, _ in em.walk_cells(g0, d, dims, t_min, t_max)]
        assert len(visited) <= sum(dims)
        for a, b in zip(visited[:-1], visited[1:]):
            assert np.abs(np.subtract(a, b)).sum() == 1, (g0, d)
        t = np.linspace(float(t_min), float(min(t_max, 60.0)), 120001)
        pos = np.floor(g0.astype(np.float64) + t[:, None] * d.astype(np.float64) + 0.5).astype(np.int64)
        inside = ((pos >= 0) & (pos < np.array(dims))).all(1)
        ids, cnt = np.unique(np.ravel_multi_index(pos[inside].T, dims), return_counts=True)
        seen = {int(np.ravel_multi_index(c, dims)) for c in visited}
        missed = [i for i, c in zip(ids, cnt) if c * (t[1] - t[0]) > 2e-3 and i not in seen]
        assert not missed, (g0, d, t_min, t_max, missed)


def test_walk_model_closed_forms():
    f32 = np.float32
    # along +k through the centre line of a 3 x 3 x 5 grid from outside: five cells, entered at the cell faces
    cells = em.walk_cells(f32([1, 1, -3]), f32([0, 0, 2]), (3, 3, 5))
    assert [c for c, _ in cells] == [(1, 1, k) for k in range(5)]
    assert [float(t) for _, t in cells] == [1.25, 1.75, 2.25, 2.75, 3.25]
    # an eye exactly on a boundary plane belongs to the upper cell: [a - 0.5, a + 0.5)
    assert em.walk_cells(f32([0.5, 1, -3]), f32([0, 0, 2]), (3, 3, 5))[0][0] == (1, 1, 0)
    assert em.walk_cells(f32([-0.5, 1, -3]), f32([0, 0, 2]), (3, 3, 5))[0][0] == (0, 1, 0)
    assert em.walk_cells(f32([2.5, 1, -3]), f32([0, 0, 2]), (3, 3, 5)) == []              # n - 0.5 is outside
    assert em.walk_cells(f32([1, 1, -3]), f32([0, 0, -2]), (3, 3, 5)) == []               # looking away
    assert em.walk_cells(f32([1, np.nan, -3]), f32([0, 0, 2]), (3, 3, 5)) == []
    assert [c for c, _ in em.walk_cells(f32([1, 1, -3]), f32([0, 0, 2]), (3, 3, 5), 2.0, 3.0)] == [(1, 1, 1), (1, 1, 2), (1, 1, 3)]
    state = np.full((3, 3, 5), em.UNKNOWN, np.uint8)
    state[:, :, 3] = em.OCCUPIED
    assert em.walk_ray(state, f32([1, 1, -3]), f32([0, 0, 2])) == (3, f32(2.75), [20, 21, 22])
    # ties go to the lowest axis: the exact diagonal steps i, then j, then k
    assert [c for c, _ in em.walk_cells(f32([0, 0, 0]), f32([1, 1, 1]), (2, 2, 2))] == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)]


def test_the_batched_walk_model_equals_the_per_ray_model_on_the_views_of_the_gpu_tests():
    state = em.random_state(em.VIEW_DIMS)
    names, T = em.view_poses()
    for t_min, t_max in ((0.0, np.inf), (0.35, np.inf), (0.0, 0.6), (0.3, 0.5)):
        a = em.view_gain_by_rays(state, em.VIEW_ORIGIN, em.VIEW_SPACING, T, em.VIEW_CAM, em.VIEW_H, em.VIEW_W, t_min, t_max)
        b = em.view_gain(state, em.VIEW_ORIGIN, em.VIEW_SPACING, T, em.VIEW_CAM, em.VIEW_H, em.VIEW_W, t_min, t_max)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (t_min, t_max)
    unknown, depth, distinct = b
    k = {n: i for i, n in enumerate(names)}
    for n in ("away", "nan", "inf"):
        assert not unknown[k[n]].any() and not depth[k[n]].any() and distinct[k[n]] == 0
    a = em.view_gain(state, em.VIEW_ORIGIN, em.VIEW_SPACING, T, em.VIEW_CAM, em.VIEW_H, em.VIEW_W)
    assert a[0][k["inside"]].any() and a[0][k["outside_in"]].any() and (a[2] <= a[0].sum((1, 2))).all()
    # the centre ray of an axis-aligned camera has two exactly zero components and its eye exactly where the name says
    for n in names[3:15]:
        g0, dg = em.ray_setup(T[k[n]], 3, 2, em.VIEW_CAM, em.VIEW_ORIGIN, em.VIEW_SPACING)
        assert (dg == 0).sum() == 2 and (np.mod(g0[dg == 0], 1) == (0.5 if "boundary" in n else 0.0)).all(), n
        assert a[0][k[n], 3, 2] > 0 or a[1][k[n], 3, 2] > 0, n


def test_look_at_is_the_reference_camera_frame():
    eye, target = np.array([1.0, 2.0, 0.5]), np.array([3.0, 1.0, 1.5])
    T = explore.look_at(eye, target)
    R = T[:3, :3]
    assert T.dtype == np.float64 and np.allclose(R.T @ R, np.eye(3), atol=1e-12) and np.linalg.det(R) > 0.999
    assert np.allclose(R[:, 2], (target - eye) / np.linalg.norm(target - eye)) and np.array_equal(T[:3, 3], eye) and T[3].tolist() == [0, 0, 0, 1]
    assert R[2, 1] < 0 and abs(R[2, 0]) < 1e-12               # y points down (against up = +z), x is horizontal
    assert np.allclose(explore.look_at(eye, target, up=(0, -1, 0)), synthetic.look_at(eye, target), atol=1e-6)
    with pytest.raises(ValueError):
        explore.look_at(eye, eye)
    with pytest.raises(ValueError):
        explore.look_at(eye, eye + [0, 0, 2.0])


def test_volume_states_grids_and_rotated_grids():
    vol = fusion.TsdfVolume((3, 2, 2), 0.1, (0.0, 0.0, 0.0), 0.4, "cpu")
    vol.weight[0] = 1.0
    vol.weight[1, 0, 0] = 2.0
    vol.tsdf[0, 0, 0], vol.tsdf[0, 1, 1], vol.tsdf[0, 0, 1], vol.tsdf[1, 0, 0] = -0.1, 0.0, 0.2, 0.05
    s = explore.volume_states(vol)
    assert s.dtype == torch.uint8 and s.is_contiguous() and s.tolist() == [[[2, 1], [2, 2]], [[1, 0], [0, 0]], [[0, 0], [0, 0]]]
    assert explore.volume_states(vol, level=0.1)[1, 0, 0] == 2
    g = explore._grid(vol)
    assert g == explore.Grid((3, 2, 2), (0.1, 0.1, 0.1), (0.0, 0.0, 0.0))
    assert np.array_equal(explore.to_world(explore.Grid((2, 2, 2), (0.5, 1.0, 2.0), (1.0, 0.0, -1.0)), [[1, 1, 1], [0, 0.5, 0]]),
                          [[1.5, 1.0, 1.0], [1.0, 0.5, -1.0]])
    assert explore.voxel_of(g, [[0.05, 0.049, 0.151], [-0.06, 0.0, 0.0]]).tolist() == [[1, 0, 2], [-1, 0, 0]]
    A = np.array([[0.1, 0, 0, 1.0], [0, 0.2, 0, 2.0], [0, 0, 0.3, 3.0]])
    assert explore.grid_from_affine(4, A) == explore.Grid((4, 4, 4), (0.1, 0.2, 0.3), (1.0, 2.0, 3.0))
    assert np.array_equal(explore.index_to_world(explore.grid_from_affine(4, A)), A)
    A[0, 1] = 0.01
    with pytest.raises(ValueError):
        explore.grid_from_affine(4, A)
    for bad in (explore.Grid((4, 4, 4), (0.1, 0.0, 0.1), (0, 0, 0)), explore.Grid((4, 0, 4), 0.1, (0, 0, 0)), A):
        with pytest.raises(ValueError):
            explore._grid(bad)


def _half_known_box(n=12):
    """a box of FREE voxels with OCCUPIED walls whose far half (i >= n / 2) is UNKNOWN"""
    s = np.full((n, n, n), em.FREE, np.uint8)
    s[[0, -1]], s[:, [0, -1]], s[:, :, [0, -1]] = em.OCCUPIED, em.OCCUPIED, em.OCCUPIED
    s[n // 2:] = em.UNKNOWN
    return s


def test_frontiers_and_clusters_over_the_stub_relaunch_once_and_refuse_orphans():
    eng = em.StubEngine()
    state = em.label_grids()["random"]
    fr = explore.frontiers(eng, torch.from_numpy(state))
    assert fr.converged and fr.label.numpy().tobytes() == em.labels(state).tobytes()
    counts, rec = em.cluster_records(fr.label.numpy())
    explore._CAPACITY["cpu"] = int(counts[0]) - 1
    cl = explore.clusters(eng, fr)
    assert [c[1] for c in eng.calls] == [counts[0] - 1, counts[0] + counts[0] // 4]                # one re-launch, then none
    assert explore.clusters(eng, fr).root.tolist() == cl.root.tolist() and len(eng.calls) == 3
    assert np.array_equal(cl.root, rec[:, 0]) and np.array_equal(cl.size, rec[:, 1]) and (np.diff(cl.root) > 0).all()
    assert np.array_equal(cl.centroid, rec[:, 2:5] / rec[:, 1:2]) and cl.centroid.dtype == np.float64
    assert np.array_equal(cl.lo, rec[:, 5:8]) and np.array_equal(cl.hi, rec[:, 8:11])
    big = explore.clusters(eng, fr, min_size=3)
    assert 0 < len(big.root) < len(cl.root) and (big.size >= 3).all()
    broken = fr.label.clone()
    roots = torch.nonzero(broken.reshape(-1) < em.NONE).reshape(-1)
    broken.reshape(-1)[roots[-1]] = roots[-1] - 1 if broken.reshape(-1)[roots[-1] - 1] >= em.NONE else roots[-1] + 1
    if em.cluster_records(broken.numpy())[0][2]:
        with pytest.raises(RuntimeError):
            explore.clusters(eng, broken)
    del explore._CAPACITY["cpu"]


def test_candidate_views_stand_on_free_voxels_and_look_at_their_cluster():
    state = _half_known_box()
    grid = explore.Grid(state.shape, 0.25, (0.5, -1.0, 0.0))
    cl = explore.clusters(em.StubEngine(), explore.frontiers(em.StubEngine(), torch.from_numpy(state)))
    assert len(cl.root) == 1 and cl.size[0] == 100 and cl.centroid[0].tolist() == [5.0, 5.5, 5.5]
    cand = explore.candidate_views(state, grid, cl, n_per_cluster=16, radius=0.8, seed=3, up=(0, -1, 0))
    again = explore.candidate_views(torch.from_numpy(state), grid, cl, n_per_cluster=16, radius=0.8, seed=3, up=(0, -1, 0))
    assert np.array_equal(cand.T_WC, again.T_WC) and 0 < len(cand.cluster) < 16 and (cand.cluster == 0).all()
    centre = explore.to_world(grid, cl.centroid[0])
    for T, vox in zip(cand.T_WC, cand.voxel):
        eye = T[:3, 3]
        assert state[tuple(vox)] == em.FREE and (explore.voxel_of(grid, eye)[0] == vox).all()
        assert abs(np.linalg.norm(eye - centre) - 0.8) < 1e-12 and abs(eye[1] - centre[1]) < 1e-12     # a ring perpendicular to up
        assert np.allclose(T[:3, 2], (centre - eye) / 0.8) and np.allclose(T, explore.look_at(eye, centre, (0, -1, 0)))
    assert len(explore.candidate_views(state, grid, cl, radius=0.8, seed=4, up=(0, -1, 0)).cluster) != 16
    none = explore.candidate_views(np.where(state == em.FREE, em.OCCUPIED, state).astype(np.uint8), grid, cl)
    assert none.T_WC.shape == (0, 4, 4) and none.voxel.shape == (0, 3)


def test_view_gain_chunks_do_not_change_the_result():
    eng = em.StubEngine()
    state = torch.from_numpy(em.random_state(em.VIEW_DIMS))
    grid = explore.Grid(em.VIEW_DIMS, em.VIEW_SPACING, em.VIEW_ORIGIN)
    _, T = em.view_poses()
    whole = explore.view_gain(eng, state, grid, T, CAM, em.VIEW_H, em.VIEW_W)
    assert eng.calls == [("view_gain", len(T), True)]
    per_view = 4 * ((state.numel() + 31) // 32)
    for budget, sizes in ((1, [1] * len(T)), (per_view * 5, [5] * (len(T) // 5) + [len(T) % 5] * (len(T) % 5 > 0))):
        eng.calls.clear()
        parts = explore.view_gain(eng, state, grid, T, CAM, em.VIEW_H, em.VIEW_W, ws_budget=budget)
        assert [c[1] for c in eng.calls] == sizes
        for a, b in zip(whole, parts):
            assert torch.equal(a, b)
    eng.calls.clear()
    nod = explore.view_gain(eng, state, grid, T, CAM, em.VIEW_H, em.VIEW_W, distinct=False, ws_budget=1)
    assert eng.calls == [("view_gain", len(T), False)] and nod.distinct is None and torch.equal(nod.unknown, whole.unknown)
    empty = explore.view_gain(eng, state, grid, T[:0], CAM, em.VIEW_H, em.VIEW_W)
    assert tuple(empty.unknown.shape) == (0, em.VIEW_H, em.VIEW_W) and tuple(empty.distinct.shape) == (0,)
    with pytest.raises(ValueError):
        explore.view_gain(eng, state, explore.Grid((9, 10, 12), em.VIEW_SPACING, em.VIEW_ORIGIN), T, CAM, em.VIEW_H, em.VIEW_W)


def test_next_best_view_over_the_stub():
    eng = em.StubEngine()
    state = _half_known_box()
    grid = explore.Grid(state.shape, 0.25, (0.5, -1.0, 0.0))
    cam = types.SimpleNamespace(fx=6.0, fy=6.0, cx=5.5, cy=3.5)
    robot = explore.to_world(grid, [1, 6, 6])
    nbv = explore.next_best_view(eng, torch.from_numpy(state), grid, robot, cam, 8, 12, radius=0.8, seed=3, up=(0, -1, 0), lam=0.5)
    t = nbv.table
    assert len(t.cluster) > 0 and nbv.gain > 0 and nbv.cost >= 0 and nbv.T_WC.shape == (4, 4)
    best = int(np.argmax(t.utility))
    assert np.array_equal(nbv.T_WC, t.T_WC[best]) and nbv.gain == t.distinct[best] and nbv.cost == t.cost[best]
    assert np.array_equal(t.utility, t.distinct * np.exp(-0.5 * t.cost))
    vox = explore.voxel_of(grid, nbv.route[1:-1])
    assert (state[tuple(vox.T)] == em.FREE).all() and (np.abs(np.diff(vox, axis=0)).max(1) == 1).all()
    assert np.array_equal(nbv.route[0], robot) and np.array_equal(nbv.route[-1], nbv.T_WC[:3, 3])
    assert (vox[0] == [1, 6, 6]).all() and (vox[-1] == t.voxel[best]).all()
    dist = em.rm.dijkstra((state == em.FREE).astype(np.uint8), [[1, 6, 6]])
    assert np.array_equal(t.cost, dist[tuple(t.voxel.T)] / 3.0 * 0.25) and len(vox) <= dist[tuple(t.voxel[best])] // 3 + 1
    # the gain of the table is the model's distinct count of the same poses
    want = em.view_gain(state, grid.origin, grid.spacing, t.T_WC.astype(np.float32), vars(cam), 8, 12)[2]
    assert np.array_equal(t.distinct, want)
    # no frontier; no reachable candidate; an explicit free mask; anisotropic voxels
    none = explore.next_best_view(eng, torch.full((6, 6, 6), em.FREE, dtype=torch.uint8), explore.Grid((6, 6, 6), 0.25, (0, 0, 0)), (0, 0, 0), cam, 8, 12)
    assert none == explore.NextBestView(None, None, None, None, None)
    cut = explore.next_best_view(eng, torch.from_numpy(state), grid, explore.to_world(grid, [0, 0, 0]), cam, 8, 12, radius=0.8, seed=3,
                                 up=(0, -1, 0))
    assert cut.T_WC is None and cut.route is None and len(cut.table.cluster) == 0
    free = torch.from_numpy((state == em.FREE).astype(np.uint8))
    free[2] = 0                                                # a slab between the robot and every eye
    assert explore.next_best_view(eng, torch.from_numpy(state), grid, robot, cam, 8, 12, free=free, radius=0.8, seed=3,
                                  up=(0, -1, 0)).T_WC is None
    with pytest.raises(ValueError):
        explore.next_best_view(eng, torch.from_numpy(state), explore.Grid(state.shape, (0.25, 0.25, 0.3), (0, 0, 0)), robot, cam, 8, 12)
