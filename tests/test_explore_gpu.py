"""Exploration on the device: isdf_frontier_init / isdf_frontier_relax / isdf_frontier_clusters / isdf_view_gain through Engine and
isdf_amd.explore.  Reference: tests/explore_model.py -- the frontier rule, union-find components with least-index labels, the
cluster records and the header's fp32 walk.  Labels, records and counts are integers and the depth is one stated fp32 sequence:
everything is compared bit for bit, no tolerance anywhere.  End to end: the partitioned analytic room of the routing tests, fused
from one side, then next_best_view."""
import types

import numpy as np
import pytest
import torch

from isdf_amd import _ffi, explore
from tests import explore_model as em

pytestmark = pytest.mark.gpu

NONE = _ffi.FRONTIER_NONE
CAM = types.SimpleNamespace(**em.VIEW_CAM)
GRID = explore.Grid(em.VIEW_DIMS, em.VIEW_SPACING, em.VIEW_ORIGIN)
H, W = em.VIEW_H, em.VIEW_W
f32 = np.float32


@pytest.fixture(scope="module")
def eng():
    from isdf_amd.engine import Engine, NetConfig
    return Engine(NetConfig(hidden=64, blocks=1), "cuda")


@pytest.fixture(scope="module")
def cases(eng):
    """name -> dict(state, model, fr): the model's labels and the device's (relaxed once), shared by the tests below"""
    out = {}
    for name, state in em.label_grids().items():
        out[name] = dict(state=state, model=em.labels(state), fr=explore.frontiers(eng, torch.from_numpy(state).cuda()))
    return out


GRIDS = list(em.label_grids())


@pytest.mark.parametrize("name", GRIDS)
def test_labels_equal_the_union_find_model_bit_for_bit(eng, cases, name):
    c = cases[name]
    dev = c["fr"].label.cpu().numpy()
    print("%s %s: converged %s after %d rounds; %d frontier voxels" % (name, c["state"].shape, c["fr"].converged, c["fr"].rounds,
                                                                      (c["model"] < NONE).sum()))
    assert c["fr"].converged and dev.dtype == np.int32 and dev.shape == c["state"].shape
    assert dev.tobytes() == c["model"].tobytes()
    init = eng.frontier_init(torch.from_numpy(c["state"]).cuda()).cpu().numpy()
    assert init.tobytes() == em.init_labels(c["state"]).tobytes()


def test_chains_cross_tile_corners_and_edges_and_corner_contact_joins(cases):
    for name in ("corner_chain", "edge_chain"):
        lab = cases[name]["fr"].label.cpu().numpy()
        assert (lab[lab < NONE] == 0).all() and (lab < NONE).sum() == 17                  # one component, rooted at voxel (0, 0, 0)
    touch, apart = (cases[n]["fr"].label.cpu().numpy() for n in ("corner_touch", "corner_apart"))
    assert len(np.unique(touch[touch < NONE])) == 1 and len(np.unique(apart[apart < NONE])) == 2
    for name in ("one_unknown", "one_free", "one_occupied", "no_frontier", "face_voxel"):
        f = cases[name]["fr"]
        assert (f.label == NONE).all() and f.converged and f.rounds == 1                   # the first round already changes nothing


def test_serpentine_convergence_does_not_depend_on_how_often_the_host_looks(eng, cases):
    c = cases["serpentine"]
    state = torch.from_numpy(c["state"]).cuda()
    ref, want = c["fr"], c["model"].tobytes()
    assert ref.converged and ref.rounds > 8, ref.rounds                                    # many rounds: several groups of the default 8
    assert len(np.unique(c["model"][c["model"] < NONE])) == 1
    label = ref.label.clone()
    assert eng.frontier_relax(label, 1).tolist() == [0] and label.cpu().numpy().tobytes() == want
    for every in (1, 8):
        f = explore.frontiers(eng, state, check_every=every)
        assert f.converged and f.rounds == ref.rounds and f.label.cpu().numpy().tobytes() == want, every
    short = explore.frontiers(eng, state, check_every=2, max_rounds=4)
    d = short.label.cpu().numpy()
    assert not short.converged and short.rounds == 4 and (d >= c["model"]).all() and (d > c["model"]).any()
    label = eng.frontier_init(state)
    flags = eng.frontier_relax(label, ref.rounds + 2).tolist()
    assert flags == [1] * (ref.rounds - 1) + [0] * 3 and label.cpu().numpy().tobytes() == want


@pytest.mark.parametrize("name", GRIDS)
def test_cluster_records_equal_the_model_int64_for_int64(eng, cases, name):
    c = cases[name]
    counts_m, rec_m = em.cluster_records(c["model"])
    m = int(counts_m[0])
    counts, records = eng.frontier_clusters(c["fr"].label, m + 3)
    assert counts.cpu().numpy().tobytes() == counts_m.tobytes()
    got = records.cpu().numpy()
    assert got.dtype == np.int64 and got[:m].tobytes() == rec_m.tobytes()
    again = eng.frontier_clusters(c["fr"].label, m + 3)[1].cpu().numpy()
    assert again[:m].tobytes() == got[:m].tobytes()                                        # two runs, the same bytes
    cl = explore.clusters(eng, c["fr"])
    assert np.array_equal(cl.root, rec_m[:, 0]) and np.array_equal(cl.size, rec_m[:, 1]) and np.array_equal(cl.lo, rec_m[:, 5:8])
    assert np.array_equal(cl.hi, rec_m[:, 8:11]) and np.array_equal(cl.centroid, rec_m[:, 2:5] / rec_m[:, 1:2].astype(np.float64))


def test_too_few_record_rows_give_the_counts_and_one_relaunch(eng, cases, monkeypatch):
    c = cases["thin"]
    counts_m, rec_m = em.cluster_records(c["model"])
    m = int(counts_m[0])
    assert m == 6
    records = torch.full((m - 1, _ffi.FRONTIER_RECORD), -7, dtype=torch.int64, device="cuda")
    counts = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(_ffi.lib().isdf_frontier_ws_bytes(*c["state"].shape)), dtype=torch.uint8, device="cuda")
    rc = _ffi.lib().isdf_frontier_clusters(_ffi.ptr(c["fr"].label), *c["state"].shape, _ffi.ptr(ws), ws.numel(), m - 1, _ffi.ptr(counts),
                                           _ffi.ptr(records), None)
    torch.cuda.synchronize()
    assert rc == 0 and counts.tolist() == counts_m.tolist() and (records == -7).all()      # the counts are written, the records are not
    calls = []
    real = eng.frontier_clusters
    monkeypatch.setattr(eng, "frontier_clusters", lambda label, cap: calls.append(cap) or real(label, cap))
    monkeypatch.setitem(explore._CAPACITY, str(eng.device), m - 1)
    cl = explore.clusters(eng, c["fr"])
    assert calls == [m - 1, m + m // 4] and np.array_equal(cl.root, rec_m[:, 0]) and np.array_equal(cl.size, rec_m[:, 1])
    explore.clusters(eng, c["fr"])
    assert calls == [m - 1, m + m // 4, m + m // 4]


def test_a_label_that_is_not_a_root_is_an_orphan(eng, cases):
    lab = cases["corner_apart"]["model"].copy()
    roots = np.flatnonzero(lab.reshape(-1) < NONE)
    lab.reshape(-1)[roots[1]] = roots[1] - 1                                               # points at a voxel that holds NONE
    lab.reshape(-1)[5] = lab.size + 10                                                     # and one past the grid
    counts_m, rec_m = em.cluster_records(lab)
    assert counts_m.tolist() == [1, 3, 2]
    counts, records = eng.frontier_clusters(torch.from_numpy(lab).cuda(), 4)
    assert counts.tolist() == [1, 3, 2] and records[:1].cpu().numpy().tobytes() == rec_m.tobytes()
    with pytest.raises(RuntimeError):
        explore.clusters(eng, torch.from_numpy(lab).cuda())


# ---- view gain ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def views(eng):
    """the random (9, 10, 11) state, the poses, and the device's and the model's results over the whole t range"""
    state = em.random_state(em.VIEW_DIMS)
    names, T = em.view_poses()
    dev = explore.view_gain(eng, torch.from_numpy(state).cuda(), GRID, T, CAM, H, W)
    return dict(state=state, names=names, T=T, dev=dev, model=em.view_gain(state, em.VIEW_ORIGIN, em.VIEW_SPACING, T, em.VIEW_CAM, H, W))


def _same(dev, model, what=""):
    for name, a, b in zip(("unknown", "depth", "distinct"), dev, model):
        a = a.cpu().numpy()
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        assert a.tobytes() == b.tobytes(), (what, name, np.argwhere(a.view(np.int32) != b.view(np.int32))[:5].tolist())


def test_view_gain_equals_the_walk_model_bit_for_bit(views):
    _same(views["dev"], views["model"])
    unknown, depth, distinct = (t.cpu().numpy() for t in views["dev"])
    k = {n: i for i, n in enumerate(views["names"])}
    for n in ("away", "nan", "inf"):
        assert not unknown[k[n]].any() and not depth[k[n]].any() and distinct[k[n]] == 0, n
    assert unknown[k["inside"]].any() and unknown[k["outside_in"]].any() and (depth > 0).any()
    assert (distinct <= unknown.sum((1, 2))).all() and (distinct[:2] > 0).all()
    print("distinct per view %s; unknown per view %s" % (distinct.tolist(), unknown.sum((1, 2)).tolist()))


@pytest.mark.parametrize("t_min,t_max", [(0.35, np.inf), (0.0, 0.6), (0.3, 0.5)])
def test_view_gain_with_t_min_inside_the_grid_and_t_max_mid_grid(eng, views, t_min, t_max):
    dev = explore.view_gain(eng, torch.from_numpy(views["state"]).cuda(), GRID, views["T"], CAM, H, W, t_min=t_min, t_max=t_max)
    model = em.view_gain(views["state"], em.VIEW_ORIGIN, em.VIEW_SPACING, views["T"], em.VIEW_CAM, H, W, t_min, t_max)
    _same(dev, model, (t_min, t_max))
    assert model[0].sum() < views["model"][0].sum() and model[0].sum() > 0                 # the range really cuts rays short


def test_view_gain_chunks_partial_bitmap_words_no_views_and_no_distinct(eng, views):
    state = torch.from_numpy(views["state"]).cuda()
    one = explore.view_gain(eng, state, GRID, views["T"], CAM, H, W, ws_budget=1)          # one view per chunk
    for a, b in zip(one, views["dev"]):
        assert torch.equal(a, b)
    nod = explore.view_gain(eng, state, GRID, views["T"], CAM, H, W, distinct=False)
    assert nod.distinct is None and torch.equal(nod.unknown, views["dev"].unknown) and torch.equal(nod.depth, views["dev"].depth)
    empty = explore.view_gain(eng, state, GRID, views["T"][:0], CAM, H, W)
    assert tuple(empty.unknown.shape) == (0, H, W) and tuple(empty.depth.shape) == (0, H, W) and tuple(empty.distinct.shape) == (0,)
    # n = 198: 7 words per view, the last one partial, and the views' words cross 32
    dims, spacing, origin = (33, 2, 3), (0.1, 0.5, 0.3), (-1.6, -0.2, 0.1)
    s = em.random_state(dims, seed=9)
    s[s == em.OCCUPIED] = em.UNKNOWN                                                        # rays run the whole length
    T = np.stack([em.axis_pose(0, 1, f32([-2.0, 0.05, 0.4])), em.axis_pose(0, -1, f32([2.0, 0.1, 0.35])),
                  explore.look_at([0.0, 3.0, 0.4], [0.1, 0.0, 0.4]).astype(f32)] * 4)
    cam = dict(fx=12.0, fy=12.0, cx=2.0, cy=3.0)
    dev = explore.view_gain(eng, torch.from_numpy(s).cuda(), explore.Grid(dims, spacing, origin), T, types.SimpleNamespace(**cam), H, W)
    model = em.view_gain(s, origin, spacing, T, cam, H, W)
    _same(dev, model, "33x2x3")
    assert model[2][0] > 32 and model[2].tolist() == model[2][:3].tolist() * 4


def test_view_gain_closed_forms(eng, views):
    k = {n: i for i, n in enumerate(views["names"])}
    T = views["T"]
    free = torch.full(em.VIEW_DIMS, em.FREE, dtype=torch.uint8, device="cuda")
    g = explore.view_gain(eng, free, GRID, T, CAM, H, W)
    assert not g.unknown.any() and not g.depth.any() and not g.distinct.any()              # an all-free grid: zeros
    unk = torch.full(em.VIEW_DIMS, em.UNKNOWN, dtype=torch.uint8, device="cuda")
    g = explore.view_gain(eng, unk, GRID, T, CAM, H, W)
    for axis in range(3):
        for sign in "+-":
            for kind in ("boundary", "centre"):
                b = k["%s%s_%s" % (sign, "ijk"[axis], kind)]
                assert g.unknown[b, 3, 2].item() == em.VIEW_DIMS[axis], (axis, sign, kind)     # the side length on the centre ray
    assert (g.distinct.cpu() <= g.unknown.sum((1, 2)).cpu()).all() and not g.depth.any()
    slab = torch.full(em.VIEW_DIMS, em.FREE, dtype=torch.uint8, device="cuda")
    slab[:, :, 5] = 7                                                                      # any value >= 2 is occupied
    b = k["+k_centre"]
    g = explore.view_gain(eng, slab, GRID, T[b:b + 1], CAM, H, W)
    g0 = (T[b, 2, 3] - f32(em.VIEW_ORIGIN[2])) / f32(em.VIEW_SPACING[2])
    inv = f32(1) / (f32(1) / f32(em.VIEW_SPACING[2]))
    want = (f32(4.5) - g0) * inv
    assert want.dtype == f32 and g.depth[0, 3, 2].cpu().numpy().tobytes() == want.tobytes()
    assert abs(float(want) - (3.0 + 4.5) * em.VIEW_SPACING[2]) < 1e-5 and not g.unknown.any()


def test_map_states_is_visibility_and_the_sign_of_the_net(eng):
    """plumbing (the net is randomly initialised): known iff metrics.visible_points counts a frame, occupied iff sdf <= clearance"""
    from isdf_amd import mesh, metrics
    grid = explore.Grid((6, 5, 7), 0.5, (0.4, 0.3, 0.2))
    cam = types.SimpleNamespace(**em.ROOM_CAM)
    T = em.room_first_views()[:2]
    depth = torch.from_numpy(np.stack([em.room_depth(t) for t in T])).cuda()
    s = explore.map_states(eng, grid, T, depth, cam, trunc=0.2, clearance=0.01)
    pts = mesh.grid_points(grid.dims, explore.index_to_world(grid).astype(np.float32), "cuda")
    count = metrics.visible_points(eng, pts, T, depth, cam, trunc=0.2)[0].reshape(grid.dims)
    occupied = (eng.sdf_eval(pts).reshape(grid.dims) <= 0.01)
    want = torch.where(count > 0, torch.where(occupied, em.OCCUPIED, em.FREE), em.UNKNOWN).to(torch.uint8)
    assert s.dtype == torch.uint8 and s.is_contiguous() and tuple(s.shape) == grid.dims and torch.equal(s, want)
    assert (s == em.UNKNOWN).any() and (s != em.UNKNOWN).any()


# ---- end to end: the partitioned room, fused from one side --------------------------------------------------------------------
def test_next_best_view_in_the_room_sees_new_space(eng):
    """fuse three views from the robot's place, choose the next view, go there and look: the unknown volume must fall.  On the host
    models (tests/explore_model.StubEngine over the same state bytes) the chosen view has distinct = 23916 and integrating the
    frame it sees clears 14683 unknown voxels, 0.614 of distinct (the rest lies behind surfaces the map does not know yet, or
    between the pixels' frusta); asserted at half of distinct, a margin of 0.11 below the models' figure."""
    vol, cam = em.room_volume(eng, "cuda")
    state = explore.volume_states(vol)
    host = state.cpu().numpy()
    assert (host == em.UNKNOWN).mean() > 0.5 and (host == em.OCCUPIED).any()               # one side only
    nbv = explore.next_best_view(eng, state, vol, em.ROOM_ROBOT, cam, cam.H, cam.W, **em.ROOM_NBV)
    eye = explore.voxel_of(vol, nbv.T_WC[:3, 3])[0]
    assert host[tuple(eye)] == em.FREE and nbv.gain > 0
    vox = explore.voxel_of(vol, nbv.route[1:-1])
    assert (host[tuple(vox.T)] == em.FREE).all() and (vox[-1] == eye).all() and (np.abs(np.diff(vox, axis=0)).max(1) == 1).all()
    assert nbv.route[0].tolist() == list(em.ROOM_ROBOT) and np.array_equal(nbv.route[-1], nbv.T_WC[:3, 3])
    # the same pipeline on the stub, over the same state bytes: the same table, row for row and bit for bit
    stub = em.StubEngine()
    ref = explore.next_best_view(stub, torch.from_numpy(host), vol, em.ROOM_ROBOT, cam, cam.H, cam.W, **em.ROOM_NBV)
    for name, a, b in zip(ref.table._fields, nbv.table, ref.table):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    assert np.array_equal(nbv.T_WC, ref.T_WC) and nbv.gain == ref.gain and nbv.cost == ref.cost and np.array_equal(nbv.route, ref.route)
    before, after = em.room_look(eng, vol, cam, nbv.T_WC)
    print("next best view: %d candidates, distinct %d, cost %.2f m; unknown %d -> %d (%.3f of distinct)" % (
        len(nbv.table.cluster), nbv.gain, nbv.cost, before, after, (before - after) / nbv.gain))
    assert after < before and before - after >= 0.5 * nbv.gain
