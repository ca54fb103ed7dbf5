"""CPU checks of the mesh reconstruction feature (no kernel is launched):

  * the marching-cubes tables the library ships (`isdf_mc_tables`, a host copy) over all 256 cases -- edge use, closed
    triangulations inside a cell, and the crack-free property across cells;
  * the numpy oracle `tests/mc_oracle.py` (what the HIP kernels are held to) on analytic volumes: closed, correctly wound surfaces;
  * `graft()`'s bound `get_sdf_grid` / `mesh_rec` on the REAL reference `Trainer` (build container only), with an oracle-backed
    engine that also answers `marching_cubes`."""
import contextlib
import ctypes as C
import io
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

from tests import golden_util as gu
from tests import mc_oracle as mo
from tests.fake_engine import FakeEngine

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "isdf")), reason="reference checkout not present")


@pytest.fixture(scope="module")
def tables():
    from isdf_amd import build
    build.build(verbose=False)
    return mo.library_tables()


def _tris(tt, case):
    row = tt[case].astype(int)
    return [tuple(row[q:q + 3]) for q in range(0, len(row), 3) if row[q] >= 0]


def _faces_of_edge(ec):
    """cube face (axis, side) -> the four edges lying in it"""
    off = [mo.corner_offset(c) for c in range(8)]
    out = {}
    for axis in range(3):
        for side in range(2):
            out[(axis, side)] = [e for e in range(12) if off[ec[e][0]][axis] == side and off[ec[e][1]][axis] == side]
    return out


# ---- 1. the shipped tables --------------------------------------------------------------------------------------------------
def test_tables_match_the_generator_and_the_header(tables):
    from isdf_amd import _ffi, mc_tables
    ec, tt = tables
    assert ec.tolist() == [list(p) for p in mc_tables.EDGE_CORNERS]
    assert tt.tolist() == mc_tables.tri_table()
    assert _ffi.MC_MAX_TRIS == mc_tables.MAX_TRIS
    assert open(mc_tables.HEADER).read() == mc_tables.header_text()           # the committed header is the generator's output


def test_edge_table_geometry(tables):
    ec, _ = tables
    for e, (a, b) in enumerate(ec):
        d = mo.corner_offset(b) - mo.corner_offset(a)
        assert d.tolist() == np.eye(3, dtype=int)[e // 4].tolist(), e      # along axis e // 4, from the lower corner


def test_every_case_uses_exactly_its_sign_changing_edges(tables):
    ec, tt = tables
    assert _tris(tt, 0) == [] and _tris(tt, 255) == []
    for case in range(256):
        inside = [(case >> c) & 1 for c in range(8)]
        changing = {e for e in range(12) if inside[ec[e][0]] != inside[ec[e][1]]}
        used = {e for t in _tris(tt, case) for e in t}
        assert used == changing, case
        for t in _tris(tt, case):
            assert len(set(t)) == 3, (case, t)


def test_triangulation_is_closed_inside_the_cell(tables):
    """every triangle edge that does not lie in one cube face is shared by exactly two triangles of the case; the ones in a face
    (the boundary) by exactly one"""
    ec, tt = tables
    faces = _faces_of_edge(ec)

    def on_face(a, b):
        return any(a in f and b in f for f in faces.values())
    for case in range(256):
        use = {}
        for t in _tris(tt, case):
            for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                use[frozenset((a, b))] = use.get(frozenset((a, b)), 0) + 1
        for k, n in use.items():
            a, b = tuple(k)
            assert n == (1 if on_face(a, b) else 2), (case, sorted(k), n)


def test_tables_are_crack_free(tables):
    """For every cube face, the boundary segments a case leaves on it depend ONLY on that face's four corner signs -- the same for
    the cell on the face's other side, whose opposite face it is.  (A table built by complement symmetry fails this.)"""
    ec, tt = tables
    faces = _faces_of_edge(ec)
    off = [mo.corner_offset(c) for c in range(8)]
    seen = {}
    for case in range(256):
        segs = {}
        for t in _tris(tt, case):
            for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                segs.setdefault(frozenset((a, b)), []).append((a, b))
        for (axis, side), fe in faces.items():
            u, v = [a for a in range(3) if a != axis]
            corners = sorted((c for c in range(8) if off[c][axis] == side), key=lambda c: (off[c][v], off[c][u]))
            signs = tuple((case >> c) & 1 for c in corners)
            # an edge of the face, named side-independently: (its axis, its position along the other in-face axis)
            name = {e: (e // 4, int(off[ec[e][0]][v if e // 4 == u else u])) for e in fe}
            on = sorted(tuple(sorted((name[a], name[b]))) for k, uses in segs.items() if len(uses) == 1
                        for a, b in [uses[0]] if a in fe and b in fe)
            key = (axis, signs)
            assert seen.setdefault(key, on) == on, (case, axis, side, signs, on, seen[key])


def test_ambiguous_faces_cut_off_the_inside_corners(tables):
    """the face rule itself: on a face whose diagonal corners share a sign, the two inside corners are separated"""
    ec, tt = tables
    case = 0b00001001          # corners 0 and 3 inside: face k = 0 is ambiguous
    tris = _tris(tt, case)
    assert len(tris) == 2 and {frozenset(t) for t in tris} == {frozenset((0, 4, 8)), frozenset((1, 5, 11))}


# ---- 2. the oracle on analytic volumes ----------------------------------------------------------------------------------------
def _grid(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")


def test_sphere_is_closed_with_the_right_volume_and_winding(tables):
    D, r = 64, 20.0
    X, Y, Z = _grid((D, D, D))
    c = (D - 1) / 2
    vol = (np.sqrt((X - c) ** 2 + (Y - c) ** 2 + (Z - c) ** 2) - r).astype(np.float32)
    v, f, n = mo.marching_cubes(vol, 0.0, tables)
    _, cnt = mo.edge_use(f)
    assert (cnt == 2).all()
    assert mo.euler_characteristic(v, f) == 2
    vol_mc = mo.signed_volume(v, f)
    assert vol_mc > 0 and abs(vol_mc - 4 / 3 * np.pi * r ** 3) < 0.01 * 4 / 3 * np.pi * r ** 3
    radial = (v - c) / np.linalg.norm(v - c, axis=1, keepdims=True)
    assert np.einsum("ij,ij->i", n, radial).min() > 0.99                  # normals toward increasing value (outward)


def test_torus_has_euler_characteristic_zero(tables):
    D, R, r = 64, 16.0, 6.0
    X, Y, Z = _grid((D, D, D))
    c = (D - 1) / 2
    q = np.sqrt((X - c) ** 2 + (Y - c) ** 2) - R
    vol = (np.sqrt(q ** 2 + (Z - c) ** 2) - r).astype(np.float32)
    v, f, _ = mo.marching_cubes(vol, 0.0, tables)
    _, cnt = mo.edge_use(f)
    assert (cnt == 2).all() and mo.euler_characteristic(v, f) == 0
    assert mo.signed_volume(v, f) > 0


def test_noise_volume_is_watertight_away_from_the_boundary_and_hits_every_case(tables):
    D = 48
    vol = np.random.RandomState(0).standard_normal((D, D, D)).astype(np.float32)
    v, f, _ = mo.marching_cubes(vol, 0.0, tables)
    u, cnt = mo.edge_use(f)
    # an edge used once must lie in the volume's boundary: both endpoints on the same boundary plane
    a, b = v[u[:, 0]], v[u[:, 1]]
    on_plane = np.zeros(len(u), bool)
    for ax in range(3):
        for val in (0.0, D - 1.0):
            on_plane |= (a[:, ax] == val) & (b[:, ax] == val)
    assert (cnt <= 2).all()
    assert on_plane[cnt == 1].all() and (cnt[~on_plane] == 2).all()
    cases = np.zeros((D - 1,) * 3, np.int64)
    for cn in range(8):
        o = mo.corner_offset(cn)
        cases |= (vol[o[0]:o[0] + D - 1, o[1]:o[1] + D - 1, o[2]:o[2] + D - 1] < 0).astype(np.int64) << cn
    assert len(np.unique(cases)) == 256


def test_non_finite_corners_never_leave_a_dangling_face(tables):
    D = 24
    vol = np.random.RandomState(4).standard_normal((D, D, D)).astype(np.float32)
    vol.reshape(-1)[np.random.RandomState(5).randint(0, vol.size, 200)] = np.nan
    v, f, _ = mo.marching_cubes(vol, 0.0, tables)
    assert np.isfinite(v).all() and f.min() >= 0 and f.max() < len(v)


def test_grid_index_to_world_is_draw_mesh_s_chain():
    from isdf_amd.mesh import grid_index_to_world
    rng = np.random.RandomState(1)
    dim, scale = 37, np.array([1.7, 0.4, 2.2])
    T = np.eye(4)
    T[:3, :3] = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    T[:3, 3] = rng.standard_normal(3)
    v = rng.uniform(0, dim - 1, (50, 3))
    w = ((v / (dim - 1) - 0.5) * 2 * scale) @ T[:3, :3].T + T[:3, 3]        # draw3D.py:111-138, restated
    A = grid_index_to_world(dim, scale, T)
    assert A.shape == (3, 4) and A.dtype == np.float32
    np.testing.assert_allclose(v @ A[:, :3].T.astype(np.float64) + A[:, 3], w, atol=1e-5)


def test_abi8_struct_layout_and_host_entry_points(tables):
    from isdf_amd import _ffi
    lib = _ffi.lib()
    assert lib.isdf_abi_version() == 8
    assert lib.isdf_mesh_ws_bytes(1, 4, 4) == -1 and lib.isdf_mesh_ws_bytes(4, 4, 1) == -1
    assert lib.isdf_mesh_ws_bytes(2048, 1024, 1024) == -1                    # 2^31 points
    assert lib.isdf_mesh_ws_bytes(200, 200, 200) >= 4 * 200 ** 3
    assert lib.isdf_mc_tables(None, None) == 0
    # invalid arguments are refused before anything is launched
    a = _ffi.McArgs()
    assert lib.isdf_marching_cubes(None, None, None, None, 0, None, 0, None, 0, None) == -1
    a.volume, a.D0, a.D1, a.D2 = 16, 1, 4, 4
    assert lib.isdf_marching_cubes(C.byref(a), 16, None, None, 0, None, 0, 16, 1 << 20, None) == -1
    a.D0 = 4
    assert lib.isdf_marching_cubes(C.byref(a), 16, None, None, 10, None, 0, 16, 1 << 20, None) == -1   # verts NULL, max_verts 10
    assert lib.isdf_marching_cubes(C.byref(a), 16, None, None, 0, None, 0, 16, 8, None) == -3          # workspace too small


# ---- 3. the graft on the REAL reference Trainer --------------------------------------------------------------------------------
class MeshFakeEngine(FakeEngine):
    """the oracle-backed stand-in engine, plus marching cubes through tests/mc_oracle.py"""

    def marching_cubes(self, volume, level=0.0, index_to_world=None):
        v, f, n = mo.marching_cubes(volume.detach().cpu().numpy(), level, mo.library_tables(), index_to_world)
        self.calls.append("marching_cubes")
        return torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(n)


@pytest.fixture(scope="module")
def ref_mods():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden as mg
    with contextlib.redirect_stdout(io.StringIO()):
        mods = mg.import_reference()
    return mg, mods


def _grafted_trainer(mg, mods, dim=12):
    from isdf_amd.hot_path import graft
    g = gu.load("step_small_k7")
    cam, net, sc, lc = gu.cam_of(g), g["net"], gu.sample_of(g), gu.loss_of(g)
    netd = dict(H=int(net[0]), B=int(net[1]), n_freqs=int(net[2]), scale_input=float(net[3]), scale_output=float(net[4]))
    lossd = dict(bounds_method=lc.bounds_method, loss_type=lc.loss_type, trunc_weight=lc.trunc_weight,
                 trunc_distance=lc.trunc_distance, eik_weight=lc.eik_weight, eik_apply_dist=lc.eik_apply_dist,
                 grad_weight=lc.grad_weight, orien_loss=lc.orien_loss)
    with contextlib.redirect_stdout(io.StringIO()):
        tr = mg.build_trainer(mods, cam, netd, lossd, sc, (g["depth_batch"], g["normal_batch"], g["T_WC_batch"]),
                              gu.params_of(g), g["bounds_T"], float(g["noise_std"][0]))
        graft(tr, rng="torch", engine_factory=MeshFakeEngine)
    # what set_scene_properties would leave (it returns mocks under the test stubs): a small box around the fixture's scene
    T_bounds = np.linalg.inv(g["bounds_T"].astype(np.float64))
    scale = np.array([1.2, 0.9, 1.5])
    t = torch.linspace(-1.0, 1.0, dim)
    G = torch.stack(torch.meshgrid(t, t, t, indexing="ij"), -1) * torch.tensor(scale, dtype=torch.float32)   # make_3D_grid
    Tt = torch.tensor(T_bounds, dtype=torch.float32)
    tr.grid_dim, tr.grid_pc = dim, (G @ Tt[:3, :3].T + Tt[:3, 3]).reshape(-1, 3)
    tr.scene_scale_np, tr.bounds_transform_np = scale, T_bounds
    tr.chunk_size = 500
    tr.gt_scene, tr.new_grid_dim, tr.new_grid_pc, tr.crop_dist = True, None, None, 0.25
    return tr, mods


@needs_ref
def test_grafted_methods_resolve_to_the_hip_binding(ref_mods):
    from isdf_amd.hot_path import HotPath
    mg, mods = ref_mods
    tr, _ = _grafted_trainer(mg, mods)
    assert type(tr).get_sdf_grid is HotPath.get_sdf_grid and type(tr).mesh_rec is HotPath.mesh_rec
    assert type(tr).write_mesh is mods[0].Trainer.write_mesh          # follows through mesh_rec, unchanged
    assert tr._hip.ref_module is mods[0]


@needs_ref
def test_get_sdf_grid_is_one_evaluation_equal_to_the_chunked_one(ref_mods):
    mg, mods = ref_mods
    tr, _ = _grafted_trainer(mg, mods)
    fc_map = mods[3]
    d = tr.grid_dim
    want = fc_map.chunks(tr.grid_pc, tr.chunk_size, tr.sdf_map).view(d, d, d)
    with mock.patch.object(tr.sdf_map.engine, "sdf_eval", wraps=tr.sdf_map.engine.sdf_eval) as ev:
        got = tr.get_sdf_grid()
    assert ev.call_count == 1 and ev.call_args[0][0].shape[0] == d ** 3
    assert got.shape == (d, d, d) and not got.requires_grad
    np.testing.assert_allclose(got.numpy(), want.detach().numpy(), rtol=1e-6, atol=1e-7)


@needs_ref
def test_mesh_rec_builds_the_world_mesh_without_the_point_cloud_when_nothing_needs_it(ref_mods):
    mg, mods = ref_mods
    tr, _ = _grafted_trainer(mg, mods)
    tr.new_grid_dim, tr.new_grid_pc = 7, torch.zeros(7 ** 3, 3)
    sdf = tr.get_sdf_grid().numpy()
    assert (sdf < 0).any() and (sdf > 0).any(), "the box must cut the surface for this test to mean anything"
    d = tr.grid_dim
    with mock.patch.object(mods[0], "trimesh") as tm, \
            mock.patch.object(type(tr), "update_vis_vars", side_effect=AssertionError("vis point cloud built")), \
            mock.patch.object(type(tr), "set_scene_properties", side_effect=AssertionError("scene re-derived")):
        out = tr.mesh_rec(crop_mesh_with_pc=False)
    assert out is tm.Trimesh.return_value and tm.Trimesh.call_count == 1
    kw = tm.Trimesh.call_args.kwargs
    v, f, n = mo.marching_cubes(sdf, 0.0)
    w = (v.astype(np.float64) / (d - 1) - 0.5) * 2 * tr.scene_scale_np                 # draw_mesh's chain, restated
    w = w @ tr.bounds_transform_np[:3, :3].T + tr.bounds_transform_np[:3, 3]
    assert len(f) > 0
    np.testing.assert_allclose(kw["vertices"], w, atol=1e-5)
    assert np.array_equal(kw["faces"], f)
    nw = n.astype(np.float64) @ np.linalg.inv(tr.bounds_transform_np[:3, :3] * (2 * tr.scene_scale_np / (d - 1)))
    nw /= np.linalg.norm(nw, axis=1, keepdims=True)
    np.testing.assert_allclose(kw["vertex_normals"], nw, atol=1e-5)
    assert out.visual.face_colors == [160, 160, 160, 255]
    assert tr.grid_dim == 7 and tr.new_grid_dim is None and tr.new_grid_pc is None       # the pending grid swapped in
    assert tr.sdf_map.engine.calls.count("marching_cubes") == 1


@needs_ref
def test_mesh_rec_crops_with_the_visualisation_point_cloud(ref_mods):
    mg, mods = ref_mods
    tr, _ = _grafted_trainer(mg, mods)
    d = tr.grid_dim
    v, f, _ = mo.marching_cubes(tr.get_sdf_grid().numpy(), 0.0)
    w = (v.astype(np.float64) / (d - 1) - 0.5) * 2 * tr.scene_scale_np
    w = w @ tr.bounds_transform_np[:3, :3].T + tr.bounds_transform_np[:3, 3]
    pc = w[: len(w) // 3] + 0.01                                 # near the first third of the vertices only
    with mock.patch.object(mods[0], "trimesh") as tm, mock.patch.object(type(tr), "_vis_pointcloud", return_value=pc) as vis:
        tr.mesh_rec(crop_mesh_with_pc=True)
    assert vis.call_count == 1
    kw = tm.Trimesh.call_args.kwargs
    from scipy.spatial import KDTree                             # the reference's crop (trainer.py:1527-1534), restated
    keep = KDTree(pc).query(w, k=1)[0] < tr.crop_dist
    fm = keep[f].any(axis=1)
    used = np.unique(f[fm])
    assert 0 < fm.sum() < len(f)
    np.testing.assert_allclose(kw["vertices"], w[used], atol=1e-5)
    remap = np.full(len(w), -1)
    remap[used] = np.arange(len(used))
    assert np.array_equal(kw["faces"], remap[f[fm]])


@needs_ref
def test_mesh_rec_rederives_the_scene_when_incremental_without_gt(ref_mods):
    mg, mods = ref_mods
    tr, _ = _grafted_trainer(mg, mods)
    tr.gt_scene, tr.incremental = False, True
    pc = np.zeros((5, 3))
    with mock.patch.object(mods[0], "trimesh") as tm, mock.patch.object(type(tr), "_vis_pointcloud", return_value=pc), \
            mock.patch.object(type(tr), "set_scene_properties") as ssp:
        tr.mesh_rec(crop_mesh_with_pc=False)
    assert ssp.call_count == 1 and ssp.call_args[0][0] is tm.PointCloud.return_value
    assert tm.PointCloud.call_args[0][0] is pc
