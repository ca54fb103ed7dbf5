"""HIP marching cubes (`isdf_marching_cubes`, isdf_amd/csrc/mesh.hip) against the numpy oracle `tests/mc_oracle.py`: identical
faces, vertices and normals within 1e-5, on analytic volumes, edge cases, the world affine and the trained default network."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import golden_util as gu
from tests import mc_oracle as mo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tables():
    from isdf_amd import build
    build.build(verbose=False)
    return mo.library_tables()


def _grid(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")


def sphere(D=64, r=20.0):
    X, Y, Z = _grid((D, D, D))
    c = (D - 1) / 2
    return (np.sqrt((X - c) ** 2 + (Y - c) ** 2 + (Z - c) ** 2) - r).astype(np.float32)


def torus(D=64, R=16.0, r=6.0):
    X, Y, Z = _grid((D, D, D))
    c = (D - 1) / 2
    q = np.sqrt((X - c) ** 2 + (Y - c) ** 2) - R
    return (np.sqrt(q ** 2 + (Z - c) ** 2) - r).astype(np.float32)


def noise(shape=(48, 48, 48), seed=0):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


def _hip(vol, level=0.0, A=None):
    from isdf_amd import mesh
    v, f, n = mesh.marching_cubes(torch.from_numpy(vol).cuda(), level, A)
    torch.cuda.synchronize()
    return v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()


def _assert_same(vol, tables, level=0.0, A=None):
    v, f, n = _hip(vol, level, A)
    rv, rf, rn = mo.marching_cubes(vol, level, tables, A)
    assert v.shape == rv.shape and f.shape == rf.shape, (v.shape, rv.shape, f.shape, rf.shape)
    assert f.dtype == np.int32 and np.array_equal(f, rf)
    np.testing.assert_allclose(v, rv, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(n, rn, rtol=1e-5, atol=1e-5)
    return v, f, n


@pytest.mark.parametrize("name", ["sphere", "torus", "noise", "box37x64x50", "single_cell"])
def test_hip_matches_oracle(tables, name):
    vol = {"sphere": sphere, "torus": torus, "noise": noise,
           "box37x64x50": lambda: noise((37, 64, 50), seed=3) + 0.3,
           "single_cell": lambda: np.array([-1, 2, 3, -4, 5, -6, 7, 0.5], np.float32).reshape(2, 2, 2)}[name]()
    v, f, n = _assert_same(vol, tables)
    assert len(f) > 0
    if name == "sphere":
        assert mo.euler_characteristic(v, f) == 2


def test_corners_exactly_at_level_count_as_outside(tables):
    vol = np.round(noise((20, 21, 22), seed=5) * 2).astype(np.float32)     # many exact zeros
    assert (vol == 0).sum() > 1000
    _assert_same(vol, tables, level=0.0)
    _assert_same(vol, tables, level=1.0)


def test_nan_and_inf_corners_are_skipped_consistently(tables):
    vol = sphere(40, 12.0)
    rng = np.random.RandomState(9)
    idx = rng.randint(0, vol.size, 300)
    vol.reshape(-1)[idx[:200]] = np.nan
    vol.reshape(-1)[idx[200:]] = np.inf
    v, f, n = _assert_same(vol, tables)
    assert f.min() >= 0 and f.max() < len(v)


def test_index_to_world_affine_and_normals(tables):
    from isdf_amd.mesh import grid_index_to_world
    T = np.eye(4)
    c, s = np.cos(0.7), np.sin(0.7)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = [0.5, -2.0, 1.25]
    A = grid_index_to_world(64, [3.0, 0.7, 1.6], T)          # anisotropic scale: normals need the inverse transpose
    vol = sphere()
    v, f, n = _assert_same(vol, tables, A=A)
    vi, _, ni = mo.marching_cubes(vol, 0.0, tables)
    np.testing.assert_allclose(v, vi @ A[:, :3].T + A[:, 3], rtol=1e-5, atol=1e-4)
    m = ni @ np.linalg.inv(A[:, :3].astype(np.float64))     # (A^-T n)^T = n^T A^-1
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    np.testing.assert_allclose(n, m, atol=1e-5)
    # winding still agrees with the normals after the affine (det > 0): face normals point along the vertex normals
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (np.einsum("ij,ij->i", fn, n[f].sum(1)) > 0).mean() > 0.99


def test_two_runs_are_bit_identical(tables):
    vol = noise((60, 50, 40), seed=11)
    a = _hip(vol)
    b = _hip(vol)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_overflow_reports_counts_and_the_wrapper_relaunches_once(tables):
    from isdf_amd import _ffi
    from isdf_amd.mesh import Mesher
    vol = noise((40, 40, 40), seed=2)
    rv, rf, rn = mo.marching_cubes(vol, 0.0, tables)
    m = Mesher("cuda")
    v, f, n = m(torch.from_numpy(vol).cuda(), capacity=(16, 16))       # too small: counts, then one exact re-launch
    assert m.launches == 2
    assert np.array_equal(f.cpu().numpy(), rf)
    np.testing.assert_allclose(v.cpu().numpy(), rv, rtol=1e-5, atol=1e-5)
    # the raw entry point: counts always written, outputs untouched when they do not fit
    lib = _ffi.lib()
    d = torch.from_numpy(vol).cuda()
    a = _ffi.McArgs()
    a.volume, a.D0, a.D1, a.D2, a.level = d.data_ptr(), 40, 40, 40, 0.0
    ws = torch.empty(int(lib.isdf_mesh_ws_bytes(40, 40, 40)), dtype=torch.uint8, device="cuda")
    counts = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    verts = torch.full((100, 3), 123.0, device="cuda")
    faces = torch.full((100, 3), -5, dtype=torch.int32, device="cuda")
    rc = lib.isdf_marching_cubes(C.byref(a), _ffi.ptr(counts), _ffi.ptr(verts), None, 100, _ffi.ptr(faces), 100, _ffi.ptr(ws),
                                 ws.numel(), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [len(rv), len(rf)]
    assert bool((verts == 123.0).all()) and bool((faces == -5).all())
    # a second call on the SAME workspace (nothing re-armed in between) gives the same counts
    m2 = Mesher("cuda")
    for _ in range(2):
        v2, f2, _ = m2(d)
        assert np.array_equal(f2.cpu().numpy(), rf)
    assert m2.launches in (2, 3)


def test_argument_checks():
    from isdf_amd import _ffi
    lib = _ffi.lib()
    assert lib.isdf_mesh_ws_bytes(1, 4, 4) == -1 and lib.isdf_mesh_ws_bytes(2048, 1024, 1024) == -1
    assert lib.isdf_mesh_ws_bytes(2, 2, 2) > 0
    a = _ffi.McArgs()
    d = torch.zeros(8, device="cuda")
    a.volume, a.D0, a.D1, a.D2 = d.data_ptr(), 2, 2, 2
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert lib.isdf_marching_cubes(C.byref(a), _ffi.ptr(cnt), None, None, 0, None, 0, None, 0, None) == -3     # no workspace
    a.has_transform = 1                                                                                       # singular affine
    ws = torch.empty(int(lib.isdf_mesh_ws_bytes(2, 2, 2)), dtype=torch.uint8, device="cuda")
    assert lib.isdf_marching_cubes(C.byref(a), _ffi.ptr(cnt), None, None, 0, None, 0, _ffi.ptr(ws), ws.numel(), None) == -1


# ---- the trained default network (fixture `trained_default`) on a grid over its bounds box
def _bounds_grid(g, dim):
    """what set_scene_properties (trainer.py:103-148) makes of this fixture: the PE transform maps world to the box frame, so its
    inverse is the bounds transform; extents from the fixture's sample points, grown by 1 / 0.9 like the reference"""
    T_bounds = np.linalg.inv(g["bounds_T"].astype(np.float64))
    pc = g["eval/pc"].reshape(-1, 3).astype(np.float64)
    local = (pc - T_bounds[:3, 3]) @ T_bounds[:3, :3]
    extents = 2 * np.abs(local).max(0)
    scale = extents / (2 * 0.9)
    t = torch.linspace(-1.0, 1.0, dim, dtype=torch.float32)
    G = torch.stack(torch.meshgrid(t, t, t, indexing="ij"), -1) * torch.tensor(scale, dtype=torch.float32)   # make_3D_grid
    Tt = torch.tensor(T_bounds, dtype=torch.float32)
    pts = G @ Tt[:3, :3].T + Tt[:3, 3]
    return pts.reshape(-1, 3), scale, T_bounds


def _engine(g):
    from isdf_amd.engine import Engine, NetConfig
    H, B, nf, si, so = g["net"]
    eng = Engine(NetConfig(hidden=int(H), blocks=int(B), n_freqs=int(nf), scale_input=float(si), scale_output=float(so),
                           transform=g["bounds_T"]), "cuda")
    eng.load_params(gu.params_of(g))
    return eng


def _vertex_to_mesh_distance(a, b):
    """symmetric mean distance between two vertex sets (nearest vertex: a fine stand-in for point-to-surface at this density)"""
    from scipy.spatial import cKDTree
    return max(cKDTree(b).query(a)[0].mean(), cKDTree(a).query(b)[0].mean())


def test_trained_net_mesh(tables):
    from oracle.torch_port import PortNet
    g = gu.load("trained_default")
    dim = 96
    pts, scale, T_bounds = _bounds_grid(g, dim)
    eng = _engine(g)
    vol = eng.sdf_eval(pts.cuda()).view(dim, dim, dim)
    H, B, nf, si, so = g["net"]
    port = PortNet(int(H), int(B), int(nf), float(si), float(so), transform=g["bounds_T"])
    port.load_state_dict({k: torch.from_numpy(v) for k, v in gu.params_of(g).items()})
    with torch.no_grad():
        ref_vol = port(pts).view(dim, dim, dim).numpy()
    hv = vol.cpu().numpy()
    assert gu.rel_err(hv, ref_vol) < 1e-3
    from isdf_amd.mesh import grid_index_to_world
    A = grid_index_to_world(dim, scale, T_bounds)
    v, f, n = eng.marching_cubes(vol, 0.0, A)
    v, f, n = v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()
    rv, rf, rn = mo.marching_cubes(hv, 0.0, tables, A)
    assert np.array_equal(f, rf) and len(f) > 1000
    np.testing.assert_allclose(v, rv, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(n, rn, rtol=1e-5, atol=1e-5)
    pv, _, _ = mo.marching_cubes(ref_vol, 0.0, tables, A)
    voxel = float(np.min(np.linalg.norm(A[:, :3], axis=0)))
    assert _vertex_to_mesh_distance(v, pv) < voxel


def test_200_cubed_grid_then_marching_cubes():
    """the default grid_dim: get_sdf_grid's one launch over 8 M points, then marching cubes, counts consistent"""
    g = gu.load("trained_default")
    dim = 200
    pts, scale, T_bounds = _bounds_grid(g, dim)
    eng = _engine(g)
    vol = eng.sdf_eval(pts.cuda()).view(dim, dim, dim)
    from isdf_amd.mesh import grid_index_to_world
    v, f, n = eng.marching_cubes(vol, 0.0, grid_index_to_world(dim, scale, T_bounds))
    torch.cuda.synchronize()
    assert v.shape[0] > 10000 and f.shape[0] > v.shape[0]
    assert int(f.min()) >= 0 and int(f.max()) < v.shape[0]
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(n).all())
    assert torch.allclose(n.norm(dim=1), torch.ones(1, device="cuda"), atol=1e-4)
