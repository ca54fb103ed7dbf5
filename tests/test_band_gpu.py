"""Narrow-band surface extraction on the device (isdf_band_*, isdf_amd/csrc/band.hip; Engine.band_volume,
isdf_amd.mesh.extract_surface / reconstruct) against the dense path -- bit for bit -- and against the numpy model of the
selection rule (tests/band_model.py), count for count."""
import numpy as np
import pytest
import torch

from tests import band_model as bm
from tests import golden_util as gu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    from isdf_amd import build
    build.build(verbose=False)
    return gu.load("trained_default")


@pytest.fixture(scope="module")
def eng(g):
    from tests.test_mesh_gpu import _engine
    return _engine(g)


def _same(a, b):
    """two (verts, faces, normals) triples, byte for byte"""
    for x, y in zip(a[:3], b[:3]):
        assert x.shape == y.shape and x.dtype == y.dtype, (x.shape, y.shape)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def _dense(eng, field, dims, A, level=0.0, points=None):
    from isdf_amd.mesh import grid_points
    pts = grid_points(dims, A, "cuda") if points is None else points
    vol = field(pts).view(*dims)
    return vol, eng.marching_cubes(vol, level, A)


def _counts(levels):
    return [(l["stride"], l.get("candidates"), l.get("kept"), l["evaluated"]) for l in levels]


# ---- 1. analytic fields through `field=`
@pytest.mark.parametrize("case", bm.CASES, ids=bm.case_id)
def test_analytic_fields_equal_dense_and_the_model(eng, case):
    from isdf_amd.mesh import extract_surface
    name, dims, kind, kw = case
    field, A = bm.torch_field(name, dims, kind, kw)
    v, f, n, st = extract_surface(eng, dims, A, slack=bm.SLACK, field=field)
    vol, dense = _dense(eng, field, dims, A)
    _same((v, f, n), dense)
    assert f.shape[0] > 1000 and st["leaks"] == 0 and len(st["attempts"]) == 1
    model = bm.band(vol.cpu().numpy(), A, 0.0, bm.SLACK, 8)
    assert model["min_margin"] > 1e-4
    print(bm.case_id(case), "device", _counts(st["levels"]), "model", _counts(model["levels"]))
    assert _counts(st["levels"]) == _counts(model["levels"])
    assert st["evaluated"] == model["evaluated"] and st["dense"] == model["dense"]


@pytest.mark.parametrize("dims", [(2, 2, 2), (5, 3, 9)])
def test_grids_smaller_than_one_coarse_cell(eng, dims):
    from isdf_amd.mesh import extract_surface
    A = bm.affine("unit", dims)
    field = lambda p: p[:, 0] * 0.48 + p[:, 1] * 0.6 + p[:, 2] * 0.64 - 1.3
    v, f, n, st = extract_surface(eng, dims, A, slack=bm.SLACK, field=field)
    vol, dense = _dense(eng, field, dims, A)
    _same((v, f, n), dense)
    model = bm.band(vol.cpu().numpy(), A, 0.0, bm.SLACK, 8)
    assert f.shape[0] > 0 and st["leaks"] == 0 and _counts(st["levels"]) == _counts(model["levels"])


# ---- 2. the trained default network over its bounds box
@pytest.fixture(scope="module", params=[96, 129])
def net_case(request, g, eng):
    from isdf_amd.mesh import grid_index_to_world
    from tests.test_mesh_gpu import _bounds_grid
    dim = request.param
    _, scale, T_bounds = _bounds_grid(g, dim)
    A = grid_index_to_world(dim, scale, T_bounds)
    vol, dense = _dense(eng, eng.sdf_eval, (dim,) * 3, A)
    return dim, A, dense


def test_trained_net_at_slack_2_is_the_dense_mesh(eng, net_case):
    from isdf_amd.mesh import extract_surface
    dim, A, dense = net_case
    v, f, n, st = extract_surface(eng, dim, A, slack=2.0, widen=False)
    print("dim", dim, "slack 2.0: fraction %.4f" % st["fraction"], _counts(st["levels"]))
    _same((v, f, n), dense)
    assert st["leaks"] == 0 and f.shape[0] > 1000
    assert st["fraction"] < 0.8


def _rows(t):
    """the rows of a [n, 3] float32 tensor as a set of their bytes"""
    return {r.tobytes() for r in np.ascontiguousarray(t.cpu().numpy())}


def test_trained_net_at_slack_0p1_leaks_and_widens(eng, net_case):
    from isdf_amd.mesh import extract_surface
    dim, A, dense = net_case
    v, f, n, st = extract_surface(eng, dim, A, slack=0.1, widen=False)
    print("dim", dim, "slack 0.1: leaks", st["leaks"], "fraction %.4f" % st["fraction"])
    assert st["leaks"] > 0 and len(st["attempts"]) == 1
    assert f.shape[0] > 0 and int(f.min()) >= 0 and int(f.max()) < v.shape[0]
    ok = torch.isfinite(n).all(1)
    assert bool(ok.any()) and _rows(v[ok]) <= _rows(dense[0])       # what it does mesh is part of the dense mesh
    v, f, n, st = extract_surface(eng, dim, A, slack=0.1, widen=True)
    print("dim", dim, "widened:", [(a["slack"], a["leaks"]) for a in st["attempts"]])
    _same((v, f, n), dense)
    assert len(st["attempts"]) > 1 and st["leaks"] == 0
    assert [a["slack"] for a in st["attempts"][:2]] == [0.1, 0.2]


# ---- 3. positions gathered from a caller's grid (as Trainer.grid_pc is made)
def test_points_gathered_from_a_linspace_grid(g, eng):
    from isdf_amd.mesh import extract_surface, grid_index_to_world
    from tests.test_mesh_gpu import _bounds_grid
    dim = 96
    pts, scale, T_bounds = _bounds_grid(g, dim)
    A = grid_index_to_world(dim, scale, T_bounds)
    pts = pts.cuda()
    dense = eng.marching_cubes(eng.sdf_eval(pts).view(dim, dim, dim), 0.0, A)
    v, f, n, st = extract_surface(eng, dim, A, slack=2.0, widen=False, points=pts)
    _same((v, f, n), dense)
    assert st["leaks"] == 0 and st["fraction"] < 0.8


# ---- 4. a field with a NaN slab
def test_nan_slab_cells_are_kept_and_the_mesh_is_dense(eng):
    from isdf_amd.mesh import BAND_UNSET_BITS, extract_surface
    name, dims, kind, kw = bm.CASES[0]
    inner, A = bm.torch_field(name, dims, kind, kw)

    def field(p):
        f = inner(p)
        return torch.where((p[:, 1] > 39.5) & (p[:, 1] < 42.5), torch.full_like(f, float("nan")), f)      # j = 40, 41, 42
    vol_b, st = eng.band_volume(dims, A, slack=bm.SLACK, field=field)
    bits = vol_b.view(torch.int32)
    assert bool((bits[:, 39:44, :] != BAND_UNSET_BITS).all())          # every cell with a corner in the slab was kept and filled
    assert bool((bits == BAND_UNSET_BITS).any())
    v, f, n, st = extract_surface(eng, dims, A, slack=bm.SLACK, field=field)
    _, dense = _dense(eng, field, dims, A)
    _same((v, f, n), dense)
    assert st["leaks"] == 0 and f.shape[0] > 1000


# ---- 5. another level
def test_level_0p05(eng):
    from isdf_amd.mesh import extract_surface
    name, dims, kind, kw = bm.CASES[8]                                  # the anisotropic affine: R is about 1, so 0.05 is a real offset
    field, A = bm.torch_field(name, dims, kind, kw)
    v, f, n, st = extract_surface(eng, dims, A, level=0.05, slack=bm.SLACK, field=field)
    _, dense = _dense(eng, field, dims, A, level=0.05)
    _same((v, f, n), dense)
    _, dense0 = _dense(eng, field, dims, A)
    assert st["leaks"] == 0 and f.shape[0] > 1000 and f.shape[0] != dense0[1].shape[0]


# ---- 6. determinism
def test_two_runs_are_bit_identical(eng, net_case):
    from isdf_amd.mesh import extract_surface
    dim, A, _ = net_case
    runs = []
    for _ in range(2):
        vol, st = eng.band_volume(dim, A, slack=1.0)
        mesh = extract_surface(eng, dim, A, slack=1.0, widen=False)
        runs.append((vol.clone(), st, mesh))
    (va, sa, ma), (vb, sb, mb) = runs
    assert torch.equal(va.view(torch.int32), vb.view(torch.int32)) and sa == sb
    _same(ma, mb)
    assert ma[3] == mb[3]


# ---- 7. a grafted trainer
def test_reconstruct_on_a_grafted_trainer():
    from bench_support.standin_trainer import HipTrainer
    from isdf_amd import synthetic
    from isdf_amd.hot_path import HotPath
    from isdf_amd.mesh import grid_index_to_world, grid_points, reconstruct
    from tests import slice_model as sm
    from tests.accuracy_experiment import config
    cam = dict(H=96, W=128, fx=100.0, fy=100.0, cx=63.5, cy=47.5)
    tr = HipTrainer("cuda", config(cam), inv_bounds_transform=synthetic.bounds_transform(), rng="philox", seed=5)
    sm.set_slice_geometry(tr, "A", "cuda")
    public = sorted(k for k in vars(HotPath) if not k.startswith("_"))
    eng = tr.engine
    # an untrained net need not cross zero: mesh the level set through the middle of its values
    A = grid_index_to_world(65, tr.scene_scale_np, tr.bounds_transform_np)
    vol = eng.sdf_eval(grid_points(65, A, "cuda")).view(65, 65, 65)
    level = float(vol.median())
    dense = eng.marching_cubes(vol, level, A)
    v, f, n, st = reconstruct(tr, grid_dim=65, level=level)
    _same((v, f, n), dense)
    assert f.shape[0] > 100 and st["leaks"] == 0 and st["dense"] == 65 ** 3
    # at the trainer's own grid_dim the positions are grid_pc's, the values get_sdf_grid's
    d = tr.grid_dim
    grid = tr.get_sdf_grid()
    level = float(grid.median())
    own = eng.marching_cubes(grid, level, grid_index_to_world(d, tr.scene_scale_np, tr.bounds_transform_np))
    v, f, n, st = reconstruct(tr, level=level)
    _same((v, f, n), own)
    assert st["dense"] == d ** 3 and tr.grid_dim == d
    assert sorted(k for k in vars(HotPath) if not k.startswith("_")) == public and not hasattr(tr, "reconstruct")
