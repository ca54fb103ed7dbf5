"""The narrow-band selection rule on the numpy model (tests/band_model.py), no kernel launched: on analytic distance fields with
|grad f| = 1 and slack 1.05 the band loses no sign-changing cell, evaluates every stencil marching cubes reads, reports no leak,
and the numpy marching cubes of the NaN-masked volume is exactly that of the dense one."""
import numpy as np
import pytest

from tests import band_model as bm
from tests import mc_oracle as mo


@pytest.fixture(scope="module")
def tables():
    from isdf_amd import build
    build.build(verbose=False)
    return mo.library_tables()


@pytest.fixture(scope="module", params=bm.CASES, ids=bm.case_id)
def case(request):
    name, dims, kind, kw = request.param
    vol, A = bm.dense_volume(name, dims, kind, kw)
    return vol, A, bm.band(vol, A, 0.0, bm.SLACK, 8)


def _dilate(mask, dims):
    """lattice points within one index of a corner of a marked unit cell, per axis: [i - 1, i + 2]"""
    pts = np.zeros(dims, bool)
    D0, D1, D2 = dims
    idx = np.argwhere(mask)
    for oi in range(-1, 3):
        for oj in range(-1, 3):
            for ok in range(-1, 3):
                q = idx + (oi, oj, ok)
                ok_ = ((q >= 0) & (q < (D0, D1, D2))).all(1)
                pts[tuple(q[ok_].T)] = True
    return pts


def test_no_cell_decided_on_the_threshold(case):
    """what makes the exact count comparisons of tests/test_band_gpu.py meaningful: the kernel's fused diagonal and the model's
    unfused one differ by a few 1e-7 relative, no decided cell of these inputs lies within 1e-4 of slack * d"""
    assert case[2]["min_margin"] > 1e-4


def test_band_covers_the_surface_and_its_stencils(case):
    vol, A, r = case
    sc = bm.sign_changing_cells(vol)
    assert sc.sum() > 1000
    assert not (sc & ~r["in_kept"]).any()                       # every sign-changing cell lies inside a kept stride-2 cell
    assert not (_dilate(sc, vol.shape) & ~r["evaluated_mask"]).any()    # corners and their central-difference neighbours
    assert r["leaks"] == 0
    assert r["evaluated"] < 0.5 * r["dense"]
    assert sum(l["evaluated"] for l in r["levels"]) == r["evaluated"]
    for up, down in zip(r["levels"], r["levels"][1:-1]):
        assert down["candidates"] <= 8 * up["kept"]


def test_marching_cubes_of_the_band_volume_is_the_dense_mesh(case, tables):
    vol, A, r = case
    assert np.isnan(r["volume"]).sum() == r["dense"] - r["evaluated"]
    dense = mo.marching_cubes(vol, 0.0, tables, A)
    band = mo.marching_cubes(r["volume"], 0.0, tables, A)
    for x, y in zip(band, dense):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()
    assert len(dense[1]) > 1000


@pytest.mark.parametrize("dims", [(2, 2, 2), (5, 3, 9)])
def test_grids_smaller_than_one_coarse_cell(dims, tables):
    A = bm.affine("unit", dims)
    p = bm.lattice_points(dims, A)
    vol = (p[..., 0] * 0.48 + p[..., 1] * 0.6 + p[..., 2] * 0.64 - 1.3).astype(np.float32)       # a plane through the grid
    r = bm.band(vol, A, 0.0, bm.SLACK, 8)
    assert [l.get("candidates") for l in r["levels"]][0] == 1                    # one clipped stride-8 cell
    assert r["kept"][8].shape == (1, 1, 1) and r["kept"][8].all()
    assert r["kept"][2].shape == tuple((d - 1 + 1) // 2 for d in dims)
    sc = bm.sign_changing_cells(vol)
    assert sc.any() and not (sc & ~r["in_kept"]).any() and r["leaks"] == 0
    dense, band = mo.marching_cubes(vol, 0.0, tables, A), mo.marching_cubes(r["volume"], 0.0, tables, A)
    for x, y in zip(band, dense):
        assert x.tobytes() == y.tobytes()


def test_too_small_a_slack_is_reported_as_leaks():
    """a slack far below the Lipschitz constant drops cells the surface crosses; where the halo of a kept cell still sees the
    surface the leak counter says so"""
    name, dims, kind, kw = bm.CASES[1]
    vol, A = bm.dense_volume(name, dims, kind, kw)
    r = bm.band(vol, A, 0.0, 0.02, 8)
    sc = bm.sign_changing_cells(vol)
    assert (sc & ~r["in_kept"]).any() and r["leaks"] > 0
    assert r["evaluated"] < bm.band(vol, A, 0.0, bm.SLACK, 8)["evaluated"]


def test_non_finite_corners_keep_their_cells():
    name, dims, kind, kw = bm.CASES[0]
    vol, A = bm.dense_volume(name, dims, kind, kw)
    vol[:, 40:43, :] = np.nan
    r = bm.band(vol, A, 0.0, bm.SLACK, 8)
    touching = np.zeros(tuple(d - 1 for d in dims), bool)
    touching[:, 39:43, :] = True                                # unit cells with a corner in the slab
    assert not (touching & ~r["in_kept"]).any()
