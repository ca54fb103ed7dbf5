"""The voxel baseline without a GPU: the numpy models of tests/fusion_model.py against the reference's recorded
sdf_from_occupancy results (fixture fusion_small) and against scipy, and the python layer of isdf_amd.fusion on a stub engine
backed by the same models."""
import types

import numpy as np
import pytest
import torch

from isdf_amd import fusion, synthetic
from tests import fusion_model as fm

CAM = dict(H=48, W=64, fx=60.0, fy=60.0, cx=31.5, cy=23.5)


@pytest.fixture(scope="module")
def golden():
    return fm.load_golden()


@pytest.mark.parametrize("k", range(4))
def test_model_equals_the_reference_bit_for_bit(golden, k):
    g = golden[k]
    assert g["occ"].any() and not g["occ"].all() and g["sdf"].dtype == np.float64
    assert fm.occupancy_sdf(g["occ"], g["voxel"], np.float64).tobytes() == g["sdf"].tobytes()
    assert fm.occupancy_sdf(g["occ"], g["voxel"]).tobytes() == g["sdf"].astype(np.float32).tobytes()


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("invert", [False, True])
def test_dist2_brute_equals_scipy_squared(golden, k, invert):
    ndimage = pytest.importorskip("scipy.ndimage")
    occ = golden[k]["occ"]
    feat = (occ != 0) != invert
    d2 = fm.dist2_brute(occ, invert)
    assert d2.dtype == np.int32 and d2.max() < fm.EDT_NONE
    assert np.sqrt(d2.astype(np.float64)).tobytes() == ndimage.distance_transform_edt(~feat).tobytes()
    assert np.array_equal(d2 == 0, feat)


@pytest.mark.parametrize("k", range(4))
def test_the_three_passes_equal_the_brute_force_minimum(golden, k):
    for invert in (False, True):
        assert np.array_equal(fm.dist2_passes(golden[k]["occ"], invert), fm.dist2_brute(golden[k]["occ"], invert))
    assert np.all(fm.dist2_passes(np.zeros((3, 1, 2))) == fm.EDT_NONE)


def test_dist2_brute_without_a_feature_voxel_and_at_a_corner():
    assert np.all(fm.dist2_brute(np.zeros((3, 4, 5), np.uint8)) == fm.EDT_NONE)
    assert np.all(fm.dist2_brute(np.ones((3, 4, 5), np.uint8), invert=True) == fm.EDT_NONE)
    one = np.zeros((4, 5, 6), np.uint8)
    one[3, 0, 5] = 1
    i, j, k = np.meshgrid(np.arange(4), np.arange(5), np.arange(6), indexing="ij")
    assert np.array_equal(fm.dist2_brute(one), (i - 3) ** 2 + j ** 2 + (k - 5) ** 2)
    assert np.all(fm.occupancy_sdf(np.zeros((2, 2, 2)), 0.1) == np.inf) and np.all(fm.occupancy_sdf(np.ones((2, 2, 2)), 0.1) == -np.inf)


def _frames(n, seed=0):
    T = synthetic.trajectory(n * 20)[::20][:n]
    depth = np.stack([synthetic.render_depth(T[i], CAM, np.random.RandomState(seed + i), invalid_frac=0.05) for i in range(n)])
    return depth, T


def _trainer(n=4):
    depth, T = _frames(n)
    frames = types.SimpleNamespace(depth_batch=torch.from_numpy(depth), T_WC_batch=torch.from_numpy(T))
    Tb = np.eye(4)
    Tb[:3, 3] = [3.0, 1.5, 2.5]
    return types.SimpleNamespace(engine=fm.StubEngine(), frames=frames, grid_dim=9, scene_scale_np=np.array([3.0, 1.5, 2.5]),
                                 bounds_transform_np=Tb, fx=CAM["fx"], fy=CAM["fy"], cx=CAM["cx"], cy=CAM["cy"])


def test_volume_shapes_nan_masking_and_the_occupancy_rule():
    vol = fusion.TsdfVolume((3, 4, 5), 0.1, (1.0, 2.0, 3.0), 0.4, "cpu", max_weight=8)
    assert vol.tsdf.shape == vol.weight.shape == (3, 4, 5) and vol.tsdf.dtype == vol.weight.dtype == torch.float32
    assert not vol.tsdf.any() and not vol.weight.any() and vol.spacing == (0.1, 0.1, 0.1) and vol.max_weight == 8.0
    assert np.array_equal(vol.index_to_world(), np.array([[0.1, 0, 0, 1], [0, 0.1, 0, 2], [0, 0, 0.1, 3]], np.float32))
    assert torch.isnan(vol.values()).all() and not vol.occupancy().any() and vol.occupancy().dtype == torch.uint8
    vol.weight[0, 0, :4] = torch.tensor([1.0, 2.0, 1.0, 0.0])
    vol.tsdf[0, 0, :4] = torch.tensor([-0.1, 0.0, 0.2, -0.3])
    v = vol.values()
    assert torch.equal(v[0, 0, :3], torch.tensor([-0.1, 0.0, 0.2])) and torch.isnan(v[0, 0, 3:]).all() and torch.isnan(v[1:]).all()
    occ = vol.occupancy()
    assert occ[0, 0].tolist() == [1, 1, 0, 0, 0] and int(occ.sum()) == 2      # weight 0 is never occupied, tsdf == 0 is
    gv = vol.gt_volume(torch.zeros(3, 4, 5))
    assert gv.spacing == vol.spacing and gv.origin == vol.origin and tuple(gv.values.shape) == (3, 4, 5)
    with pytest.raises(ValueError):
        vol.gt_volume(torch.zeros(3, 4, 6))
    for bad in (dict(dims=(0, 2, 2)), dict(spacing=-0.1), dict(trunc=0.0), dict(trunc=float("nan")), dict(max_weight=0.5),
                dict(origin=(0, float("inf"), 0))):
        kw = dict(dims=(2, 2, 2), spacing=0.1, origin=(0, 0, 0), trunc=0.3, device="cpu")
        kw.update(bad)
        with pytest.raises(ValueError):
            fusion.TsdfVolume(**kw)


def test_from_bounds_and_for_trainer_boxes():
    vol = fusion.TsdfVolume.from_bounds((0.0, -1.0, 2.0), (1.0, -0.75, 2.01), 0.25, device="cpu")
    assert vol.dims == (5, 2, 2) and vol.origin == (0.0, -1.0, 2.0) and vol.spacing == (0.25,) * 3 and vol.trunc == 1.0
    top = np.array(vol.origin) + (np.array(vol.dims) - 1) * 0.25
    assert np.all(top >= [1.0, -0.75, 2.01]) and np.all(top - 0.25 < [1.0, -0.75, 2.01])
    assert fusion.TsdfVolume.from_bounds((0, 0, 0), (0.3, 0.3, 0.3), 0.1, trunc=0.2, device="cpu").dims == (4, 4, 4)
    tr = _trainer()
    lo, hi = fusion.trainer_box(tr)
    assert np.allclose(lo, [0, 0, 0], atol=1e-6) and np.allclose(hi, [6, 3, 5], atol=1e-6)     # the synthetic room
    vt = fusion.TsdfVolume.for_trainer(tr, 0.5)
    assert vt.dims == (13, 7, 11) and np.allclose(vt.origin, lo) and vt.trunc == 2.0
    # a rotated box: the axis-aligned hull of its eight corners
    c, s = np.cos(0.3), np.sin(0.3)
    tr.bounds_transform_np = np.array([[c, -s, 0, 1.0], [s, c, 0, 2.0], [0, 0, 1, 3.0], [0, 0, 0, 1]])
    lo, hi = fusion.trainer_box(tr)
    corners = np.array([[x, y, z] for x in (-3, 3) for y in (-1.5, 1.5) for z in (-2.5, 2.5)]) @ tr.bounds_transform_np[:3, :3].T + [1, 2, 3]
    assert np.allclose(lo, corners.min(0), atol=1e-5) and np.allclose(hi, corners.max(0), atol=1e-5)


def test_fuse_frames_reads_the_keyframes_in_order_and_leaves_them_untouched():
    tr = _trainer(4)
    before = (tr.frames.depth_batch.clone(), tr.frames.T_WC_batch.clone())
    vol = fusion.fuse_frames(tr, voxel=0.5)
    assert tr.engine.calls == [("integrate", 4)] and vol.dims == (13, 7, 11)
    assert torch.equal(before[0], tr.frames.depth_batch) and torch.equal(before[1], tr.frames.T_WC_batch)
    assert float(vol.weight.max()) >= 2 and bool((vol.weight > 0).any()) and bool(vol.occupancy().any())
    T_CW = torch.linalg.inv(tr.frames.T_WC_batch).numpy()
    t, w = fm.integrate32(np.zeros(vol.dims, np.float32), np.zeros(vol.dims, np.float32), before[0].numpy(), T_CW, CAM, vol.origin,
                          vol.spacing, vol.trunc)
    assert vol.tsdf.numpy().tobytes() == t.tobytes() and vol.weight.numpy().tobytes() == w.tobytes()
    # a selection, in the order given; frame by frame equals all at once
    sel = fusion.fuse_frames(tr, voxel=0.5, idxs=[2, 0])
    step = fusion.TsdfVolume.for_trainer(tr, 0.5)
    for i in (2, 0):
        fusion.integrate(tr, step, before[0][i:i + 1], before[1][i:i + 1], tr)
    assert torch.equal(sel.tsdf, step.tsdf) and torch.equal(sel.weight, step.weight) and not torch.equal(sel.weight, vol.weight)
    by_dims = fusion.fuse_frames(tr, dims=(7, 4, 6), max_weight=2.0)
    assert by_dims.dims == (7, 4, 6) and np.allclose(by_dims.spacing, (1.0, 1.0, 1.0)) and float(by_dims.weight.max()) == 2.0
    for kw in (dict(), dict(voxel=0.5, dims=4), dict(dims=1)):
        with pytest.raises(ValueError):
            fusion.fuse_frames(tr, **kw)
    assert torch.equal(before[0], tr.frames.depth_batch) and torch.equal(before[1], tr.frames.T_WC_batch)


def test_full_sdf_blend_rule_and_its_anisotropy_error():
    eng = fm.StubEngine()
    vol = fusion.TsdfVolume((4, 3, 6), 0.1, (0, 0, 0), 0.25, "cpu")
    vol.weight[:] = 1.0
    vol.tsdf[:] = 0.25                                   # at the truncation: outside the band
    vol.tsdf[:, :, 3], vol.tsdf[:, :, 4:] = 0.05, -0.05
    vol.weight[0, 0, 5] = 0.0                            # in the band but never measured
    vol.tsdf[1, 1, 0] = -0.25                            # measured, occupied, |tsdf| == trunc: not blended
    plain = fusion.full_sdf(eng, vol, blend=False)
    assert plain.numpy().tobytes() == fm.occupancy_sdf(vol.occupancy().numpy(), 0.1).tobytes()
    assert eng.calls == [("occupancy_sdf", 0.1)]
    out = fusion.full_sdf(eng, vol)
    band = (vol.weight > 0) & (vol.tsdf.abs() < 0.25)
    assert bool(band[:, :, 3:].sum() == 4 * 3 * 3 - 1) and not bool(band[:, :, :3].any()) and not bool(band[0, 0, 5])
    assert torch.equal(out[band], vol.tsdf[band]) and torch.equal(out[~band], plain[~band])
    assert float(out[1, 1, 0]) == float(plain[1, 1, 0]) < 0 and float(out[0, 0, 5]) == float(plain[0, 0, 5])
    with pytest.raises(ValueError):
        fusion.full_sdf(eng, fusion.TsdfVolume((4, 3, 6), (0.1, 0.1, 0.2), (0, 0, 0), 0.25, "cpu"))


def test_thin_wrappers_pass_through():
    eng = fm.StubEngine()
    occ = torch.from_numpy(fm.load_golden()[0]["occ"])
    assert np.array_equal(fusion.distance_transform(eng, occ, invert=True).numpy(), fm.dist2_brute(occ.numpy(), True))
    assert fusion.signed_distance(types.SimpleNamespace(engine=eng), occ, 0.05).dtype == torch.float32
    assert eng.calls == [("edt", True), ("occupancy_sdf", 0.05)]
