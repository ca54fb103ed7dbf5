"""The voxel baseline on the device: isdf_tsdf_integrate, isdf_distance_transform and isdf_occupancy_sdf through Engine and
isdf_amd.fusion.  References: tests/fusion_model.py -- the fused (tsdf, weight) pair must equal its float32 sequence on EVERY voxel
bit for bit, the squared distances its exact integer minimum -- and the reference's own sdf_from_occupancy results (fixture
fusion_small, made by tests/golden/make_fusion_golden.py), equal after the float32 cast bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

from isdf_amd import fusion, synthetic
from tests import eval_model as em
from tests import fusion_model as fm

pytestmark = pytest.mark.gpu

CAM = dict(H=48, W=64, fx=60.0, fy=60.0, cx=31.5, cy=23.5)
EPS32 = float(np.finfo(np.float32).eps)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Cam:
    fx, fy, cx, cy = CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"]


def _constant(name):
    src = open(os.path.join(ROOT, "isdf_amd", "csrc", "fusion.hip")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


STAGE, UNROLL, EDT_PC, EDT_QC = (_constant(n) for n in ("TSDF_STAGE", "TSDF_UNROLL", "EDT_PC", "EDT_QC"))
F_ALL = STAGE + 6          # one stage and a last group that is not full
VOLUMES = {
    # nz one past a wave; a thin column in front of the first camera, through the wall at z = 5
    "5x6x67": dict(dims=(5, 6, 67), origin=(4.0, 1.55, 1.8), spacing=(0.05, 0.05, 0.05)),
    # 11 700 voxels, no multiple of 256; through the whole room and 0.5 m past its wall, so that cameras have part of it behind
    # them and part of it outside their images
    "9x10x130": dict(dims=(9, 10, 130), origin=(2.5, 0.2, -0.5), spacing=(0.3, 0.25, 0.04)),
}
TRUNC = 0.2


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def eng():
    from isdf_amd.engine import Engine, NetConfig
    return Engine(NetConfig(hidden=64, blocks=1), "cuda")


def make_frames():
    """F_ALL frames of 48 x 64 along the synthetic trajectory with zero pixels (invalid_frac) and a few NaN pixels written in; the
    camera-from-world matrices inverted once on the host: kernel and model read the same float32 entries"""
    assert F_ALL > STAGE and F_ALL % UNROLL != 0
    T = synthetic.trajectory(F_ALL * 9)[::9][:F_ALL]
    depth = np.stack([synthetic.render_depth(T[i], CAM, np.random.RandomState(100 + i), invalid_frac=0.05) for i in range(F_ALL)])
    rng = np.random.RandomState(7)
    for f in range(F_ALL):
        depth[f, rng.randint(0, 48, 6), rng.randint(0, 64, 6)] = np.nan
    assert (depth == 0).mean() > 0.03 and np.isnan(depth).sum() > F_ALL
    T_CW = np.linalg.inv(T.astype(np.float64)).astype(np.float32)
    return dict(depth=depth, T_WC=T, T_CW=T_CW, models={})


@pytest.fixture(scope="module")
def frames():
    return make_frames()


def _model(frames, name, F, max_weight, **kw):
    """the float32 model of a case, computed once and shared"""
    key = (name, F, max_weight, tuple(sorted(kw.items())))
    if key not in frames["models"]:
        v = VOLUMES[name]
        z = np.zeros(v["dims"], np.float32)
        frames["models"][key] = fm.integrate32(z, z, frames["depth"][:F], frames["T_CW"][:F], CAM, v["origin"], v["spacing"], TRUNC,
                                               max_weight, **kw)
    return frames["models"][key]


def _run(eng, frames, name, spans, max_weight, **kw):
    v = VOLUMES[name]
    tsdf, weight = (torch.zeros(v["dims"], dtype=torch.float32, device="cuda") for _ in range(2))
    for a, b in spans:
        eng.tsdf_integrate(tsdf, weight, _cuda(frames["depth"][a:b]), _cuda(frames["T_CW"][a:b]), Cam, v["origin"], v["spacing"], TRUNC,
                           max_weight=max_weight, **kw)
    return tsdf.cpu().numpy(), weight.cpu().numpy()


def test_the_second_volume_reaches_behind_cameras_and_outside_images(frames):
    v = VOLUMES["9x10x130"]
    ax = [o + np.arange(n) * s for n, o, s in zip(v["dims"], v["origin"], v["spacing"])]
    p = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    pc = np.einsum("frc,nc->fnr", frames["T_CW"].astype(np.float64), np.concatenate([p, np.ones((len(p), 1))], 1))
    behind = pc[..., 2] <= 0
    with np.errstate(all="ignore"):
        u, w = CAM["fx"] * pc[..., 0] / pc[..., 2] + CAM["cx"] + 0.5, CAM["fy"] * pc[..., 1] / pc[..., 2] + CAM["cy"] + 0.5
    outside = ~behind & ((u < 0) | (u >= CAM["W"]) | (w < 0) | (w >= CAM["H"]))
    inside = ~behind & ~outside
    print("pairs behind %.2f, outside %.2f, inside %.2f" % (behind.mean(), outside.mean(), inside.mean()))
    assert behind.mean() > 0.03 and outside.mean() > 0.03 and inside.mean() > 0.03
    both = behind.any(1) & (~behind).any(1)
    print("%d of %d cameras have part of the volume behind them and part in front" % (both.sum(), len(both)))
    assert both.sum() >= 8


@pytest.mark.parametrize("max_weight", [float("inf"), 4.0])
@pytest.mark.parametrize("F", [0, 1, 3, F_ALL])
@pytest.mark.parametrize("name", list(VOLUMES))
def test_integrate_equals_the_float32_model_on_every_voxel(eng, frames, name, F, max_weight):
    want_t, want_w = _model(frames, name, F, max_weight)
    t, w = _run(eng, frames, name, [(0, F)], max_weight)
    print("%s F %d max_weight %g: %d voxels differ, observed %.2f, weight max %g, %d voxels on or behind the surface"
          % (name, F, max_weight, ((t != want_t) | (w != want_w)).sum(), (want_w > 0).mean(), want_w.max(), (want_t < 0).sum()))
    assert t.tobytes() == want_t.tobytes() and w.tobytes() == want_w.tobytes()
    if F == 0:
        assert not t.any() and not w.any()
    else:
        assert (want_w > 0).any() and (want_w == 0).any() and want_w.max() <= max_weight
    if F == F_ALL:
        assert (want_t < 0).any() and (want_t == np.float32(TRUNC)).any()
        assert want_w.max() == 4.0 if max_weight == 4.0 else want_w.max() > 4.0


def test_depth_limits_select_the_measurements(eng, frames):
    kw = dict(min_depth=1.5, max_depth=2.5)
    want_t, want_w = _model(frames, "9x10x130", 3, float("inf"), **kw)
    t, w = _run(eng, frames, "9x10x130", [(0, 3)], float("inf"), **kw)
    assert t.tobytes() == want_t.tobytes() and w.tobytes() == want_w.tobytes()
    assert 0 < (want_w > 0).sum() < (_model(frames, "9x10x130", 3, float("inf"))[1] > 0).sum()


@pytest.mark.parametrize("name", list(VOLUMES))
def test_chunks_of_ten_equal_one_call_and_runs_repeat(eng, frames, name):
    one = _run(eng, frames, name, [(0, F_ALL)], 4.0)
    again = _run(eng, frames, name, [(0, F_ALL)], 4.0)
    split = _run(eng, frames, name, [(s, min(s + 10, F_ALL)) for s in range(0, F_ALL, 10)], 4.0)
    for a, b, c in zip(one, again, split):
        assert a.tobytes() == b.tobytes() == c.tobytes()


def test_engine_argument_checks(eng, frames):
    v = VOLUMES["5x6x67"]
    t = torch.zeros(v["dims"], device="cuda")
    d, T = _cuda(frames["depth"][:2]), _cuda(frames["T_CW"][:2])
    with pytest.raises(ValueError):
        eng.tsdf_integrate(t, torch.zeros(5, 6, 66, device="cuda"), d, T, Cam, v["origin"], v["spacing"], TRUNC)
    with pytest.raises(ValueError):
        eng.tsdf_integrate(t.double(), t.double(), d, T, Cam, v["origin"], v["spacing"], TRUNC)
    with pytest.raises(ValueError):
        eng.tsdf_integrate(t, t.clone(), d, T[:1], Cam, v["origin"], v["spacing"], TRUNC)
    with pytest.raises(ValueError):
        eng.tsdf_integrate(t, t.clone(), d[0], T, Cam, v["origin"], v["spacing"], TRUNC)
    with pytest.raises(ValueError):
        eng.distance_transform(torch.zeros(4, 4, device="cuda"))
    from isdf_amd._ffi import IsdfError
    with pytest.raises(IsdfError):
        eng.distance_transform(torch.zeros(1025, 1, 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(IsdfError):
        eng.occupancy_sdf(torch.zeros(4, 4, 4, dtype=torch.uint8, device="cuda"), 0.0)
    assert not t.any()


# ---- the distance transform
def _grids():
    """name -> feature grid: the fixture's four, a single line along z one past the line tile's lanes, a side one past the outputs
    of a workgroup, a side one past the staged chunk"""
    g = {"fixture %d" % k: c["occ"] for k, c in enumerate(fm.load_golden())}
    rng = np.random.RandomState(3)
    g["1x1x70"] = (rng.uniform(size=(1, 1, 70)) < 0.1).astype(np.uint8)
    g["65x2x3"] = (rng.uniform(size=(EDT_PC + 1, 2, 3)) < 0.05).astype(np.uint8)
    g["2x129x3"] = (rng.uniform(size=(2, EDT_QC + 1, 3)) < 0.02).astype(np.uint8)
    g["3x2x129"] = (rng.uniform(size=(3, 2, EDT_QC + 1)) < 0.02).astype(np.uint8)
    return g


GRID_NAMES = ["fixture 0", "fixture 1", "fixture 2", "fixture 3", "1x1x70", "65x2x3", "2x129x3", "3x2x129"]


@pytest.fixture(scope="module")
def grids():
    g = _grids()
    assert list(g) == GRID_NAMES and all(v.any() and not v.all() for v in g.values())
    return g


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("name", GRID_NAMES)
def test_distance_transform_equals_the_integer_minimum(eng, grids, name, invert):
    want = fm.dist2_brute(grids[name], invert)
    got = eng.distance_transform(_cuda(grids[name]), invert=invert)
    assert got.dtype == torch.int32 and tuple(got.shape) == grids[name].shape
    assert np.array_equal(got.cpu().numpy(), want)
    again = fusion.distance_transform(eng, _cuda(grids[name]).bool(), invert=invert)          # any dtype: != 0 decides
    assert torch.equal(got, again)


def test_distance_transform_corner_feature_long_side_and_no_feature(eng):
    one = np.zeros((40, 40, 40), np.uint8)
    one[39, 0, 39] = 1
    i, j, k = np.meshgrid(np.arange(40), np.arange(40), np.arange(40), indexing="ij")
    assert np.array_equal(eng.distance_transform(_cuda(one)).cpu().numpy(), (i - 39) ** 2 + j ** 2 + (k - 39) ** 2)
    for axis in range(3):
        dims = [2, 2, 2]
        dims[axis] = 1024
        long = np.zeros(dims, np.uint8)
        long[0, 0, 0] = 1
        got = eng.distance_transform(_cuda(long)).cpu().numpy()
        idx = np.stack(np.meshgrid(*[np.arange(n) for n in dims], indexing="ij"), -1).astype(np.int64)
        assert np.array_equal(got, (idx ** 2).sum(-1))
        far = [1, 1, 1]
        far[axis] = 1023
        assert got[tuple(far)] == 1023 ** 2 + 2 and got.max() == 1023 ** 2 + 2
        end = [0, 0, 0]
        end[axis] = 1023
        assert got[tuple(end)] == 1023 ** 2                           # the far end of the line itself: exactly 1023^2
    none = eng.distance_transform(torch.zeros(7, 66, 5, dtype=torch.uint8, device="cuda")).cpu().numpy()
    assert none.dtype == np.int32 and np.all(none == fm.EDT_NONE)
    assert np.all(eng.distance_transform(torch.ones(7, 66, 5, dtype=torch.uint8, device="cuda"), invert=True).cpu().numpy() == fm.EDT_NONE)


@pytest.mark.parametrize("k", range(4))
def test_occupancy_sdf_equals_the_reference_after_the_cast(eng, k):
    g = fm.load_golden()[k]
    got = eng.occupancy_sdf(_cuda(g["occ"]), g["voxel"])
    assert got.dtype == torch.float32 and tuple(got.shape) == g["dims"]
    assert got.cpu().numpy().tobytes() == g["sdf"].astype(np.float32).tobytes()
    assert torch.equal(got, fusion.signed_distance(eng, _cuda(g["occ"]), g["voxel"]))


def test_occupancy_sdf_of_an_empty_and_of_a_full_grid(eng):
    free = eng.occupancy_sdf(torch.zeros(5, 66, 3, dtype=torch.uint8, device="cuda"), 0.05).cpu().numpy()
    full = eng.occupancy_sdf(torch.ones(5, 66, 3, dtype=torch.uint8, device="cuda"), 0.05).cpu().numpy()
    assert np.all(free == np.inf) and np.all(full == -np.inf)


# ---- end to end on the analytic room
def room_case():
    """eight views of the analytic room at 48 x 64 and the 0.1 m grid over its box"""
    T = synthetic.trajectory(8 * 40)[::40][:8]
    depth = np.stack([synthetic.render_depth(T[i], CAM, np.random.RandomState(40 + i), invalid_frac=0.02) for i in range(8)])
    vol = fusion.TsdfVolume.from_bounds(synthetic.ROOM_LO, synthetic.ROOM_HI, 0.1, device="cpu")
    return dict(depth=depth, T_WC=T, T_CW=np.linalg.inv(T.astype(np.float64)).astype(np.float32), cam=CAM, dims=vol.dims,
                origin=vol.origin, spacing=vol.spacing, trunc=vol.trunc)


# mean |true SDF| over the vertices of the float64 model's mesh (fusion_model.integrate64 on these frames, tests/mc_oracle.py),
# measured on the CPU: 4596 vertices, mean 0.004104 m (the largest 0.25 m, where the views end inside an obstacle's shadow)
ROOM_MEAN_ABS_SDF_F64 = 0.004104


@pytest.fixture(scope="module")
def room(eng):
    c = room_case()
    vol = fusion.TsdfVolume.from_bounds(synthetic.ROOM_LO, synthetic.ROOM_HI, 0.1)
    assert vol.dims == (61, 31, 51) and vol.trunc == 0.4
    T = _cuda(c["T_WC"])
    fusion.integrate(eng, vol, _cuda(c["depth"]), T, Cam)
    T_CW = torch.linalg.inv(T).cpu().numpy()            # the inverse the device made: the model reads the same entries
    z = np.zeros(vol.dims, np.float32)
    c["vol"] = vol
    c["model"] = fm.integrate32(z, z, c["depth"], T_CW, CAM, vol.origin, vol.spacing, vol.trunc)
    return c


def test_room_volume_and_mesh(eng, room):
    """The device volume equals the float32 model on every voxel, and its mesh is the mesh of the model's volume.  The mesh lies on
    the room's surfaces: the mean |analytic SDF| over its vertices stays within 1.5 x ROOM_MEAN_ABS_SDF_F64 = 0.004104 m, the figure
    of the float64 model on the same frames (measured on the CPU; a tenth-of-a-metre grid, eight views of 48 x 64).  The margin
    covers float32 against float64 zero crossings; it is not a target."""
    vol, (t, w) = room["vol"], room["model"]
    assert vol.tsdf.cpu().numpy().tobytes() == t.tobytes() and vol.weight.cpu().numpy().tobytes() == w.tobytes()
    A = vol.index_to_world()
    verts, faces, normals = eng.marching_cubes(vol.values(), 0.0, A)
    mv, mf, mn = eng.marching_cubes(_cuda(np.where(w > 0, t, np.float32(np.nan))), 0.0, A)
    assert verts.shape[0] > 1000 and faces.shape[0] > 1000
    # normals by their bits: the central differences next to an unobserved voxel read its NaN
    assert torch.equal(verts, mv) and torch.equal(faces, mf) and torch.equal(normals.view(torch.int32), mn.view(torch.int32))
    assert torch.isfinite(verts).all() and torch.isfinite(normals).any()
    err = np.abs(synthetic.gt_sdf(verts.cpu().numpy().astype(np.float64)))
    print("fused mesh: %d vertices, %d faces, mean |sdf| %.6f m (float64 model %.6f), max %.3f, %.2f of the voxels observed"
          % (verts.shape[0], faces.shape[0], err.mean(), ROOM_MEAN_ABS_SDF_F64, err.max(), (w > 0).mean()))
    assert err.mean() <= 1.5 * ROOM_MEAN_ABS_SDF_F64


def test_room_full_sdf_and_baseline_metrics(eng, room):
    """full_sdf equals the host model bit for bit (exact distances, the same blend), and baseline_metrics of it against the room's
    analytic field agrees with the float64 numpy lookup and sums within tests/test_eval_gpu.py's bound, 16 * eps32 * (max |p| +
    max |value|): two float32 trilinear lookups stand against two float64 ones.  Points float32 could place in another bin or on
    the other side of a face are left out beforehand, by that file's rule."""
    from isdf_amd.metrics import GtVolume
    vol, (t, w) = room["vol"], room["model"]
    occ = (w > 0) & (t <= 0)
    assert occ.any() and not occ.all()
    assert np.array_equal(vol.occupancy().cpu().numpy(), occ.astype(np.uint8))
    plain = fm.sdf_from_dist2(fm.dist2_passes(occ), fm.dist2_passes(occ, invert=True), vol.spacing[0])
    assert fusion.full_sdf(eng, vol, blend=False).cpu().numpy().tobytes() == plain.tobytes()
    band = (w > 0) & (np.abs(t) < np.float32(vol.trunc))
    field = np.where(band, t, plain)
    got_field = fusion.full_sdf(eng, vol)
    assert got_field.cpu().numpy().tobytes() == field.tobytes() and band.any() and not band.all()
    with pytest.raises(ValueError):
        fusion.full_sdf(eng, fusion.TsdfVolume((4, 4, 4), (0.1, 0.1, 0.2), (0, 0, 0), 0.3, "cuda"))
    # ground truth: the analytic field on a grid that reaches past the room on every side
    gsp, gor = np.array([0.1, 0.125, 0.1]), np.array([-0.5, -0.25, -0.5])
    ax = tuple(np.arange(n) * h + o for n, h, o in zip((71, 29, 61), gsp, gor))
    values = synthetic.gt_sdf(np.stack(np.meshgrid(*ax, indexing="ij"), -1)).astype(np.float32)
    pts = np.random.RandomState(11).uniform([-0.3, -0.2, -0.3], [6.3, 3.2, 5.3], (6000, 3)).astype(np.float32)
    p64 = pts.astype(np.float64)
    near = np.zeros(len(pts), bool)
    for sp, org, shape in ((np.array(vol.spacing), np.array(vol.origin), vol.dims), (gsp, gor, values.shape)):
        u = (p64 - org) / sp
        near |= np.any((np.abs(u) < 1e-4) | (np.abs(u - (np.array(shape) - 1)) < 1e-4), axis=1)
    gt, ginb = em.trilinear(values, gsp, gor, p64)
    for edge in (0.0, 0.1, 0.2, 0.5, 1.0, 1.5, 2.0):
        near |= ginb & (np.abs(gt - edge) < 1e-5)
    assert near.mean() < 0.01 and ginb.all()
    pts = pts[~near]
    looked, inb = em.trilinear(field, vol.spacing, vol.origin, pts)
    assert 0.5 < inb.mean() < 0.95                                  # some points lie outside the baseline's grid
    model, gt, valid = em.sdf_metrics(values, gsp, gor, pts[inb], looked[inb])
    want = em.result_dict(model)
    m = fusion.baseline_metrics(eng, got_field, vol, GtVolume(values, gsp, gor, "cuda"), _cuda(pts))
    res = m.as_dict()
    bound = 16 * EPS32 * (float(np.abs(pts).max()) + max(float(np.abs(values).max()), float(np.abs(field).max())))
    print("baseline: av_l1 %.6f (model %.6f), bound %.2e, n_valid %d of %d points" % (res["av_l1"], want["av_l1"], bound, model[0], len(pts)))
    assert m.n_valid == int(model[0]) == int(inb.sum()) and m.n_in_bounds == int(inb.sum())
    assert sorted(res) == ["av_l1", "binned_l1", "l1_chomp_costs"]
    assert abs(res["av_l1"] - want["av_l1"]) <= bound
    wb, rb = np.asarray(want["binned_l1"]), np.asarray(res["binned_l1"])
    assert np.array_equal(np.isnan(wb), np.isnan(rb)) and (~np.isnan(wb)).sum() >= 4
    assert np.abs(wb[~np.isnan(wb)] - rb[~np.isnan(wb)]).max() <= bound
    assert np.abs(np.asarray(want["l1_chomp_costs"]) - np.asarray(res["l1_chomp_costs"])).max() <= bound
    assert np.array_equal(np.bincount(np.digitize(gt[valid], em.BIN_LIMITS[1:-1]), minlength=6), m.bin_counts)


def test_fuse_frames_on_a_grafted_trainer_leaves_the_keyframes_and_the_graft_alone():
    import contextlib
    import io
    from bench_support.standin_trainer import HipTrainer
    from isdf_amd.hot_path import HotPath
    from tests import slice_model as sm
    from tests.accuracy_experiment import config
    cam = dict(H=96, W=128, fx=100.0, fy=100.0, cx=63.5, cy=47.5)
    tr = HipTrainer("cuda", config(cam), inv_bounds_transform=synthetic.bounds_transform(), rng="philox", seed=5)
    sm.set_slice_geometry(tr, "A", "cuda")
    public = sorted(k for k in vars(HotPath) if not k.startswith("_"))
    traj, rng = synthetic.trajectory(40), np.random.RandomState(7)
    with contextlib.redirect_stdout(io.StringIO()):
        for k in range(3):
            tr.last_is_keyframe = True
            tr.add_frame(tr.make_frame(k * 5, synthetic.render_depth(traj[k * 5], cam, rng), traj[k * 5]))
    before = (tr.frames.depth_batch.clone(), tr.frames.T_WC_batch.clone())
    vol = fusion.fuse_frames(tr, voxel=0.2)
    lo, hi = fusion.trainer_box(tr)
    assert np.allclose(vol.origin, lo) and np.all(np.array(vol.origin) + (np.array(vol.dims) - 1) * 0.2 >= hi - 1e-6)
    T_CW = torch.linalg.inv(before[1].float()).cpu().numpy()
    z = np.zeros(vol.dims, np.float32)
    t, w = fm.integrate32(z, z, before[0].cpu().numpy(), T_CW, cam, vol.origin, vol.spacing, vol.trunc)
    assert vol.tsdf.cpu().numpy().tobytes() == t.tobytes() and vol.weight.cpu().numpy().tobytes() == w.tobytes()
    assert w.max() == 3 and (w == 0).any() and (t < 0).any()
    last = fusion.fuse_frames(tr, voxel=0.2, idxs=[2])
    t1, w1 = fm.integrate32(z, z, before[0][2:].cpu().numpy(), T_CW[2:], cam, vol.origin, vol.spacing, vol.trunc)
    assert last.tsdf.cpu().numpy().tobytes() == t1.tobytes() and last.weight.cpu().numpy().tobytes() == w1.tobytes()
    assert torch.isfinite(fusion.full_sdf(tr, vol)).all()
    assert torch.equal(tr.frames.depth_batch, before[0]) and torch.equal(tr.frames.T_WC_batch, before[1])
    assert sorted(k for k in vars(HotPath) if not k.startswith("_")) == public and not hasattr(tr, "fuse_frames")


def measure_room_bound():
    """ROOM_MEAN_ABS_SDF_F64 again, on the CPU: `python -m tests.test_fusion_gpu` (the float64 model on the room's frames, the
    numpy marching cubes of tests/mc_oracle.py, the analytic field at its vertices)"""
    from tests import mc_oracle
    c = room_case()
    z = np.zeros(c["dims"])
    t, w = fm.integrate64(z, z, c["depth"], c["T_CW"], CAM, c["origin"], c["spacing"], c["trunc"])
    A = np.zeros((3, 4))
    A[:, :3], A[:, 3] = np.diag(c["spacing"]), c["origin"]
    verts, _, _ = mc_oracle.marching_cubes(np.where(w > 0, t, np.nan), 0.0, index_to_world=A)
    err = np.abs(synthetic.gt_sdf(verts.astype(np.float64)))
    return len(verts), float(err.mean()), float(err.max())


if __name__ == "__main__":
    print("vertices %d, mean |sdf| %.6f m, max %.3f m" % measure_room_bound())
