"""Evaluation against ground truth, host side (no GPU): the numpy models of tests/eval_model.py against scipy and against the
reference's recorded results (fixture eval_metrics_small, tests/golden/make_eval_golden.py), isdf_amd.metrics' host objects, and
the five evaluation methods graft() binds -- on the REAL reference Trainer with an engine stand-in that answers sdf_metrics /
nn_distance from the float64 model."""
import contextlib
import io
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import eval_model as em
from tests import golden_util as gu
from tests.fake_engine import FakeEngine

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "isdf")), reason="reference checkout not present")


@pytest.fixture(scope="module")
def g():
    return em.load_golden()


# ------------------------------------------------------------------ models
def test_trilinear_model_equals_scipy(g):
    interpolate = pytest.importorskip("scipy.interpolate")
    for name in ("signed", "zeroed"):
        vol = g[name].astype(np.float64)
        ax = [np.arange(n) * h + o for n, h, o in zip(vol.shape, g["spacing"], g["origin"])]
        itp = interpolate.RegularGridInterpolator(ax, vol, bounds_error=False, fill_value=1e99)
        ref = itp(g["pts"].astype(np.float64))
        gt, inb = em.trilinear(vol, g["spacing"], g["origin"], g["pts"])
        assert np.array_equal(inb, ref != 1e99)
        assert np.abs(gt[inb] - ref[inb]).max() <= 1e-12
    # the faces are inclusive, one ulp outside is out
    hi = g["origin"] + (np.array(g["signed"].shape) - 1) * g["spacing"]
    ax = [np.arange(n) * h + o for n, h, o in zip(g["signed"].shape, g["spacing"], g["origin"])]
    corners = np.array([g["origin"], [ax[0][-1], ax[1][-1], ax[2][-1]], [ax[0][-1], g["origin"][1], ax[2][3]]])
    assert np.abs(corners[1] - hi).max() < 1e-12
    itp = interpolate.RegularGridInterpolator(ax, g["signed"].astype(np.float64), bounds_error=False, fill_value=1e99)
    sp = [np.asarray(a[1] - a[0]) for a in ax]
    gt, inb = em.trilinear(g["signed"], sp, g["origin"], corners)
    assert inb[0] and inb[2] and np.abs(gt[[0, 2]] - itp(corners)[[0, 2]]).max() <= 1e-12
    out = corners[0].copy()
    out[0] = np.nextafter(out[0], -np.inf)
    assert not em.trilinear(g["signed"], g["spacing"], g["origin"], out[None])[1][0] and itp(out[None])[0] == 1e99


def test_float64_model_equals_the_reference_record(g):
    for name in ("signed", "zeroed"):
        rec, gt, valid = em.sdf_metrics(g[name], g["spacing"], g["origin"], g["pts"], g["sdf"], exclude_zero_gt=True)
        inb = g[name + "/in_bounds"]
        assert np.array_equal(valid, g[name + "/valid"])
        assert int(rec[0]) == valid.sum() and int(rec[1]) == inb.sum()
        assert np.abs(gt[inb] - g[name + "/gt"][inb]).max() <= 1e-12 * max(1.0, np.abs(g[name + "/gt"]).max())
        assert np.array_equal(rec[9:15].astype(np.int64), g[name + "/bin_counts"])
        res = em.result_dict(rec)
        np.testing.assert_allclose(res["av_l1"], g[name + "/av_l1"][0], rtol=1e-12)
        ref_bins = g[name + "/binned_l1"]
        assert np.array_equal(np.isnan(res["binned_l1"]), np.isnan(ref_bins))
        np.testing.assert_allclose(res["binned_l1"], ref_bins, rtol=1e-12)
        np.testing.assert_allclose(res["binned_l1"], g[name + "/binned_l1_np"], rtol=1e-12)
        np.testing.assert_allclose(rec[15:24:3] / rec[0], g[name + "/chomp_diff_means"], rtol=1e-12)
        # Trainer.eval_sdf evaluates the predicted cost in float32 (a torch tensor): its recorded means agree to that precision
        np.testing.assert_allclose(res["l1_chomp_costs"], g[name + "/l1_chomp_costs"], rtol=0, atol=4 * np.finfo(np.float32).eps)
        np.testing.assert_allclose(rec[16:24:3], g[name + "/pred_chomp_sums"], rtol=1e-12)
        np.testing.assert_allclose(rec[17:24:3], g[name + "/gt_chomp_sums"], rtol=1e-12)
        keep, _, _ = em.sdf_metrics(g[name], g["spacing"], g["origin"], g["pts"], g["sdf"], exclude_zero_gt=False)
        assert int(keep[0]) == inb.sum()
        np.testing.assert_allclose(keep[2] / keep[0], g[name + "/l1_keep_zero"][0], rtol=1e-12)
    assert np.isnan(g["zeroed/binned_l1"][0]) and g["zeroed/bin_counts"][0] == 0       # the empty bin is in the fixture
    assert (g["zeroed/in_bounds"] & (g["zeroed/gt"] == 0)).sum() > 100                 # ... and so is zero-valued ground truth


def test_fixture_masks_are_decidable_in_float32(g):
    """what make_eval_golden.py promises: no point near a bin limit, a CHOMP epsilon, zero or a face, so float32 decides alike"""
    assert len(g["pts"]) > 0.99 * int(g["n_generated"][0])
    for name in ("signed", "zeroed"):
        gt32, inb32 = em.trilinear32(g[name], g["spacing"], g["origin"], g["pts"])
        assert np.array_equal(inb32, g[name + "/in_bounds"])
        assert np.array_equal(inb32 & (gt32 != 0), g[name + "/valid"])
        inb = inb32
        assert np.abs(gt32[inb].astype(np.float64) - g[name + "/gt"][inb]).max() < 5e-6
        for e in (0.1, 0.2, 0.5, 1.0, 1.5, 2.0):
            assert np.abs(g[name + "/gt"][inb] - e).min() >= 1e-5


def test_nearest_neighbour_model_equals_ckdtree(g):
    """float32 squared distances of the differences: each difference, square and sum rounds once (relative 2^-24 each), so the
    squared distance is within 5 * 2^-24 relative of the exact one and its root within 3 * 2^-24 -- asserted at 4e-7"""
    spatial = pytest.importorskip("scipy.spatial")
    a, b = g["rec_points"], g["gt_points"]
    d2, idx = em.nn_sq_dist32(a, b)
    ref, ref_idx = spatial.cKDTree(b.astype(np.float64)).query(a.astype(np.float64))
    d = np.sqrt(d2.astype(np.float64))
    assert np.abs(d - ref).max() <= 4e-7 * ref.max()
    assert (idx == ref_idx).mean() > 0.999
    np.testing.assert_allclose(em.nn_dist64(a, b), ref, rtol=1e-12)
    np.testing.assert_allclose(em.nn_dist64(a, b).mean(), g["accuracy"][0], rtol=1e-12)
    np.testing.assert_allclose(em.nn_dist64(b, a).mean(), g["completion"][0], rtol=1e-12)
    # duplicate targets: the lowest index wins
    t = np.concatenate([b[:50], b[:50]])
    assert nn_lowest(a[:200], t)


def nn_lowest(q, t):
    _, idx = em.nn_sq_dist32(q, t)
    return bool((idx < 50).all())


# ------------------------------------------------------------------ isdf_amd.metrics, host objects
class _Itp:
    def __init__(self, grid, values):
        self.grid, self.values = grid, values


def test_gt_volume_reads_grid_and_values_only(g):
    from isdf_amd.metrics import GtVolume
    ax = tuple(np.arange(n) * h + o for n, h, o in zip(g["signed"].shape, g["spacing"], g["origin"]))
    v = GtVolume.from_interpolator(_Itp(ax, g["signed"].astype(np.float64)), "cpu")
    assert v.values.dtype == torch.float32 and tuple(v.values.shape) == g["signed"].shape
    np.testing.assert_allclose(v.spacing, g["spacing"], rtol=1e-12)
    np.testing.assert_allclose(v.origin, g["origin"], rtol=1e-12)
    c = v.to_c()
    assert (c.nx, c.ny, c.nz) == g["signed"].shape and c.values == v.values.data_ptr()
    uneven = (ax[0], ax[1], np.concatenate([ax[2][:-1], [ax[2][-1] + 0.01]]))
    with pytest.raises(ValueError):
        GtVolume.from_interpolator(_Itp(uneven, g["signed"]), "cpu")
    with pytest.raises(ValueError):
        GtVolume.from_interpolator(_Itp((ax[0][::-1], ax[1], ax[2]), g["signed"]), "cpu")
    with pytest.raises(ValueError):
        GtVolume(g["signed"], (0.1, -0.1, 0.1), (0, 0, 0), "cpu")


class EvalFakeEngine(FakeEngine):
    """FakeEngine + the two evaluation calls, answered by the float64 model (same return contract as engine.Engine)"""

    def sdf_metrics(self, volume, pts, sdf, exclude_zero_gt=True, per_point=False, oob_fill=0.0):
        rec, gt, valid = em.sdf_metrics(volume.values.numpy().astype(np.float64), volume.spacing, volume.origin,
                                        pts.detach().double().numpy(), sdf.detach().double().numpy(), exclude_zero_gt)
        self.calls.append("sdf_metrics")
        if not per_point:
            return torch.from_numpy(rec), None, None
        gt = np.where(valid | (gt != 0), gt, oob_fill)
        return torch.from_numpy(rec), torch.from_numpy(gt.astype(np.float32)), torch.from_numpy(valid.astype(np.uint8))

    def nn_distance(self, query, target, want_index=False):
        d2, idx = em.nn_sq_dist32(query.numpy(), target.numpy())
        d = np.sqrt(d2)
        self.calls.append("nn_distance")
        return (torch.from_numpy(d), torch.from_numpy(idx.astype(np.int32)) if want_index else None,
                torch.tensor([d.astype(np.float64).sum()], dtype=torch.float64))


def test_metrics_module_names_the_record(g):
    from isdf_amd import metrics
    from isdf_amd.engine import NetConfig
    eng = EvalFakeEngine(NetConfig(hidden=64, blocks=1))
    for name in ("signed", "zeroed"):
        vol = metrics.GtVolume(g[name], g["spacing"], g["origin"], "cpu")
        m = metrics.sdf_metrics(eng, vol, torch.from_numpy(g["pts"]), torch.from_numpy(g["sdf"]))
        assert m.n_valid == g[name + "/valid"].sum() and m.n_in_bounds == g[name + "/in_bounds"].sum()
        assert list(m.bin_counts) == list(g[name + "/bin_counts"])
        d = m.as_dict()
        assert sorted(d) == ["av_l1", "binned_l1", "l1_chomp_costs"] and len(d["binned_l1"]) == 6 and len(d["l1_chomp_costs"]) == 3
        np.testing.assert_allclose(d["av_l1"], g[name + "/av_l1"][0], rtol=1e-12)
        np.testing.assert_allclose(d["binned_l1"], g[name + "/binned_l1"], rtol=1e-12)
        np.testing.assert_allclose(m.gt_chomp_sums, g[name + "/gt_chomp_sums"], rtol=1e-12)
    empty = metrics.SdfMetrics(np.zeros(24))
    assert np.isnan(empty.av_l1) and all(np.isnan(empty.binned_l1)) and all(np.isnan(empty.l1_chomp_costs))
    acc, comp = metrics.accuracy_completion(eng, g["gt_points"], g["rec_points"])
    np.testing.assert_allclose([acc, comp], [g["accuracy"][0], g["completion"][0]], rtol=1e-6)


# ------------------------------------------------------------------ the bound methods on the real reference Trainer
@pytest.fixture(scope="module")
def ref_mods():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden as mg
    with contextlib.redirect_stdout(io.StringIO()):
        mods = mg.import_reference()
    return mg, mods


class CountingInterp:
    """scipy's interpolator behind a call counter; `.grid` / `.values` and the two attributes eval_sdf_interp sets pass through"""

    def __init__(self, itp):
        self.__dict__["itp"], self.__dict__["n_calls"] = itp, 0

    def __getattr__(self, k):
        return getattr(self.itp, k)

    def __setattr__(self, k, v):
        setattr(self.itp, k, v)

    def __call__(self, x):
        self.__dict__["n_calls"] += 1
        return self.itp(x)


def _field(p):
    return np.linalg.norm(p - np.array([0.3, 0.2, 2.0]), axis=-1) - 1.0


def _eval_trainer(mg, mods, tmp_path, grafted):
    from tests.test_graft_reference import _reference_trainer
    from isdf.datasets import sdf_util
    g3 = gu.load("step_small_k3")
    tr = _reference_trainer(mg, mods, g3)
    ax = [np.arange(49) * 0.25 - 6.0] * 3
    vol = _field(np.stack(np.meshgrid(*ax, indexing="ij"), -1)).astype(np.float32).astype(np.float64)
    T = np.eye(4)
    T[[0, 1, 2], [0, 1, 2]] = 0.25
    T[:3, 3] = -6.0
    tr.gt_sdf_interp = CountingInterp(sdf_util.sdf_interpolator(vol, T))
    tr.cached_dataset = em.CountingDataset(g3["depth_batch"], g3["T_WC_batch"], 90)
    tr.fps, tr.dataset_format, tr.tot_step_time, tr.up_ix = 30, "replicaCAD", 1.0, 1
    tr.last_is_keyframe, tr.optim_frames = False, 0
    # two evaluation boxes: one in free space in front of the first camera (visible), one far outside every frustum
    c = (g3["T_WC_batch"][0] @ np.array([0.0, 0.0, 0.4, 1.0]))[:3]
    bounds = np.array([[c - 0.02, c + 0.02], [[40, 40, 40], [40.1, 40.1, 40.1]]])
    bounds[:, 1] -= 0.08                                  # get_obj_eval_bounds expands the top by 0.08 and the sides' bottom
    bounds[:, 0, [0, 2]] += 0.08
    tr.obj_bounds_file = str(tmp_path / ("bounds%d.txt" % grafted))
    np.savetxt(tr.obj_bounds_file, bounds.reshape(-1, 6))
    traj = np.tile(np.eye(4).reshape(1, 16), (200, 1))
    s = np.linspace(0, 1, 200)
    traj[:, 3], traj[:, 7], traj[:, 11] = -2 + 3 * s, 0.5 * np.sin(3 * s), -1 + 2.5 * s
    tr.traj_file = str(tmp_path / ("traj%d.txt" % grafted))
    np.savetxt(tr.traj_file, traj)
    if grafted:
        from isdf_amd.hot_path import graft
        with contextlib.redirect_stdout(io.StringIO()):
            graft(tr, rng="torch", engine_factory=EvalFakeEngine)
    return tr


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    assert np.array_equal(np.isnan(a), np.isnan(b)), (what, a, b)
    ok = ~np.isnan(a)
    assert np.abs(a[ok] - b[ok]).max(initial=0.0) <= 1e-6 * np.maximum(1.0, np.abs(b[ok])).max(initial=1.0), (what, a, b)


@needs_ref
def test_bound_evaluation_equals_the_reference_methods(ref_mods, tmp_path):
    mg, mods = ref_mods
    from isdf_amd.hot_path import HotPath
    ref, hip = _eval_trainer(mg, mods, tmp_path, False), _eval_trainer(mg, mods, tmp_path, True)
    for name in ("eval_sdf", "eval_sdf_visible", "eval_object_sdf", "eval_traj_cost", "eval_mesh"):
        assert getattr(type(hip), name) is getattr(HotPath, name), name
    out = {}
    for key, tr in (("ref", ref), ("hip", hip)):
        torch.manual_seed(11); np.random.seed(11)
        with contextlib.redirect_stdout(io.StringIO()):
            out[key] = dict(sdf=tr.eval_sdf(samples=3000, visible_region=True), obj=tr.eval_object_sdf(samples=500),
                            traj=tr.eval_traj_cost(), short=tr.eval_traj_cost(t_ahead=0.5),
                            after=torch.rand(1).item())
    r, h = out["ref"], out["hip"]
    assert sorted(h["sdf"]) == sorted(r["sdf"]) == ["av_l1", "binned_l1", "l1_chomp_costs"]
    assert len(h["sdf"]["binned_l1"]) == 6 and len(h["sdf"]["l1_chomp_costs"]) == 3
    for k in r["sdf"]:
        _close(h["sdf"][k], r["sdf"][k], k)
    assert np.isfinite(r["sdf"]["av_l1"]) and np.isfinite(r["sdf"]["binned_l1"][2:]).all()
    assert len(h["obj"]) == len(r["obj"]) == 2 and np.isfinite(r["obj"][0]) and np.isnan(r["obj"][1])
    _close(h["obj"], r["obj"], "eval_object_sdf")
    assert len(h["traj"]) == 2 and len(h["traj"][0]) == len(h["traj"][1]) == 3
    _close(h["traj"][0], r["traj"][0], "pred chomp sums")
    _close(h["traj"][1], [float(v) for v in r["traj"][1]], "gt chomp sums")
    assert np.isnan(r["short"][0]) and np.isnan(r["short"][1]) and np.isnan(h["short"][0]) and np.isnan(h["short"][1])
    assert h["after"] == r["after"]                       # the torch generator advanced exactly as in the reference
    assert ref.gt_sdf_interp.n_calls > 0 and hip.gt_sdf_interp.n_calls == 0
    assert hip._hip.gt_volume[0] is hip.gt_sdf_interp
    hip.gt_sdf_interp = CountingInterp(hip.gt_sdf_interp.itp)       # replaced: the volume is made again
    old = hip._hip.gt_volume[1]
    hip.eval_traj_cost()
    assert hip._hip.gt_volume[1] is not old and hip.gt_sdf_interp.n_calls == 0


@needs_ref
def test_eval_frames_stay_resident_and_only_new_ones_are_read(ref_mods, tmp_path):
    mg, mods = ref_mods
    hip = _eval_trainer(mg, mods, tmp_path, True)
    ds = hip.cached_dataset
    torch.manual_seed(3)
    sdf, pts = hip.eval_sdf_visible(600)
    assert ds.reads == [30] and sdf.dim() == 1 and pts.shape == (sdf.shape[0], 3)
    first = hip._hip.eval_cache.uploaded_bytes
    hip.tot_step_time += 1.0
    hip.eval_sdf_visible(600)
    assert ds.reads == [30, 30]                                        # the 30 new frames, not the 60 of the sequence so far
    H, W = hip.H, hip.W
    assert hip._hip.eval_cache.uploaded_bytes - first == 30 * (H * W + 16) * 4
    depth, T = hip._eval_frames()
    assert depth.shape[0] == 60 and len(ds.reads) == 2                 # a call at the same clock reads nothing
    k = np.arange(60) % len(ds.depth)
    assert np.array_equal(depth.numpy(), ds.depth[k]) and np.array_equal(T.numpy(), ds.T[k])
    hip.eval_object_sdf(samples=50)                                    # shares the cache
    assert len(ds.reads) == 2
    assert "eval_cache" not in hip.hip_state_dict() and all("eval" not in k for k in hip.hip_state_dict())
    hip.drop_eval_cache()
    assert hip._hip.eval_cache is None
    hip.eval_sdf_visible(600)
    assert ds.reads == [30, 30, 60]
    hip.incremental = False                                            # the whole sequence, once
    hip.eval_sdf_visible(900)
    hip.eval_sdf_visible(900)
    assert ds.reads == [30, 30, 60, 90]


@needs_ref
def test_eval_mesh_runs_both_nearest_neighbour_passes_on_the_engine(ref_mods, tmp_path):
    """mesh_rec and trimesh are not available without a GPU / the package: stand-ins record the calls and hand over point sets"""
    mg, mods = ref_mods
    hip = _eval_trainer(mg, mods, tmp_path, True)
    g = em.load_golden()
    calls = []
    fake_tm = types.SimpleNamespace(
        load=lambda f: calls.append(("load", f)) or "GT",
        sample=types.SimpleNamespace(sample_surface=lambda mesh, n: calls.append(("sample", mesh, n)) or
                                     ((g["gt_points"] if mesh == "GT" else g["rec_points"]), None)))
    hip._hip.ref_module = types.SimpleNamespace(trimesh=fake_tm)
    hip.scene_file = "scene.obj"
    hip.mesh_rec = lambda: calls.append(("mesh_rec",)) or "REC"
    hip.engine.calls.clear()
    acc, comp = hip.eval_mesh(samples=1234)
    assert calls == [("load", "scene.obj"), ("mesh_rec",), ("sample", "REC", 1234), ("sample", "GT", 1234)]   # metrics.py:62-68
    assert hip.engine.calls == ["nn_distance", "nn_distance"]
    np.testing.assert_allclose([acc, comp], [g["accuracy"][0], g["completion"][0]], rtol=1e-6)
