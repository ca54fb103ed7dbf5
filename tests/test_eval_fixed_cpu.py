"""Trainer.eval_fixed behind graft(), host side (no GPU): the float64 numpy model of isdf_region_metrics
(tests/eval_fixed_model.py) against what the reference's eval_pts.fixed_pts_eval recorded (fixture eval_fixed_small,
tests/golden/make_eval_fixed_golden.py), the flag construction against the reference's chained boolean indexing, and the bound
method on the REAL reference Trainer next to the unbound one on a twin, with an engine stand-in that answers region_metrics from
the model."""
import contextlib
import io
import json
import os
import warnings

import numpy as np
import pytest
import torch

from tests import eval_fixed_model as fm
from tests import eval_model as em
from tests import golden_util as gu
from tests.test_eval_cpu import CountingInterp, EvalFakeEngine, _close, _field, needs_ref, ref_mods  # noqa: F401

EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def g():
    return fm.load_golden()


def _compare_with_recorded(res, g, rtol):
    """every figure of a result dict against the fixture's: same keys, same NaN pattern; means to rtol, the CHOMP figures to
    4 * eps32 (the reference forms the predicted cost in float32, as test_eval_cpu.py explains)"""
    flat = fm.flatten(res)
    recorded = {k[4:]: v for k, v in g.items() if k.startswith("res/")}
    assert sorted(flat) == sorted(recorded)
    for k, want in recorded.items():
        got = flat[k]
        assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), k
        ok = ~np.isnan(want)
        if k.endswith("l1_chomp_costs"):
            assert np.abs(got[ok] - want[ok]).max(initial=0.0) <= 4 * EPS32, k
        else:
            assert np.abs(got[ok] - want[ok]).max(initial=0.0) <= rtol * np.abs(want[ok]).max(initial=1.0), (k, got, want)


# ------------------------------------------------------------------ the model against the reference's record
def test_float64_model_reproduces_the_recorded_result(g):
    """Every figure to 1e-12 relative (CHOMP: 4 * eps32).  av_cossim needs the reference's own arithmetic for that: torch
    normalises the float32 predicted gradient in float32 before the float64 product (fm.cos_distance_reference).  The kernel's
    formula, which widens the gradient first, is then within the float32 roundings of that normalisation -- under 4 * eps32 per
    point, hence for the mean.  Measured on this fixture: vis 1.50e-10, vox 2.23e-10 absolute (1.9e-8 and 1.7e-8 relative)."""
    def reference_arithmetic(*a, **k):
        return fm.region_records(*a, cos_fn=fm.cos_distance_reference, **k)
    _compare_with_recorded(fm.result_from_fixture(g, reference_arithmetic), g, 1e-12)
    assert len(g["vis_pts"]) == len(g["gt_grad_all"]) and len(g["obj_ids"]) == 2
    widened = fm.result_from_fixture(g)
    for name in ("vis", "vox"):
        got, want = widened["rays"][name]["av_cossim"], g["res/rays.%s.av_cossim" % name]
        print("av_cossim %s: widened %.15g recorded %.15g" % (name, got[0], want[0]))
        assert np.abs(np.asarray(got) - want).max() <= 4 * EPS32
        widened["rays"][name]["av_cossim"] = want.tolist()
    _compare_with_recorded(widened, g, 1e-12)                                # everything else is the same arithmetic


def test_float64_model_reproduces_the_recorded_ground_truth_gradient(g):
    grad = fm.gt_gradient(g["volume"], g["spacing"], g["origin"], g["vis_pts"].astype(np.float64), 0.01)
    ref = g["gt_grad_all"]
    assert np.array_equal(np.isnan(grad), np.isnan(ref)) and np.isnan(ref).any()
    ok = ~np.isnan(ref)
    assert np.abs(grad[ok] - ref[ok]).max() <= 1e-12 * max(1.0, np.abs(ref[ok]).max())
    # the gradient mask selects finite gradients only, so the recorded av_cossim is finite
    assert np.isfinite(ref[g["vis_valid_gt_grad"]]).all()
    assert np.isfinite(g["res/rays.vis.av_cossim"]).all() and np.isfinite(g["res/rays.vox.av_cossim"]).all()


def test_fixture_keeps_what_its_generator_promises(g):
    dropped, total = (int(v) for v in g["n_dropped"])
    assert dropped < 0.01 * total
    for name in ("vis", "surf", "obj0", "obj2"):
        A, B = g[name + "_valid_gt_sdf"], g[name + "_valid_vox_sdf"]
        assert A.mean() >= 0.5 and 0.3 <= B.mean() <= 0.7 and len(B) == A.sum(), name
    gt, inb = em.trilinear(g["volume"], g["spacing"], g["origin"], g["vis_pts"].astype(np.float64))
    sel = g["vis_valid_gt_sdf"]
    assert inb[sel].all() and (gt[sel] < 0).sum() > 50 and (gt[sel] == 0).sum() > 50
    for e in (0.1, 0.2, 0.5, 1.0, 1.5, 2.0):
        assert np.abs(gt[sel] - e).min() >= 1e-5
    assert "obj1_valid_gt_sdf" not in g and len(g["obj_bounds_raw"]) == 3       # the middle object has no files: skipped


def test_cosine_distance_is_torchs(g):
    cos = torch.nn.CosineSimilarity(dim=1, eps=1e-6)
    x, y = np.array([[1e-8, 0, 0], [1.0, 2.0, -0.5], [0, 0, 0]]), np.array([[1e-3, 0, 0], [0.3, -0.1, 0.9], [1.0, 0, 0]])
    want = 1 - cos(torch.tensor(x), torch.tensor(y)).numpy()
    np.testing.assert_allclose(fm.cos_distance(x, y), want, rtol=1e-14, atol=1e-16)
    assert abs((1 - fm.cos_distance(x, y))[0] - 0.01) < 1e-15                    # not 1e-5: each norm is clamped on its own


# ------------------------------------------------------------------ flags
def test_flag_construction_selects_the_reference_index_sets(g):
    from isdf_amd import _ffi
    from isdf_amd.hot_path import HotPath
    A, B, G = g["vis_valid_gt_sdf"], g["vis_valid_vox_sdf"], g["vis_valid_gt_grad"]
    flags = HotPath._region_flags(A, B, G)
    assert flags.dtype == np.uint8 and np.array_equal(flags, fm.chained_flags(A, B, G))
    n = len(A)
    ix = np.arange(n)
    # eval_pts.py:130-152, the reference's own chained indexing on an index array
    vis_sdf = ix[A]
    vox_sdf = ix[A][B]
    vis_grad = ix[G]
    vox_grad = ix[A][B][G[A][B]]
    for bit, want in ((_ffi.FLAG_VIS_SDF, vis_sdf), (_ffi.FLAG_VOX_SDF, vox_sdf), (_ffi.FLAG_VIS_GRAD, vis_grad),
                      (_ffi.FLAG_VOX_GRAD, vox_grad)):
        assert np.array_equal(np.nonzero(flags & bit)[0], want), bit
    assert len(vox_grad) > 0 and len(vox_grad) < len(vis_grad) and (G & ~A).any()
    surf = HotPath._region_flags(g["surf_valid_gt_sdf"], g["surf_valid_vox_sdf"])
    assert np.array_equal(surf, fm.chained_flags(g["surf_valid_gt_sdf"], g["surf_valid_vox_sdf"])) and (surf & 12).max() == 0


# ------------------------------------------------------------------ isdf_amd.metrics host objects
class FixedFakeEngine(EvalFakeEngine):
    """EvalFakeEngine + region_metrics answered by the float64 model (same return contract as engine.Engine)"""

    def region_metrics(self, pts, sdf, volume=None, gt=None, sdf_grad=None, flags=None, delta=0.01, out=None):
        assert (volume is None) != (gt is None)
        kw = {} if volume is None else dict(values=volume.values.numpy().astype(np.float64), spacing=volume.spacing,
                                            origin=volume.origin)
        rec = fm.region_records(pts.detach().float().numpy(), sdf.detach().numpy(), gt=None if gt is None else gt.numpy(),
                                sdf_grad=None if sdf_grad is None else sdf_grad.detach().numpy(),
                                flags=None if flags is None else flags.numpy(), delta=delta, **kw)
        self.calls.append("region_metrics")
        rec = torch.from_numpy(rec)
        if out is not None:
            out.copy_(rec)
            return out
        return rec


def test_metrics_module_names_the_region_records(g):
    from isdf_amd import metrics
    from isdf_amd.engine import NetConfig
    eng = FixedFakeEngine(NetConfig(hidden=64, blocks=1))
    vol = metrics.GtVolume(g["volume"], g["spacing"], g["origin"], "cpu")
    vis, vox = metrics.region_metrics(eng, torch.from_numpy(g["vis_pts"]), torch.from_numpy(g["vis_sdf"]), volume=vol,
                                      sdf_grad=torch.from_numpy(g["vis_grad"]), flags=torch.from_numpy(g["vis_flags"]))
    res = {"vis": vis.as_dict(cossim=True), "vox": vox.as_dict(cossim=True)}
    for k, v in fm.flatten(res).items():
        atol = 4 * EPS32 if "chomp" in k else 1e-9 if "cossim" in k else 0     # (av_cossim: see the first test's docstring)
        np.testing.assert_allclose(v, g["res/rays." + k], rtol=0 if atol else 1e-9, atol=atol)
    assert vis.n_grad == g["vis_valid_gt_grad"].sum() and vis.n_grad_nonfinite == 0 and vox.sdf.n_valid == g["vis_valid_vox_sdf"].sum()
    json.dumps(res)
    rec = np.zeros(27)
    rec[24], rec[25], rec[26] = 5, 1.0, 1
    assert np.isnan(metrics.RegionMetrics(rec).av_cossim)                        # a non-finite ground-truth gradient: NaN
    rec[26] = 0
    assert metrics.RegionMetrics(rec).av_cossim == 0.2
    assert np.isnan(metrics.RegionMetrics(np.zeros(27)).av_cossim)               # an empty set: 0 / 0


# ------------------------------------------------------------------ the bound method on the real reference Trainer
SEQ_LEN, KEEP_EVERY = 60, 5


def _tree(mods, tr, root, times):
    """the files fixed_pts_eval reads for `tr`, made with the reference's own sampling functions: masks that select in-bounds
    points (thinned at random, so that every set is a proper part of its parent), three object boxes of which the middle one has
    no files, a full-volume point file"""
    from isdf.datasets import sdf_util
    from isdf.eval import eval_pts
    rng = np.random.RandomState(5)
    itp, ds = tr.gt_sdf_interp.itp, tr.cached_dataset
    c = (ds.T[0] @ np.array([0.0, 0.0, 0.4, 1.0]))[:3]
    obj_raw = np.array([[c - 0.1, c + 0.1], [c + 1.0, c + 1.2], [c - 0.3, c - 0.1]])
    vol_pts = rng.uniform(-2, 2, size=(500, 3))
    vol_gt = _field(vol_pts) + 0.01 * rng.standard_normal(500)
    out = None
    for t in times:
        t_str = f"{t:.3f}"
        sample = ds[np.arange(0, min(np.floor(t * 30), SEQ_LEN)).astype(int)]
        ds.reads.clear()
        depth_batch, T_WC_batch = torch.FloatTensor(sample["depth"]), torch.FloatTensor(sample["T"])
        dirs_C = tr.dirs_C.cpu()
        vis = eval_pts.sample_visible_region(t_str, depth_batch, T_WC_batch, "replicaCAD", dirs_C).numpy().astype(np.float64)
        surf = eval_pts.sample_surface(t_str, depth_batch, T_WC_batch, dirs_C).numpy().astype(np.float64)
        masks = {}
        for name, p in (("vis", vis), ("surf", surf), ("obj0", eval_pts.object_eval_pts(fm.load_obj_bounds(obj_raw)[0])),
                        ("obj2", eval_pts.object_eval_pts(fm.load_obj_bounds(obj_raw)[2]))):
            _, inb = sdf_util.eval_sdf_interp(itp, p, handle_oob="mask")
            A = inb & (rng.uniform(size=len(p)) > 0.1)
            masks[name + "_valid_gt_sdf"], masks[name + "_valid_vox_sdf"] = A, rng.uniform(size=A.sum()) > 0.5
        _, ok = eval_pts.eval_grad(itp, vis, 0.01, is_gt_sdf=True)
        G = ok & (rng.uniform(size=len(vis)) > 0.2)
        masks["vis_valid_gt_grad"], masks["vis_valid_vox_grad"] = G, rng.uniform(size=G.sum()) > 0.5
        assert G.sum() > 100 and (G & ~masks["vis_valid_gt_sdf"]).any()
        out = fm.write_tree(root, t_str, masks, obj_raw, vol_pts, vol_gt)
    return out


def _fixed_trainer(mg, mods, grafted):
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
    k = np.arange(SEQ_LEN // KEEP_EVERY) % len(g3["depth_batch"])
    tr.cached_dataset = fm.KeepIxsDataset(g3["depth_batch"][k], g3["T_WC_batch"][k], np.arange(0, SEQ_LEN, KEEP_EVERY))
    tr.scene_dataset = range(SEQ_LEN)
    tr.fps, tr.dataset_format, tr.tot_step_time, tr.up_ix = 30, "replicaCAD", 1.0, 1
    tr.last_is_keyframe, tr.optim_frames = False, 0
    if grafted:
        from isdf_amd.hot_path import graft
        with contextlib.redirect_stdout(io.StringIO()):
            graft(tr, rng="philox", engine_factory=FixedFakeEngine)       # philox: the draws are the torch CPU generator's all the same
    return tr


def _run(tr):
    torch.manual_seed(11); np.random.seed(11)
    with contextlib.redirect_stdout(io.StringIO()):
        res = tr.eval_fixed()
    return res, torch.rand(1).item(), np.random.rand()


def _same(a, b):
    fa, fb = fm.flatten(a), fm.flatten(b)
    assert list(fa) == list(fb)
    for k in fa:
        _close(fa[k], fb[k], k)


@needs_ref
def test_bound_eval_fixed_equals_the_reference_method(ref_mods, tmp_path):
    mg, mods = ref_mods
    from isdf_amd.hot_path import HotPath
    ref, hip = _fixed_trainer(mg, mods, False), _fixed_trainer(mg, mods, True)
    assert type(hip).eval_fixed is HotPath.eval_fixed and type(ref).eval_fixed is not HotPath.eval_fixed
    dirs = _tree(mods, ref, tmp_path, [0.5, 1.0])
    for tr in (ref, hip):
        tr.eval_pts_dir, tr.seq_dir, tr.eval_pts_root = dirs
        tr.eval_times = [0.5, 1.0]
    draws = hip._hip.draw_count
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                      # no selected point is out of bounds: no warning
        h, h_torch, h_numpy = _run(hip)
    r, r_torch, r_numpy = _run(ref)
    assert ref.eval_times == [1.0] and hip.eval_times == [1.0]              # popped once
    assert list(h) == list(r) == ["time", "rays", "visible_surf", "objects", "vol"] and h["time"] == 0.5
    assert len(h["objects"]) == len(r["objects"]) == 2                       # the object without files is skipped
    _same(h, r)
    assert np.isfinite(r["rays"]["vis"]["av_cossim"]).all() and np.isfinite(r["rays"]["vox"]["av_l1"])
    json.dumps(h)
    assert h_torch == r_torch and h_numpy == r_numpy                        # both generators are where the reference leaves them
    assert ref.gt_sdf_interp.n_calls > 0 and hip.gt_sdf_interp.n_calls == 0
    assert hip.engine.calls.count("sample") == 1 and hip.engine.calls.count("region_metrics") == 5
    assert hip._hip.draw_count == draws
    # a later timestamp reads only the new frames
    ds = hip.cached_dataset
    assert ds.reads == [3] and hip._hip.eval_cache.uploaded_frames == 3
    h2, _, _ = _run(hip)
    r2, _, _ = _run(ref)
    _same(h2, r2)
    assert ds.reads == [3, 3] and hip._hip.eval_cache.uploaded_frames == 6 and hip.eval_times == []
    depth, T = hip._eval_frames()                                           # the clock's 30 frames are the 6 held: nothing is read
    assert depth.shape[0] == 6 and ds.reads == [3, 3]


@needs_ref
def test_a_prefix_of_the_resident_frames_uploads_nothing(ref_mods, tmp_path):
    mg, mods = ref_mods
    hip = _fixed_trainer(mg, mods, True)
    hip.eval_pts_dir, hip.seq_dir, hip.eval_pts_root = _tree(mods, hip, tmp_path, [0.5])
    ds = hip.cached_dataset
    torch.manual_seed(3)
    hip.eval_sdf_visible(600)                                               # the clock stands at 1.0 s: indices 0..29, 6 held
    assert ds.reads == [6]
    bytes_before = hip._hip.eval_cache.uploaded_bytes
    hip.eval_times = [0.5]
    first, _, _ = _run(hip)
    assert ds.reads == [6] and hip._hip.eval_cache.uploaded_bytes == bytes_before and hip._hip.eval_cache.uploaded_frames == 6
    depth, _ = hip._eval_frames(15)
    assert depth.shape[0] == 3 and hip._eval_frames()[0].shape[0] == 6 and ds.reads == [6]
    # ... and gives what a fresh cache gives
    hip.drop_eval_cache()
    hip.eval_times = [0.5]
    again, _, _ = _run(hip)
    assert ds.reads == [6, 3]
    fa, fb = fm.flatten(first), fm.flatten(again)
    for k in fa:
        assert np.array_equal(fa[k], fb[k], equal_nan=True), k


@needs_ref
def test_out_of_bounds_selection_is_left_out_with_one_warning(ref_mods, tmp_path):
    mg, mods = ref_mods
    hip = _fixed_trainer(mg, mods, True)
    dirs = _tree(mods, hip, tmp_path, [0.5])
    hip.eval_pts_dir, hip.seq_dir, hip.eval_pts_root = dirs
    # a full-volume file is no mask; select an object box far outside the grid instead
    raw = np.loadtxt(dirs[1] + "obj_bounds.txt").reshape(-1, 2, 3)
    raw[0] += 100.0
    np.savetxt(dirs[1] + "obj_bounds.txt", raw.reshape(-1, 6))
    hip.eval_times = [0.5]
    with pytest.warns(UserWarning, match="outside the ground-truth grid") as rec:
        res, _, _ = _run(hip)
    assert len([w for w in rec if "outside the ground-truth grid" in str(w.message)]) == 1
    assert np.isnan(res["objects"][0]["vis"]["av_l1"]) and np.isfinite(res["objects"][1]["vis"]["av_l1"])
    hip.dataset_format, hip.eval_times = "realsense", [0.5]                  # another format: the reference's own method, which fails
    with pytest.raises(Exception):
        hip.eval_fixed()
