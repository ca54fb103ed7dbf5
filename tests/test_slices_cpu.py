"""SDF slice images, host side (no GPU): the numpy float32 models of tests/slice_model.py against matplotlib and against the
colours matplotlib recorded in the fixture (tests/golden/make_slices_golden.py), isdf_amd.slices' host objects, and the three slice
methods graft() binds -- on the REAL reference Trainer with an engine stand-in that answers slice_images / plane_points /
nn_distance from the models, against the reference's own unbound methods on the same object.  cv2 and imgviz are not installed
here: stand-ins record what they are handed (agreement of anything behind them with the real packages is not checked)."""
import contextlib
import io
import os
import sys
import types
from unittest import mock

import numpy as np
import pytest
import torch

from tests import eval_model as em
from tests import golden_util as gu
from tests import render_oracle as ro
from tests import slice_model as sm
from tests.fake_engine import FakeEngine

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "isdf")), reason="reference checkout not present")
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def g():
    return sm.load_golden()


def _patch_get_cmap():
    """matplotlib >= 3.9 has no cm.get_cmap, which sdf_util.get_colormap calls: what it was"""
    import matplotlib
    from matplotlib import cm
    if not hasattr(cm, "get_cmap"):
        cm.get_cmap = lambda name, lut=None: matplotlib.colormaps[name].resampled(lut)


# ------------------------------------------------------------------ models
@pytest.mark.parametrize("name", ["t2", "t05"])
def test_colour_model_equals_the_recorded_matplotlib_colours(g, name):
    lim = g[name + "/lim"]
    got = sm.colours(g["values"], g[name + "/rgb"], lim[0], lim[1])
    assert got.dtype == np.uint8 and got.shape == g[name + "/colours"].shape
    assert np.array_equal(got, g[name + "/colours"])
    v = g["values"]
    k = sm.colour_index(v, len(g[name + "/rgb"]) - 3, lim[0], lim[1])
    N = len(g[name + "/rgb"]) - 3
    assert (k == N).sum() > 100 and (k == N + 1).sum() > 100 and (k == N + 2).sum() == np.isnan(v).sum() == 1   # under, over, bad
    assert set(k[v == np.float32(lim[1])]) == {N - 1} and set(k[v == np.float32(lim[0])]) == {0}                    # the range ends
    assert len(v) >= 20000


def test_colour_model_equals_matplotlib():
    """limits float32 holds exactly (as the reference's two tables have: -2, 2 and -0.5, 0.5): equal on every value"""
    colors = pytest.importorskip("matplotlib.colors")
    cm = pytest.importorskip("matplotlib.cm")
    from isdf_amd.slices import Colormap
    rng = np.random.RandomState(3)
    table = rng.uniform(size=(37, 4))
    cmap = colors.ListedColormap(table)
    cmap.set_under([0.1, 0.2, 0.3, 1.0]); cmap.set_over([0.9, 0.8, 0.7, 1.0]); cmap.set_bad([0.5, 0.25, 0.125, 1.0])
    v = np.concatenate([rng.uniform(-1, 2, 50000), [-0.375, 1.25, -0.37, 1.21, np.nan, np.inf, -np.inf, 0.0]]).astype(np.float32)
    m = cm.ScalarMappable(norm=colors.Normalize(-0.375, 1.25), cmap=cmap)
    ref = (m.to_rgba(v, alpha=1., bytes=False) * 255).astype(np.uint8)[..., :3]
    c = Colormap.from_scalar_mappable(m)
    assert np.array_equal(sm.colours(v, c.rgb, c.vmin, c.vmax), ref)
    one = colors.ListedColormap(table[:1])                                    # N = 1
    m1 = cm.ScalarMappable(norm=colors.Normalize(0.0, 1.0), cmap=one)
    ref1 = (m1.to_rgba(v, alpha=1., bytes=False) * 255).astype(np.uint8)[..., :3]
    c1 = Colormap.from_scalar_mappable(m1)
    assert c1.n_colors == 1 and np.array_equal(sm.colours(v, c1.rgb, 0.0, 1.0), ref1)
    # limits float32 does not hold: matplotlib subtracts and divides by the float64 limits and rounds each result to float32, the
    # rule rounds the limits first.  x differs by at most 4 roundings (2^-24 relative each, of |v| + |vmin| for the difference), so
    # the colour can differ only where x lies that close to a whole number
    lo, hi, N = -0.37, 1.21, 37
    m2 = cm.ScalarMappable(norm=colors.Normalize(lo, hi), cmap=cmap)
    ref2 = (m2.to_rgba(v, alpha=1., bytes=False) * 255).astype(np.uint8)[..., :3]
    c2 = Colormap.from_scalar_mappable(m2)
    differ = (sm.colours(v, c2.rgb, lo, hi) != ref2).any(-1)
    x = (v[differ].astype(np.float64) - lo) / (hi - lo) * N
    slack = 4 * 2.0 ** -24 * (np.abs(v[differ].astype(np.float64)) + abs(lo)) / (hi - lo) * N
    assert differ.sum() < 10 and np.all(np.abs(x - np.round(x)) <= slack)


def test_decode_index_inverts_the_table(g):
    rgb = g["t2/rgb"]
    N = len(rgb) - 3
    k = sm.colour_index(g["values"], N, -2.0, 2.0)
    dec = sm.decode_index(rgb[k], rgb)
    assert (dec >= 0).all() and np.array_equal(rgb[dec], rgb[k]) and (dec <= k).all()      # the first entry of that colour
    inside = k < N
    a, b = rgb[k[inside]], rgb[np.minimum(k[inside] + 2, N - 1)]
    d = sm.index_distance(a, b, rgb)
    assert d.max() == 2 and d.min() == 0 and (d >= 1).mean() > 0.9          # neighbours that share a colour count as one place
    assert sm.index_distance(rgb[[0]], rgb[[N]], rgb)[0] == 0 and sm.index_distance(rgb[[N + 2]], rgb[[5]], rgb)[0] == np.inf


def test_cost_and_plane_models():
    s = np.array([-1.0, 0.0, 0.5, 2.0, 2.5, np.nan], np.float32)
    c = sm.chomp32(s, 2.0)
    assert c.dtype == np.float32 and np.array_equal(c[:5], np.array([2.0, 1.0, 0.5625, 0.0, 0.0], np.float32)) and np.isnan(c[5])
    p = sm.plane_points([1, 2, 3], [0.5, 0, 0], [0, 0, -0.25], 3, 5)
    assert p.shape == (3, 5, 3) and p.dtype == np.float32
    assert p[2, 4].tolist() == [2.0, 2.0, 2.0] and p[0, 0].tolist() == [1.0, 2.0, 3.0]


# ------------------------------------------------------------------ isdf_amd.slices, host objects
def test_colormap_from_arrays_and_by_duck_typing(g):
    from isdf_amd.slices import Colormap
    src = open(os.path.join(os.path.dirname(os.path.abspath(sm.__file__)), "..", "isdf_amd", "slices.py")).read()
    assert "import matplotlib" not in src and "from matplotlib" not in src          # the product never imports it
    rgb = g["t2/rgb"]
    a = Colormap(rgb[:-3], rgb[-3], rgb[-2], rgb[-1], -2.0, 2.0)
    b = Colormap.from_scalar_mappable(sm.TableMappable(rgb, -2.0, 2.0))
    for c in (a, b):
        assert c.n_colors == 401 and np.array_equal(c.rgb, rgb) and c.lut.dtype == np.uint32 and c.lut.shape == (404,)
        assert np.array_equal(c.lut & 0xff, rgb[:, 0]) and np.array_equal(c.lut >> 16, rgb[:, 2])
        t = c.to_c("cpu")
        assert t.n_colors == 401 and t.vmin == -2.0 and t.range == 4.0 and t.lut == c._dev[torch.device("cpu")].data_ptr()
        assert c.to_c("cpu").lut == t.lut                                          # uploaded once
    assert a.key() == b.key() != Colormap(rgb[:-3], rgb[-3], rgb[-2], rgb[-1], -2.0, 2.5).key()
    for bad in (dict(vmin=1.0, vmax=1.0), dict(vmin=0.0, vmax=np.inf), dict(vmin=np.nan, vmax=1.0)):
        with pytest.raises(ValueError):
            Colormap(rgb[:-3], rgb[-3], rgb[-2], rgb[-1], **bad)
    with pytest.raises(ValueError):
        Colormap(np.zeros((0, 3), np.uint8), rgb[-3], rgb[-2], rgb[-1], 0.0, 1.0)


# ------------------------------------------------------------------ the bound methods on the real reference Trainer
def _field(p):
    """a cheap stand-in network: the synthetic room's distance with a ripple, float32"""
    from isdf_amd import synthetic
    p = np.asarray(p, np.float64)
    return (synthetic.gt_sdf(p) + 0.04 * np.sin(3.0 * p).sum(-1)).astype(np.float32)


class SliceFakeEngine(FakeEngine):
    """FakeEngine with an analytic forward (the oracle's takes seconds per slice) and the slice calls answered by the models:
    colours and costs by tests/slice_model.py, the ground truth by the float64 trilinear model rounded to float32, distances by
    the float32 nearest-neighbour model -- the return contract of engine.Engine"""

    def sdf_eval(self, pts, noise=None, want_grad=False):
        assert noise is None and not want_grad
        self.calls.append(("sdf_eval", int(pts.reshape(-1, 3).shape[0])))
        return torch.from_numpy(_field(pts.detach().numpy().reshape(-1, 3))).view(pts.shape[:-1])

    def slice_images(self, pts, sdf, cmap=None, volume=None, chomp_eps=None, oob_fill=0.0):
        self.calls.append("slice_images")
        s = None if sdf is None else sdf.detach().numpy().reshape(-1).astype(np.float32)
        out = [None] * 5
        if s is not None and cmap is not None:
            out[0] = sm.colours(s, cmap.rgb, cmap.vmin, cmap.vmax)
        if s is not None and chomp_eps is not None:
            out[3] = sm.chomp32(s, chomp_eps)
        if volume is not None:
            gt, inb = em.trilinear(volume.values.numpy().astype(np.float64), volume.spacing, volume.origin,
                                   pts.detach().numpy().reshape(-1, 3).astype(np.float64))
            gt = np.where(inb, gt, oob_fill).astype(np.float32)
            out[1] = gt
            if cmap is not None:
                out[2] = sm.colours(gt, cmap.rgb, cmap.vmin, cmap.vmax)
            if chomp_eps is not None:
                out[4] = sm.chomp32(gt, chomp_eps)
        return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)) for a in out)

    def plane_points(self, origin, du, dv, H, W):
        self.calls.append("plane_points")
        return torch.from_numpy(sm.plane_points(origin, du, dv, H, W))

    def nn_distance(self, query, target, want_index=False):
        self.calls.append("nn_distance")
        d2, idx = em.nn_sq_dist32(query.numpy(), target.numpy())
        d = np.sqrt(d2)
        return (torch.from_numpy(d), torch.from_numpy(idx.astype(np.int32)) if want_index else None,
                torch.tensor([d.astype(np.float64).sum()], dtype=torch.float64))


class CountingInterp:
    """scipy's interpolator behind a call counter; `.grid` / `.values` and the attributes the reference sets pass through"""

    def __init__(self, itp):
        self.__dict__["itp"], self.__dict__["n_calls"] = itp, 0

    def __getattr__(self, k):
        return getattr(self.itp, k)

    def __setattr__(self, k, v):
        setattr(self.itp, k, v)

    def __call__(self, x):
        self.__dict__["n_calls"] += 1
        return self.itp(x)


@pytest.fixture(scope="module")
def ref_mods():
    pytest.importorskip("matplotlib")
    _patch_get_cmap()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden as mg
    with contextlib.redirect_stdout(io.StringIO()):
        mods = mg.import_reference()
    return mg, mods


class Recorder:
    """cv2 / imgviz stand-ins that keep what they are handed"""

    def __init__(self):
        self.resized, self.depth2rgb_in, self.lines = [], [], 0
        self.cv2 = types.SimpleNamespace(resize=self.resize, line=self.line)
        self.imgviz = types.SimpleNamespace(depth2rgb=self.depth2rgb)

    def resize(self, img, dsize):
        img = np.asarray(img)
        self.resized.append(img.copy())
        W, H = int(dsize[0]), int(dsize[1])
        return np.stack([ro.cv_resize_linear(img[..., c].astype(np.float32), W, H) for c in range(img.shape[-1])], -1).astype(img.dtype)

    def depth2rgb(self, depth, min_value=None, max_value=None):
        d = np.asarray(depth)
        self.depth2rgb_in.append((d.copy(), min_value, max_value))
        v = np.clip((d.astype(np.float64) - min_value) / (max_value - min_value), 0, 1)
        return np.repeat((v * 255).astype(np.uint8)[..., None], 3, -1)

    def line(self, im, a, b, colour, width):
        self.lines += 1
        return im


def _slice_trainer(mg, mods, g, case, tmp_path):
    from tests.test_graft_reference import _reference_trainer
    from isdf.datasets import sdf_util
    from isdf_amd.hot_path import graft
    tr = sm.set_slice_geometry(_reference_trainer(mg, mods, gu.load("step_small_k3")), case)
    T = np.eye(4)
    T[[0, 1, 2], [0, 1, 2]] = g["vol_spacing"]
    T[:3, 3] = g["vol_origin"]
    tr.gt_sdf_interp = CountingInterp(sdf_util.sdf_interpolator(g["vol"].astype(np.float64), T))
    tr.dataset_format, tr.incremental = "replicaCAD", True
    fr = tr.frames
    fr.T_WC_batch_np, fr.T_WC_gt = fr.T_WC_batch.numpy().copy(), None
    bounds = np.array([[[1.0, 1.9, 1.0], [2.0, 2.9, 2.0]], [[3.6, 2.0, 3.0], [4.8, 2.9, 4.2]]])
    tr.obj_bounds_file = str(tmp_path / "bounds.txt")
    np.savetxt(tr.obj_bounds_file, bounds.reshape(-1, 6))
    with contextlib.redirect_stdout(io.StringIO()):
        graft(tr, rng="torch", engine_factory=SliceFakeEngine)
    return tr


def _both(tr, tmod, name, rec_pair, *a, **k):
    """(bound result, reference result, interpolator calls of the bound one): the bound method, then the reference's own unbound
    method on the same object, each with fresh cv2 / imgviz / draw stand-ins"""
    out = []
    calls = []
    for rec, fn in zip(rec_pair, (getattr(tr, name), types.MethodType(getattr(tmod.Trainer, name), tr))):
        before = tr.gt_sdf_interp.n_calls
        kw = {key: (list(v) if isinstance(v, list) else v) for key, v in k.items()}
        with mock.patch.object(tmod, "cv2", rec.cv2), mock.patch.object(tmod, "imgviz", rec.imgviz), \
                mock.patch.object(tmod, "draw", mock.MagicMock()), contextlib.redirect_stdout(io.StringIO()):
            out.append((fn(*a, **kw), kw))
        calls.append(tr.gt_sdf_interp.n_calls - before)
    assert calls[0] == 0, "the bound %s called the host interpolator" % name
    uses_gt = k.get("include_gt", name == "obj_slices_vis")
    assert (calls[1] > 0) == bool(uses_gt), calls
    return out[0], out[1]


def _same_images(a, b, what):
    assert type(a) is type(b) and len(a) == len(b), what
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype == np.uint8, what
        assert np.array_equal(x, y), what


@needs_ref
@pytest.mark.parametrize("case", ["A", "B"])
def test_bound_compute_slices_equals_the_reference_method(ref_mods, g, case, tmp_path):
    from isdf_amd.hot_path import HotPath
    mg, mods = ref_mods
    tmod = mods[0]
    tr = _slice_trainer(mg, mods, g, case, tmp_path)
    for name in ("compute_slices", "obj_slices_vis", "get_sdf_grid_pc"):
        assert getattr(type(tr), name) is getattr(HotPath, name), name
    assert type(tr).write_slices is tmod.Trainer.write_slices and type(tr).slices_vis is tmod.Trainer.slices_vis
    n_pts = 3 * sm.GRID_DIM ** 2
    assert tr.chunk_size >= n_pts
    recs = Recorder(), Recorder()
    tr.engine.calls.clear()
    (hip, kw_h), (ref, kw_r) = _both(tr, tmod, "compute_slices", recs, n_slices=3, include_gt=True, include_diff=True,
                                     include_chomp=True, sdf_range=[-2, 2])
    # ONE forward over all slices and one kernel pass for the bound call; the reference's forward is the identical call
    assert tr.engine.calls == [("sdf_eval", n_pts), "slice_images", ("sdf_eval", n_pts)]
    assert kw_h["sdf_range"] == kw_r["sdf_range"] == [-2.0, 2.0] and [type(v) for v in kw_h["sdf_range"]] == [float, float]
    assert sorted(hip) == sorted(ref) == ["diff", "gt_cost", "gt_sdf", "pred_cost", "pred_sdf"]
    _same_images(hip["pred_sdf"], ref["pred_sdf"], "pred_sdf")
    _same_images(hip["gt_sdf"], ref["gt_sdf"], "gt_sdf")
    _same_images(hip["diff"], ref["diff"], "diff")
    assert len(hip["pred_sdf"]) == 3 and all((d == 255).all() for d in hip["diff"])
    assert hip["pred_sdf"][0].shape == tuple(g[case + "/im_size"]) + (3,)
    # what cv2.resize was handed: the same slabs in the same order (pred, pred cost, gt, gt cost, diff)
    assert len(recs[0].resized) == len(recs[1].resized) == 15
    for k, (a, b) in enumerate(zip(recs[0].resized, recs[1].resized)):
        assert a.shape == b.shape == (sm.GRID_DIM, sm.GRID_DIM, 3) and a.dtype == b.dtype == np.uint8
        if not 3 <= k < 6 and not 9 <= k < 12:                 # (the cost images go through the imgviz stand-in: compared below)
            assert np.array_equal(a, b), k
    # the cost fields handed to imgviz.depth2rgb: the predicted one is the same float32 arithmetic; the ground truth's is the
    # float32 evaluation of a float32-rounded value where the reference has float64: the cost is 1-Lipschitz in the distance
    # (slopes -1, (s - e) / e in [-1, 0], 0), so the input's rounding (eps32 / 2 relative) moves it by no more than itself, and its
    # own three float32 operations add eps32 / 2 relative each: 2 * eps32 * (max |gt| + epsilon) in all
    (pc_h, lo_h, hi_h), (gc_h, _, _) = recs[0].depth2rgb_in
    (pc_r, lo_r, hi_r), (gc_r, _, _) = recs[1].depth2rgb_in[:2]       # (the reference also colours the difference it discards)
    assert len(recs[1].depth2rgb_in) == 3
    assert (lo_h, hi_h) == (lo_r, hi_r) == (0., 1.5)
    assert pc_h.shape == pc_r.shape == gc_h.shape == gc_r.shape == (sm.GRID_DIM, n_pts // sm.GRID_DIM)
    assert pc_h.dtype == pc_r.dtype == np.float32 and np.array_equal(pc_h, pc_r)
    assert gc_h.dtype == gc_r.dtype == np.float64
    bound = 2 * EPS32 * (np.abs(g[case + "/gt"]).max() + 2.0)
    err = np.abs(gc_h - gc_r).max()
    print("gt cost field: max error %.3e (bound %.3e)" % (err, bound))
    assert err <= bound
    # the fixture's record of the reference's run on the real network agrees on the ground truth (the same volume and points)
    assert np.array_equal(np.stack(recs[1].resized[6:9]), g[case + "/gt_slabs"])


@needs_ref
def test_compute_slices_options_range_list_and_markers(ref_mods, g, tmp_path):
    mg, mods = ref_mods
    tmod = mods[0]
    tr = _slice_trainer(mg, mods, g, "A", tmp_path)
    # defaults: pred_sdf only, default z_ixs
    (hip, _), (ref, _) = _both(tr, tmod, "compute_slices", (Recorder(), Recorder()), n_slices=2)
    assert sorted(hip) == sorted(ref) == ["pred_sdf"]
    _same_images(hip["pred_sdf"], ref["pred_sdf"], "pred_sdf")
    # explicit z_ixs, a range the reference rounds outwards in place, markers drawn through the reference's own calls
    recs = Recorder(), Recorder()
    z = torch.tensor([5, 40, 17, 23])
    (hip, kw_h), (ref, kw_r) = _both(tr, tmod, "compute_slices", recs, z_ixs=z, include_gt=True, draw_cams=True,
                                     sdf_range=[-0.745, 0.245])
    assert kw_h["sdf_range"] == kw_r["sdf_range"] and kw_h["sdf_range"] != [-0.745, 0.245]
    assert sorted(hip) == sorted(ref) == ["gt_sdf", "pred_sdf"] and len(hip["pred_sdf"]) == 4
    _same_images(hip["pred_sdf"], ref["pred_sdf"], "pred_sdf")
    _same_images(hip["gt_sdf"], ref["gt_sdf"], "gt_sdf")
    assert recs[0].lines == recs[1].lines > 0
    # include_diff without include_gt raises in the reference (its gt_sdf is never assigned); so does the bound method
    for fn in (tr.compute_slices, types.MethodType(tmod.Trainer.compute_slices, tr)):
        r = Recorder()
        with mock.patch.object(tmod, "cv2", r.cv2), mock.patch.object(tmod, "imgviz", r.imgviz), pytest.raises(UnboundLocalError):
            fn(n_slices=2, include_diff=True)
    # slices_vis (the reference's own method) runs through the bound compute_slices
    r = Recorder()
    with mock.patch.object(tmod, "cv2", r.cv2), mock.patch.object(tmod, "imgviz", r.imgviz), mock.patch.object(tmod, "draw", mock.MagicMock()):
        tr.engine.calls.clear()
        viz = tr.slices_vis(n_slices=2)
    assert tr.engine.calls == [("sdf_eval", 2 * sm.GRID_DIM ** 2), "slice_images"]
    h, w = g["A/im_size"]
    assert viz.shape == (3 * h, 2 * w, 3) and viz.dtype == np.uint8 and (viz[2 * h:] == 255).all()
    assert len(tr._hip.slice_cmaps) == 2                       # one map per distinct table ([-2, 2] and the rounded range)


@needs_ref
def test_bound_obj_slices_vis_equals_the_reference_method(ref_mods, g, tmp_path):
    mg, mods = ref_mods
    tmod = mods[0]
    tr = _slice_trainer(mg, mods, g, "A", tmp_path)
    tr.engine.calls.clear()
    (hip, _), (ref, _) = _both(tr, tmod, "obj_slices_vis", (Recorder(), Recorder()), n_slices=2)
    n = 256 * 2 * 256
    assert tr.engine.calls == [("sdf_eval", n), "slice_images"] * 2 + [("sdf_eval", n)] * 2     # per object one forward, one pass
    assert hip.shape == ref.shape == (2 * 2 * 256, 2 * 256, 3) and hip.dtype == ref.dtype == np.uint8
    assert np.array_equal(hip, ref)
    assert len(np.unique(hip.reshape(-1, 3), axis=0)) > 20
    tr.obj_bounds_file = None
    assert tr.obj_slices_vis() is None and types.MethodType(tmod.Trainer.obj_slices_vis, tr)() is None


@needs_ref
def test_bound_get_sdf_grid_pc_equals_the_reference_method(ref_mods, g, tmp_path):
    mg, mods = ref_mods
    tmod = mods[0]
    tr = _slice_trainer(mg, mods, g, "A", tmp_path)
    d = tr.grid_dim = 20
    tr.grid_pc = sm.grid_pc(d)
    rng = np.random.RandomState(4)
    pc = (np.array([3.0, 1.5, 2.5]) + rng.uniform(-1, 1, (4000, 3)) * np.array([2.5, 1.2, 2.0]))
    tr.update_vis_vars = lambda: None
    tr.gt_depth_vis = tr.fx_vis = tr.fy_vis = tr.cx_vis = tr.cy_vis = None
    with mock.patch.object(tmod.geometry.transform, "backproject_pointclouds", lambda *a: None), \
            mock.patch.object(tmod.draw3D, "draw_pc", lambda n, pcs, T: (pc, None)):
        (hip, _), (ref, _) = _both(tr, tmod, "get_sdf_grid_pc", (Recorder(), Recorder()), include_gt=True, mask_near_pc=True)
        plain_h, plain_r = tr.get_sdf_grid_pc(), types.MethodType(tmod.Trainer.get_sdf_grid_pc, tr)()
    (grid_h, mask_h), (grid_r, mask_r) = hip, ref
    assert grid_h.shape == grid_r.shape == (d, d, d, 5) and grid_h.dtype == grid_r.dtype == np.float64
    assert np.array_equal(grid_h[..., :4], grid_r[..., :4])
    err = np.abs(grid_h[..., 4] - grid_r[..., 4]).max()
    assert err <= EPS32 / 2 * np.abs(grid_r[..., 4]).max() + 1e-12 and (grid_r[..., 4] == 0).any()       # float32 rounding of the float64 value
    assert mask_h.shape == mask_r.shape == (20, 20, 20) and mask_h.dtype == mask_r.dtype == bool
    assert np.array_equal(mask_h, mask_r) and 0 < mask_r.mean() < 1
    assert tr.gt_sdf_interp.bounds_error is True and tr.gt_sdf_interp.fill_value == 0.0
    assert plain_h[1] is None and plain_r[1] is None
    assert plain_h[0].shape == plain_r[0].shape == (d, d, d, 4) and plain_h[0].dtype == plain_r[0].dtype == np.float32
    assert np.array_equal(plain_h[0], plain_r[0])


@needs_ref
def test_slices_module_runs_one_forward_for_all_points(ref_mods, g, tmp_path):
    from isdf_amd import slices
    from isdf_amd.metrics import GtVolume
    mg, mods = ref_mods
    tr = _slice_trainer(mg, mods, g, "A", tmp_path)
    eng = tr.engine
    rgb = g["t05/rgb"]
    cmap = slices.Colormap(rgb[:-3], rgb[-3], rgb[-2], rgb[-1], *g["t05/lim"])
    vol = GtVolume(g["vol"], g["vol_spacing"], g["vol_origin"], "cpu")
    pts = torch.from_numpy(g["A/pts"])
    eng.calls.clear()
    res = slices.slice_images(eng, pts, cmap, gt_volume=vol, chomp_eps=2.0)
    assert eng.calls == [("sdf_eval", pts.shape[0] * pts.shape[1] * pts.shape[2]), "slice_images"]
    lead = tuple(pts.shape[:-1])
    assert res.sdf.shape == res.gt.shape == res.pred_cost.shape == res.gt_cost.shape == lead
    assert res.pred_rgb.shape == res.gt_rgb.shape == lead + (3,) and res.pred_rgb.dtype == torch.uint8
    plain = slices.slice_images(eng, pts[:2], cmap)
    assert plain.gt is None and plain.gt_rgb is None and plain.pred_cost is None and plain.gt_cost is None
    eng.calls.clear()
    pl = slices.plane(eng, [0.5, 1.0, 0.5], [0.1, 0, 0], [0, 0, 0.1], 7, 9, cmap, gt_volume=vol)
    assert eng.calls == ["plane_points", ("sdf_eval", 63), "slice_images"]
    assert pl.pts.shape == (7, 9, 3) and pl.pred_rgb.shape == (7, 9, 3) and pl.gt.shape == (7, 9)
