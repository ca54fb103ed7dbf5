"""isdf_region_metrics and the bound Trainer.eval_fixed on the device.  References: what the reference's eval_pts.fixed_pts_eval
recorded (fixture eval_fixed_small, made by tests/golden/make_eval_fixed_golden.py; this file does not read the reference) and
the float64 numpy model of tests/eval_fixed_model.py.

Bounds.  The kernel works in double on the same float32 inputs as the reference, so a mean is a double sum of <= 2e5 terms that
agree to a few ulps: 1e-9 relative.  The reference forms the predicted CHOMP cost in float32: 4 * eps32.  The object legs take
their points rounded to float32 where the reference looks them up in float64: each coordinate rounds once (2^-24 relative) and the
trilinear blend of a 1-Lipschitz field moves by no more than the sum of the three coordinate moves, 3 * 2^-24 * max|p|.
av_cossim is held to 1e-9 ABSOLUTE against the recorded figure (a cosine distance lies in [0, 2]): the reference normalises the
float32 predicted gradient in float32 (tests/test_eval_fixed_cpu.py, first test), the kernel widens it first as its
specification says, and on this fixture the two differ by 1.5e-10 (vis) and 2.2e-10 (vox), 1.9e-8 and 1.7e-8 relative; against the
model, which uses the kernel's formula, av_cossim is held to 1e-9 relative like every other mean."""
import json
import warnings

import numpy as np
import pytest
import torch

from tests import eval_fixed_model as fm
from tests import eval_model as em
from tests import reduce_model as rm

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def g():
    return fm.load_golden()


@pytest.fixture(scope="module")
def eng():
    from isdf_amd.engine import Engine, NetConfig
    return Engine(NetConfig(hidden=64, blocks=1), "cuda")


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _volume(g):
    from isdf_amd.metrics import GtVolume
    return GtVolume(g["volume"], g["spacing"], g["origin"], "cuda")


def _run(eng, g, pts, sdf, **kw):
    """(device records [2, 27] as numpy, model records) for one leg; ground truth from the fixture's volume unless gt= is given"""
    dev = {k: _cuda(v) for k, v in kw.items() if k in ("sdf_grad", "flags", "gt")}
    if "gt" not in kw:
        dev["volume"] = _volume(g)
    rec = eng.region_metrics(_cuda(np.asarray(pts, np.float32)), _cuda(sdf), delta=0.01, **dev).cpu().numpy()
    mk = dict(kw) if "gt" in kw else dict(kw, values=g["volume"], spacing=g["spacing"], origin=g["origin"])
    return rec, fm.region_records(np.asarray(pts, np.float32), sdf, delta=0.01, **mk)


def _counts_equal(rec, model):
    for k in range(2):
        assert np.array_equal(rec[k, [0, 1, 24, 26]], model[k, [0, 1, 24, 26]]), (k, rec[k, [0, 1, 24, 26]], model[k, [0, 1, 24, 26]])
        assert np.array_equal(rec[k, 9:15], model[k, 9:15]), (k, rec[k, 9:15], model[k, 9:15])


def _sums_close(rec, model, rtol=1e-9):
    _counts_equal(rec, model)
    scale = np.maximum(np.abs(model), 1e-3)            # a sum of a handful of terms near zero: absolute against a millimetre
    err = np.abs(rec - model) / scale
    assert np.array_equal(np.isnan(rec), np.isnan(model)) and np.nanmax(err) <= rtol, (np.nanmax(err), np.nanargmax(err))
    return float(np.nanmax(err))


def _against_recorded(got, g, prefix, tol_l1=None):
    """one set's dict against the fixture's res/<prefix>.*: means to 1e-9 relative (or tol_l1 absolute: the object legs), CHOMP to
    4 * eps32, av_cossim to 1e-9 absolute"""
    for key, v in fm.flatten(got).items():
        want, v = g["res/%s.%s" % (prefix, key)], np.asarray(v)
        err = np.abs(v - want).max()
        print("  %s.%s: %s (recorded %s), error %.3e" % (prefix, key, v, want, err))
        assert np.array_equal(np.isnan(v), np.isnan(want))
        if "chomp" in key:
            assert err <= 4 * EPS32
        elif "cossim" in key:
            assert err <= 1e-9
        elif tol_l1 is not None:
            assert err <= tol_l1
        else:
            assert (np.abs(v - want) <= 1e-9 * np.abs(want)).all()


# ------------------------------------------------------------------ the fixture's legs
def test_visible_region_leg_equals_the_reference_record(eng, g):
    from isdf_amd.metrics import RegionMetrics
    rec, model = _run(eng, g, g["vis_pts"], g["vis_sdf"], sdf_grad=g["vis_grad"], flags=g["vis_flags"])
    print("visible region: worst relative error against the model %.3e" % _sums_close(rec, model))
    A, B, G = g["vis_valid_gt_sdf"], g["vis_valid_vox_sdf"], g["vis_valid_gt_grad"]
    assert rec[0, 0] == A.sum() and rec[1, 0] == B.sum() and rec[0, 24] == G.sum() and rec[0, 26] == 0 and rec[1, 26] == 0
    assert rec[1, 24] == (g["vis_flags"] & 8).astype(bool).sum() > 0
    assert rec[0, 9] > 0 and rec[0, 9:15].sum() < rec[0, 0]                 # the first bin is populated; zero-valued ground truth is kept
    for k, name in enumerate(("vis", "vox")):
        _against_recorded(RegionMetrics(rec[k]).as_dict(cossim=True), g, "rays." + name)


def test_surface_leg_equals_the_reference_record(eng, g):
    from isdf_amd.metrics import RegionMetrics
    rec, model = _run(eng, g, g["surf_pts"], g["surf_sdf"], flags=g["surf_flags"])
    _sums_close(rec, model)
    assert rec[0, 0] == g["surf_valid_gt_sdf"].sum() and rec[1, 0] == g["surf_valid_vox_sdf"].sum() and rec[:, 24:].max() == 0
    for k, name in enumerate(("vis", "vox")):
        _against_recorded(RegionMetrics(rec[k]).as_dict(), g, "visible_surf." + name)


def test_object_legs_equal_the_reference_record(eng, g):
    from isdf_amd.metrics import RegionMetrics
    for leg in range(len(g["obj_ids"])):
        p64 = g["obj_leg%d_pts" % leg]
        rec, model = _run(eng, g, p64.astype(np.float32), g["obj_leg%d_sdf" % leg], flags=g["obj_leg%d_flags" % leg])
        _sums_close(rec, model)
        assert rec[0, 0] == len(p64) and rec[1, 0] == (g["obj_leg%d_flags" % leg] & 2).astype(bool).sum()
        tol = 3 * 2.0 ** -24 * float(np.abs(p64).max())
        for k, name in enumerate(("vis", "vox")):
            _against_recorded({"av_l1": RegionMetrics(rec[k]).sdf.av_l1}, g, "objects.%d.%s" % (leg, name), tol_l1=tol)


def test_given_ground_truth_path_equals_the_volume_leg(eng, g):
    from isdf_amd.metrics import RegionMetrics
    rec, model = _run(eng, g, g["vol_pts"], g["vol_sdf"], gt=g["vol_gt"])
    _sums_close(rec, model)
    assert rec[0, 0] == rec[0, 1] == len(g["vol_pts"])                       # every point counts as in bounds
    assert np.array_equal(rec[0], rec[1])                                    # no flags: both sets hold every point
    _against_recorded(RegionMetrics(rec[0]).as_dict(), g, "vol")
    far = g["vol_pts"] + np.float32(1000.0)                                  # no lookup is done: the points do not matter
    again = eng.region_metrics(_cuda(far), _cuda(g["vol_sdf"]), gt=_cuda(g["vol_gt"])).cpu().numpy()
    assert np.array_equal(again, rec)


# ------------------------------------------------------------------ edge cases
@pytest.mark.parametrize("n", [0, 1, 255, 257, 4099])
def test_sizes_around_the_block_and_grid_limits(eng, g, n):
    rng = np.random.RandomState(n + 1)
    lo = g["origin"]
    hi = lo + (np.array(g["volume"].shape) - 1) * g["spacing"]
    pts = (lo - 0.2 + rng.uniform(size=(n, 3)) * (hi - lo + 0.4)).astype(np.float32)       # some outside
    sdf, grad = fm.pred_sdf(pts) if n else np.zeros(0, np.float32), rng.standard_normal((n, 3)).astype(np.float32)
    flags = rng.randint(0, 16, n).astype(np.uint8)
    rec, model = _run(eng, g, pts, sdf, sdf_grad=grad, flags=flags)
    if n == 0:
        assert not rec.any()
        return
    _sums_close(rec, model)
    again, _ = _run(eng, g, pts, sdf, sdf_grad=grad, flags=flags)
    assert np.array_equal(rec.view(np.int64), again.view(np.int64))          # bit-identical over two runs
    none, model = _run(eng, g, pts, sdf)                                     # no flags: both sdf sets, no gradient set
    _sums_close(none, model)
    assert np.array_equal(none[0], none[1]) and none[0, 24:].max() == 0 and none[0, 0] == model[0, 0] <= n
    nograd, model = _run(eng, g, pts, sdf, flags=flags)                      # gradient bits without sdf_grad are not honoured
    _sums_close(nograd, model)
    assert nograd[:, 24:].max() == 0


def _region_terms(sdf, gt, flags):
    """[n, 2, 15] float64: what every point adds to entries 0..14 of the two sets on the given-ground-truth leg"""
    s, g = sdf.astype(np.float64), np.asarray(gt, np.float64)
    d = np.abs(s - g)
    c = np.zeros((len(s), 15))
    c[:, 0], c[:, 1], c[:, 2] = 1.0, 1.0, d
    for b in range(6):
        m = (g > em.BIN_LIMITS[b]) & (g < em.BIN_LIMITS[b + 1])
        c[:, 3 + b], c[:, 9 + b] = np.where(m, d, 0.0), m
    return np.stack([np.where((flags >> k & 1).astype(bool)[:, None], c, 0.0) for k in range(2)], 1)


@pytest.mark.parametrize("n", [257, 4099])
def test_region_records_equal_the_ordered_sums_bit_for_bit(eng, n):
    """entries 0..14 of both sets against tests/reduce_model.py on the float64 ground-truth leg; points in one set, in both and
    in neither; magnitudes from 2^-20 to 2^20, so another order gives other bytes (asserted against np.sum)"""
    from isdf_amd import _ffi
    rng = np.random.RandomState(n)
    sdf = rm.wide(rng, n)
    gt = rm.wide(rng, n).astype(np.float64) * (1.0 + rng.uniform(0, 2.0 ** -30, n))      # doubles no float32 holds
    flags = rng.randint(0, 4, n).astype(np.uint8)
    assert all((flags == f).sum() > n // 8 for f in range(4))
    pts = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    rec = eng.region_metrics(_cuda(pts), _cuda(sdf), gt=_cuda(gt), flags=_cuda(flags)).cpu().numpy()
    terms = _region_terms(sdf, gt, flags)
    assert _ffi.REGION_METRICS_WS_BYTES == 1024 * 2 * _ffi.REGION_RECORD * 8            # ISDF_METRICS_MAX_BLOCKS partial records
    model = rm.close_strided(rm.grid_stride_record(terms.reshape(n, 30), 1024)).reshape(2, 15)
    plain = terms.sum(0)
    print("n = %d: entries where the ordered sum is not np.sum: %d of 30" % (n, (model != plain).sum()))
    assert (model != plain).any(1).all()
    assert rec[:, :15].tobytes() == model.tobytes(), np.argwhere(rec[:, :15] != model)


def test_all_outside_points(eng, g):
    n = 1000
    rng = np.random.RandomState(3)
    pts = (g["origin"] - 5.0 - rng.uniform(size=(n, 3))).astype(np.float32)
    flags = np.full(n, 15, np.uint8)
    rec, model = _run(eng, g, pts, np.zeros(n, np.float32), sdf_grad=np.ones((n, 3), np.float32), flags=flags)
    _counts_equal(rec, model)
    assert not rec[:, :24].any()                                             # nothing is in bounds: no figure, means are 0 / 0
    assert np.array_equal(rec[:, 24:], [[n, 0, n]] * 2)                      # every ground-truth gradient is non-finite
    from isdf_amd.metrics import RegionMetrics
    m = RegionMetrics(rec[0])
    assert np.isnan(m.sdf.av_l1) and np.isnan(m.av_cossim) and all(np.isnan(m.sdf.binned_l1))


def test_a_non_finite_ground_truth_gradient_in_a_gradient_set(eng, g):
    """points whose recorded gt_grad_all is NaN (a lookup at p +- delta out of bounds or == 0), put into the gradient sets"""
    from isdf_amd.metrics import region_metrics
    bad = np.isnan(g["gt_grad_all"]).any(axis=1)
    assert bad.sum() > 100 and g["vis_valid_gt_grad"].sum() > 100
    flags = g["vis_flags"].copy()
    pick = np.nonzero(bad)[0][:7]
    flags[pick] |= 4
    flags[pick[:3]] |= 8
    rec, model = _run(eng, g, g["vis_pts"], g["vis_sdf"], sdf_grad=g["vis_grad"], flags=flags)
    _sums_close(rec, model)
    assert rec[0, 26] == 7 and rec[1, 26] == 3 and rec[0, 24] == g["vis_valid_gt_grad"].sum() + 7
    clean, _ = _run(eng, g, g["vis_pts"], g["vis_sdf"], sdf_grad=g["vis_grad"], flags=g["vis_flags"])
    assert np.array_equal(rec[:, 25], clean[:, 25])                          # they add nothing to the sum ...
    vis, vox = region_metrics(eng, _cuda(g["vis_pts"]), _cuda(g["vis_sdf"]), volume=_volume(g), sdf_grad=_cuda(g["vis_grad"]),
                              flags=_cuda(flags))
    assert np.isnan(vis.av_cossim) and np.isnan(vox.av_cossim)               # ... and the mean is NaN, as the reference's is
    assert vis.n_grad_nonfinite == 7 and vox.n_grad_nonfinite == 3 and np.isfinite(vis.sdf.av_l1)
    # the device gradient agrees with the recorded one wherever that is finite: cosine of a gradient with itself is 1
    G = g["vis_valid_gt_grad"]
    self_rec = eng.region_metrics(_cuda(g["vis_pts"]), _cuda(g["vis_sdf"]), volume=_volume(g),
                                  sdf_grad=_cuda(g["gt_grad_all"].astype(np.float32)), flags=_cuda(g["vis_flags"])).cpu().numpy()
    assert self_rec[0, 24] == G.sum() and abs(self_rec[0, 25] / G.sum()) <= 4 * EPS32


# ------------------------------------------------------------------ end to end
class _Grid:
    """what graft() reads of trainer.gt_sdf_interp: `.grid` and `.values`; calling it is an error"""

    def __init__(self, grid, values):
        self.grid, self.values = grid, values

    def __call__(self, *a, **k):
        raise AssertionError("the bound evaluation must not call the host interpolator")


def _n_drawn(t, depth):
    """the number of points eval_pts.sample_rays draws at timestamp t on these frames (the torch CPU generator, eval_pts.py:354-379)"""
    state = torch.get_rng_state()
    torch.manual_seed(float(f"{t:.3f}") * 1e3)
    F, H, W = depth.shape
    rpf = 200000 // F
    ih, iw = torch.randint(0, H, (rpf * F,)).numpy(), torch.randint(0, W, (rpf * F,)).numpy()
    torch.set_rng_state(state)
    return int((depth[np.repeat(np.arange(F), rpf), ih, iw] != 0).sum())


def test_grafted_eval_fixed_on_the_standin_trainer(tmp_path):
    from bench_support.standin_trainer import HipTrainer
    from isdf_amd import synthetic
    from isdf_amd.hot_path import HotPath
    from tests.accuracy_experiment import config
    cam = dict(H=96, W=128, fx=100.0, fy=100.0, cx=63.5, cy=47.5)
    tr = HipTrainer("cuda", config(cam), inv_bounds_transform=synthetic.bounds_transform(), rng="philox", seed=5)
    assert type(tr).eval_fixed is HotPath.eval_fixed
    seq_len, every = 90, 5
    keep = np.arange(0, seq_len, every)
    T = synthetic.trajectory(seq_len)[keep]
    depth = np.stack([synthetic.render_depth(T[i], cam, np.random.RandomState(i)) for i in range(len(T))]).astype(np.float32)
    ds = fm.KeepIxsDataset(depth, T, keep)
    spacing, origin = np.array([0.1, 0.125, 0.1]), np.array([-0.5, -0.25, -0.5])
    dims = (71, 29, 61)
    ax = tuple(np.arange(n) * h + o for n, h, o in zip(dims, spacing, origin))
    values = synthetic.gt_sdf(np.stack(np.meshgrid(*ax, indexing="ij"), -1)).astype(np.float32)
    rng = np.random.RandomState(17)
    times = [1.0, 2.0]                                                        # frames below 30 (6 held), then below 60 (12 held)
    obj_raw = np.array([[[1.0, 0.5, 1.0], [1.5, 1.0, 1.5]], [[9.0, 9.0, 9.0], [9.5, 9.5, 9.5]], [[3.0, 1.0, 3.0], [3.4, 1.4, 3.4]]])
    hi = origin + (np.array(dims) - 1) * spacing
    vol_pts = origin + rng.uniform(size=(2000, 3)) * (hi - origin)
    vol_gt = synthetic.gt_sdf(vol_pts) + 0.01 * rng.standard_normal(2000)
    for t in times:
        n = _n_drawn(t, depth[:int(np.searchsorted(keep, int(t * 30)))])
        masks = {}
        for name, m in (("vis", n), ("surf", n), ("obj0", 10000), ("obj2", 10000)):
            A = rng.uniform(size=m) > 0.2
            masks[name + "_valid_gt_sdf"], masks[name + "_valid_vox_sdf"] = A, rng.uniform(size=A.sum()) > 0.5
        G = rng.uniform(size=n) > 0.3
        masks["vis_valid_gt_grad"], masks["vis_valid_vox_grad"] = G, rng.uniform(size=G.sum()) > 0.5
        dirs = fm.write_tree(tmp_path, f"{t:.3f}", masks, obj_raw, vol_pts, vol_gt)
    tr.eval_pts_dir, tr.seq_dir, tr.eval_pts_root = dirs
    tr.eval_times, tr.scene_dataset, tr.dataset_format = list(times), range(seq_len), "replicaCAD"
    tr.gt_sdf_interp, tr.cached_dataset, tr.tot_step_time = _Grid(ax, values), ds, 3.0
    e = tr.engine
    before = [t.clone() for t in (e.params, e.exp_avg, e.exp_avg_sq)]
    draws = tr._hip.draw_count
    calls = []
    inner = e.region_metrics

    def spy(pts, sdf, volume=None, gt=None, sdf_grad=None, flags=None, delta=0.01, out=None):
        calls.append(dict(pts=pts.detach().cpu().numpy().copy(), sdf=sdf.detach().cpu().numpy().copy(), delta=delta,
                          gt=None if gt is None else gt.cpu().numpy().copy(),
                          sdf_grad=None if sdf_grad is None else sdf_grad.detach().cpu().numpy().copy(),
                          flags=None if flags is None else flags.cpu().numpy().copy()))
        return inner(pts, sdf, volume=volume, gt=gt, sdf_grad=sdf_grad, flags=flags, delta=delta, out=out)
    e.region_metrics = spy

    for step, t in enumerate(times):
        calls.clear()
        torch.manual_seed(7); np.random.seed(7)
        with warnings.catch_warnings(record=True) as caught:               # random masks select points outside the grid
            warnings.simplefilter("always")
            res = tr.eval_fixed()
        assert len([w for w in caught if "outside the ground-truth grid" in str(w.message)]) <= 1
        assert list(res) == ["time", "rays", "visible_surf", "objects", "vol"] and res["time"] == t
        json.dumps(res)
        assert len(calls) == 5 and len(res["objects"]) == 2 and tr.eval_times == times[step + 1:]
        # the float64 model on exactly what the method handed to the kernel
        recs = []
        for c in calls:
            kw = dict(gt=c["gt"]) if c["gt"] is not None else dict(values=values, spacing=spacing, origin=origin)
            recs.append(fm.region_records(c["pts"], c["sdf"], sdf_grad=c["sdf_grad"], flags=c["flags"], delta=c["delta"], **kw))
        want = {"time": t,
                "rays": {"vis": fm.set_dict(recs[0][0], cossim=True), "vox": fm.set_dict(recs[0][1], cossim=True)},
                "visible_surf": {"vis": fm.set_dict(recs[1][0]), "vox": fm.set_dict(recs[1][1])},
                "objects": [{"vis": fm.set_dict(r[0], only_l1=True), "vox": fm.set_dict(r[1], only_l1=True)} for r in recs[2:4]],
                "vol": fm.set_dict(recs[4][0])}
        pmax = max(float(np.abs(c["pts"]).max()) for c in calls[:4])
        bound = 16 * EPS32 * (pmax + float(np.abs(values).max()))             # test_grafted_evaluation_on_the_standin_trainer's
        fw, fr = fm.flatten(want), fm.flatten(res)
        assert list(fw) == list(fr)
        worst = 0.0
        for k in fw:
            assert np.array_equal(np.isnan(fw[k]), np.isnan(fr[k])), (k, fw[k], fr[k])
            ok = ~np.isnan(fw[k])
            worst = max(worst, np.abs(fw[k][ok] - fr[k][ok]).max(initial=0.0))
        print("eval_fixed t=%.1f: %d points, worst error against the model %.3e (bound %.3e), av_l1 %.6f, av_cossim %.6f"
              % (t, len(calls[0]["pts"]), worst, bound, res["rays"]["vis"]["av_l1"], res["rays"]["vis"]["av_cossim"][0]))
        assert worst <= bound
        n = len(calls[0]["pts"])
        assert n == _n_drawn(t, depth[:6 * (step + 1)]) and calls[0]["sdf_grad"].shape == (n, 3) and calls[1]["pts"].shape == (n, 3)
        assert np.isfinite(res["rays"]["vis"]["av_l1"]) and np.isfinite(res["vol"]["av_l1"])
        # the draws were the torch CPU generator's: afterwards it stands where seed + two randint leave it
        state = torch.get_rng_state()
        torch.manual_seed(float(f"{t:.3f}") * 1e3)
        F = 6 * (step + 1)
        torch.randint(0, 96, (200000 // F * F,)); torch.randint(0, 128, (200000 // F * F,))
        assert torch.equal(state, torch.get_rng_state())
        # frames: each uploaded once
        assert ds.reads == [6] * (step + 1) and tr._hip.eval_cache.uploaded_frames == 6 * (step + 1)
    assert tr._hip.draw_count == draws                                          # the Philox counter did not advance
    for a, b in zip(before, (e.params, e.exp_avg, e.exp_avg_sq)):              # evaluation trains nothing
        assert torch.equal(a, b)
    tr.eval_sdf_visible(600)                                                    # the clock (3.0 s) wants all 18: 6 more
    assert ds.reads == [6, 6, 6] and tr._hip.eval_cache.uploaded_frames == 18
    depth_d, _ = tr._eval_frames(30)
    assert depth_d.shape[0] == 6 and ds.reads == [6, 6, 6] and np.array_equal(depth_d.cpu().numpy(), depth[:6])
