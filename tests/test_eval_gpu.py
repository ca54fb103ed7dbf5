"""Evaluation against ground truth on the device: isdf_sdf_metrics and isdf_nn_distance through Engine / isdf_amd.metrics and
through graft().  References: the reference's own recorded results (fixture eval_metrics_small, made by
tests/golden/make_eval_golden.py from the reference's interpolator, bins, CHOMP cost, accuracy and completion) and the float64 /
float32 numpy models of tests/eval_model.py.

The bound on anything derived from the interpolated ground truth is 16 * eps32 * (max|p| + max|gt|): a point's coordinate, its
division by the spacing and seven interpolation steps each cost a few float32 roundings, and an SDF is 1-Lipschitz, so a
coordinate error moves the value by no more than itself; av_l1, the bins and the CHOMP figures are means of 1-Lipschitz functions
of the ground truth and inherit it.  7.2e-6 m for the fixture's extent."""
import numpy as np
import pytest
import torch

from tests import eval_model as em
from tests import reduce_model as rm

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def g():
    return em.load_golden()


@pytest.fixture(scope="module")
def eng():
    from isdf_amd.engine import Engine, NetConfig
    return Engine(NetConfig(hidden=64, blocks=1), "cuda")


def _bound(pts, gt):
    return 16 * EPS32 * (float(np.abs(pts).max()) + float(np.abs(gt).max()))


def _volume(g, name):
    from isdf_amd.metrics import GtVolume
    return GtVolume(g[name], g["spacing"], g["origin"], "cuda")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", ["signed", "zeroed"])
@pytest.mark.parametrize("exclude", [True, False])
def test_per_point_ground_truth_masks_and_record(eng, g, name, exclude):
    from isdf_amd.metrics import SdfMetrics
    vol = _volume(g, name)
    rec, gt, valid = eng.sdf_metrics(vol, _cuda(g["pts"]), _cuda(g["sdf"]), exclude_zero_gt=exclude, per_point=True, oob_fill=-7.0)
    rec, gt, valid = rec.cpu().numpy(), gt.cpu().numpy(), valid.cpu().numpy().astype(bool)
    inb, ref_gt = g[name + "/in_bounds"], g[name + "/gt"]
    bound = _bound(g["pts"], ref_gt[inb])
    err = np.abs(gt[inb].astype(np.float64) - ref_gt[inb]).max()
    print("%s exclude=%s: per-point gt error %.3e (bound %.3e)" % (name, exclude, err, bound))
    assert err <= bound
    assert np.all(gt[~inb] == np.float32(-7.0))
    assert np.array_equal(valid, g[name + "/valid"] if exclude else inb)
    m = SdfMetrics(rec)
    assert m.n_in_bounds == inb.sum() and m.n_valid == (g[name + "/valid"].sum() if exclude else inb.sum())
    model, _, _ = em.sdf_metrics(g[name], g["spacing"], g["origin"], g["pts"], g["sdf"], exclude_zero_gt=exclude)
    assert np.array_equal(m.bin_counts, model[9:15].astype(np.int64))
    want = em.result_dict(model)
    if exclude:          # the reference's own figures
        assert np.array_equal(m.bin_counts, g[name + "/bin_counts"])
        want = {"av_l1": g[name + "/av_l1"][0], "binned_l1": g[name + "/binned_l1_np"], "l1_chomp_costs": g[name + "/chomp_diff_means"]}
        assert np.abs(np.array(m.pred_chomp_sums) / m.n_valid - g[name + "/pred_chomp_sums"] / m.n_valid).max() <= bound
        assert np.abs(np.array(m.gt_chomp_sums) / m.n_valid - g[name + "/gt_chomp_sums"] / m.n_valid).max() <= bound
    else:                # eval_object_sdf's mean keeps the zeros
        assert abs(m.av_l1 - g[name + "/l1_keep_zero"][0]) <= bound
    got = m.as_dict()
    print("  av_l1 error %.3e" % abs(got["av_l1"] - want["av_l1"]))
    assert abs(got["av_l1"] - want["av_l1"]) <= bound
    empty = np.isnan(np.asarray(want["binned_l1"], np.float64))
    assert np.array_equal(np.isnan(got["binned_l1"]), empty) and np.array_equal(empty, m.bin_counts == 0)
    assert np.abs(np.asarray(got["binned_l1"])[~empty] - np.asarray(want["binned_l1"])[~empty]).max() <= bound
    assert np.abs(np.asarray(got["l1_chomp_costs"]) - np.asarray(want["l1_chomp_costs"])).max() <= bound


def test_sizes_that_do_not_fill_a_block_and_points_all_outside(eng, g):
    from isdf_amd.metrics import SdfMetrics, sdf_metrics
    vol = _volume(g, "signed")
    m = sdf_metrics(eng, vol, torch.zeros(0, 3, device="cuda"), torch.zeros(0, device="cuda"))
    assert m.n_valid == 0 and m.n_in_bounds == 0 and np.all(m.record == 0)
    assert np.isnan(m.av_l1) and all(np.isnan(m.binned_l1)) and all(np.isnan(m.l1_chomp_costs))
    for n in (1, 255, 257, 1000, 4099):
        model, _, _ = em.sdf_metrics(g["signed"], g["spacing"], g["origin"], g["pts"][:n], g["sdf"][:n])
        rec = eng.sdf_metrics(vol, _cuda(g["pts"][:n]), _cuda(g["sdf"][:n]))[0].cpu().numpy()
        assert np.array_equal(rec[[0, 1]], model[[0, 1]]) and np.array_equal(rec[9:15], model[9:15]), n
        bound = _bound(g["pts"], g["signed/gt"])
        assert np.abs(rec - model).max() <= bound * max(1.0, model[0]), n
    far = g["pts"] + np.float32(100.0)
    rec, gt, valid = eng.sdf_metrics(vol, _cuda(far), _cuda(g["sdf"]), per_point=True, oob_fill=0.0)
    assert np.all(rec.cpu().numpy() == 0) and not valid.any().item() and not gt.any().item()
    assert np.isnan(SdfMetrics(rec.cpu().numpy()).av_l1)


def test_record_is_bit_identical_run_to_run_and_stable_under_permutation(eng, g):
    vol = _volume(g, "zeroed")
    p, s = _cuda(g["pts"]), _cuda(g["sdf"])
    a = eng.sdf_metrics(vol, p, s)[0].clone()
    b = eng.sdf_metrics(vol, p, s)[0].clone()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    perm = torch.from_numpy(np.random.RandomState(0).permutation(len(g["pts"]))).cuda()
    c = eng.sdf_metrics(vol, p[perm].contiguous(), s[perm].contiguous())[0].cpu().numpy()
    a = a.cpu().numpy()
    assert np.array_equal(a[[0, 1]], c[[0, 1]]) and np.array_equal(a[9:15], c[9:15])
    assert np.abs(a - c).max() <= _bound(g["pts"], g["zeroed/gt"])


def _chomp_as_the_kernel(s, e):
    """eval.hip's chomp(): the three assignments, the quadratic written (1.0 / (2.0 * e)) * (s - e) * (s - e)"""
    c = -s + 0.5 * e
    c = np.where(s > 0.0, (1.0 / (2.0 * e)) * (s - e) * (s - e), c)
    return np.where(s > e, 0.0, c)


def _sdf_metrics_terms(sdf, gt, valid):
    """[n, 24] float64: what every point adds to the record, from the float32 inputs and the device's own per-point ground
    truth and validity (out of bounds = the NaN the call was given as oob_fill)"""
    s, g = sdf.astype(np.float64), gt.astype(np.float64)
    d = np.abs(s - g)
    t = np.zeros((len(s), em.RECORD))
    t[:, 0], t[:, 1], t[:, 2] = 1.0, 1.0, d
    lim = em.BIN_LIMITS.astype(np.float32)                      # compared in float32 against the float32 ground truth
    for b in range(6):
        with np.errstate(invalid="ignore"):
            m = (gt > lim[b]) & (gt < lim[b + 1])
        t[:, 3 + b], t[:, 9 + b] = np.where(m, d, 0.0), m
    for e, eps in enumerate(em.EPSILONS):
        cp, cg = _chomp_as_the_kernel(s, eps), _chomp_as_the_kernel(g, eps)
        t[:, 15 + 3 * e], t[:, 16 + 3 * e], t[:, 17 + 3 * e] = np.abs(cp - cg), cp, cg
    t[~valid] = 0.0
    t[:, 1] = ~np.isnan(gt)
    return t


@pytest.mark.parametrize("n", [1, 255, 257, 4099, 1024 * 256 + 257])
def test_sdf_metrics_record_equals_the_ordered_sums_bit_for_bit(eng, n):
    """all 24 entries against tests/reduce_model.py: a grid-stride share per thread, the block's order, the strided closing.
    Volume and predictions span 2^-20 .. 2^20 in magnitude, so another order gives other bytes (asserted against np.sum; a
    single term has one order only).  The last size is past 1024 blocks of 256: threads take a second element."""
    from isdf_amd.metrics import GtVolume
    rng = np.random.RandomState(n % 1000)
    vol = GtVolume(rm.wide(rng, (9, 8, 7)), [0.5, 0.25, 0.5], [-2.0, -1.0, -1.5], "cuda")
    pts = rng.uniform([-2.2, -1.1, -1.6], [2.2, 0.85, 1.6], (n, 3)).astype(np.float32)     # about one in four outside
    sdf = rm.wide(rng, n)
    sdf[::5] = np.abs(sdf[::5])                                  # every branch of the CHOMP cost
    vol.values.view(-1)[::11] = 0.0                              # ground truth == 0 on some faces: in bounds, not valid
    pts[::13] = np.float32([-2.0, -1.0, -1.5]) + np.float32([0.5, 0.25, 0.5]) * rng.randint(0, 7, (len(pts[::13]), 3)).astype(np.float32)
    rec, gt, valid = eng.sdf_metrics(vol, _cuda(pts), _cuda(sdf), per_point=True, oob_fill=float("nan"))
    rec, gt, valid = rec.cpu().numpy(), gt.cpu().numpy(), valid.cpu().numpy().astype(bool)
    terms = _sdf_metrics_terms(sdf, gt, valid)
    model = rm.close_strided(rm.grid_stride_record(terms, 1024))
    plain = terms.sum(0)
    print("n = %d: %d in bounds, %d valid; columns where the ordered sum is not np.sum: %d" % (n, rec[1], rec[0], (model != plain).sum()))
    if n >= 255:
        assert 0 < rec[0] < rec[1] < n and (model != plain).any()
    assert rec.tobytes() == model.tobytes(), np.flatnonzero(rec != model)


@pytest.mark.parametrize("n", [1, 257, 65536 + 300])
def test_nn_dist_sum_equals_the_ordered_sum_of_the_returned_distances(eng, n):
    """distances from 2^-20 to 2^20 against three targets; the last size gives more than 256 partials, so the closing threads take
    a second one"""
    rng = np.random.RandomState(2)             # a seed at which both larger sizes' ordered sums differ from np.sum
    t = rng.uniform(-1e-7, 1e-7, (3, 3)).astype(np.float32)
    q = (rm.wide(rng, (n, 1)) * rng.standard_normal((n, 3))).astype(np.float32)
    dist, _, total = eng.nn_distance(_cuda(q), _cuda(t))
    dist = dist.cpu().numpy()
    model = rm.ordered_sum(dist)
    if n > 1:
        assert model != dist.astype(np.float64).sum() and dist.max() > 2.0 ** 20 * dist.min()
    assert np.float64(total.item()).tobytes() == np.float64(model).tobytes()


def _keys(eng, n):
    """the squared distances the kernel compared: the high halves of the keys the workspace begins with (include/isdf_hip.h)"""
    k = eng._nn_ws[:8 * n].view(torch.int64).cpu().numpy()
    return ((k >> 32) & 0xffffffff).astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("n,m", [(1000, 777), (1025, 1), (300, 2049), (5000, 4097), (1, 5000), (2500, 2366)])
@pytest.mark.parametrize("want_index", [False, True])
def test_nn_squared_distances_equal_the_float32_model_bit_for_bit(eng, n, m, want_index):
    rng = np.random.RandomState(n + m)
    q = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    t = rng.uniform(-2, 2, (m, 3)).astype(np.float32)
    if m > 100:                                     # duplicate targets, the copy at the higher index: the lowest index wins
        t[m // 2:m // 2 + 40] = t[:40]
        q[:40] = (t[:40] + np.float32(1e-3))[:n]
    d2, idx = em.nn_sq_dist32(q, t)
    dist, index, total = eng.nn_distance(_cuda(q), _cuda(t), want_index=want_index)
    got2 = _keys(eng, n)
    assert np.array_equal(got2.view(np.uint32), d2.view(np.uint32))
    dist = dist.cpu().numpy()
    ref = np.sqrt(d2.astype(np.float64))
    assert np.all(np.abs(dist.astype(np.float64) - ref) <= np.spacing(ref.astype(np.float32)))       # within 1 ulp
    if want_index:
        assert np.array_equal(index.cpu().numpy().astype(np.int64), idx)
    else:
        assert index is None
    again = eng.nn_distance(_cuda(q), _cuda(t), want_index=want_index)[2]
    assert torch.equal(total.view(torch.int64), again.view(torch.int64))                              # the sum repeats bit for bit
    assert abs(float(total.item()) - dist.astype(np.float64).sum()) <= 1e-12 * max(1.0, dist.astype(np.float64).sum())


def test_nn_empty_query_set(eng):
    dist, _, total = eng.nn_distance(torch.zeros(0, 3, device="cuda"), torch.zeros(5, 3, device="cuda"))
    assert dist.numel() == 0 and float(total.item()) == 0.0


def test_accuracy_and_completion_equal_the_reference(eng, g):
    from isdf_amd.metrics import accuracy_completion
    acc, comp = accuracy_completion(eng, g["gt_points"], g["rec_points"])
    print("accuracy %.9f (ref %.9f) completion %.9f (ref %.9f)" % (acc, g["accuracy"][0], comp, g["completion"][0]))
    assert abs(acc - g["accuracy"][0]) <= 1e-6 * g["accuracy"][0]
    assert abs(comp - g["completion"][0]) <= 1e-6 * g["completion"][0]


class _Grid:
    """what graft() reads of trainer.gt_sdf_interp: `.grid` and `.values`; calling it is an error"""

    def __init__(self, grid, values):
        self.grid, self.values = grid, values

    def __call__(self, *a, **k):
        raise AssertionError("the bound evaluation must not call the host interpolator")


def test_grafted_evaluation_on_the_standin_trainer():
    from bench_support.standin_trainer import HipTrainer
    from isdf_amd import synthetic
    from isdf_amd.hot_path import HotPath
    from tests.accuracy_experiment import config
    cam = dict(H=96, W=128, fx=100.0, fy=100.0, cx=63.5, cy=47.5)
    tr = HipTrainer("cuda", config(cam), inv_bounds_transform=synthetic.bounds_transform(), rng="philox", seed=5)
    assert type(tr).eval_sdf is HotPath.eval_sdf and type(tr).eval_sdf_visible is HotPath.eval_sdf_visible
    T = synthetic.trajectory(90)[::15]
    depth = np.stack([synthetic.render_depth(T[i], cam, np.random.RandomState(i)) for i in range(len(T))])
    ds = em.CountingDataset(depth, T, 90)
    spacing, origin = np.array([0.1, 0.125, 0.1]), np.array([-0.5, -0.25, -0.5])
    ax = tuple(np.arange(n) * h + o for n, h, o in zip((71, 29, 61), spacing, origin))
    values = synthetic.gt_sdf(np.stack(np.meshgrid(*ax, indexing="ij"), -1)).astype(np.float32)
    tr.gt_sdf_interp, tr.cached_dataset, tr.tot_step_time = _Grid(ax, values), ds, 1.0
    e = tr.engine
    before = [t.clone() for t in (e.params, e.exp_avg, e.exp_avg_sq)]
    seen = {}
    inner = tr.eval_sdf_visible

    def spy(samples):
        # the bound eval_sdf_visible, minus the points float32 could bin differently from float64 (the rule of
        # tests/golden/make_eval_golden.py: within 1e-5 m of a bin limit, a CHOMP epsilon or zero, or 1e-4 voxel of a face)
        sdf, pts = inner(samples)
        p = pts.cpu().numpy().astype(np.float64)
        u = (p - origin) / spacing
        near = np.any((np.abs(u) < 1e-4) | (np.abs(u - (np.array(values.shape) - 1)) < 1e-4), axis=1)
        gt, inb = em.trilinear(values, spacing, origin, p)
        for edge in (0.0, 0.1, 0.2, 0.5, 1.0, 1.5, 2.0):
            near |= inb & (np.abs(gt - edge) < 1e-5)
        seen["dropped"] = float(near.mean())
        keep = torch.from_numpy(~near).to(pts.device)
        seen["out"] = (sdf[keep], pts[keep])
        return seen["out"]
    tr.eval_sdf_visible = spy
    res = tr.eval_sdf(samples=6000, visible_region=True)
    assert ds.reads == [30] and tr._hip.eval_cache.uploaded_frames == 30
    assert seen["dropped"] < 0.01
    sdf, pts = (t.cpu().numpy() for t in seen["out"])
    assert sdf.ndim == 1 and pts.shape == (len(sdf), 3) and len(sdf) > 4000
    model, gt, valid = em.sdf_metrics(values, spacing, origin, pts, sdf)
    want = em.result_dict(model)
    bound = _bound(pts, gt)
    print("graft: av_l1 %.6f (model %.6f), bound %.2e, n_valid %d" % (res["av_l1"], want["av_l1"], bound, model[0]))
    assert sorted(res) == ["av_l1", "binned_l1", "l1_chomp_costs"]
    assert abs(res["av_l1"] - want["av_l1"]) <= bound
    w, r = np.asarray(want["binned_l1"]), np.asarray(res["binned_l1"])
    assert np.array_equal(np.isnan(w), np.isnan(r)) and np.abs(w[~np.isnan(w)] - r[~np.isnan(w)]).max() <= bound
    assert np.abs(np.asarray(want["l1_chomp_costs"]) - np.asarray(res["l1_chomp_costs"])).max() <= bound
    for a, b in zip(before, (e.params, e.exp_avg, e.exp_avg_sq)):                    # evaluation trains nothing
        assert torch.equal(a, b)
    tr.tot_step_time += 1.0
    tr.eval_sdf(samples=6000)
    assert ds.reads == [30, 30] and tr._hip.eval_cache.uploaded_frames == 60         # 30 new frames, not the sequence
    assert tr._hip.eval_cache.uploaded_bytes == 60 * (96 * 128 + 16) * 4
    tr.drop_eval_cache()
    assert tr._hip.eval_cache is None and tr._hip.gt_volume is None
