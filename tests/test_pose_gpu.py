"""Pose alignment on the device: isdf_pose_points / isdf_pose_system through Engine.pose_points, Engine.pose_system and
isdf_amd.tracking.  References: tests/pose_model.py -- the points must equal its float32 chain bit for bit, every entry of a
record must lie within 4e-12 x (sum of |term|) of its float64 sums over the very arrays the kernel read (twice the worst-case
reordering bound (N - 1) x 2^-53 at N = 19 200, the largest pose here; derived, not measured), the counts exactly."""
import contextlib
import io

import numpy as np
import pytest
import torch

from isdf_amd import tracking
from tests import pose_model as pm
from tests import reduce_model as rm

pytestmark = pytest.mark.gpu

CAM = pm.cam_of(48, 64, 60.0)
BOUND = 4e-12
MIN_D, MAX_D = 0.5, 4.0          # both exact in float32


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _special_depth(T):
    """a rendered frame with every kind of unusable pixel written into it, and pixels exactly on both limits"""
    d = pm.render(T[:1], CAM, seed=3)[0]
    flat = d.reshape(-1)
    vals = [0.0, np.nan, np.inf, -np.inf, -1.0, np.nextafter(np.float32(MIN_D), np.float32(0)), MIN_D, MAX_D,
            np.nextafter(np.float32(MAX_D), np.float32(np.inf)), 0.25, 1e-30]
    for k, v in enumerate(vals * 12):
        flat[5 * k + 1] = v
    return d[None]


@pytest.fixture(scope="module")
def cases():
    """name -> dict(depth, T, cam, fop, stride, min_depth, max_depth); rendered once, shared by the tests below"""
    T = pm.poses8()
    c = {}
    c["48x64 stride 1"] = dict(depth=pm.render(T, CAM, seed=0), T=pm.perturb(T, 0.03, 2.0, seed=1), cam=CAM, fop=None, stride=1)
    ragged = pm.cam_of(37, 53, 50.0)
    c["37x53 stride 3"] = dict(depth=pm.render(T[:2], ragged, seed=1), T=pm.perturb(T[:2], 0.03, 2.0, seed=2), cam=ragged, fop=None, stride=3)
    c["two poses on one frame"] = dict(depth=c["48x64 stride 1"]["depth"][:2], T=pm.perturb(T[[0, 1, 1]], 0.08, 5.0, seed=3), cam=CAM,
                                       fop=[0, 1, 1], stride=4)
    c["special depth values"] = dict(depth=_special_depth(T), T=pm.perturb(T[:1], 0.03, 2.0, seed=4), cam=CAM, fop=None, stride=1,
                                     min_depth=MIN_D, max_depth=MAX_D)
    big = pm.cam_of(120, 160, 150.0)
    c["120x160 stride 1"] = dict(depth=pm.render(T[:2], big, seed=2), T=pm.perturb(T[:2], 0.03, 2.0, seed=5), cam=big, fop=None, stride=1)
    for v in c.values():
        v.setdefault("min_depth", 0.0)
        v.setdefault("max_depth", float("inf"))
        v["kw"] = dict(frame_of_pose=v["fop"], stride=v["stride"], min_depth=v["min_depth"], max_depth=v["max_depth"])
        v["model_pts"], v["model_valid"] = pm.points32(v["depth"], v["T"], v["cam"], **v["kw"])
    return c


@pytest.fixture(scope="module")
def eng():
    from isdf_amd.engine import Engine, NetConfig
    return Engine(NetConfig(hidden=64, blocks=1), "cuda")


POINT_CASES = ["48x64 stride 1", "37x53 stride 3", "two poses on one frame", "special depth values"]


@pytest.mark.parametrize("name", POINT_CASES)
def test_points_equal_the_float32_model_bit_for_bit(eng, cases, name):
    c = cases[name]
    pts = eng.pose_points(_cuda(c["depth"]), c["T"], c["cam"], **c["kw"]).cpu().numpy()
    H, W = c["depth"].shape[1:]
    n_pix = -(-H // c["stride"]) * -(-W // c["stride"])
    assert pts.shape == (len(c["T"]) * n_pix, 3) and pts.dtype == np.float32 and np.isfinite(pts).all()
    differ = int((pts.view(np.uint32) != c["model_pts"].view(np.uint32)).any(-1).sum())
    print("%s: %d points, %d valid, %d differ from the model" % (name, len(pts), c["model_valid"].sum(), differ))
    assert differ == 0
    if name == "special depth values":
        # the limits themselves are valid, everything outside them and every non-number is not; those points are the camera centre
        flat, ok = c["depth"].reshape(-1), c["model_valid"]
        assert ok[flat == np.float32(MIN_D)].all() and ok[flat == np.float32(MAX_D)].all() and (flat == np.float32(MIN_D)).sum() >= 12
        with np.errstate(invalid="ignore"):
            assert not ok[~np.isfinite(flat) | (flat < MIN_D) | (flat > MAX_D)].any()
        assert (pts[~ok] == c["T"][0, :3, 3].astype(np.float32)).all()


def _system(eng, c, sdf=None, grad=None, huber=0.05, trunc=0.3, **kw):
    """(records [B, 32] from the device, the arrays the kernel read)"""
    depth = _cuda(c["depth"])
    pts = eng.pose_points(depth, c["T"], c["cam"], **c["kw"])
    if sdf is None:
        sdf, grad = pm.room_field_torch(pts)
    rec = eng.pose_system(depth, c["T"], c["cam"], pts, sdf, grad, huber=huber, trunc=trunc, **c["kw"], **kw)
    return rec.cpu().numpy(), (pts.cpu().numpy(), sdf.cpu().numpy(), grad.cpu().numpy())


def _assert_records(name, rec, model, scale):
    err = np.abs(rec - model)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(scale > 0, err / scale, np.where(err == 0, 0.0, np.inf))
    print("%s: used %s of valid %s, worst |record - model| / sum |term| = %.3g (bound %.1g)"
          % (name, rec[:, 0].astype(int).tolist(), rec[:, 1].astype(int).tolist(), rel[:, 2:].max(), BOUND))
    assert np.array_equal(rec[:, :2], model[:, :2])                    # the counts, exactly
    assert (err <= BOUND * scale).all()


@pytest.mark.parametrize("name", POINT_CASES + ["120x160 stride 1"])
def test_records_are_within_the_reordering_bound_of_the_float64_model(eng, cases, name):
    c = cases[name]
    rec, (pts, sdf, grad) = _system(eng, c)
    assert rec.shape == (len(c["T"]), 32) and rec.dtype == np.float64
    model, scale = pm.records64(pts, sdf, grad, c["model_valid"], c["T"])
    _assert_records(name, rec, model, scale)
    assert (rec[:, 0] >= 64).all() and (rec[:, 1] == c["model_valid"].reshape(len(c["T"]), -1).sum(1)).all()
    if name == "120x160 stride 1":
        assert c["model_valid"].size // 2 == 19200 > 64 * 256              # more than one pass of the capped grid


@pytest.mark.parametrize("name", ["12x16 stride 1", "120x160 stride 1"])
def test_records_equal_the_ordered_sums_of_the_model_bit_for_bit(eng, cases, name):
    """all 32 entries against tests/reduce_model.py: a grid-stride share per thread, the block's order, then a pose's partial
    records in block order.  192 pixels are one partial block; 19 200 are more than 64 x 256, so threads take a second pixel.
    Residuals and gradients span 2^-20 .. 2^20 in magnitude, so another order gives other bytes (asserted against np.sum)."""
    if name == "12x16 stride 1":
        cam, T = pm.cam_of(12, 16, 15.0), pm.poses8()[:2]
        c = dict(depth=pm.render(T, cam, seed=6, invalid_frac=0.1), T=pm.perturb(T, 0.03, 2.0, seed=7), cam=cam,
                 kw=dict(frame_of_pose=None, stride=1, min_depth=0.0, max_depth=float("inf")))
        c["model_valid"] = pm.points32(c["depth"], c["T"], cam, **c["kw"])[1]
    else:
        c = cases[name]
    n = c["model_valid"].size
    rng = np.random.RandomState(n)
    sdf, grad = rm.wide(rng, n), rm.wide(rng, (n, 3))
    sdf[::17] = np.float32(2.0 ** 21)                   # beyond the truncation: not used
    sdf[5::29] = np.nan
    huber, trunc = 1.0, 2.0 ** 20                       # about half of the residuals on either branch of the Huber weight
    rec, (pts, _, _) = _system(eng, c, sdf=_cuda(sdf), grad=_cuda(grad), huber=huber, trunc=trunc)
    terms = pm.terms64(pts, sdf, grad, c["model_valid"], c["T"], huber, trunc)
    assert terms.shape == (2, n // 2, 32)
    model = np.stack([rm.close_serial(rm.grid_stride_record(t, 64)) for t in terms])       # ISDF_POSE_MAX_BLOCKS
    plain = terms.sum(1)
    print("%s: used %s of valid %s; entries where the ordered sum is not np.sum: %s of 32"
          % (name, rec[:, 0].astype(int).tolist(), rec[:, 1].astype(int).tolist(), (model != plain).sum(1).tolist()))
    assert (0 < rec[:, 0]).all() and (rec[:, 0] < rec[:, 1]).all() and (rec[:, 1] < n // 2).all()
    assert (model != plain).any(1).all()
    assert rec.tobytes() == model.tobytes(), np.argwhere(rec != model)


def test_huber_and_truncation_borders(eng):
    """one valid pixel, eight copies of the pose, one hand-made residual each: every record is a single term, so the weight and
    the used flag are read off exactly.  huber and trunc are float32, as the ABI takes them."""
    h, t = np.float32(0.05), np.float32(0.3)
    up = lambda v: np.nextafter(v, np.float32(np.inf))
    sdf = np.array([h, -h, up(h), -up(h), t, -t, up(t), -up(t)], np.float32)
    depth = np.zeros((1, 8, 8), np.float32)
    depth[0, 3, 5] = 2.0
    cam = pm.cam_of(8, 8, 10.0)
    T = np.repeat(pm.poses8()[:1], 8, 0)
    c = dict(depth=depth, T=T, cam=cam, kw=dict(frame_of_pose=[0] * 8, stride=1, min_depth=0.0, max_depth=float("inf")))
    full = np.zeros((8, 64), np.float32)
    full[:, 3 * 8 + 5] = sdf
    full[:, 0] = 0.01                                # an invalid pixel's residual must not count
    grad = np.random.RandomState(0).standard_normal((8 * 64, 3)).astype(np.float32)
    rec, (pts, _, _) = _system(eng, c, sdf=_cuda(full.reshape(-1)), grad=_cuda(grad), huber=float(h), trunc=float(t))
    model, scale = pm.records64(pts, full.reshape(-1), grad, pm.points32(depth, T, cam, **c["kw"])[1], T, h, t)
    r = sdf.astype(np.float64)
    assert np.array_equal(rec[:, 1], np.ones(8))
    assert np.array_equal(rec[:, 0], [1, 1, 1, 1, 1, 1, 0, 0])                      # used AT the truncation border, not beyond it
    assert np.array_equal(rec[:2, 2], r[:2] * r[:2]) and np.array_equal(rec[:2, 3], 0.5 * (r[:2] * r[:2]))   # weight 1 AT the Huber border
    w = float(h) / np.abs(r[2:6])
    assert (w < 1).all() and np.array_equal(rec[2:6, 2], (w * r[2:6]) * r[2:6])    # ... and huber / |r| one ulp beyond
    assert np.array_equal(rec[2:6, 3], float(h) * (np.abs(r[2:6]) - 0.5 * float(h)))
    assert np.array_equal(rec[6:, 2:], np.zeros((2, 30)))
    assert np.array_equal(rec[:, 31], np.abs(r) * rec[:, 0])
    _assert_records("borders", rec, model, scale)


def test_two_runs_are_bit_identical_and_a_pose_alone_equals_itself_in_a_batch(eng, cases):
    c = cases["two poses on one frame"]
    depth = _cuda(c["depth"])
    pts = eng.pose_points(depth, c["T"], c["cam"], **c["kw"])
    sdf, grad = pm.room_field_torch(pts)
    a = eng.pose_system(depth, c["T"], c["cam"], pts, sdf, grad, **c["kw"]).cpu().numpy()
    b = eng.pose_system(depth, c["T"], c["cam"], pts, sdf, grad, **c["kw"]).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    n = pts.shape[0] // 3
    for k in range(3):
        kw = dict(c["kw"], frame_of_pose=[c["fop"][k]])
        s = slice(k * n, (k + 1) * n)
        alone_pts = eng.pose_points(depth, c["T"][k:k + 1], c["cam"], **kw)
        assert torch.equal(alone_pts, pts[s])
        alone = eng.pose_system(depth, c["T"][k:k + 1], c["cam"], pts[s], sdf[s], grad[s], **kw).cpu().numpy()
        assert alone.tobytes() == a[k:k + 1].tobytes(), k


def test_refine_pose_on_the_exact_field_finds_the_true_pose(eng, cases):
    T_true = pm.poses8()[::2]
    depth = _cuda(cases["48x64 stride 1"]["depth"][::2])
    T0 = pm.perturb(T_true, 0.08, 5.0, seed=11)
    res = tracking.refine_pose(eng, depth, T0, CAM, stride=4, field=pm.room_field_torch)
    dt, dr = pm.pose_error(res.T_WC, T_true)
    print("iterations %s, reasons %s, worst error %.3g m %.3g deg" % (res.iterations.tolist(), res.reason, dt.max(), dr.max()))
    assert res.converged.all() and res.iterations.max() <= 10
    assert dt.max() <= 1e-5 and dr.max() <= 1e-4
    assert res.T_WC.dtype == np.float64 and res.T_WC.shape == (4, 4, 4)


@pytest.fixture(scope="module")
def trainer():
    from bench_support.standin_trainer import HipTrainer
    from isdf_amd import synthetic
    from tests.accuracy_experiment import config
    cam = dict(H=96, W=128, fx=100.0, fy=100.0, cx=63.5, cy=47.5)
    np.random.seed(5)
    torch.manual_seed(5)
    tr = HipTrainer("cuda", config(cam), inv_bounds_transform=synthetic.bounds_transform(), rng="philox", seed=5)
    return tr, cam


def test_pose_system_with_the_network_equals_the_model_on_the_engines_own_outputs(trainer):
    """default-shape engine (hidden 256, two blocks) at its initial weights; trunc wide enough that an untrained field's
    residuals are used"""
    tr, cam = trainer
    eng = tr.engine
    c = pm.cam_of(96, 128, 100.0)
    T = pm.perturb(pm.poses8()[:3], 0.03, 2.0, seed=6)
    depth = pm.render(pm.poses8()[:3], c, seed=4)
    kw = dict(frame_of_pose=None, stride=4, min_depth=0.0, max_depth=float("inf"))
    pts = eng.pose_points(_cuda(depth), T, c, **kw)
    with torch.no_grad():
        sdf, grad = eng.sdf_eval(pts, want_grad=True)
    model, scale = pm.records64(pts.cpu().numpy(), sdf.cpu().numpy(), grad.cpu().numpy(), pm.points32(depth, T, c, **kw)[1], T,
                                0.05, 10.0)
    s = tracking.pose_system(eng, _cuda(depth), T, c, stride=4, huber=0.05, trunc=10.0)
    _assert_records("network field", s.records, model, scale)
    assert (s.used >= 64).all() and np.isfinite(s.records).all()
    assert np.array_equal(s.H, np.transpose(s.H, (0, 2, 1))) and np.array_equal(s.H[:, 0, 5], s.records[:, 15])


def test_refine_pose_and_refine_frames_on_a_grafted_trainer_leave_the_keyframes_alone(trainer):
    from isdf_amd import synthetic
    tr, cam = trainer
    traj = synthetic.trajectory(40)
    rng = np.random.RandomState(7)
    with contextlib.redirect_stdout(io.StringIO()):
        for k in range(3):
            fr = tr.make_frame(k * 5, synthetic.render_depth(traj[k * 5], cam, rng, noise_std=0.0), traj[k * 5])
            tr.last_is_keyframe = True
            tr.add_frame(fr)
            tr.noise_std = tr.noise_kf
            for _ in range(3):
                tr.step()
    before = tr.frames.T_WC_batch.clone()
    depth_before = tr.frames.depth_batch.clone()
    res = tracking.refine_frames(tr, iters=3)
    assert res.T_WC.shape == (3, 4, 4) and np.isfinite(res.T_WC).all() and len(res.reason) == 3
    assert all(1 <= n <= 3 for n in res.iterations) and all(np.isfinite(h[0][0]) for h in res.history)
    one = tracking.refine_frames(tr, idxs=[2], iters=2, trunc=1.0)
    assert one.T_WC.shape == (1, 4, 4) and np.isfinite(one.T_WC).all()
    T0 = pm.perturb(before.cpu().numpy()[:2], 0.03, 2.0, seed=8)
    res2 = tracking.refine_pose(tr, tr.frames.depth_batch, T0, tr, frame_of_pose=[0, 1], iters=3, trunc=1.0)
    assert res2.T_WC.shape == (2, 4, 4) and np.isfinite(res2.T_WC).all()
    assert all(np.isfinite(h[0][0]) and h[0][1] >= 0 for h in res2.history)
    print("refine_frames:", res.reason, res.iterations.tolist(), "| refine_pose:", res2.reason, [h[-1] for h in res2.history])
    assert torch.equal(tr.frames.T_WC_batch, before) and torch.equal(tr.frames.depth_batch, depth_before)
