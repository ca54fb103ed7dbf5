"""Point visibility against posed depth frames on the device: isdf_visible_points through Engine.visible_points,
isdf_amd.metrics.visible_points and graft().  References: the float32 model of tests/visible_model.py, which the kernel must equal
on EVERY pair (the header states the predicate operation by operation, every one rounded to float32), and the reference's own
masks (fixture visible_small, made by tests/golden/make_visible_golden.py from frustum.is_visible_torch on the CPU), compared
outside the fixture's `border` pairs (those on a limit in float64: under 1 % of them)."""
import types

import numpy as np
import pytest
import torch

from tests import eval_model as em
from tests import visible_model as vm

pytestmark = pytest.mark.gpu

CAM = vm.Cam(**vm.CAM)


@pytest.fixture(scope="module")
def g():
    g = vm.load_golden()
    for c in g["cases"]:              # the model once per case, shared by the tests below
        F = c["F"]
        c["model"] = vm.visible32(c["pts"], g["T_CW"][:F], g["depth"][:F], CAM.fx, CAM.fy, CAM.cx, CAM.cy, c["trunc"])
    return g


@pytest.fixture(scope="module")
def eng():
    from isdf_amd.engine import Engine, NetConfig
    return Engine(NetConfig(hidden=64, blocks=1), "cuda")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(eng, g, c, pts=None, **kw):
    F = c["F"]
    count, mask, n_seen = eng.visible_points(_cuda(c["pts"] if pts is None else pts), _cuda(g["T_CW"][:F]), _cuda(g["depth"][:F]), CAM,
                                             trunc=c["trunc"], **kw)
    return count.cpu().numpy(), None if mask is None else mask.cpu().numpy(), int(n_seen.item())


@pytest.mark.parametrize("case", range(6))
def test_mask_count_and_n_seen_against_model_and_reference(eng, g, case):
    c = g["cases"][case]
    count, mask, n_seen = _run(eng, g, c, want_mask=True)
    assert mask.dtype == np.uint8 and mask.shape == (c["F"], c["n"]) and count.dtype == np.int32 and mask.max() <= 1
    differ = int((mask.astype(bool) != c["model"]).sum())
    off_border = int(((mask.astype(bool) != c["mask"]) & ~c["border"]).sum())
    print("F %d n %d trunc %g: %d pairs differ from the model, %d from the reference outside the border (%d border pairs), "
          "%.2f %% visible" % (c["F"], c["n"], c["trunc"], differ, off_border, c["border"].sum(), 100 * mask.mean()))
    assert np.array_equal(mask.astype(bool), c["model"])                           # every pair
    assert np.array_equal(mask.astype(bool)[~c["border"]], c["mask"][~c["border"]])
    assert np.array_equal(count, mask.sum(0)) and n_seen == int((count > 0).sum())
    plain, none, seen2 = _run(eng, g, c)                                            # count only
    assert none is None and np.array_equal(plain, count) and seen2 == n_seen


def test_empty_and_partial_blocks_and_no_frames(eng, g):
    c = g["cases"][5]                                                               # 70 frames
    for n in (0, 1, 255):
        count, mask, n_seen = _run(eng, g, c, pts=c["pts"][:n], want_mask=True)
        assert count.shape == (n,) and mask.shape == (c["F"], n)
        assert np.array_equal(mask.astype(bool), c["model"][:, :n]) and np.array_equal(count, c["model"][:, :n].sum(0))
        assert n_seen == int((count > 0).sum())
    count, mask, n_seen = eng.visible_points(_cuda(c["pts"]), torch.zeros(0, 4, 4, device="cuda"), torch.zeros(0, 48, 64, device="cuda"),
                                             CAM, want_mask=True)
    assert count.shape == (c["n"],) and not count.any().item() and tuple(mask.shape) == (0, c["n"]) and int(n_seen.item()) == 0
    count, mask, n_seen = eng.visible_points(torch.zeros(0, 3, device="cuda"), torch.zeros(0, 4, 4, device="cuda"),
                                             torch.zeros(0, 48, 64, device="cuda"), CAM)
    assert count.numel() == 0 and mask is None and int(n_seen.item()) == 0


def test_runs_are_byte_identical_and_a_permutation_permutes_the_count(eng, g):
    c = g["cases"][3]                                                               # 3 frames, 4099 points
    a = _run(eng, g, c, want_mask=True)
    b = _run(eng, g, c, want_mask=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    perm = np.random.RandomState(0).permutation(c["n"])
    p = _run(eng, g, c, pts=c["pts"][perm], want_mask=True)
    assert np.array_equal(p[0], a[0][perm]) and np.array_equal(p[1], a[1][:, perm]) and p[2] == a[2]


def test_points_far_from_the_scene_are_seen_by_no_frame(eng, g):
    """100 m away every projection falls outside every image (or behind the camera): no pair may reach into `depth`"""
    c = g["cases"][5]
    far = c["pts"] + np.float32(100.0)
    assert not vm.visible32(far, g["T_CW"][:c["F"]], g["depth"][:c["F"]], CAM.fx, CAM.fy, CAM.cx, CAM.cy, c["trunc"]).any()
    count, mask, n_seen = _run(eng, g, c, pts=far, want_mask=True)
    assert not count.any() and not mask.any() and n_seen == 0


def test_metrics_visible_points_inverts_the_poses_on_the_device(eng, g):
    """T_WC in, torch.linalg.inv on the device: its inverse need not equal the CPU's bit for bit, so the comparison is with the
    reference's mask outside the border only"""
    from isdf_amd import metrics
    for c in (g["cases"][2], g["cases"][5]):
        F = c["F"]
        count, mask, n_seen = metrics.visible_points(eng, _cuda(c["pts"]), _cuda(g["T_WC"][:F]), _cuda(g["depth"][:F]), CAM,
                                                     trunc=c["trunc"], want_mask=True)
        mask, count = mask.cpu().numpy().astype(bool), count.cpu().numpy()
        keep = ~c["border"]
        print("F %d n %d: %d pairs differ from the reference outside the border" % (F, c["n"], (mask[keep] != c["mask"][keep]).sum()))
        assert np.array_equal(mask[keep], c["mask"][keep])
        assert np.array_equal(count, mask.sum(0)) and int(n_seen.item()) == int((count > 0).sum())


def _launcher_split(n, F):
    """(splits, frames per block) as launch_visible_points derives them, from the constants in visible.hip"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "isdf_amd", "csrc", "visible.hip")).read()
    k = {name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) for name in ("VIS_STAGE", "VIS_UNROLL", "VIS_BLOCKS")}
    pblocks = (n + 255) // 256
    splits = min(-(-k["VIS_BLOCKS"] // pblocks), -(-F // k["VIS_UNROLL"]), 65535)
    fpb = min(-(-(-(-F // splits)) // k["VIS_UNROLL"]) * k["VIS_UNROLL"], F)
    return -(-F // fpb), fpb, k["VIS_STAGE"]


def test_a_block_that_stages_its_frames_twice_equals_the_model_on_every_pair(eng):
    """The launcher splits the frames over blocks until about 2048 blocks exist, so the fixture's cases never give a block more than
    8 frames.  Here 150 frames meet 262 300 points (1025 point blocks, the last one partial): two block rows of 80 and 70 frames, and
    both re-stage their LDS rows (64 frames, then 16; 64, then 6 padded to a group of 8).  Frames as the fixture's (golden_util.synth_frames at 48 x 64); a quarter
    of the points back-projected pixels pushed -0.6 .. 0.3 m along the ray, the rest uniform in [-5, 5]^3; every pair against
    the float32 model, with and without the mask."""
    from tests.golden_util import synth_frames
    F, n = 150, 262300
    splits, fpb, stage = _launcher_split(n, F)
    assert fpb > stage and splits >= 2, "this case no longer makes a block stage twice: choose n and F again (%d, %d)" % (splits, fpb)
    rng = np.random.RandomState(5)
    c = vm.CAM
    depth, _, T_WC = synth_frames(rng, F, c["H"], c["W"], c["fx"], c["fy"], c["cx"], c["cy"])
    T_CW = np.linalg.inv(T_WC.astype(np.float64)).astype(np.float32)
    k = n // 4
    f = rng.randint(0, F, k)
    u, v = rng.uniform(0, c["W"], k), rng.uniform(0, c["H"], k)
    zc = depth[f, v.astype(int), u.astype(int)].astype(np.float64) + rng.uniform(-0.6, 0.3, k)
    pc = np.stack([(u - c["cx"]) / c["fx"] * zc, (v - c["cy"]) / c["fy"] * zc, zc, np.ones(k)], axis=1)
    near = np.einsum("nrc,nc->nr", T_WC[f].astype(np.float64), pc)[:, :3]
    pts = np.concatenate([near, rng.uniform(-5, 5, (n - k, 3))])[rng.permutation(n)].astype(np.float32)
    model = np.concatenate([vm.visible32(pts[s:s + 65536], T_CW, depth, CAM.fx, CAM.fy, CAM.cx, CAM.cy, 0.2)
                            for s in range(0, n, 65536)], axis=1)
    count, mask, n_seen = eng.visible_points(_cuda(pts), _cuda(T_CW), _cuda(depth), CAM, trunc=0.2, want_mask=True)
    mask, count = mask.cpu().numpy().astype(bool), count.cpu().numpy()
    print("F %d n %d, %d block rows of %d frames: %d pairs differ from the model, %.2f %% visible, frames past the first stage see "
          "%d pairs" % (F, n, splits, fpb, (mask != model).sum(), 100 * model.mean(), model[stage:fpb].sum()))
    assert model[stage:fpb].sum() > 1000 and model[fpb:].sum() > 1000          # the re-staged frames and the second row decide pairs
    assert np.array_equal(mask, model)
    assert np.array_equal(count, model.sum(0)) and int(n_seen.item()) == int((model.sum(0) > 0).sum())
    plain, none, seen2 = eng.visible_points(_cuda(pts), _cuda(T_CW), _cuda(depth), CAM, trunc=0.2)
    assert none is None and np.array_equal(plain.cpu().numpy(), count) and int(seen2.item()) == int(n_seen.item())


class _Grid:
    """what graft() reads of trainer.gt_sdf_interp: `.grid` and `.values`; calling it is an error"""

    def __init__(self, grid, values):
        self.grid, self.values = grid, values

    def __call__(self, *a, **k):
        raise AssertionError("the bound evaluation must not call the host interpolator")


def test_grafted_eval_object_sdf_reads_back_the_counts_only(tmp_path):
    from bench_support.standin_trainer import HipTrainer
    from isdf_amd import synthetic
    from isdf_amd.hot_path import HotPath
    from tests.accuracy_experiment import config
    cam = dict(H=96, W=128, fx=100.0, fy=100.0, cx=63.5, cy=47.5)
    tr = HipTrainer("cuda", config(cam), inv_bounds_transform=synthetic.bounds_transform(), rng="philox", seed=5)
    assert type(tr).eval_object_sdf is HotPath.eval_object_sdf
    T = synthetic.trajectory(90)[::15]
    depth = np.stack([synthetic.render_depth(T[i], cam, np.random.RandomState(i)) for i in range(len(T))])
    spacing, origin = np.array([0.1, 0.125, 0.1]), np.array([-0.5, -0.25, -0.5])
    ax = tuple(np.arange(n) * h + o for n, h, o in zip((71, 29, 61), spacing, origin))
    values = synthetic.gt_sdf(np.stack(np.meshgrid(*ax, indexing="ij"), -1)).astype(np.float32)
    tr.gt_sdf_interp, tr.cached_dataset, tr.tot_step_time = _Grid(ax, values), em.CountingDataset(depth, T, 90), 1.0
    # two boxes: one in free space 0.4 m in front of the first camera, one 40 m away from everything
    c = (T[0] @ np.array([0.0, 0.0, 0.4, 1.0]))[:3]
    bounds = np.array([[c - 0.02, c + 0.02], [[40, 40, 40], [40.1, 40.1, 40.1]]])
    tr.obj_bounds_file, tr.up_ix = str(tmp_path / "bounds.npy"), 1
    np.save(tr.obj_bounds_file, bounds)

    def refuse(*a, **k):
        raise AssertionError("frustum.is_visible_torch must not be entered")
    tr._hip.ref_module = types.SimpleNamespace(
        metrics=types.SimpleNamespace(get_obj_eval_bounds=lambda f, up_ix: np.load(f)),
        geometry=types.SimpleNamespace(frustum=types.SimpleNamespace(is_visible_torch=refuse)))
    seen = []
    inner = tr.engine.visible_points

    def spy(*a, **k):
        out = inner(*a, **k)
        seen.append((tuple(out[0].shape), out[1], tuple(a[2].shape), k))
        return out
    tr.engine.visible_points = spy
    errors = tr.eval_object_sdf(samples=2000)
    print("eval_object_sdf:", errors)
    assert len(errors) == 2 and np.isfinite(errors[0]) and np.isnan(errors[1])
    assert len(seen) == 1
    shape, mask, depth_shape, kw = seen[0]
    assert shape == (100 * 2,) and mask is None and depth_shape == (30, 96, 128)     # the counts, not an [F, N] mask
    assert kw.get("trunc") == 0.05 and not kw.get("want_mask", False)
