"""SDF slice images on the device: isdf_slice_images and isdf_plane_points through Engine / isdf_amd.slices and through graft().
References: matplotlib's own colours and the reference's compute_slices slabs recorded in fixture slices_small
(tests/golden/make_slices_golden.py), the float32 models of tests/slice_model.py (colour index, cost fields, plane points: bit for
bit) and the float64 trilinear model of tests/eval_model.py (the ground truth, within a bound derived from the volume)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import eval_model as em
from tests import golden_util as gu
from tests import slice_model as sm

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def g():
    return sm.load_golden()


@pytest.fixture(scope="module")
def sdf_map():
    """the trained default net (fixture trained_default) the reference's slabs were recorded with"""
    from isdf_amd.modules import PositionalEncodingHIP, SDFMapHIP
    t = gu.load("trained_default")
    net = t["net"]
    pe = PositionalEncodingHIP(min_deg=0, max_deg=int(net[2]) - 1, scale=float(net[3]),
                               transform=torch.from_numpy(t["bounds_T"].astype(np.float32)))
    m = SDFMapHIP(pe, hidden_size=int(net[0]), hidden_layers_block=int(net[1]), scale_output=float(net[4]), device="cuda")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in gu.params_of(t).items()})
    return m


@pytest.fixture(scope="module")
def eng(sdf_map):
    return sdf_map.engine


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cmap(g, name):
    from isdf_amd.slices import Colormap
    rgb, lim = g[name + "/rgb"], g[name + "/lim"]
    return Colormap(rgb[:-3], rgb[-3], rgb[-2], rgb[-1], lim[0], lim[1])


def _volume(g):
    from isdf_amd.metrics import GtVolume
    return GtVolume(g["vol"], g["vol_spacing"], g["vol_origin"], "cuda")


def _gt_bound(g, pts):
    """|kernel ground truth - float64 trilinear model| for in-bounds points.  The grid coordinate u = (p - o) / h is made of
    float32 roundings of the origin, the difference, the spacing and the quotient (2^-24 relative each): |du| <= 2 eps32 (max |u|
    + max |o| / min h).  A coordinate error moves the trilinear value by at most the largest difference D between neighbouring
    grid values per axis, 3 D |du| in all (the value is continuous across cells, so a cell chosen differently costs nothing
    more).  Each of the seven blends rounds its difference and its result, eps32 (max |v| + D) per blend at most, and later blends
    pass earlier errors on with weights that sum to one: seven value roundings."""
    v = g["vol"].astype(np.float64)
    D = max(np.abs(np.diff(v, axis=a)).max() for a in range(3))
    u = (np.asarray(pts, np.float64).reshape(-1, 3) - g["vol_origin"]) / g["vol_spacing"]
    inb = np.all((u >= 0) & (u <= np.array(v.shape) - 1), axis=1)
    du = 2 * EPS32 * (np.abs(u[inb]).max(initial=0.0) + np.abs(g["vol_origin"]).max() / g["vol_spacing"].min())
    return 7 * EPS32 * (np.abs(v).max() + D) + 3 * D * du


def _check_gt(g, pts, gt, fill):
    """the kernel's ground truth against the float64 model; -> number of in-bounds points.  No slab point lies within 1e-4 voxel
    of a face of the volume (asserted), so float32 and float64 agree on which points are inside."""
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    u = (p - g["vol_origin"]) / g["vol_spacing"]
    assert not np.any((np.abs(u) < 1e-4) | (np.abs(u - (np.array(g["vol"].shape) - 1)) < 1e-4))
    ref, inb = em.trilinear(g["vol"], g["vol_spacing"], g["vol_origin"], p)
    gt = np.asarray(gt).reshape(-1)
    assert np.all(gt[~inb] == np.float32(fill))
    bound = _gt_bound(g, p)
    err = np.abs(gt[inb].astype(np.float64) - ref[inb]).max(initial=0.0)
    print("ground truth: %d of %d points inside, max error %.3e (bound %.3e)" % (inb.sum(), len(inb), err, bound))
    assert err <= bound
    return int(inb.sum())


# ------------------------------------------------------------------ the kernels through Engine / isdf_amd.slices
@pytest.mark.parametrize("name", ["t2", "t05"])
def test_fixture_values_reproduce_the_recorded_matplotlib_colours(eng, g, name):
    cmap = _cmap(g, name)
    v = g["values"]
    rgb = eng.slice_images(None, _cuda(v), cmap)[0]
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (len(v), 3)
    got = rgb.cpu().numpy()
    wrong = (got != g[name + "/colours"]).any(-1)
    print("%s: %d values, %d colours differ from matplotlib's" % (name, len(v), wrong.sum()))
    assert not wrong.any(), v[wrong][:10]


@pytest.mark.parametrize("case", ["A", "B"])
def test_slice_images_against_the_models(eng, g, case):
    from isdf_amd import slices
    cmap, vol = _cmap(g, "t2"), _volume(g)
    pts = _cuda(g[case + "/pts"])
    res = slices.slice_images(eng, pts, cmap, gt_volume=vol, chomp_eps=2.0, oob_fill=0.0)
    lead = tuple(pts.shape[:-1])
    assert tuple(res.sdf.shape) == tuple(res.gt.shape) == tuple(res.pred_cost.shape) == tuple(res.gt_cost.shape) == lead
    assert tuple(res.pred_rgb.shape) == tuple(res.gt_rgb.shape) == lead + (3,)
    assert res.pred_rgb.dtype == res.gt_rgb.dtype == torch.uint8 and res.gt.dtype == res.pred_cost.dtype == torch.float32
    sdf, gt = res.sdf.cpu().numpy(), res.gt.cpu().numpy()
    assert np.array_equal(sdf, eng.sdf_eval(pts).cpu().numpy())                               # the one forward over all slices
    lim = g["t2/lim"]
    assert np.array_equal(res.pred_rgb.cpu().numpy(), sm.colours(sdf, cmap.rgb, lim[0], lim[1]))
    assert np.array_equal(res.gt_rgb.cpu().numpy(), sm.colours(gt, cmap.rgb, lim[0], lim[1]))
    assert np.array_equal(res.pred_cost.cpu().numpy().view(np.uint32), sm.chomp32(sdf, 2.0).view(np.uint32))
    assert np.array_equal(res.gt_cost.cpu().numpy().view(np.uint32), sm.chomp32(gt, 2.0).view(np.uint32))
    n_in = _check_gt(g, g[case + "/pts"], gt, 0.0)
    assert 0.4 * gt.size < n_in < gt.size
    # the same ground truth as isdf_sdf_metrics (one shared device function), another fill value
    gt7 = eng.slice_images(pts, None, None, vol, None, oob_fill=-7.0)[1]
    _, gtm, _ = eng.sdf_metrics(vol, pts, res.sdf, per_point=True, oob_fill=-7.0)
    assert torch.equal(gt7.view(torch.int32), gtm.view(torch.int32))
    # two runs give identical bytes
    again = slices.slice_images(eng, pts, cmap, gt_volume=vol, chomp_eps=2.0, oob_fill=0.0)
    for a, b in ((res.pred_rgb, again.pred_rgb), (res.gt_rgb, again.gt_rgb), (res.gt.view(torch.int32), again.gt.view(torch.int32)),
                 (res.pred_cost.view(torch.int32), again.pred_cost.view(torch.int32)),
                 (res.gt_cost.view(torch.int32), again.gt_cost.view(torch.int32))):
        assert torch.equal(a, b)


def test_cost_fields_at_other_epsilons_and_special_values(eng, g):
    v = _cuda(g["values"])
    for eps in (0.5, 1.0, 1.5, 2.0):
        cost = eng.slice_images(None, v, None, None, eps)[3].cpu().numpy()
        want = sm.chomp32(g["values"], eps)
        assert np.array_equal(cost.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)]), eps
        assert np.array_equal(np.isnan(cost), np.isnan(want))


@pytest.mark.parametrize("n", [0, 1, 2, 3, 5, 255, 1023, 1025, 4099])
def test_sizes_that_do_not_fill_a_quad_or_a_block(eng, g, n):
    cmap, vol = _cmap(g, "t05"), _volume(g)
    pts = g["A/pts"].reshape(-1, 3)[7:7 + n]
    sdf = g["values"][11:11 + n]
    out = eng.slice_images(_cuda(pts), _cuda(sdf), cmap, vol, 1.5, oob_fill=0.25)
    pred_rgb, gt, gt_rgb, pred_cost, gt_cost = (t.cpu().numpy() for t in out)
    assert pred_rgb.shape == gt_rgb.shape == (n, 3) and gt.shape == pred_cost.shape == gt_cost.shape == (n,)
    if n == 0:
        return
    lim = g["t05/lim"]
    assert np.array_equal(pred_rgb, sm.colours(sdf, cmap.rgb, lim[0], lim[1]))
    assert np.array_equal(gt_rgb, sm.colours(gt, cmap.rgb, lim[0], lim[1]))
    assert np.array_equal(pred_cost.view(np.uint32), sm.chomp32(sdf, 1.5).view(np.uint32))
    assert np.array_equal(gt_cost.view(np.uint32), sm.chomp32(gt, 1.5).view(np.uint32))
    _check_gt(g, pts, gt, 0.25)


def test_unaligned_buffers_take_the_element_wise_path(eng, g):
    """inputs and outputs that start off a 16-byte (colours: 4-byte) boundary: the kernel must not use its wide accesses; bytes
    around the outputs stay untouched"""
    from isdf_amd import _ffi
    from isdf_amd.engine import _stream
    cmap, vol = _cmap(g, "t2"), _volume(g)
    n = 1001
    pts_h, sdf_h = g["B/pts"].reshape(-1, 3)[:n], g["B/sdf"].reshape(-1)[:n]
    pts = torch.zeros(3 * n + 1, device="cuda")
    sdf = torch.zeros(n + 1, device="cuda")
    pts[1:].copy_(_cuda(pts_h).reshape(-1)); sdf[1:].copy_(_cuda(sdf_h))
    rgb = torch.full((2, 3 * n + 8), 77, dtype=torch.uint8, device="cuda")
    f32 = torch.full((3, n + 2), -123.0, device="cuda")
    cm, v = cmap.to_c("cuda"), vol.to_c()
    rc = eng.lib.isdf_slice_images(pts.data_ptr() + 4, sdf.data_ptr() + 4, n, C.byref(cm), C.byref(v), 0.0, 2.0,
                                   rgb[0].data_ptr() + 1, f32[0].data_ptr() + 4, rgb[1].data_ptr() + 3, f32[1].data_ptr() + 4,
                                   f32[2].data_ptr() + 4, _stream(eng.device))
    _ffi.check(rc, "isdf_slice_images")
    want = eng.slice_images(_cuda(pts_h), _cuda(sdf_h), cmap, vol, 2.0)
    rgb_h, f_h = rgb.cpu().numpy(), f32.cpu().numpy()
    assert np.array_equal(rgb_h[0, 1:1 + 3 * n].reshape(n, 3), want[0].cpu().numpy())
    assert np.array_equal(rgb_h[1, 3:3 + 3 * n].reshape(n, 3), want[2].cpu().numpy())
    assert (rgb_h[0, :1] == 77).all() and (rgb_h[0, 1 + 3 * n:] == 77).all() and (rgb_h[1, :3] == 77).all() and (rgb_h[1, 3 + 3 * n:] == 77).all()
    for row, k in ((0, 1), (1, 3), (2, 4)):
        assert np.array_equal(f_h[row, 1:1 + n].view(np.uint32), want[k].cpu().numpy().view(np.uint32))
        assert f_h[row, 0] == -123.0 and f_h[row, n + 1] == -123.0


def test_a_table_of_one_colour_and_a_large_table(eng, g):
    from isdf_amd.slices import Colormap
    v = g["values"]
    u8 = lambda *c: np.array(c, np.uint8)
    one = Colormap(u8([10, 20, 30]), u8(1, 2, 3), u8(4, 5, 6), u8(7, 8, 9), -0.5, 0.5)
    got = eng.slice_images(None, _cuda(v), one)[0].cpu().numpy()
    assert np.array_equal(got, sm.colours(v, one.rgb, -0.5, 0.5))
    assert {tuple(c) for c in got.tolist()} == {(10, 20, 30), (1, 2, 3), (4, 5, 6), (7, 8, 9)}
    rng = np.random.RandomState(1)
    big = Colormap(rng.randint(0, 256, (16381, 3)).astype(np.uint8), u8(1, 2, 3), u8(4, 5, 6), u8(7, 8, 9), -2.0, 2.0)   # 64 KiB of LDS
    got = eng.slice_images(None, _cuda(v), big)[0].cpu().numpy()
    assert np.array_equal(got, sm.colours(v, big.rgb, -2.0, 2.0))
    with pytest.raises(ValueError):
        Colormap(np.zeros((16382, 3), np.uint8), u8(1, 2, 3), u8(4, 5, 6), u8(7, 8, 9), -2.0, 2.0)


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (48, 48), (37, 101), (256, 256), (0, 7)])
def test_plane_points_equal_the_model_bit_for_bit(eng, H, W):
    rng = np.random.RandomState(H * 1000 + W)
    o, du, dv = rng.uniform(-3, 3, 3), rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.05, 0.05, 3)
    got = eng.plane_points(o, du, dv, H, W)
    assert tuple(got.shape) == (H, W, 3) and got.dtype == torch.float32
    want = sm.plane_points(o, du, dv, H, W)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_plane_slices_equal_slices_of_the_same_points(eng, g):
    from isdf_amd import slices
    cmap, vol = _cmap(g, "t2"), _volume(g)
    pl = slices.plane(eng, [0.3, 1.4, 0.2], [0.11, 0.0, 0.0], [0.0, 0.0, 0.09], 50, 52, cmap, gt_volume=vol, chomp_eps=2.0)
    assert np.array_equal(pl.pts.cpu().numpy(), sm.plane_points([0.3, 1.4, 0.2], [0.11, 0.0, 0.0], [0.0, 0.0, 0.09], 50, 52))
    same = slices.slice_images(eng, pl.pts.clone(), cmap, gt_volume=vol, chomp_eps=2.0)
    assert torch.equal(pl.pred_rgb, same.pred_rgb) and torch.equal(pl.gt_rgb, same.gt_rgb) and torch.equal(pl.gt, same.gt)
    assert tuple(pl.pred_rgb.shape) == (50, 52, 3)
    _check_gt(g, pl.pts.cpu().numpy(), pl.gt.cpu().numpy(), 0.0)


# ------------------------------------------------------------------ the bound methods on a grafted trainer
class _Recorder:
    """stands in for the reference module's cv2 and imgviz: keeps what it is handed"""

    def __init__(self):
        self.resized, self.costs = [], []

    def resize(self, img, dsize):
        self.resized.append(np.asarray(img).copy())
        return np.zeros((int(dsize[1]), int(dsize[0]), 3), np.uint8)

    def depth2rgb(self, depth, min_value=None, max_value=None):
        self.costs.append(np.asarray(depth).copy())
        return np.zeros(np.asarray(depth).shape + (3,), np.uint8)


def _trainer(g, case, sdf_map_fixture):
    from bench_support.standin_trainer import HipTrainer
    from isdf_amd import synthetic
    from tests.accuracy_experiment import config
    cam = dict(H=96, W=128, fx=100.0, fy=100.0, cx=63.5, cy=47.5)
    tr = HipTrainer("cuda", config(cam), inv_bounds_transform=synthetic.bounds_transform(), rng="philox", seed=5)
    tr.sdf_map.load_state_dict({k: v.detach().clone() for k, v in sdf_map_fixture.state_dict().items()})
    sm.set_slice_geometry(tr, case, "cuda")
    tr.gt_sdf_interp = sm.GridInterp(g["vol"], g["vol_spacing"], g["vol_origin"])
    tr.obj_bounds_file = None
    rec = _Recorder()
    tables = {(-2, 2): "t2", (-0.5, 0.5): "t05"}

    def get_colormap(sdf_range=[-2, 2], surface_cutoff=0.01):
        name = tables[(sdf_range[0], sdf_range[1])]
        sdf_range[0], sdf_range[1] = float(g[name + "/lim"][0]), float(g[name + "/lim"][1])       # the reference edits its argument
        return sm.TableMappable(g[name + "/rgb"], *g[name + "/lim"])
    tr._hip.ref_module = types.SimpleNamespace(
        sdf_util=types.SimpleNamespace(get_colormap=get_colormap), cv2=types.SimpleNamespace(resize=rec.resize),
        imgviz=types.SimpleNamespace(depth2rgb=rec.depth2rgb),
        metrics=types.SimpleNamespace(get_obj_eval_bounds=lambda f, up_ix: np.load(f)))
    return tr, rec


def _state(tr):
    e = tr.engine
    return [t.clone() for t in (e.params, e.exp_avg, e.exp_avg_sq)]


def _unchanged(tr, before):
    e = tr.engine
    for a, b in zip(before, (e.params, e.exp_avg, e.exp_avg_sq)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("case", ["A", "B"])
def test_bound_compute_slices_against_the_reference_slabs(g, sdf_map, case):
    """Every pixel of every slab against the reference's recorded one, through the decoded table index (tests/slice_model.
    index_distance).  With bin width w = (vmax - vmin) / N and the two values d apart, the indices floor(x) of x = (v - vmin) / w
    differ by at most floor(d / w) + 1: at most one wherever the values differ by less than a bin (1e-3 of a bin is added to d / w
    for the float32 rounding of x itself, N * 2^-23 of a bin).  No pixel is exempt."""
    from isdf_amd.hot_path import HotPath
    tr, rec = _trainer(g, case, sdf_map)
    assert type(tr).compute_slices is HotPath.compute_slices and type(tr).get_sdf_grid_pc is HotPath.get_sdf_grid_pc
    before = _state(tr)
    rng_list = [-2, 2]
    slices = tr.compute_slices(n_slices=3, include_gt=True, include_diff=True, include_chomp=True, sdf_range=rng_list)
    _unchanged(tr, before)
    assert rng_list == [-2.0, 2.0]
    assert sorted(slices) == ["diff", "gt_cost", "gt_sdf", "pred_cost", "pred_sdf"] and all(len(v) == 3 for v in slices.values())
    h, w = g[case + "/im_size"]
    assert all(im.shape == (h, w, 3) and im.dtype == np.uint8 for v in slices.values() for im in v)
    assert len(rec.resized) == 15 and all(s.shape == (sm.GRID_DIM, sm.GRID_DIM, 3) and s.dtype == np.uint8 for s in rec.resized)
    pred, gt, diff = np.stack(rec.resized[0:3]), np.stack(rec.resized[6:9]), np.stack(rec.resized[12:15])
    assert (diff == 255).all()
    # the points behind the slabs are the reference's (same selection, same reversal)
    up_ix = sm.CASES[case]["up_ix"]
    pts = torch.from_numpy(g[case + "/pts"]).cuda()
    sdf = np.moveaxis(tr.engine.sdf_eval(pts).cpu().numpy(), up_ix, 0)
    ref_sdf, ref_gt = np.moveaxis(g[case + "/sdf"], up_ix, 0), np.moveaxis(g[case + "/gt"], up_ix, 0)
    gt_val = tr.engine.slice_images(pts, None, None, tr._gt_volume(), None)[1].cpu().numpy().reshape(g[case + "/gt"].shape)
    gt_val = np.moveaxis(gt_val, up_ix, 0)
    rgb, lim = g["t2/rgb"], g["t2/lim"]
    width = (lim[1] - lim[0]) / (len(rgb) - 3)
    for what, got, ref_img, val, ref_val in (("pred_sdf", pred, g[case + "/pred_slabs"], sdf, ref_sdf),
                                             ("gt_sdf", gt, g[case + "/gt_slabs"], gt_val, ref_gt)):
        assert np.array_equal(got, sm.colours(val, rgb, lim[0], lim[1])), what               # the slabs ARE the colours of these values
        apart = np.abs(val.astype(np.float64) - ref_val)
        allowed = np.floor(apart / width + 1e-3) + 1
        dist = sm.index_distance(got, ref_img, rgb)
        print("%s %s: values differ by up to %.3e (bin width %.3e); %d of %d pixels one index apart, none further"
              % (case, what, apart.max(), width, (dist == 1).sum(), dist.size))
        assert np.all(dist <= allowed), (what, int((dist > allowed).sum()))
        assert apart.max() < width
    # the cost fields handed to imgviz: float32 / float64 as in the reference, the model's bits
    assert [c.dtype for c in rec.costs] == [np.float32, np.float64] and all(c.shape == (sm.GRID_DIM, 3 * sm.GRID_DIM) for c in rec.costs)
    flat = tr.engine.sdf_eval(pts).cpu().numpy().reshape(sm.GRID_DIM, -1)
    assert np.array_equal(rec.costs[0].view(np.uint32), sm.chomp32(flat, 2.0).view(np.uint32))
    with pytest.raises(UnboundLocalError):
        tr.compute_slices(n_slices=3, include_diff=True)
    _unchanged(tr, before)


def test_bound_obj_slices_vis(g, sdf_map, tmp_path):
    tr, rec = _trainer(g, "A", sdf_map)
    assert tr.obj_slices_vis() is None
    bounds = np.array([[[1.0, 1.9, 1.0], [2.0, 2.9, 2.0]], [[3.6, 2.0, 3.0], [4.8, 2.9, 4.2]]])
    tr.obj_bounds_file = str(tmp_path / "bounds.npy")
    np.save(tr.obj_bounds_file, bounds)
    before = _state(tr)
    img = tr.obj_slices_vis(n_slices=2)
    _unchanged(tr, before)
    assert img.shape == (2 * 2 * 256, 2 * 256, 3) and img.dtype == np.uint8
    # object 0, slice 1: the predicted image over the ground-truth one, against the models on the same points
    b = bounds[0]
    x, y, z = (torch.linspace(b[0, k], b[1, k], n) for k, n in ((0, 256), (1, 2), (2, 256)))
    pc = torch.stack(torch.meshgrid(x, y, z, indexing="ij"), dim=3).cuda()
    rgb, lim = g["t05/rgb"], g["t05/lim"]
    sdf = tr.engine.sdf_eval(pc).cpu().numpy()
    gt = tr.engine.slice_images(pc, None, None, tr._gt_volume(), None)[1].cpu().numpy().reshape(sdf.shape)
    assert np.array_equal(img[:256, 256:], sm.colours(sdf[:, 1], rgb, lim[0], lim[1]))
    assert np.array_equal(img[256:512, 256:], sm.colours(gt[:, 1], rgb, lim[0], lim[1]))
    _check_gt(g, pc.cpu().numpy(), gt, 0.0)


def test_bound_get_sdf_grid_pc_and_its_mask(g, sdf_map):
    tr, rec = _trainer(g, "A", sdf_map)
    d = sm.GRID_DIM
    rng = np.random.RandomState(4)
    pc = (np.array([3.0, 1.5, 2.5]) + rng.uniform(-1, 1, (5000, 3)) * np.array([2.6, 1.3, 2.1])).astype(np.float64)
    tr._vis_pointcloud = lambda: pc
    before = _state(tr)
    grid, mask = tr.get_sdf_grid_pc(include_gt=True, mask_near_pc=True)
    plain, none = tr.get_sdf_grid_pc()
    _unchanged(tr, before)
    assert grid.shape == (d, d, d, 5) and grid.dtype == np.float64
    assert plain.shape == (d, d, d, 4) and plain.dtype == np.float32 and none is None
    assert np.array_equal(grid[..., :4], plain.astype(np.float64))
    gp = sm.grid_pc().numpy().reshape(d, d, d, 3)
    assert np.array_equal(plain[..., :3], gp)
    assert np.array_equal(plain[..., 3], tr.engine.sdf_eval(tr.grid_pc).cpu().numpy().reshape(d, d, d))
    assert np.array_equal(grid[..., 4], grid[..., 4].astype(np.float32).astype(np.float64))          # float32 values, widened
    _check_gt(g, gp, grid[..., 4], 0.0)
    assert tr.gt_sdf_interp.bounds_error is True and tr.gt_sdf_interp.fill_value == 0.0
    # the mask: the float32 nearest-neighbour model on every tenth grid point, compared with crop_dist, repeated ten times
    sparse = gp[::10, ::10, ::10]
    d2, _ = em.nn_sq_dist32(sparse.reshape(-1, 3), pc.astype(np.float32))
    want = (np.sqrt(d2).astype(np.float64) < tr.crop_dist).reshape(sparse.shape[:-1])
    want = want.repeat(10, axis=0).repeat(10, axis=1).repeat(10, axis=2)
    assert mask.dtype == bool and mask.shape == want.shape == (50, 50, 50)
    assert np.array_equal(mask, want) and 0 < want.mean() < 1
