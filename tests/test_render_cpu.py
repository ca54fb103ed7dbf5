"""Rendered views on the host: the numpy oracle (tests/render_oracle.py) against the REAL reference functions, and the three
graft() bindings (render_depth_vis, render_normals_vis, latest_frame_vis) on the REAL reference Trainer with an oracle-backed
engine, against an ungrafted twin.  cv2 and imgviz are not installed here: the reference's calls to them are answered by the
oracle's restatement of OpenCV's INTER_LINEAR mapping and a trivial depth2rgb (agreement with real cv2 is unverified)."""
import contextlib
import io
import os
import sys
import types
from unittest import mock

import numpy as np
import pytest
import torch

import oracle.isdf_oracle as orc
from tests import golden_util as gu
from tests import render_oracle as ro
from tests.fake_engine import FakeEngine

REF = os.environ.get("ISDF_REFERENCE", "/root/reference")
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "isdf")), reason="reference checkout not present")


# ---- the oracle-backed engine ---------------------------------------------------------------------------------------------
class RenderFakeEngine(FakeEngine):
    """FakeEngine plus render_views through the numpy oracle (the Engine.render_views surface)"""

    def render_views(self, T_WC, dirs_C, H, W, n_samples=0, scalar_range=None, depth_images=None, min_depth=0.0, upsample=None,
                     depth_offset=0.0, draws=None, seed=0, counter=0, depth=None, want_depth=True, want_normals=False):
        self.calls.append("render_views")
        T = T_WC.detach().cpu().numpy().astype(np.float32).reshape(-1, 4, 4)
        B, R = T.shape[0], H * W
        dC = dirs_C.detach().cpu().numpy().astype(np.float32).reshape(R, 3)
        depths, normals = [], []
        for b in range(B):
            if depth is not None:
                d = depth.detach().cpu().numpy().reshape(B, R)[b].astype(np.float32)
                want_depth, want_normals = False, True
            else:
                S = n_samples
                U = (draws.detach().cpu().numpy().reshape(B, R, S)[b] if draws is not None
                     else np.random.RandomState([seed & 0xffffffff, counter, b]).uniform(size=(R, S)).astype(np.float32))
                if scalar_range is not None:
                    z = ro.z_scalar(scalar_range[0], scalar_range[1], U)
                elif depth_images is not None:
                    img = depth_images[b].detach().cpu().numpy()
                    z = ro.z_ranged(min_depth, (ro.cv_resize_linear(img, W, H).reshape(-1) + np.float32(depth_offset)), U)
                else:
                    up = ro.upsample_align_corners(upsample[b].detach().cpu().numpy(), H, W).reshape(-1)
                    z = ro.z_ranged(up - np.float32(depth_offset), up + np.float32(depth_offset), U)
                pc = ro.points(T[b], dC, z)
                sdf = orc.sdf_forward(self._np_params(), self._cfg(), pc.reshape(-1, 3)).astype(np.float32).reshape(R, S)
                d = ro.render_depth(z, sdf)
            depths.append(d)
            if want_normals:
                _, g = orc.sdf_forward_grad(self._np_params(), self._cfg(), ro.points(T[b], dC, d))
                normals.append(ro.normals_C(T[b], g.astype(np.float32)))
        return (torch.from_numpy(np.stack(depths)) if want_depth else None,
                torch.from_numpy(np.stack(normals)) if want_normals else None)


# ---- reference set-up -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref_mods():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden as mg
    with contextlib.redirect_stdout(io.StringIO()):
        mods = mg.import_reference()
    return mg, mods


def _depth2rgb(depth, min_value=None, max_value=None):
    """trivial stand-in for imgviz.depth2rgb: a grey ramp, uint8 [H, W, 3]"""
    d = np.asarray(depth, np.float64)
    lo = np.nanmin(d) if min_value is None else min_value
    hi = np.nanmax(d) if max_value is None else max_value
    v = np.clip((d - lo) / max(hi - lo, 1e-9), 0, 1)
    return np.repeat((v * 255).astype(np.uint8)[..., None], 3, -1)


def _cv2_resize(img, dsize):
    img = np.asarray(img)
    W, H = dsize
    if img.ndim == 2:
        return ro.cv_resize_linear(img.astype(np.float32), W, H).astype(img.dtype)
    return np.stack([ro.cv_resize_linear(img[..., c].astype(np.float32), W, H) for c in range(img.shape[-1])],
                    -1).astype(img.dtype)


STANDINS = dict(cv2=types.SimpleNamespace(resize=_cv2_resize), imgviz=types.SimpleNamespace(depth2rgb=_depth2rgb))

G = "trained_default"
K = 3                      # keyframes
HV, WV, HU, WU = 12, 16, 24, 32


def _trainer(mg, mods, grafted, rng="torch"):
    from isdf_amd.hot_path import graft
    g = gu.load(G)
    cam = gu.cam_of(g)
    H, W = 96, 128                                              # keyframe raster (the vis rasters are 1/8 and 1/4 of it)
    fx, fy, cx, cy = cam["fx"] * W / cam["W"], cam["fy"] * H / cam["H"], cam["cx"] * W / cam["W"], cam["cy"] * H / cam["H"]
    depth, normal, _ = gu.synth_frames(np.random.RandomState(5), K, H, W, fx, fy, cx, cy)
    T = g["T_WC_batch"][:K].astype(np.float32)
    net = g["net"]
    netd = dict(H=int(net[0]), B=int(net[1]), n_freqs=int(net[2]), scale_input=float(net[3]), scale_output=float(net[4]))
    lossd = dict(mg.LOSS_DEFAULT)
    with contextlib.redirect_stdout(io.StringIO()):
        tr = mg.build_trainer(mods, dict(H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy), netd, lossd, mg.SAMPLE_DEFAULT,
                              (depth, normal, T), gu.params_of(g), g["bounds_T"], 0.0)
    transform = mods[5]
    tr.min_depth, tr.max_depth, tr.live = 0.07, 6.0, False
    tr.H_vis, tr.W_vis, tr.H_vis_up, tr.W_vis_up = HV, WV, HU, WU
    tr.dirs_C_vis = transform.ray_dirs_C(1, HV, WV, fx * HV / H, fy * HV / H, cx * HV / H, cy * HV / H, "cpu").view(1, -1, 3)
    tr.dirs_C_vis_up = transform.ray_dirs_C(1, HU, WU, fx * HU / H, fy * HU / H, cx * HU / H, cy * HU / H, "cpu").view(1, -1, 3)
    fr = tr.frames
    fr.depth_batch_np, fr.T_WC_batch_np = depth.copy(), T.copy()
    fr.im_batch_np = (np.random.RandomState(6).uniform(size=(K, H, W, 3)) * 255).astype(np.uint8)
    tr.gt_depth_vis = np.stack([ro.cv_resize_linear(d, WV, HV) for d in depth])
    tr.gt_im_vis = None
    if grafted:
        with contextlib.redirect_stdout(io.StringIO()):
            graft(tr, rng=rng, engine_factory=RenderFakeEngine)
    return tr


@pytest.fixture()
def standins(ref_mods):
    tmod = ref_mods[1][0]
    with mock.patch.object(tmod, "cv2", STANDINS["cv2"]), mock.patch.object(tmod, "imgviz", STANDINS["imgviz"]):
        yield


# ---- 1. the oracle against the reference's functions ----------------------------------------------------------------------
def _ref_net(mods, g):
    net = g["net"]
    pe = mods[2].PostionalEncoding(min_deg=0, max_deg=int(net[2]) - 1, scale=float(net[3]),
                                   transform=torch.from_numpy(g["bounds_T"].astype(np.float32)))
    m = mods[3].SDFMap(pe, hidden_size=int(net[0]), hidden_layers_block=int(net[1]), scale_output=float(net[4]))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in gu.params_of(g).items()})
    return m


def _crossing_agreement(z, sdf_ref, d_ref, d_orc):
    """fraction of rays on which the reference's crossing sample (stored order) is the oracle's (z order), and the max depth
    difference on those rays"""
    n = sdf_ref.shape[1]
    inside = sdf_ref < 0
    mx = np.argmax(inside * np.arange(n, 0, -1), 1)
    c, _ = ro.first_crossing(z, sdf_ref)
    same = mx == c
    return same.mean(), float(np.abs(d_ref - d_orc)[same].max(initial=0.0))


@needs_ref
@pytest.mark.parametrize("source", ["scalar", "depth", "upsample"])
def test_oracle_matches_the_reference_functions(ref_mods, source):
    mg, mods = ref_mods
    sample, render = mods[1], mods[0].render
    g = gu.load(G)
    sdf_map = _ref_net(mods, g)
    transform = mods[5]
    T = torch.from_numpy(g["T_WC_batch"][1:2].astype(np.float32))
    cam = gu.cam_of(g)
    H, W = (HV, WV) if source != "upsample" else (HU, WU)
    f = H / cam["H"]
    dC = transform.ray_dirs_C(1, H, W, cam["fx"] * f, cam["fy"] * f, cam["cx"] * f, cam["cy"] * f, "cpu").view(1, -1, 3)
    R = H * W
    if source == "scalar":
        S, args = 20, (0.07, 6.0)
    elif source == "depth":
        img = gu.synth_frames(np.random.RandomState(3), 1, 96, 128, 100.0, 100.0, 64.0, 48.0)[0][0]
        rs = ro.cv_resize_linear(img, W, H)
        S, args = 19, (0.07, (torch.from_numpy(rs) + 0.8).flatten())
    else:
        coarse = (2.0 + np.random.RandomState(4).uniform(size=(HV, WV))).astype(np.float32)
        up_ref = torch.nn.functional.interpolate(torch.from_numpy(coarse).view(1, 1, HV, WV), size=[HU, WU], mode="bilinear",
                                                 align_corners=True).view(-1)
        up = ro.upsample_align_corners(coarse, HU, WU).reshape(-1)
        np.testing.assert_allclose(up, up_ref.numpy(), rtol=0, atol=1e-6)
        S, args = 12, (up_ref - 0.1, up_ref + 0.1)
    torch.manual_seed(11)
    with torch.no_grad():
        pc_r, z_r = sample.sample_along_rays(T, args[0], args[1], S, 0, dC if source != "depth" else dC[0])
    torch.manual_seed(11)
    U = torch.rand(R, S).numpy()
    if source == "scalar":
        z = ro.z_scalar(args[0], args[1], U)
    elif source == "depth":
        z = ro.z_ranged(args[0], args[1].numpy(), U)
    else:
        z = ro.z_ranged(up - np.float32(0.1), up + np.float32(0.1), U)
    pc = ro.points(T[0].numpy(), dC.numpy(), z)
    np.testing.assert_allclose(z, z_r.numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(pc, pc_r.reshape(R, S, 3).numpy(), rtol=0, atol=4e-6)
    with torch.no_grad():
        sdf_r = sdf_map(pc_r)
        d_r = render.sdf_render_depth(z_r, sdf_r)
    d = ro.render_depth(z, sdf_r.numpy())
    frac, err = _crossing_agreement(z, sdf_r.numpy(), d_r.numpy(), d)
    assert frac >= 0.995 and err <= 1e-5, (frac, err)
    n_r = render.render_normals(T, d_r.view(H, W), sdf_map, dC[0]).detach().reshape(R, 3).numpy()
    x = ro.points(T[0].numpy(), dC.numpy(), d_r.numpy())
    xt = torch.from_numpy(x).requires_grad_()
    g_r = mods[3].gradient(xt, sdf_map(xt)).detach().numpy()
    np.testing.assert_allclose(ro.normals_C(T[0].numpy(), g_r), n_r, rtol=0, atol=1e-4)


def test_cv_resize_restatement_on_an_exact_ramp():
    """the INTER_LINEAR mapping reproduces a linear ramp away from the clamped borders and halves exactly on 2x"""
    img = np.add.outer(np.arange(8, dtype=np.float32), 10 * np.arange(12, dtype=np.float32))
    out = ro.cv_resize_linear(img, 6, 4)
    np.testing.assert_allclose(out, np.add.outer(2 * np.arange(4) + 0.5, 10 * (2 * np.arange(6) + 0.5)), atol=1e-5)


# ---- 2. the bound methods on the reference Trainer ---------------------------------------------------------------------------
@needs_ref
def test_bound_methods_resolve_to_the_hip_binding(ref_mods):
    from isdf_amd.hot_path import HotPath
    mg, mods = ref_mods
    tr = _trainer(mg, mods, True)
    for m in ("render_depth_vis", "render_normals_vis", "latest_frame_vis"):
        assert getattr(type(tr), m) is getattr(HotPath, m), m
    assert type(tr).frames_vis is mods[0].Trainer.frames_vis


def _same_crossing_depth(got, want):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    close = np.abs(got - want) <= 1e-5
    assert close.mean() >= 0.995, close.mean()
    return close


@needs_ref
def test_render_depth_and_normals_vis_match_the_reference(ref_mods, standins):
    mg, mods = ref_mods
    hip, ref = _trainer(mg, mods, True), _trainer(mg, mods, False)
    torch.manual_seed(21)
    with mock.patch.object(hip.sdf_map.engine, "render_views", wraps=hip.sdf_map.engine.render_views) as spy:
        d = hip.render_depth_vis()
    st_hip = torch.get_rng_state()
    assert spy.call_count == 1
    torch.manual_seed(21)
    d_ref = ref.render_depth_vis()
    assert torch.equal(torch.get_rng_state(), st_hip)
    assert d.shape == d_ref.shape == (K, HV, WV) and d.dtype == d_ref.dtype and d.device == d_ref.device
    _same_crossing_depth(d.numpy(), d_ref.numpy())
    n = hip.render_normals_vis(d_ref)
    n_ref = ref.render_normals_vis(d_ref).detach()
    assert n.shape == n_ref.shape == (K, HV, WV, 3) and n.dtype == n_ref.dtype
    np.testing.assert_allclose(n.numpy(), n_ref.numpy(), rtol=0, atol=1e-4)


@needs_ref
def test_render_depth_vis_uses_the_tracked_poses_when_present(ref_mods, standins):
    mg, mods = ref_mods
    hip, ref = _trainer(mg, mods, True), _trainer(mg, mods, False)
    track = hip.frames.T_WC_batch.clone()
    track[:, :3, 3] += 0.05
    hip.frames.T_WC_track = [t for t in track]                 # truthy: a list of tracked poses
    ref.frames.T_WC_track = [t.clone() for t in track]
    torch.manual_seed(3)
    d = hip.render_depth_vis()
    torch.manual_seed(3)
    d_ref = ref.render_depth_vis()
    _same_crossing_depth(d.numpy(), d_ref.numpy())


@needs_ref
def test_latest_frame_vis_matches_the_reference(ref_mods, standins):
    mg, mods = ref_mods
    hip, ref = _trainer(mg, mods, True), _trainer(mg, mods, False)
    torch.manual_seed(8)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rgbd, vis, T = hip.latest_frame_vis()
    st_hip = torch.get_rng_state()
    assert "Time for depth and normal render" in out.getvalue()
    torch.manual_seed(8)
    with contextlib.redirect_stdout(io.StringIO()):
        rgbd_r, vis_r, T_r = ref.latest_frame_vis()
    assert torch.equal(torch.get_rng_state(), st_hip)
    assert np.array_equal(rgbd, rgbd_r) and np.array_equal(T, T_r)
    assert vis.shape == vis_r.shape and vis.dtype == vis_r.dtype
    # normals image: uint8 of values within 1e-4 -> at most one step; the depth half agrees on >= 99.5 % of the pixels
    diff = np.abs(vis.astype(np.int32) - vis_r.astype(np.int32))
    half = vis.shape[1] // 2
    assert diff[:, :half].max() <= 1
    assert (diff[:, half:] <= 1).mean() >= 0.995
    with contextlib.redirect_stdout(io.StringIO()):
        r2 = hip.latest_frame_vis(do_render=False)
    assert r2[1] is None and np.array_equal(r2[0], rgbd)


@needs_ref
def test_philox_leaves_the_torch_generator_alone_and_frames_vis_runs(ref_mods, standins):
    mg, mods = ref_mods
    hip = _trainer(mg, mods, True, rng="philox")
    torch.manual_seed(2)
    st = torch.get_rng_state()
    d = hip.render_depth_vis()
    with contextlib.redirect_stdout(io.StringIO()):
        hip.latest_frame_vis()
    assert torch.equal(torch.get_rng_state(), st)
    assert d.shape == (K, HV, WV) and hip._hip.render_count == 3
    viz = hip.frames_vis()
    assert viz.shape == (4 * HV, K * WV, 3) and viz.dtype == np.uint8
