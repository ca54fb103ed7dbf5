"""`isdf_render_views` (rendered views: render_depth_vis / render_normals_vis / latest_frame_vis) on the device.

References: the numpy oracle tests/render_oracle.py (pinned to the reference's own functions by tests/test_render_cpu.py) for
the samples, and a float64 PortNet on the device for the network's sdf and input gradient at the library's own points."""
import ctypes as C
from unittest import mock

import numpy as np
import pytest
import torch

from tests import golden_util as gu
from tests import render_oracle as ro
from tests.test_forward_only_gpu import Net

pytestmark = pytest.mark.gpu

HV, WV, HU, WU = 30, 40, 60, 80          # the 480 x 640 camera's vis rasters (trainer.py:349-359)


def _dirs(g, H, W):
    """the camera of fixture g scaled to an H-row raster of W columns"""
    H0, W0, fx, fy, cx, cy = (float(v) for v in g["cam"])
    f = H / H0
    return torch.from_numpy(ro_dirs(H, W, fx * f, fy * f, cx * f, cy * f)).cuda()


def ro_dirs(H, W, fx, fy, cx, cy):
    """transform.ray_dirs_C (transform.py:13-33, depth_type 'z') as [H*W, 3] float32"""
    c, r = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    return np.stack([(c - np.float32(cx)) / np.float32(fx), (r - np.float32(cy)) / np.float32(fy), np.ones_like(c)],
                    -1).reshape(-1, 3).astype(np.float32)


@pytest.fixture(scope="module", params=["trained_default", "trained_franka"])
def trained(request):
    g = gu.load(request.param)
    return g, Net.of_fixture(g)


def _poses(g, K):
    return torch.from_numpy(g["T_WC_batch"][:K].astype(np.float32)).cuda()


def _synth_depth(K, H=96, W=128):
    return torch.from_numpy(gu.synth_frames(np.random.RandomState(5), K, H, W, 100.0, 100.0, 64.0, 48.0)[0]).cuda()


def _render(net, source, T, U=None, want_normals=False, **kw):
    """one call of the given range source; -> (depth, normals, z, pc, args)"""
    g = kw.pop("g")
    K = T.shape[0]
    if source == "scalar":
        H, W, S, extra = HV, WV, 20, dict(scalar_range=(0.07, 6.0))
    elif source == "depth":
        H, W, S, extra = HV, WV, 19, dict(depth_images=kw.pop("images", None) if "images" in kw else _synth_depth(K),
                                          min_depth=0.07, depth_offset=0.8)
    else:
        coarse = kw.pop("coarse", None)
        if coarse is None:
            coarse = (2.0 + torch.rand(K, HV, WV, generator=torch.Generator().manual_seed(4))).cuda()
        H, W, S, extra = HU, WU, 12, dict(upsample=coarse, depth_offset=0.1)
    if U is None and "seed" not in kw:
        U = torch.rand(K, H * W, S, generator=torch.Generator().manual_seed(11)).cuda()
    d, n = net.eng.render_views(T, _dirs(g, H, W), H, W, S, draws=U, want_normals=want_normals, **extra, **kw)
    z, pc = net.eng._renderer.samples(K, H, W, S)
    return d, n, z.clone(), pc.clone(), (H, W, S, extra, U)


def _oracle_z(source, extra, U, H, W):
    U = U.cpu().numpy()
    out = []
    for b in range(U.shape[0]):
        if source == "scalar":
            out.append(ro.z_scalar(*extra["scalar_range"], U[b]))
        elif source == "depth":
            rs = ro.cv_resize_linear(extra["depth_images"][b].cpu().numpy(), W, H).reshape(-1)
            out.append(ro.z_ranged(np.float32(0.07), rs + np.float32(0.8), U[b]))
        else:
            up = ro.upsample_align_corners(extra["upsample"][b].cpu().numpy(), H, W).reshape(-1)
            out.append(ro.z_ranged(up - np.float32(0.1), up + np.float32(0.1), U[b]))
    return np.stack(out)


@pytest.mark.parametrize("source", ["scalar", "depth", "upsample"])
def test_samples_depth_and_normals_against_oracle_and_float64(trained, source):
    g, net = trained
    K = 3
    T = _poses(g, K)
    d, n, z, pc, (H, W, S, extra, U) = _render(net, source, T, want_normals=True, g=g)
    zo = _oracle_z(source, extra, U, H, W)
    np.testing.assert_allclose(z.cpu().numpy(), zo, rtol=0, atol=1e-6)
    dC = _dirs(g, H, W).cpu().numpy()
    pco = np.stack([ro.points(T[b].cpu().numpy(), dC, zo[b]) for b in range(K)])
    np.testing.assert_allclose(pc.cpu().numpy(), pco, rtol=0, atol=4e-6)
    if source == "upsample":       # u = 0 puts sample 0 on the range's lower end: the upsample itself, to 1e-6
        _, _, z0, _, _ = _render(net, source, T, U=torch.zeros_like(U), coarse=extra["upsample"], g=g)
        up = np.stack([ro.upsample_align_corners(extra["upsample"][b].cpu().numpy(), H, W).reshape(-1) for b in range(K)])
        np.testing.assert_allclose(z0[..., 0].cpu().numpy() + 0.1, up, rtol=0, atol=1e-6)
    # first crossing against the float64 network on the same points
    sdf64 = net.ref(pc.reshape(-1, 3)).reshape(K * H * W, S).float().cpu().numpy()
    zz = z.reshape(K * H * W, S).cpu().numpy()
    c64, _ = ro.first_crossing(zz, sdf64)
    d64 = ro.render_depth(zz, sdf64)
    sdf_h = net.eng.sdf_eval(pc.reshape(-1, 3)).reshape(K * H * W, S).cpu().numpy()
    ch, _ = ro.first_crossing(zz, sdf_h)
    same = ch == c64
    assert same.mean() >= 0.995, same.mean()
    assert np.abs(d.reshape(-1).cpu().numpy() - d64)[same].max() <= 1e-3
    # normals at the rendered depth against the float64 formula
    x = torch.stack([torch.from_numpy(ro.points(T[b].cpu().numpy(), dC, d[b].cpu().numpy())) for b in range(K)]).reshape(-1, 3)
    _, g64 = net.ref(x, want_grad=True)
    g64 = g64.reshape(K, H * W, 3)
    Rinv = torch.linalg.inv(T[:, :3, :3].double())
    nW = -g64 / (g64.norm(dim=-1, keepdim=True) + 1e-4)
    n64 = torch.einsum("bij,brj->bri", Rinv, nW)
    assert gu.rel_err(n.double().cpu(), n64.cpu()) <= 2e-3


def test_pipeline_depth_is_render_depth_of_its_own_samples_bit_for_bit(trained):
    g, net = trained
    T = _poses(g, 4)
    for source in ("scalar", "depth", "upsample"):
        d, _, z, pc, (H, W, S, _, _) = _render(net, source, T, g=g)
        sdf = net.eng.sdf_eval(pc.reshape(-1, 3)).reshape(-1, S)
        want, _ = net.eng.render_depth(z.reshape(-1, S), sdf)
        assert torch.equal(d.reshape(-1), want), source


def test_k_views_in_one_call_equal_k_one_view_calls(trained):
    g, net = trained
    K = 5
    T = _poses(g, K)
    images = _synth_depth(K)
    U = torch.rand(K, HV * WV, 19, generator=torch.Generator().manual_seed(2)).cuda()
    d, n, _, _, _ = _render(net, "depth", T, U=U, images=images, want_normals=True, g=g)
    for b in range(K):
        d1, n1, _, _, _ = _render(net, "depth", T[b:b + 1], U=U[b:b + 1], images=images[b:b + 1], want_normals=True, g=g)
        assert torch.equal(d[b], d1[0]) and torch.equal(n[b], n1[0]), b
    n_given = net.eng.render_views(T, _dirs(g, HV, WV), HV, WV, depth=d)[1]
    assert torch.equal(n_given, n)                              # the normals of a render = the normals at its depth


def test_philox_is_deterministic_per_seed_and_counter(trained):
    g, net = trained
    T = _poses(g, 2)
    a = _render(net, "depth", T, U=None, seed=9, counter=1, g=g)[2]
    b = _render(net, "depth", T, U=None, seed=9, counter=1, g=g)[2]
    c = _render(net, "depth", T, U=None, seed=9, counter=2, g=g)[2]
    e = _render(net, "depth", T, U=None, seed=10, counter=1, g=g)[2]
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, e)
    # the uniforms it implies lie in [0, 1): z stays inside its bins
    assert bool(torch.isfinite(a).all())


def _abi_call(net, args, depth, normals):
    eng = net.eng
    lib = eng.lib
    nb = lib.isdf_render_ws_bytes(C.byref(eng.cnet), max(args.n_views, 1), args.H, args.W, max(args.n_samples, 1))
    ws = torch.empty(int(nb), dtype=torch.uint8, device="cuda")
    from isdf_amd import _ffi
    from isdf_amd.engine import _stream
    rc = lib.isdf_render_views(C.byref(eng.cnet), _ffi.ptr(eng.params), _ffi.ptr(eng.shadow), C.byref(args), _ffi.ptr(depth),
                               _ffi.ptr(normals), _ffi.ptr(ws), ws.numel(), _stream(torch.device("cuda")))
    torch.cuda.synchronize()
    return rc


def test_c_abi_stores_nothing_past_the_outputs_and_zero_views_is_a_no_op(trained):
    from isdf_amd import _ffi
    g, net = trained
    K, H, W, S = 2, 7, 9, 5
    T, dC = _poses(g, K), _dirs(g, HV, WV)[:H * W].contiguous()
    U = torch.rand(K, H * W, S, device="cuda")
    keep = [T, dC, U]
    a = _ffi.RenderArgs()
    a.n_views, a.H, a.W, a.n_samples, a.T_WC, a.dirs_C = K, H, W, S, T.data_ptr(), dC.data_ptr()
    a.range_mode, a.min_depth, a.max_depth, a.bin_length = _ffi.RANGE_SCALAR, 0.07, 6.0, (6.0 - 0.07) / S
    a.rng_mode, a.draw_u = 0, U.data_ptr()
    canary = 1234.5
    depth = torch.full((K * H * W + 333,), canary, device="cuda")
    normals = torch.full((K * H * W * 3 + 333,), canary, device="cuda")
    assert _abi_call(net, a, depth, normals) == 0
    assert bool((depth[K * H * W:] == canary).all()) and bool((normals[K * H * W * 3:] == canary).all())
    assert bool((depth[:K * H * W] != canary).all())
    a.n_views = 0
    d0, n0 = torch.full_like(depth, canary), torch.full_like(normals, canary)
    assert _abi_call(net, a, d0, n0) == 0
    assert bool((d0 == canary).all()) and bool((n0 == canary).all())
    a.n_views = K
    assert _abi_call(net, a, None, None) == -1                  # no output
    a.rng_mode, a.draw_u = 0, None
    assert _abi_call(net, a, depth, None) == -1                 # injected mode without draws
    del keep


# ---- every instantiated network shape: forward (pair kernel or chain MODE 0) and input gradient (chain MODE 1) ------------------
SHAPES = [("default", "eval_full_ray", "fp16x2"), ("b1_256", "eval_b1_256", "fp16x2"), ("rs_franka", "eval_rs_franka", "fp16x2"),
          ("wide_512", "eval_wide_512", "fp16x2"), ("default-fp16", "eval_full_ray", "fp16"),
          ("default-bf16", "eval_full_ray", "bf16")]


@pytest.mark.parametrize("cid,src,oper", SHAPES, ids=[s[0] for s in SHAPES])
def test_every_net_shape_against_float64(cid, src, oper):
    g = gu.load(src)
    net = Net.of_fixture(g, oper)
    gt = gu.load("trained_default")
    T = _poses(gt, 2)
    d, n, z, pc, (H, W, S, _, _) = _render(net, "depth", T, want_normals=True, g=gt)
    sdf64 = net.ref(pc.reshape(-1, 3)).reshape(-1, S).float().cpu().numpy()
    zz = z.reshape(-1, S).cpu().numpy()
    sdf_h = net.eng.sdf_eval(pc.reshape(-1, 3)).reshape(-1, S).cpu().numpy()
    same = ro.first_crossing(zz, sdf_h)[0] == ro.first_crossing(zz, sdf64)[0]
    # bf16 operands sit on their ~1e-2 floor: near-zero samples of an untrained net flip sign more often
    assert same.mean() >= (0.9 if oper == "bf16" else 0.98), same.mean()
    scale = max(float(np.abs(sdf64).max()), 1e-6)
    tol = 3e-2 if oper == "bf16" else 5e-3
    assert np.abs(d.reshape(-1).cpu().numpy() - ro.render_depth(zz, sdf64))[same].max() <= tol * scale
    dC = _dirs(gt, H, W).cpu().numpy()
    x = torch.stack([torch.from_numpy(ro.points(T[b].cpu().numpy(), dC, d[b].cpu().numpy())) for b in range(2)]).reshape(-1, 3)
    _, g64 = net.ref(x, want_grad=True)
    g64 = g64.reshape(2, H * W, 3)
    nW = -g64 / (g64.norm(dim=-1, keepdim=True) + 1e-4)
    n64 = torch.einsum("bij,brj->bri", torch.linalg.inv(T[:, :3, :3].double()), nW)
    assert gu.rel_err(n.double().cpu(), n64.cpu()) <= (5e-2 if oper == "bf16" else 1e-2)


# ---- the bound methods on hardware ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 20])
def test_bound_methods_on_the_standin_trainer(K):
    from bench_support.standin_trainer import HipTrainer, FrameData
    from isdf_amd import synthetic
    from tests.accuracy_experiment import config
    cam = dict(H=120, W=160, fx=150.0, fy=150.0, cx=79.5, cy=59.5)
    tr = HipTrainer("cuda:0", config(cam), inv_bounds_transform=synthetic.bounds_transform(), rng="philox", seed=3)
    depth, normal, T = synthetic.keyframes(K, cam, seed=3, stride=7)
    dev = tr.device
    tr.frames = FrameData(frame_id=np.arange(K), depth_batch=torch.from_numpy(depth).to(dev), T_WC_batch=torch.from_numpy(T).to(dev),
                          normal_batch=torch.from_numpy(normal).to(dev), frame_avg_losses=torch.zeros(K, device=dev))
    tr.H_vis, tr.W_vis = cam["H"] // 16, cam["W"] // 16
    tr.dirs_C_vis = torch.from_numpy(ro_dirs(tr.H_vis, tr.W_vis, 150.0 / 16, 150.0 / 16, 79.5 / 16, 59.5 / 16)).to(dev)[None]
    tr.n_strat_samples, tr.min_depth = 19, 0.07
    eng = tr.engine
    with mock.patch.object(eng.lib, "isdf_render_views", wraps=eng.lib.isdf_render_views) as spy:
        d = tr.render_depth_vis()
        assert spy.call_count == 1                              # all K views in one native call
        n = tr.render_normals_vis(d)
        assert spy.call_count == 2
    assert d.shape == (K, tr.H_vis, tr.W_vis) and d.device.type == "cuda" and d.dtype == torch.float32
    assert n.shape == (K, tr.H_vis, tr.W_vis, 3) and bool(torch.isfinite(n).all())
