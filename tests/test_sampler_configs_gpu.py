"""`isdf_sample_rays` with SUPPLIED draws (rng_mode 0) against the host model of tests/sampler_model.py, over the sample
configurations, ray counts and windows the fixtures do not reach.  Needs a real MI355X: `pytest -m gpu`.

n_valid, indices_b/h/w, depth_sample, norm_sample and T_WC_sample are compared exactly; dirs_C, dirs_W, z_vals and pc against the
float64 values within the bound derived in sampler_model (rows at or beyond n_valid are not compared).  Cases: even and odd bin
counts, no surface sample, a surface sample without offsets, S above and below 64 and not dividing the 256-point group; 1, 37, 64 and
65 rays per frame; more than 4096 rays (the look-back instantiation, two launches on one workspace); non-monotone, repeating, 8-entry
inline and 9-entry device windows, normal_idx != frame_idx; inline windows byte-identical to the same window as device tensors.
The in-kernel Philox mode is not used here.

Measured on an MI355X (each test prints its figures): every case within the bounds; worst error / bound dirs_C 0.39, dirs_W 0.35,
z_vals 0.50, pc 0.25.  Against the float32 torch transcription on the CPU, dirs_C and z_vals are bit-equal in every case; dirs_W
and pc are NOT (dirs_W is only in four 1-ray cases): numpy's and torch's dirs_W agree with each other bit for bit, so the
difference is the kernel's -- its product-and-sum chains compile to fused multiply-adds (the toolchain's __fmul_rn / __fadd_rn are
plain `*` and `+`), one rounding fewer than the reference, within 1 ulp of it and inside the bounds above.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import sampler_model as sm

pytestmark = pytest.mark.gpu

K, H, W = 10, 24, 40
CAM = dict(H=H, W=W, fx=31.5, fy=29.25, cx=17.3, cy=12.6)
MIN_DEPTH, DIST = 0.5, 0.05          # with depths from 0.55 m and offsets of sigma 0.1 both clamps of the near-surface samples bind
CONFIGS = [(1, 0), (1, 1), (2, 1), (3, 2), (8, 8), (19, 8), (20, 8), (37, 27), (64, 1)]


@pytest.fixture(scope="module")
def world():
    from isdf_amd.engine import Engine, NetConfig
    depth, normal, T = sm.keyframes(K, H, W)
    dev = lambda a: torch.as_tensor(a).cuda()
    return dict(eng=Engine(NetConfig(), "cuda"), depth=depth, normal=normal, T=T, d=dev(depth), n=dev(normal), t=dev(T))


def _cfg(n_rays, n_strat, n_surf):
    from isdf_amd.engine import SampleConfig
    return SampleConfig(n_rays=n_rays, n_strat=n_strat, n_surf=n_surf, min_depth=MIN_DEPTH, dist_behind_surf=DIST, **CAM)


def _run(world, sc, frame_idx, normal_idx, draws, inline):
    if inline:
        fi, ni = tuple(int(v) for v in frame_idx), tuple(int(v) for v in normal_idx)
    else:
        fi = torch.tensor(list(frame_idx), dtype=torch.int32, device="cuda")
        ni = torch.tensor(list(normal_idx), dtype=torch.int32, device="cuda")
    s = world["eng"].sample(world["d"], world["t"], world["n"], fi, ni, sc, draws={k: torch.as_tensor(v).cuda() for k, v in draws.items()},
                            want_T=True)
    torch.cuda.synchronize()
    R = int(s["n_valid"].item())
    out = {k: s[k][:R].cpu().numpy() for k in sm.EXACT + sm.BOUNDED}
    out["n_valid"] = R
    return out


def _model(world, sc, frame_idx, normal_idx, draws):
    g = sm.gather(world["depth"], world["normal"], world["T"], frame_idx, normal_idx, draws, sc.n_rays)
    cfg = dict(n_strat=sc.n_strat, n_surf=sc.n_surf, min_depth=sc.min_depth, dist_behind_surf=sc.dist_behind_surf, **CAM)
    m = sm.model(g, draws, cfg)
    if g["n_valid"]:                       # a wrong bin is far outside the bound
        assert m["bin_length_min"] >= 100 * m["z_vals"][1].max()
    return g, m, cfg


def _report(label, out, g, m, cfg, draws):
    worst = sm.check(out, g, m, label)
    ref = sm.torch_f32(g, draws, cfg)
    bits = {k: bool(np.array_equal(out[k], ref[k])) for k in sm.BOUNDED}
    short = lambda k: k.replace("_sample", "").replace("_vals", "")
    print("%-34s R=%-5d worst error/bound %s   bit-equal to the torch transcription %s" %
          (label, g["n_valid"], " ".join("%s %.2f" % (short(k), v) for k, v in worst.items()),
           " ".join("%s %s" % (short(k), "yes" if v else "NO") for k, v in bits.items())))
    return worst


@pytest.mark.parametrize("n_strat,n_surf", CONFIGS)
def test_sample_configurations_against_the_model(world, n_strat, n_surf):
    lower = upper = by_depth = by_normal = 0
    for n_rays in (1, 37, 64, 65):
        sc = _cfg(n_rays, n_strat, n_surf)
        window = (2, 6, 8)                          # a zero-depth frame and two NaN-normal frames
        draws = sm.make_draws(np.random.RandomState(1000 * n_strat + 10 * n_surf + n_rays), 3, n_rays, n_strat, n_surf, H, W)
        g, m, cfg = _model(world, sc, window, window, draws)
        out = _run(world, sc, window, window, draws, inline=True)
        _report("n_strat %d n_surf %d n_rays %d" % (n_strat, n_surf, n_rays), out, g, m, cfg, draws)
        lower, upper = lower + m["lower_clamped"], upper + m["upper_clamped"]
        by_depth, by_normal = by_depth + g["dropped_by_depth"], by_normal + g["dropped_by_normal"]
    assert by_depth > 0 and by_normal > 0           # both validity tests bite
    if n_surf > 1:
        assert lower > 0 and upper > 0, (lower, upper)      # both clamps of the near-surface samples bind


def test_more_than_4096_rays_rearms_the_workspace_across_launches(world):
    """F * n_rays = 4200: the look-back instantiation (five 1024-ray chunks), twice on the same workspace with different draws"""
    sc = _cfg(1400, 19, 8)
    window = (7, 1, 4)
    for rep in range(2):
        draws = sm.make_draws(np.random.RandomState(77 + rep), 3, 1400, 19, 8, H, W)
        g, m, cfg = _model(world, sc, window, window, draws)
        out = _run(world, sc, window, window, draws, inline=bool(rep))
        _report("4200 rays, launch %d" % rep, out, g, m, cfg, draws)
        assert m["lower_clamped"] > 0 and m["upper_clamped"] > 0 and 0 < g["n_valid"] < 4200


WINDOWS = [("non-monotone", (3, 0, 2), (3, 0, 2)), ("repeated frame", (1, 1, 4), (1, 1, 4)),
           ("eight inline", (9, 3, 3, 0, 7, 5, 1, 8), (9, 3, 3, 0, 7, 5, 1, 8)),
           ("nine, device only", (8, 2, 5, 0, 9, 1, 7, 3, 6), (8, 2, 5, 0, 9, 1, 7, 3, 6)),
           ("normal_idx = arange(F)", (7, 2, 9), (0, 1, 2)),                # the reference's quirk q4: un-windowed normals
           ("normal_idx permuted", (4, 8, 0, 6), (6, 0, 8, 4))]


@pytest.mark.parametrize("name,frame_idx,normal_idx", WINDOWS, ids=[w[0].replace(" ", "_") for w in WINDOWS])
def test_windows_inline_and_as_device_arrays(world, name, frame_idx, normal_idx):
    F = len(frame_idx)
    for n_rays, (n_strat, n_surf) in ((65, (19, 8)), (37, (3, 2))):
        sc = _cfg(n_rays, n_strat, n_surf)
        draws = sm.make_draws(np.random.RandomState(31 * F + n_rays), F, n_rays, n_strat, n_surf, H, W)
        g, m, cfg = _model(world, sc, frame_idx, normal_idx, draws)
        dev = _run(world, sc, frame_idx, normal_idx, draws, inline=False)
        _report("%s, n_rays %d, device" % (name, n_rays), dev, g, m, cfg, draws)
        assert 0 < g["n_valid"] < F * n_rays
        if F <= 8:
            inl = _run(world, sc, frame_idx, normal_idx, draws, inline=True)
            sm.check(inl, g, m, name + " inline")
            for k in sm.EXACT + sm.BOUNDED:
                assert inl[k].tobytes() == dev[k].tobytes(), (name, k)
            assert inl["n_valid"] == dev["n_valid"]


def test_inline_windows_that_do_not_fit_raise(world):
    sc = _cfg(4, 3, 2)
    draws = {k: torch.as_tensor(v).cuda() for k, v in sm.make_draws(np.random.RandomState(0), 9, 4, 3, 2, H, W).items()}
    eng = world["eng"]
    with pytest.raises(ValueError):
        eng.sample(world["d"], world["t"], world["n"], tuple(range(9)), tuple(range(9)), sc, draws=draws)
    with pytest.raises(ValueError):
        eng.sample(world["d"], world["t"], world["n"], (0, 1, 2), (0, 1), sc, draws=draws)
    with pytest.raises(ValueError):
        eng.sample(world["d"], world["t"], world["n"], (0, 1, 2), None, sc, draws=draws)


def test_c_entry_point_rejects_bad_inline_windows(world):
    """n_inline = 9 and a negative inline index are ISDF_EINVAL from the C call, before anything is launched"""
    from isdf_amd import _ffi
    from isdf_amd.engine import _stream
    eng, F, n_rays, n_strat, n_surf = world["eng"], 3, 5, 3, 2
    R0, S = 9 * n_rays, n_strat + n_surf
    draws = {k: torch.as_tensor(v).cuda() for k, v in sm.make_draws(np.random.RandomState(1), 9, n_rays, n_strat, n_surf, H, W).items()}
    e = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device="cuda")
    bufs = dict(n_valid=e(1, dt=torch.int32), indices_b=e(R0, dt=torch.int64), indices_h=e(R0, dt=torch.int64), indices_w=e(R0, dt=torch.int64),
                depth_sample=e(R0), dirs_C_sample=e(R0, 3), norm_sample=e(R0, 3), T_WC_sample=e(R0, 4, 4), dirs_W_sample=e(R0, 3),
                z_vals=e(R0, S), pc=e(R0, S, 3))
    o = _ffi.SampleOut()
    for k, v in bufs.items():
        setattr(o, k, v.data_ptr())
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")

    def args(n_frames, n_inline, frame, normal):
        a = _ffi.SampleArgs()
        a.depth_batch, a.normal_batch, a.T_WC_batch = world["d"].data_ptr(), world["n"].data_ptr(), world["t"].data_ptr()
        a.n_frames, a.n_rays, a.H, a.W = n_frames, n_rays, H, W
        a.fx, a.fy, a.cx, a.cy = CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"]
        a.n_strat, a.n_surf, a.min_depth, a.dist_behind_surf, a.rng_mode = n_strat, n_surf, MIN_DEPTH, DIST, 0
        a.draw_h, a.draw_w = draws["indices_h"].data_ptr(), draws["indices_w"].data_ptr()
        a.draw_u, a.draw_n = draws["U"].data_ptr(), draws["N_off"].data_ptr()
        a.n_inline = n_inline
        a.frame_idx_inline[:len(frame)] = frame
        a.normal_idx_inline[:len(normal)] = normal
        return a

    call = lambda a: _ffi.lib().isdf_sample_rays(C.byref(a), C.byref(o), _ffi.ptr(ws), ws.numel(), _stream(eng.device))
    assert call(args(F, F, (3, 0, 2), (3, 0, 2))) == 0                         # the well-formed call goes through
    torch.cuda.synchronize()
    assert 0 < int(bufs["n_valid"].item()) <= F * n_rays
    assert call(args(9, 9, tuple(range(8)), tuple(range(8)))) == -1            # ISDF_EINVAL: more than ISDF_MAX_INLINE_FRAMES
    assert call(args(F, 2, (3, 0), (3, 0))) == -1                              # n_inline != n_frames
    assert call(args(F, F, (3, -1, 2), (3, 0, 2))) == -1                       # a negative frame index
    assert call(args(F, F, (3, 0, 2), (3, 0, -2))) == -1                       # a negative normal index
    torch.cuda.synchronize()
