"""The sampler's host model (tests/sampler_model.py) on any host: the float32 oracle (`oracle.isdf_oracle.get_batch_data` and
`sample_along_rays`, numpy) and the float32 torch transcription both lie within the model's bounds on the configurations
tests/test_sampler_configs_gpu.py runs, and a wrong bin, a wrong draw row or a wrong window frame does not.  That, and the derivation
in sampler_model's docstring, is what justifies the bounds; nothing is taken from the kernel's output."""
import numpy as np
import pytest

import oracle.isdf_oracle as orc
from tests import sampler_model as sm

K, H, W = 10, 24, 40
CAM = dict(fx=31.5, fy=29.25, cx=17.3, cy=12.6)
CONFIGS = [(1, 0), (1, 1), (2, 1), (3, 2), (8, 8), (19, 8), (20, 8), (37, 27), (64, 1)]


@pytest.fixture(scope="module")
def frames():
    return sm.keyframes(K, H, W)


def _oracle(frames, frame_idx, normal_idx, draws, cfg, n_rays):
    depth, normal, T = frames
    fi, ni = np.asarray(frame_idx), np.asarray(normal_idx)
    ib = orc.sample_pixels_indices_b(n_rays, len(fi))
    b = orc.get_batch_data(depth[fi], T[fi], orc.ray_dirs_C(H, W, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"]), ib, draws["indices_h"],
                           draws["indices_w"], normal[ni])
    R = b["depth_sample"].shape[0]
    max_depth = b["depth_sample"] + np.float32(cfg["dist_behind_surf"])
    pc, z = orc.sample_along_rays(b["T_WC_sample"], cfg["min_depth"], max_depth, cfg["n_strat"], cfg["n_surf"], b["dirs_C_sample"],
                                  b["depth_sample"], draws["U"][:R], draws["N_off"][:R])
    _, dW = orc.origin_dirs_W(b["T_WC_sample"], b["dirs_C_sample"])
    return dict(n_valid=R, indices_b=b["indices_b"], indices_h=b["indices_h"], indices_w=b["indices_w"], depth_sample=b["depth_sample"],
                norm_sample=b["norm_sample"], T_WC_sample=b["T_WC_sample"], dirs_C_sample=b["dirs_C_sample"], dirs_W_sample=dW, z_vals=z, pc=pc)


@pytest.mark.parametrize("n_strat,n_surf", CONFIGS)
def test_float32_references_lie_within_the_model_bounds(frames, n_strat, n_surf):
    cfg = dict(n_strat=n_strat, n_surf=n_surf, min_depth=0.5, dist_behind_surf=0.05, **CAM)
    for window, nidx in (((2, 6, 8), (2, 6, 8)), ((7, 2, 9), (0, 1, 2))):
        draws = sm.make_draws(np.random.RandomState(n_strat + n_surf), 3, 65, n_strat, n_surf, H, W)
        g = sm.gather(*frames, window, nidx, draws, 65)
        m = sm.model(g, draws, cfg)
        out = _oracle(frames, window, nidx, draws, cfg, 65)
        worst = sm.check(out, g, m, "oracle")
        t = dict(out, **sm.torch_f32(g, draws, cfg))
        worst_t = sm.check(t, g, m, "torch")
        print("n_strat %d n_surf %d window %s: R=%d worst error/bound oracle %s torch %s" % (n_strat, n_surf, window, g["n_valid"],
              {k: round(v, 2) for k, v in worst.items()}, {k: round(v, 2) for k, v in worst_t.items()}))
        assert 0 < g["n_valid"] < 195 and g["dropped_by_depth"] > 0
        # the un-windowed normals (quirk q4) come from frames 0..2, which have no NaN normal: only the windowed read drops any
        assert (g["dropped_by_normal"] > 0) == (nidx == window)


def test_defects_leave_the_bounds(frames):
    cfg = dict(n_strat=19, n_surf=8, min_depth=0.5, dist_behind_surf=0.05, **CAM)
    window = (3, 0, 2)
    draws = sm.make_draws(np.random.RandomState(4), 3, 65, 19, 8, H, W)
    g = sm.gather(*frames, window, window, draws, 65)
    m = sm.model(g, draws, cfg)
    good = _oracle(frames, window, window, draws, cfg, 65)
    sm.check(good, g, m)

    def fails(out):
        try:
            sm.check(out, g, m)
        except AssertionError:
            return True
        return False
    z = good["z_vals"].copy(); z[:, 8:] = np.roll(z[:, 8:], 1, axis=1)                       # a wrong bin
    assert fails(dict(good, z_vals=z))
    shifted = dict(draws, U=np.roll(draws["U"], 1, axis=0))                                 # U indexed by the wrong (e.g. drawn, not compacted) ray
    assert fails(_oracle(frames, window, window, shifted, cfg, 65))
    assert fails(_oracle(frames, (0, 2, 3), (0, 2, 3), draws, cfg, 65))                     # the window sorted
    assert fails(_oracle(frames, window, (0, 1, 2), draws, cfg, 65))                        # normals read un-windowed
    pc = good["pc"].copy(); pc[1:] = pc[:-1]                                                # points of the neighbouring ray
    assert fails(dict(good, pc=pc))
