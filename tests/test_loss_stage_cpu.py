"""tests/loss_model.py and tests/loss_cases.py against the oracle alone (no GPU): the model the GPU file holds the loss stage to is
the oracle's loss on the committed fixtures, its bounds_pc is the oracle's, and every hand-made batch is what its case table says."""
import functools
import os

import numpy as np
import pytest

import oracle.isdf_oracle as orc
from tests import golden_util as gu
from tests import loss_cases as lcs
from tests import loss_model as lm
from tests import tail_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_CAP = 0.005


@functools.lru_cache(maxsize=None)
def _fixture(name):
    """(g, batch, net cfg, oracle sdf fp32 [R,S], oracle d sdf/dx fp32 [R,S,3]): one float64 forward per fixture, shared, read-only"""
    g, b = lcs.fixture_batch(name)
    cfg = gu.net_of(g, np.float64)
    params = {k: v.astype(np.float64) for k, v in gu.params_of(g).items()}
    R, S = b["z_vals"].shape
    sdf, grad = orc.sdf_forward_grad(params, cfg, b["pc"].reshape(-1, 3).astype(np.float64), noise=b["noise"].reshape(-1).astype(np.float64))
    sdf, grad = sdf.reshape(R, S).astype(np.float32), grad.reshape(R, S, 3).astype(np.float32)
    for a in (sdf, grad):
        a.setflags(write=False)
    return g, b, cfg, sdf, grad


def _model(b, lc, cfg, sdf, grad):
    R, S = b["z_vals"].shape
    if lc.bounds_method == "ray":
        bnd, band, near, tgt = lm.ray_inputs(b, lc)
    else:
        bnd, gv, _ = lm.bounds_pc_f32(b["pc"], b["z_vals"], b["depth_sample"])
        band, near, tgt = None, np.zeros((R, S), bool), gv
    return lm.point_terms(sdf, grad, bnd, tgt, b["norm_sample"], lm.sample_index(R, S), lc, cfg, band), bnd, near


@pytest.mark.parametrize("config", sorted(lcs.CONFIGS))
@pytest.mark.parametrize("fix", lcs.FIXTURES)
def test_model_is_the_oracle_on_the_fixtures(fix, config):
    """per point and on the kernel's scale: point_terms, with the bounds and targets assembled the kernel's way (fp32 bound,
    -dirs_W or pc_grad_vec, the normal at sample 0 and at NaN targets), against the oracle run its own way in float64"""
    g, b, cfg, sdf, grad = _fixture(fix)
    lc = lcs.loss_cfg(gu.loss_of(g), **lcs.CONFIGS[config])
    m, bnd, near = _model(b, lc, cfg, sdf, grad)
    d = lambda k: b[k].astype(np.float64)
    if lc.bounds_method == "ray":
        bo, gv = orc.bounds_ray(d("depth_sample"), d("z_vals"), d("dirs_C_sample"), d("T_WC_sample"))
    else:
        bo, gv = orc.bounds_pc(d("pc"), d("z_vals"), d("depth_sample"))
    N = sdf.size
    args = (sdf.astype(np.float64), grad.astype(np.float64), bo, gv, d("norm_sample"), lm.lc32(lc))
    t = orc.loss_terms(*args)
    sb, gb = orc.loss_adjoints(*args)
    ok = ~m["flag"] & ~near
    assert np.mean(~ok) <= FLAG_CAP
    # (the model's bound is the fp32 value of the oracle's: 2^-24 |bnd| through trunc_weight, and through exp's argument nowhere)
    for k, ref in (("sl", t["sdf_loss_mat"]), ("gl", t["grad_loss_mat"]), ("ek", t["eik_loss_mat"]), ("tot", t["tot_loss_mat"]), ("sbar", sb * N)):
        np.testing.assert_allclose(m[k][ok], ref[ok], rtol=1e-6, atol=2e-6, err_msg=k)
    # (pc: the model's target is the unit vector of the fp32 difference p - surf, the oracle's of the float64 one)
    np.testing.assert_allclose(m["gbar"][ok], (gb * N)[ok], rtol=1e-6, atol=1e-6 * np.abs(gb * N).max())
    if fix == "eval_full_ray" and config == "ray_L1":      # the fixture's own configuration: the reference's recorded means
        for k, mk in (("sdf_loss", "sl"), ("grad_loss", "gl"), ("eikonal_loss", "ek"), ("total_loss", "tot")):
            assert abs(m[mk].mean() - float(g[k][0])) <= 2e-3 * abs(float(g[k][0])), k   # (the reference's fp32 forward vs float64)


@pytest.mark.parametrize("config", sorted(lcs.CONFIGS))
@pytest.mark.parametrize("fix", lcs.FIXTURES)
def test_flagged_share_of_the_fixtures_is_under_the_cap(fix, config):
    g, b, cfg, sdf, grad = _fixture(fix)
    lc = lcs.loss_cfg(gu.loss_of(g), **lcs.CONFIGS[config])
    m, _, near = _model(b, lc, cfg, sdf, grad)
    share = float(np.mean(m["flag"] | near))
    print(fix, config, "flagged", int(np.sum(m["flag"] | near)), "of", sdf.size)
    assert share <= FLAG_CAP, share


def test_bounds_pc_f32_is_the_oracles_bounds_pc():
    g, b = lcs.fixture_batch("eval_full_ray")
    bo, go = orc.bounds_pc(b["pc"].astype(np.float64), b["z_vals"].astype(np.float64), b["depth_sample"].astype(np.float64))
    bm, gm, idx = lm.bounds_pc_f32(b["pc"], b["z_vals"], b["depth_sample"])
    np.testing.assert_allclose(bm, bo, rtol=1e-5, atol=1e-6)
    d = np.linalg.norm(b["pc"][:, :, None, :].astype(np.float64) - b["pc"][None, None, :, 0].astype(np.float64), axis=-1)
    near_tie = np.sort(d, -1)[..., 1] - np.sort(d, -1)[..., 0] < 1e-6
    assert np.array_equal(idx[~near_tie], d.argmin(-1)[~near_tie])
    nan_o, nan_m = np.isnan(go).any(-1), np.isnan(gm[:, 1:]).any(-1)
    assert np.array_equal(nan_o, nan_m)
    ok = ~nan_o & ~near_tie[:, 1:]
    np.testing.assert_allclose(gm[:, 1:][ok], go[ok], rtol=0, atol=1e-5)          # fp32 differences against float64 ones
    assert np.isnan(gm[:, 0]).all()                                                # a surface sample is its own nearest point: 0 / 0


def test_bounds_pc_f32_first_minimum_and_strict_behind():
    pc = np.zeros((3, 2, 3), np.float32)
    pc[:, 0] = [[1, 0, 0], [-1, 0, 0], [0, 5, 0]]
    pc[:, 1] = [[0, 0, 0], [0, 0, 0.5], [0, 4, 0]]                   # sample 1 of rays 0, 1: equidistant from surface points 0 and 1
    z = np.array([[1, 1], [1, 2], [1, 0.5]], np.float32)
    bnd, gv, idx = lm.bounds_pc_f32(pc, z, np.ones(3, np.float32))
    assert idx[0, 1] == 0 and idx[1, 1] == 0                         # the first index wins, as argmin does
    assert bnd[0, 1] == 1.0 and bnd[1, 1] == -np.float32(np.sqrt(np.float32(1.25)))    # z == depth: not behind; z > depth: behind
    assert np.array_equal(gv[0, 1], [-1, 0, 0]) and np.isnan(gv[:, 0]).all()


def test_shapes_straddle_the_tile():
    src = lambda *p: open(os.path.join(ROOT, *p)).read()
    T = tm.kernel_constants(src("isdf_amd", "csrc", "optim.hip"), src("isdf_amd", "csrc", "isdf_common.h"))["TILE_PTS"]
    assert [r * s for r, s in lcs.SHAPES] == [1, T - 1, T, T + 1, 2 * T + 1]


def _cfg0():
    return orc.NetCfg(256, 2, 6, 0.05937489, 1.0, gu.bounds_transform())


def _hand_model(b, lc):
    R, S = b["z_vals"].shape
    bnd, band, near, tgt = lm.ray_inputs(b, lc)
    m = lm.point_terms(b["noise"], np.zeros((R, S, 3), np.float32), bnd, tgt, b["norm_sample"], lm.sample_index(R, S), lc, _cfg0(), band)
    return m, bnd.astype(np.float64), band, near


@pytest.mark.parametrize("loss_type", ["L1", "L2"])
@pytest.mark.parametrize("S", [1, 3, 27])
@pytest.mark.parametrize("cls", lcs.CLASSES_A)
def test_every_sdf_class_batch_is_what_the_table_says(cls, S, loss_type):
    lc = orc.LossCfg(loss_type=loss_type, **lcs.LC_A)
    b = lcs.make_batch([cls] * 8, S, seed=S)
    m, bnd, band, near = _hand_model(b, lc)
    sd = b["noise"].astype(np.float64)
    assert not near.any() and not m["flag"].any() and not band.any()
    assert set(m["label"].ravel()) == lcs.LABELS[cls] or (S == 1 and set(m["label"].ravel()) <= lcs.LABELS[cls])
    sl, sb, ek = lcs.closed_form(cls, loss_type, bnd, sd, lm.lc32(lc))
    for k, want in (("sl", sl), ("sbar", sb), ("ek", ek), ("gl", np.ones_like(sl)), ("tot", sl + lc.grad_weight + ek)):
        np.testing.assert_allclose(m[k], want, rtol=1e-14, atol=0, err_msg=k)
    if cls == "free_v0":
        assert (sd == 0).any() and (sd == bnd).any()
    if cls == "free_zero" and S > 1:
        assert np.signbit(b["noise"]).any() and not np.signbit(b["noise"]).all()
    if cls in lcs.EXACT:      # every value and every partial sum in any order is an fp32 value: multiples of 2^-9 whose |.| sum < 2^15
        for k in ("sl", "ek", "tot", "sbar"):
            # (sbar went through the oracle's / N and back: 2^-52 off the dyadic value it stands for)
            assert np.abs(m[k] * 512 - np.rint(m[k] * 512)).max() <= 1e-9 and np.abs(m[k]).sum() < 2 ** 15, k
        assert not m["d_tot"][m["tot"] == 0].any()


@pytest.mark.parametrize("cls,on", [("eik_at_border", True), ("eik_below_border", False)])
def test_eikonal_border_batches(cls, on):
    lc = orc.LossCfg(**lcs.LC_B)
    b = lcs.make_batch([cls] * 8, 3, seed=5)
    m, bnd, band, near = _hand_model(b, lc)
    l = lm.lc32(lc)
    assert not near.any() and not m["flag"].any() and not band.any()
    assert np.all(bnd == (lcs.EIK if on else float(np.nextafter(np.float32(lcs.EIK), np.float32(0)))))
    assert np.all(m["eik_on"] == on) and np.all(m["ek"] == (l.eik_weight if on else 0.0)) and np.all(m["gl"] == 1.0)
    assert np.all(m["sl"] == 0) and np.all(m["sbar"] == 0)
    assert np.all(m["tot"] == l.grad_weight + (l.eik_weight if on else 0.0))
    # gbar = -(grad_weight / 1e-6) h with h the unit target: the normal at sample 0, -dirs_W at the others
    h = np.broadcast_to(-b["dirs_W_sample"].astype(np.float64)[:, None, :], (8, 3, 3)).copy()
    h[:, 0] = b["norm_sample"]
    h /= np.linalg.norm(h, axis=-1, keepdims=True)
    np.testing.assert_allclose(m["gbar"], -(l.grad_weight / 1e-6) * h, rtol=1e-13)
    assert set(m["target_kind"][:, 0]) == {"normal"} and set(m["target_kind"][:, 1:].ravel()) == {"given"}
    assert np.all(m["sG"] == 2.0 ** (np.floor(np.log2(np.abs(m["gbar_x"].astype(np.float32)).max(-1))) + 1 - 1))


def test_pc_batch_has_nan_targets_that_take_the_normal():
    lc = orc.LossCfg(bounds_method="pc", **lcs.LC_B)
    b = lcs.pc_nan_batch(7)
    bnd, gv, idx = lm.bounds_pc_f32(b["pc"], b["z_vals"], b["depth_sample"])
    assert idx[0, 1] == 1 and idx[3, 2] == 5 and bnd[0, 1] == 0 and bnd[3, 2] == 0
    assert np.isnan(gv[0, 1]).all() and np.isnan(gv[3, 2]).all() and np.isnan(gv[:, 0]).all()
    assert (bnd[:, 2] <= 0).all() and (bnd[:, 1] >= 0).all()
    m = lm.point_terms(b["noise"], np.zeros((6, 3, 3), np.float32), bnd, gv, b["norm_sample"], lm.sample_index(6, 3), lc, _cfg0())
    assert m["target_kind"][0, 1] == "normal(nan)" and m["target_kind"][3, 2] == "normal(nan)"
    assert (m["target_kind"][:, 1:] == "given").sum() >= 8 and not m["flag"].any()
    k = lm.lc32(lc).grad_weight / 1e-6
    n = b["norm_sample"].astype(np.float64)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    for r, s in ((0, 1), (3, 2), (2, 0)):
        np.testing.assert_allclose(m["gbar"][r, s], -k * n[r], rtol=1e-13)


@pytest.mark.parametrize("R,S", lcs.SHAPES)
def test_mixed_batches_hold_every_class_they_can(R, S):
    lc = orc.LossCfg(**lcs.LC_A)
    b = lcs.mixed_batch(R, S, seed=R)
    m, bnd, band, near = _hand_model(b, lc)
    assert not near.any() and not m["flag"].any()
    assert list(b["cls"][:10]) == list(lcs.CLASSES_A[:R])
    for r in range(R):
        assert set(m["label"][r]) <= lcs.LABELS[b["cls"][r]]
    dead = lcs.pad_dead(b, 5)
    assert dead["n_valid"] == R and np.isnan(dead["noise"][R:]).all() and np.isnan(dead["dirs_C_sample"][R:]).all()
    assert np.array_equal(dead["pc"][:R], b["pc"])


def test_exp_allowance_is_a_few_ulp():
    assert 2 * lm.U32 < lm.exp_hw_rel() <= 16 * lm.U32
