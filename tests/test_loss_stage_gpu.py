"""The chain kernel's loss stage (chain.hip, `// loss + adjoints`) and bounds_pc_kernel (optim.hip), PER POINT and on every branch
border, against tests/loss_model.py.  Needs a real MI355X: `pytest -m gpu`.

  a. one hand-made batch per sdf-loss class of tests/loss_cases.py's table (zero-head net: sdf = noise bit for bit, d sdf/dx = 0):
     per-point totals, the per-term sums and sum(sbar) EXACT wherever the operands are dyadic, within the derived bound on the exp branch
  b. the eikonal border, the target rule (normal at sample 0, -dirs_W, pc_grad_vec, the normal at a NaN target), gbar' and s_G per point
     at gn = 0, orien_loss, each weight at 0
  c. a mixed batch at 1, TILE_PTS - 1 .. TILE_PTS + 1 and 2 TILE_PTS + 1 points, and in NaN-filled dead ray slots
  d. real gradients (random initialisation and trained weights) under five loss configurations: every point's total and gbar'
     within the derived bound of the model AT THE KERNEL'S OWN sdf / d sdf/dx, s_G bit for bit, the sums within the summation bound
  e. isdf_bounds_pc alone against the fp32 model: bounds bit for bit, the nearest index through grad_vec
The `ratio` lines printed are |kernel - model| / bound, the figures of DESIGN 5g.  tests/test_loss_stage_cpu.py checks the model and the
batches themselves.
"""
import dataclasses
import functools
import os

import numpy as np
import pytest
import torch

import oracle.isdf_oracle as orc
from tests import golden_util as gu
from tests import loss_cases as lcs
from tests import loss_model as lm
from tests import spill_model as sm
from tests import tail_model as tm
from tests.gpu_step_util import pe_aux, smp

pytestmark = pytest.mark.gpu

U = lm.U32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_src = lambda *p: open(os.path.join(ROOT, *p)).read()
C = tm.kernel_constants(_src("isdf_amd", "csrc", "optim.hip"), _src("isdf_amd", "csrc", "isdf_common.h"))
FLAG_CAP = 0.005
# zero-head nets: the default one; EP > HD (nine octaves: the WIDE_E path requests the loss inputs behind another GEMM); 512 wide
NETS = {"default": (256, 2, 6), "wide_e": (256, 2, 9), "w512": (512, 3, 10)}
SI = 0.05937489


@functools.lru_cache(maxsize=None)
def _zero_head(net):
    from isdf_amd.engine import Engine, NetConfig
    H, B, nf = NETS[net]
    T = gu.bounds_transform()
    eng = Engine(NetConfig(hidden=H, blocks=B, n_freqs=nf, scale_input=SI, scale_output=1.0, transform=T), "cuda")
    p = orc.init_params(H, B, nf, np.random.RandomState(3))
    p["out_alpha.weight"][:] = 0
    p["out_alpha.bias"][:] = 0
    eng.load_params(p)
    return eng, orc.NetCfg(H, B, nf, SI, 1.0, T)


def _lc(lo):
    from isdf_amd.engine import LossConfig
    return LossConfig(**{f.name: getattr(lo, f.name) for f in dataclasses.fields(LossConfig)})


def _run(eng, b, lo, sc=None, padded=False):
    """one training step on a batch dict -> host arrays.  padded: the batch sits in max_rays > n_valid ray slots (lcs.pad_dead)"""
    from isdf_amd.engine import SampleConfig
    sc = SampleConfig(**lcs.CAM) if sc is None else sc
    R0, S = b["z_vals"].shape
    dbg = eng.train_step(smp(b, R0 if padded else None), _lc(lo), sc, noise=torch.as_tensor(b["noise"]).cuda(), debug=True)
    torch.cuda.synchronize()
    out = {k: dbg[k].cpu().numpy() for k in ("sdf", "sdf_grad", "tot_loss_mat", "pc_bounds", "pc_grad_vec") if k in dbg}
    out["ls"] = eng.loss_sums().cpu().numpy().copy()
    out["bias"] = float(eng.grad_view("out_alpha.bias").cpu().numpy()[0])
    out["aux"] = pe_aux(eng, R0 * S)
    return out


def _d_loss(n_points):
    return C["TILE_PTS"] - 1 + tm.loss_chain_length(-(-n_points // C["TILE_PTS"]), C)


def _d_vec(n_points):
    return C["TILE_PTS"] - 1 + tm.vec_chain_length(-(-n_points // C["TILE_PTS"]), C)


def _is32(x64, got32):
    """got32 (fp32 from the device) IS the fp32 value of the model's float64 number"""
    return np.array_equal(np.asarray(x64, np.float64).astype(np.float32), np.asarray(got32, np.float32))


def _check_aux(out, m, nf, worst, tag):
    """gbar' per point within its bound, s_G bit for bit the rule of the kernel's own gbar', and the model's s_G unless |gbar'|_inf
    sits within its bound of a binade edge"""
    N = m["tot"].size
    gk, sk = out["aux"][:N, 4:7], out["aux"][:N, 7]
    gm, dg = m["gbar_x"].reshape(N, 3), m["d_gbar_x"].reshape(N, 3)
    ok = ~m["flag"].reshape(N)
    err = np.abs(gk - gm)
    assert np.all(err[ok] <= dg[ok]), (tag, "gbar'", np.argwhere(err > dg)[:5], err[err > dg][:5], dg[err > dg][:5])
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(dg > 0, err / dg, 0.0)[ok]
    worst["gbar'"] = max(worst.get("gbar'", 0.0), float(r.max()) if r.size else 0.0)
    want = sm.gb_scale(np.abs(gk.astype(np.float32)).max(-1), nf)
    assert np.array_equal(sk, want), (tag, "s_G", np.flatnonzero(sk != want)[:5])
    gmax = np.abs(gm).max(-1)
    edge = np.abs(gmax - 2.0 ** np.rint(np.log2(np.maximum(gmax, 1e-300)))) <= dg.max(-1)
    assert np.all((sk == m["sG"].reshape(N)) | edge | ~ok), (tag, "s_G vs the model's")


def _check_hand(out, b, lo, cfg, tag, worst, m=None):
    """a hand-made zero-head batch (live rays only) against the model: everything of the docstring's a."""
    R, S = b["z_vals"].shape
    N = R * S
    assert np.array_equal(out["sdf"], b["noise"]), (tag, "sdf is not the noise")
    assert not out["sdf_grad"].any(), (tag, "d sdf/dx is not 0")
    if m is None:
        bnd, band, near, tgt = lm.ray_inputs(b, lo)
        assert not near.any()
        m = lm.point_terms(b["noise"], out["sdf_grad"], bnd, tgt, b["norm_sample"], lm.sample_index(R, S), lo, cfg, band)
    assert not m["flag"].any(), tag
    exact_ray = np.array([c in lcs.EXACT or c.startswith("eik") for c in b["cls"]])      # per point: every value an fp32 value
    exact_sum = all(c in lcs.EXACT for c in b["cls"])                                       # ... and every partial sum (LC_A)
    tot = out["tot_loss_mat"]
    print(tag, "tot", tot.ravel()[:4], "model", m["tot"].ravel()[:4], "sums", out["ls"][:5], "bias", out["bias"])
    assert _is32(m["tot"][exact_ray], tot[exact_ray]), (tag, "tot (exact classes)", tot[exact_ray].ravel()[:6], m["tot"][exact_ray].ravel()[:6])
    err = np.abs(tot.astype(np.float64) - m["tot"])
    assert np.all(err <= m["d_tot"]), (tag, "tot", err.max(), np.argwhere(err > m["d_tot"])[:5])
    if (~exact_ray).any():
        with np.errstate(invalid="ignore", divide="ignore"):
            worst["tot"] = max(worst.get("tot", 0.0), float(np.where(m["d_tot"] > 0, err / m["d_tot"], 0.0)[~exact_ray].max()))
    ls = out["ls"].astype(np.float64)
    assert ls[4] == N, (tag, ls[4])
    for i, (k, dk) in enumerate((("sl", "d_sl"), ("gl", "d_gl"), ("ek", "d_ek"), ("tot", "d_tot"))):
        if exact_sum:
            assert _is32(m[k].sum(), out["ls"][i]), (tag, k + " sum", out["ls"][i], m[k].sum())
        else:
            bound = m[dk].sum() + _d_loss(N) * U * np.abs(m[k]).sum()
            assert abs(ls[i] - m[k].sum()) <= bound, (tag, k + " sum", ls[i], m[k].sum(), bound)
    sb = m["sbar"].sum() * cfg.scale_output
    if exact_sum:
        assert _is32(sb, np.float32(out["bias"])), (tag, "sum sbar", out["bias"], sb)
    else:
        bound = m["d_sbar"].sum() + _d_vec(N) * U * np.abs(m["sbar"]).sum()
        assert abs(out["bias"] - sb) <= bound, (tag, "sum sbar", out["bias"], sb, bound)
        worst["sum sbar"] = max(worst.get("sum sbar", 0.0), float(abs(out["bias"] - sb) / bound) if bound else 0.0)
    _check_aux(out, m, cfg.n_freqs, worst, tag)
    return m


# ---- a. sdf-loss classes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_type", ["L1", "L2"])
@pytest.mark.parametrize("cls", lcs.CLASSES_A)
def test_sdf_loss_class(cls, loss_type):
    eng, cfg = _zero_head("default")
    lo = orc.LossCfg(loss_type=loss_type, **lcs.LC_A)
    worst = {}
    for S in (1, 3, 27):
        b = lcs.make_batch([cls] * 8, S, seed=S)
        _check_hand(_run(eng, b, lo), b, lo, cfg, "%s %s S=%d" % (cls, loss_type, S), worst)
    print("ratio a.", cls, loss_type, worst)


@pytest.mark.parametrize("loss_type", ["L1", "L2"])
@pytest.mark.parametrize("net", ["wide_e", "w512"])
def test_first_class_on_the_other_chain_instantiations(net, loss_type):
    eng, cfg = _zero_head(net)
    lo = orc.LossCfg(loss_type=loss_type, **lcs.LC_A)
    worst = {}
    for S in (1, 3, 27):
        b = lcs.make_batch([lcs.CLASSES_A[0]] * 8, S, seed=S)
        _check_hand(_run(eng, b, lo), b, lo, cfg, "%s %s S=%d" % (net, loss_type, S), worst)
    b = lcs.mixed_batch(21, 3, seed=21)            # ... and every class once more, on a ragged tile
    _check_hand(_run(eng, b, lo), b, lo, cfg, "%s %s mixed" % (net, loss_type), worst)
    print("ratio a.", net, loss_type, worst)


# ---- b. eikonal and normal term at gn = 0 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_type", ["L1", "L2"])
@pytest.mark.parametrize("cls,on", [("eik_at_border", True), ("eik_below_border", False)])
def test_eikonal_border_and_target_rule(cls, on, loss_type):
    """bnd == eik_apply_dist: the term applies (`<` is strict); one ulp below: zero.  gl = 1, ek = eik_weight, tot their fp32 sum;
    gbar' = -(grad_weight / 1e-6) si R h per point with h the normal at sample 0 and -dirs_W at the others"""
    eng, cfg = _zero_head("default")
    lo = orc.LossCfg(loss_type=loss_type, **lcs.LC_B)
    l = lm.lc32(lo)
    worst = {}
    for S in (1, 3, 27):
        b = lcs.make_batch([cls] * 8, S, seed=40 + S)
        out = _run(eng, b, lo)
        m = _check_hand(out, b, lo, cfg, "%s %s S=%d" % (cls, loss_type, S), worst)
        N = 8 * S
        assert out["ls"][1] == N and out["ls"][0] == 0 and out["bias"] == 0
        ek = l.eik_weight if on else 0.0
        assert np.all(out["tot_loss_mat"] == np.float32(l.grad_weight + ek))
        assert abs(float(out["ls"][2]) - N * ek) <= _d_loss(N) * U * N * ek
        assert set(m["target_kind"][:, 0]) == {"normal"} and (S == 1 or set(m["target_kind"][:, 1:].ravel()) == {"given"})
    print("ratio b.", cls, loss_type, worst)


@pytest.mark.parametrize("loss_type", ["L1", "L2"])
def test_pc_target_and_the_normal_at_nan_targets(loss_type):
    eng, cfg = _zero_head("default")
    lo = orc.LossCfg(bounds_method="pc", loss_type=loss_type, **lcs.LC_B)
    b = lcs.pc_nan_batch(7)
    out = _run(eng, b, lo)
    bnd, gv, _ = lm.bounds_pc_f32(b["pc"], b["z_vals"], b["depth_sample"])
    assert np.array_equal(out["pc_bounds"], bnd)
    nan = np.isnan(gv).any(-1)
    assert np.array_equal(np.isnan(out["pc_grad_vec"]).any(-1), nan) and nan[0, 1] and nan[3, 2] and nan[:, 0].all()
    assert np.all(np.abs(out["pc_grad_vec"] - gv)[~nan] <= lm.GRAD_VEC_K * U * np.abs(gv[~nan]))
    # the model at what the kernel used
    m = lm.point_terms(b["noise"], out["sdf_grad"], out["pc_bounds"], out["pc_grad_vec"], b["norm_sample"], lm.sample_index(6, 3), lo, cfg)
    assert m["target_kind"][0, 1] == "normal(nan)" and m["target_kind"][3, 2] == "normal(nan)"
    worst = {}
    b = dict(b, cls=np.array(["inexact"] * 6))          # (the shipped trunc_weight: totals within the bound, not dyadic)
    _check_hand(out, b, lo, cfg, "pc " + loss_type, worst, m=m)
    print("ratio b. pc", loss_type, worst)


@pytest.mark.parametrize("loss_type", ["L1", "L2"])
def test_orien_loss_at_zero_cosine(loss_type):
    """cs = 0: gl = (1 - cs > 1) = 0, and no adjoint: gbar' = 0, s_G = 1"""
    eng, cfg = _zero_head("default")
    lo = orc.LossCfg(loss_type=loss_type, orien_loss=True, **lcs.LC_B)
    b = lcs.make_batch(["eik_at_border"] * 8, 3, seed=43)
    out = _run(eng, b, lo)
    _check_hand(out, b, lo, cfg, "orien " + loss_type, {})
    assert out["ls"][1] == 0 and not out["aux"][:24, 4:7].any() and np.all(out["aux"][:24, 7] == 1.0)
    assert np.all(out["tot_loss_mat"] == np.float32(lm.lc32(lo).eik_weight))


@pytest.mark.parametrize("loss_type", ["L1", "L2"])
def test_each_weight_at_zero(loss_type):
    """grad_weight = 0: the normal term's sum is exactly 0 and, the eikonal adjoint being 0 at gn = 0, gbar' = 0 and s_G = 1.
    eik_weight = 0: the eikonal sum is exactly 0; gbar' is the normal term's (s_G follows its rule).  Both 0: s_G = 1."""
    eng, cfg = _zero_head("default")
    b = lcs.make_batch(["eik_at_border"] * 8, 3, seed=43)
    for gw, ew in ((0.0, None), (None, 0.0), (0.0, 0.0)):
        kw = dict(lcs.LC_B)
        if gw is not None:
            kw["grad_weight"] = gw
        if ew is not None:
            kw["eik_weight"] = ew
        lo = orc.LossCfg(loss_type=loss_type, **kw)
        out = _run(eng, b, lo)
        _check_hand(out, b, lo, cfg, "gw %s ew %s %s" % (gw, ew, loss_type), {})
        if gw == 0.0:
            assert out["ls"][1] == 0 and not out["aux"][:24, 4:7].any() and np.all(out["aux"][:24, 7] == 1.0)
        if ew == 0.0:
            assert out["ls"][2] == 0
        if gw is None:
            assert np.abs(out["aux"][:24, 4:7]).max(-1).min() > 0 and np.all(out["aux"][:24, 7] != 1.0)


# ---- c. shapes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_type", ["L1", "L2"])
@pytest.mark.parametrize("R,S", lcs.SHAPES, ids=lambda v: str(v))
def test_mixed_batch_shapes_and_dead_ray_slots(R, S, loss_type):
    eng, cfg = _zero_head("default")
    lo = orc.LossCfg(loss_type=loss_type, **lcs.LC_A)
    b = lcs.mixed_batch(R, S, seed=R)
    live = _run(eng, b, lo)
    worst = {}
    _check_hand(live, b, lo, cfg, "mixed %dx%d %s" % (R, S, loss_type), worst)
    dead = _run(eng, lcs.pad_dead(b, 5), lo, padded=True)       # every float input of the 5 dead slots NaN, the noise too
    assert dead["ls"][4] == R * S
    assert np.isfinite(dead["ls"]).all() and np.array_equal(dead["ls"], live["ls"]), (dead["ls"], live["ls"])
    assert dead["bias"] == live["bias"]
    assert np.array_equal(dead["tot_loss_mat"][:R], live["tot_loss_mat"]) and not dead["tot_loss_mat"][R:].any()   # (allocated as zeros)
    assert np.array_equal(dead["aux"][:R * S, 4:], live["aux"][:R * S, 4:])
    print("ratio c.", R, S, loss_type, worst)


# ---- d. real gradients, per point -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture_engine(fix):
    from isdf_amd.engine import Engine, NetConfig
    g, b = lcs.fixture_batch(fix)
    H, B, nf, si, so = g["net"]
    eng = Engine(NetConfig(hidden=int(H), blocks=int(B), n_freqs=int(nf), scale_input=float(si), scale_output=float(so),
                           transform=g["bounds_T"]), "cuda")
    eng.load_params(gu.params_of(g))
    return g, b, eng


@pytest.mark.parametrize("config", sorted(lcs.CONFIGS))
@pytest.mark.parametrize("fix", lcs.FIXTURES)
def test_real_gradients_per_point(fix, config):
    from isdf_amd.engine import SampleConfig
    g, b, eng = _fixture_engine(fix)
    cfg = gu.net_of(g)
    lo = lcs.loss_cfg(gu.loss_of(g), **lcs.CONFIGS[config])
    out = _run(eng, b, lo, SampleConfig(**gu.cam_of(g)))
    R, S = b["z_vals"].shape
    N = R * S
    if lo.bounds_method == "ray":
        bnd, band, near, tgt = lm.ray_inputs(b, lo)
    else:
        bnd, band, near, tgt = out["pc_bounds"], None, np.zeros((R, S), bool), out["pc_grad_vec"]
    args = (out["sdf"], out["sdf_grad"], bnd, tgt, b["norm_sample"], lm.sample_index(R, S), lo, cfg, band)
    m = lm.point_terms(*args)
    flag = m["flag"] | near
    share = float(flag.mean())
    print(fix, config, "flagged", int(flag.sum()), "of", N, "classes", dict(zip(*np.unique(m["label"], return_counts=True))))
    assert share <= FLAG_CAP, share
    tot = out["tot_loss_mat"].astype(np.float64)
    gk = out["aux"][:N, 4:7].reshape(R, S, 3)
    e_t, e_g = np.abs(tot - m["tot"]), np.abs(gk - m["gbar_x"])
    with np.errstate(invalid="ignore", divide="ignore"):
        r_t = np.where(m["d_tot"] > 0, e_t / m["d_tot"], 0.0)
        r_g = np.where(m["d_gbar_x"] > 0, e_g / m["d_gbar_x"], np.where(e_g > 0, np.inf, 0.0))
    print("ratio d.", fix, config, "tot %.3f gbar' %.3f" % (r_t[~flag].max(), r_g[~flag].max()))
    slack = np.zeros((R, S))
    if flag.any():          # a flagged point took one side of a border its inputs sit on: the model's value or a corner's
        alts = [m] + lm.alternatives(*args)
        okf = np.zeros((R, S), bool)
        for a in alts:
            okf |= (np.abs(tot - a["tot"]) <= a["d_tot"]) & np.all(np.abs(gk - a["gbar_x"]) <= a["d_gbar_x"], -1)
            slack = np.maximum(slack, np.abs(a["tot"] - m["tot"]) + np.abs(a["sl"] - m["sl"]) + np.abs(a["gl"] - m["gl"]) + np.abs(a["ek"] - m["ek"]))
        assert np.all(okf[flag]), (fix, config, "flagged points on neither side", np.argwhere(flag & ~okf)[:5])
    assert np.all(r_t[~flag] <= 1), (fix, config, "tot", np.argwhere((r_t > 1) & ~flag)[:5], r_t[~flag].max())
    assert np.all(r_g[~flag] <= 1), (fix, config, "gbar'", np.argwhere((r_g > 1) & ~flag[..., None])[:5], r_g[~flag].max())
    sk = out["aux"][:N, 7]
    want = sm.gb_scale(np.abs(gk.reshape(N, 3).astype(np.float32)).max(-1), cfg.n_freqs)
    assert np.array_equal(sk, want), np.flatnonzero(sk != want)[:5]
    ls = out["ls"].astype(np.float64)
    assert ls[4] == N
    worst = 0.0
    for i, (k, dk) in enumerate((("sl", "d_sl"), ("gl", "d_gl"), ("ek", "d_ek"), ("tot", "d_tot"))):
        # each point's own bound, the flagged points' two sides, and the kernel's fp32 summation (test_step_tail_gpu.py's d U)
        bound = m[dk].sum() + slack[flag].sum() + _d_loss(N) * U * np.abs(m[k]).sum()
        assert abs(ls[i] - m[k].sum()) <= bound, (fix, config, k, ls[i], m[k].sum(), bound)
        worst = max(worst, abs(ls[i] - m[k].sum()) / bound if bound else 0.0)
    print("ratio d. sums", fix, config, "%.3f" % worst)


# ---- e. bounds_pc alone -----------------------------------------------------------------------------------------------------------
SENTINEL = 777.0


def _bounds_pc(pc, z, depth, n_valid, surf=None):
    from isdf_amd import _ffi
    R0, S = z.shape
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()
    pcs, zs, ds = d(pc), d(z), d(depth)
    sf = None if surf is None else d(surf)
    nv = torch.tensor([n_valid], dtype=torch.int32, device="cuda")
    pb = torch.full((R0 * S,), SENTINEL, device="cuda")
    pg = torch.full((R0 * S, 3), SENTINEL, device="cuda")
    _ffi.check(_ffi.lib().isdf_bounds_pc(_ffi.ptr(nv), R0, S, _ffi.ptr(pcs), _ffi.ptr(zs), _ffi.ptr(ds), _ffi.ptr(sf),
                                         0 if sf is None else sf.shape[0], _ffi.ptr(pb), _ffi.ptr(pg), None), "isdf_bounds_pc")
    torch.cuda.synchronize()
    return pb.view(R0, S).cpu().numpy(), pg.view(R0, S, 3).cpu().numpy()


def _check_bounds_pc(pc, z, depth, n_valid, surf=None, tag=""):
    got_b, got_g = _bounds_pc(pc, z, depth, n_valid, surf)
    R = n_valid
    bnd, gv, idx = lm.bounds_pc_f32(pc[:R], z[:R], depth[:R], surf)
    assert np.array_equal(got_b[:R], bnd), (tag, "bounds", np.argwhere(got_b[:R] != bnd)[:5])
    nan = np.isnan(gv).any(-1)
    assert np.array_equal(np.isnan(got_g[:R]).any(-1), nan), (tag, "NaN pattern")
    err, bound = np.abs(got_g[:R] - gv)[~nan], lm.GRAD_VEC_K * U * np.abs(gv[~nan])
    assert np.all(err <= bound), (tag, "grad_vec (the nearest index shows here)", err.max())
    assert np.all(got_b[R:] == SENTINEL) and np.all(got_g[R:] == SENTINEL), (tag, "dead slots written")
    with np.errstate(invalid="ignore", divide="ignore"):
        r = float(np.where(bound > 0, err / bound, 0.0).max()) if err.size else 0.0
    print("ratio e.", tag, "grad_vec %.3f" % r)
    return idx, got_b, got_g


@pytest.mark.parametrize("R", [1, 255, 256, 257])
def test_bounds_pc_around_the_lds_tile(R):
    rng = np.random.default_rng(R)
    S = 3
    pc = rng.uniform(-2, 2, (R, S, 3)).astype(np.float32)
    z = rng.uniform(0.5, 2, (R, S)).astype(np.float32)
    depth = z[:, 0].copy()
    idx, _, _ = _check_bounds_pc(pc, z, depth, R, tag="R=%d" % R)
    assert R == 1 or len(np.unique(idx)) > R // 2              # the search really ranges over the set, last tile included
    # dead ray slots at the end, NaN in every input of theirs
    pad = lambda a: np.concatenate((a, np.full((7,) + a.shape[1:], np.nan, np.float32)))
    _check_bounds_pc(pad(pc), pad(z), pad(depth), R, tag="R=%d + 7 dead" % R)


def test_bounds_pc_tie_takes_the_first_index_and_behind_is_strict():
    R, S = 260, 2
    rng = np.random.default_rng(9)
    pc = (rng.integers(-64, 65, (R, S, 3)) / 8.0).astype(np.float32)
    pc[:, 0, 0] += 100.0                                                # the random surface points: far from the tie
    pc[3, 0], pc[258, 0] = [1, 0, 0], [-1, 0, 0]                        # two surface points in different LDS tiles ...
    pc[7, 1] = [0, 0, 0]                                                # ... at distance exactly 1 from this sample
    pc[200, 0], pc[100, 0] = [0, 40, 3], [0, 40, -3]                    # ... and two within one tile, at distance exactly 3
    pc[8, 1] = [0, 40, 0]
    z = np.full((R, S), 1.0, np.float32)
    depth = np.ones(R, np.float32)                                      # z == depth everywhere: not behind (`>` is strict)
    z[9, 1] = np.nextafter(np.float32(1), np.float32(2))                # one ulp behind
    idx, got_b, got_g = _check_bounds_pc(pc, z, depth, R, tag="tie")
    assert idx[7, 1] == 3 and np.array_equal(got_g[7, 1], [-1, 0, 0]) and got_b[7, 1] == 1.0
    assert idx[8, 1] == 100 and np.array_equal(got_g[8, 1], [0, 0, 1]) and got_b[8, 1] == 3.0
    assert (got_b[:, 1] >= 0).sum() == R - 1 and got_b[9, 1] < 0


def test_bounds_pc_gathered_surface_set_with_far_slots():
    from isdf_amd import dp
    rng = np.random.default_rng(11)
    R, S = 300, 2
    pc = rng.uniform(-2, 2, (R, S, 3)).astype(np.float32)
    z = rng.uniform(0.5, 2, (R, S)).astype(np.float32)
    depth = rng.uniform(0.5, 2, R).astype(np.float32)
    far = np.full((7, 3), dp.FAR, np.float32)
    surf = np.concatenate((pc[:100, 0], far, pc[100:, 0], far))        # two ranks' slots, 314 = no multiple of 256
    rows = np.arange(100, 300)                                          # this rank holds the second shard, + 7 dead slots
    pad = lambda a: np.concatenate((a[rows], np.full((7,) + a.shape[1:], np.nan, np.float32)))
    idx, _, _ = _check_bounds_pc(pad(pc), pad(z), pad(depth), len(rows), surf=surf, tag="gathered")
    assert not np.isin(idx, np.r_[100:107, 307:314]).any() and (idx < 100).any() and (idx >= 107).any()
