"""The training step under every spill format (`isdf_net_cfg.spill_operand`: auto / 16bit / e4m3 / e4m3_gb) on every train-mode
kernel instantiation, against `tests/spill_model.py` (float64 oracle with P and GB rounded exactly where the kernels read the spill)
and against the oracle itself.  Needs a real MI355X: `pytest -m gpu`.

  * coverage matrix: one case per `chain_kernel<HD, EP, OPER, 2, BW, SP8>` (CHAIN_CASES) -- and with them every
    `dw_kernel<HD, F16, SP8>` (DW_KERNELS) -- on ragged batches of 1, 63, 64, 65 and ~3 000 points (the small ones have fewer tiles than
    any dW unit has K-splits: the zero-slab path).  Losses against the oracle; every gradient tensor, with the loss adjoints taken at
    the kernel's own outputs, against the model of its own format, held to a bar derived from the 16-bit twin's distance to the oracle
  * invariants, bit-exact: the forward, the loss and the frame bins do not depend on the format; `auto` is what it resolves to; with
    eik_weight = grad_weight = 0 the gradient does not depend on the format either
  * direction of the format's effect at BASELINE size: HIP(e4m3) - HIP(16bit) tracks model(e4m3) - model(16bit)
  * loss-weight sweep (the per-point GB scale across magnitudes) and trained weights (signed projections)
tests/test_spill_formats_cpu.py checks the model itself and that this file's table is the built library's.
"""
import dataclasses
import os

import numpy as np
import pytest
import torch

import oracle.isdf_oracle as orc
from tests import golden_util as gu
from tests import spill_model as sm
from tests.gpu_step_util import pe_aux as _pe_aux, smp as _smp

pytestmark = pytest.mark.gpu

OPERS = ("bf16", "fp16", "fp16x2", "fp16x2_full")
SPILL_SP8 = {"16bit": 0, "e4m3": 3, "e4m3_gb": 1}

# (HD, EP, OPER, BW, SP8) of chain_kernel<HD, EP, OPER, MODE 2, BW, SP8> -> (fixture, fwd_operand, bwd_operand, spill_operand) that
# reaches it.  Fixtures: eval_full_ray (256 x 2 blocks, 6 octaves), eval_small_ray (64 x 1, 6), eval_rs_franka (256 x 2, 9: the
# realsense_franka net), eval_small_b3_f11 (64 x 3, 11), eval_wide_512 (512 x 3, 10), eval_h300_f10 (300 x 2, 10).
# `new`: no test launched the kernel before this file (found by dispatch reading: the suite only ever ran `auto`).
CHAIN_CASES = {
    (256, 256, 0, 0, 0): ("eval_full_ray", "bf16", "bf16", "16bit"),
    (256, 256, 1, 0, 0): ("eval_small_ray", "fp16", "bf16", "16bit"),
    (256, 256, 1, 1, 0): ("eval_small_ray", "fp16", "fp16", "16bit"),          # new
    (256, 256, 1, 1, 3): ("eval_small_ray", "fp16", "fp16", "e4m3"),
    (256, 256, 1, 1, 1): ("eval_small_ray", "fp16", "fp16", "e4m3_gb"),        # new
    (256, 256, 2, 0, 0): ("eval_full_ray", "fp16x2", "bf16", "16bit"),
    (256, 256, 2, 1, 0): ("eval_full_ray", "fp16x2", "fp16", "16bit"),         # new
    (256, 256, 2, 1, 3): ("eval_full_ray", "fp16x2", "fp16", "e4m3"),
    (256, 256, 2, 1, 1): ("eval_full_ray", "fp16x2", "fp16", "e4m3_gb"),       # new
    (256, 256, 3, 0, 0): ("eval_full_ray", "fp16x2_full", "bf16", "16bit"),
    (256, 256, 3, 1, 0): ("eval_full_ray", "fp16x2_full", "fp16", "16bit"),    # new
    (256, 256, 3, 1, 3): ("eval_full_ray", "fp16x2_full", "fp16", "e4m3"),
    (256, 256, 3, 1, 1): ("eval_full_ray", "fp16x2_full", "fp16", "e4m3_gb"),  # new
    (256, 512, 0, 0, 0): ("eval_rs_franka", "bf16", "bf16", "16bit"),
    (256, 512, 1, 0, 0): ("eval_small_b3_f11", "fp16", "bf16", "16bit"),
    (256, 512, 1, 1, 0): ("eval_small_b3_f11", "fp16", "fp16", "16bit"),
    (256, 512, 1, 1, 3): ("eval_small_b3_f11", "fp16", "fp16", "e4m3"),        # new
    (256, 512, 1, 1, 1): ("eval_small_b3_f11", "fp16", "fp16", "e4m3_gb"),     # new
    (256, 512, 2, 0, 0): ("eval_rs_franka", "fp16x2", "bf16", "16bit"),
    (256, 512, 2, 1, 0): ("eval_rs_franka", "fp16x2", "fp16", "16bit"),
    (256, 512, 2, 1, 3): ("eval_rs_franka", "fp16x2", "fp16", "e4m3"),         # new
    (256, 512, 2, 1, 1): ("eval_rs_franka", "fp16x2", "fp16", "e4m3_gb"),      # new
    (512, 512, 0, 0, 0): ("eval_wide_512", "bf16", "bf16", "16bit"),
    (512, 512, 1, 0, 0): ("eval_h300_f10", "fp16", "bf16", "16bit"),
    (512, 512, 1, 1, 0): ("eval_h300_f10", "fp16", "fp16", "16bit"),
    (512, 512, 2, 0, 0): ("eval_wide_512", "fp16x2", "bf16", "16bit"),
    (512, 512, 2, 1, 0): ("eval_wide_512", "fp16x2", "fp16", "16bit"),
}
# dw_kernel<HD, F16, SP8>: one per (HD, BW, SP8) of the chain table
DW_KERNELS = sorted({(hd, bw, sp8) for (hd, ep, op, bw, sp8) in CHAIN_CASES})

SIZES = ((1, 1), (7, 9), (4, 16), (5, 13), (111, 27))      # (rays, samples per ray): 1, 63, 64, 65 and 2 997 points
TOL_LOSS = {"bf16": 8e-3, "fp16": 2e-3, "fp16x2": 1e-3, "fp16x2_full": 1e-3}    # test_gpu_parity.py's loss bars per forward operand
# HIP vs the model of its own format, per tensor: at most TWIN_FACTOR x (twin + eff) + TWIN_FLOOR, twin = the 16-bit twin's rel-L2 to
# the oracle (the kernels' 16-bit operand floor), eff = the model's own e4m3 effect, rel-L2(model(fmt), model(16bit)).  The kernel rounds
# to e4m3 values that differ from the model's by that floor, so its rounding DECISIONS differ near every tie: measured, its e4m3 effect
# has the model's size but is only partly aligned with it (cosines 0.54 .. 0.98 at BASELINE size) -- up to sqrt(2) eff apart
# when fully decorrelated.  A scale or binade slip moves the whole second-order term instead (16 x eff and more).
TWIN_FACTOR, TWIN_FLOOR = 1.5, 2e-4
# direction of the e4m3 effect at BASELINE size, per tensor: cosine and norm ratio of HIP(fmt) - HIP(16bit) against model(fmt) -
# model(16bit).  Measured on MI355X: cosines 0.54 .. 0.98, ratios 0.93 .. 1.13 (the 0.9 cosine the design expected does not hold:
# the decorrelated rounding above; a model run with 3e-3 relative noise on the rounded values reproduces cosines of 0.8 at ratio 1.0)
DIR_COS, DIR_RATIO = 0.45, (0.8, 1.25)
TOL_DW = 1e-2       # test_gpu_parity.py's gradient bar
# absolute ceilings at EVERY batch size on the worst gradient tensor's rel-L2 to the oracle (adjoints at the kernel's own outputs), by
# the operand types (bf16 forward?, second-order sweeps).  Measured on MI355X over 1 .. 3 000 points: 8.7e-3 (fp16 sweeps; the 512-wide
# net at one point), 1.1e-2 (bf16 sweeps), 5.8e-2 (bf16 forward and sweeps on the nine-octave net, whose positional encoding amplifies
# the adjoints by 2^8).  A dropped, doubled or garbage K-split slab -- at the small sizes most slabs of every unit are zero slabs --
# moves a whole tensor (rel-L2 ~1).  The e4m3 formats add 1.5 x their model-predicted effect on top.
CEIL = {(False, "fp16"): 1.5e-2, (False, "bf16"): 2e-2, (True, "bf16"): 1e-1}
# loss sums against the oracle at every size: |HIP - oracle| <= TOL_LOSS x (|oracle| + floor), floor = the term's scale (a unit
# residual on the sdf output scale x the truncation weight; 1 for the cosine and eikonal terms before their weights).  Below 1 000
# points the bf16 forward gets TOL_LOSS_BF16_SMALL: one point's normal-alignment term carries its d sdf / dx error unaveraged (measured
# 1.9e-2 of the term's scale at one point on the default net)
TOL_LOSS_BF16_SMALL = 3e-2
EFFECT_RATIO = (0.5, 2.0)   # ~3 000 points: |HIP(fmt) - HIP(16bit)| / |model(fmt) - model(16bit)|, all parameters (measured ~1)


def _fixture(name):
    g = dict(np.load(os.path.join(gu.GOLDEN_DIR, name + ".npz"), allow_pickle=False))
    # (the BASELINE-size fixtures keep no T_WC_sample: gu.load regenerates their keyframes and gathers it)
    return g if "T_WC_sample" in g else gu.load(name)


def _has_T(g):
    return int(g["has_transform"][0]) if "has_transform" in g else 1


def _engine(g, fwd, bwd, spill, params=None):
    from isdf_amd.engine import Engine, NetConfig
    H, B, nf, si, so = g["net"]
    net = NetConfig(hidden=int(H), blocks=int(B), n_freqs=int(nf), scale_input=float(si), scale_output=float(so),
                    transform=g["bounds_T"] if _has_T(g) else None, fwd_operand=fwd, bwd_operand=bwd, spill_operand=spill)
    eng = Engine(net, "cuda")
    eng.load_params(gu.params_of(g) if params is None else params)
    return eng


def _cfgs(g, weight=1.0, **over):
    from isdf_amd.engine import LossConfig, SampleConfig
    lo = gu.loss_of(g)
    lo.eik_weight *= weight
    lo.grad_weight *= weight
    for k, v in over.items():
        setattr(lo, k, v)
    lc = LossConfig(**{f.name: getattr(lo, f.name) for f in dataclasses.fields(LossConfig)})
    cam = gu.cam_of(g)
    return lc, lo, SampleConfig(**cam)


def _batch(g, R, S, prefix=""):
    """the first R rays x first S samples of a fixture's (or a trained fixture's `prefix`) sampled batch: sample 0 is the surface
    sample, the others a subset of the ray's stratified / surface samples; bounds, targets and bins stay well defined"""
    src = gu.trained_batch(g, prefix) if prefix else None
    get = (lambda k: src[k]) if src else (lambda k: g[k])
    T_WC = get("T_WC_sample")[:R].astype(np.float32)
    dC = get("dirs_C_sample")[:R].astype(np.float32)
    b = dict(pc=get("pc")[:R, :S], z_vals=get("z_vals")[:R, :S], depth_sample=get("depth_sample")[:R], dirs_C_sample=dC,
             T_WC_sample=T_WC, dirs_W_sample=orc.origin_dirs_W(T_WC, dC)[1].astype(np.float32),
             norm_sample=get("norm_sample")[:R] if gu.with_normals(g) else None,
             indices_b=get("indices_b")[:R].astype(np.int64), indices_h=get("indices_h")[:R].astype(np.int64),
             indices_w=get("indices_w")[:R].astype(np.int64))
    if src:
        b["noise"] = src["noise"][:R, :S]
        b["n_frames"] = int(g["n_frames"][0])
    else:
        R0 = g["z_vals"].shape[0]
        b["noise"] = (g["draw_noise"].reshape(R0, -1)[:R, :S] * np.float32(g["noise_std"][0])).astype(np.float32)
        b["n_frames"] = int(g["indices_b"].max()) + 1
    return {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in b.items()}


def _step(eng, b, lc, sc):
    """one training step -> dict of float64 host arrays: grads (sums / N), sdf, sdf_grad, tot_loss_mat, loss sums, bins, raw buffer"""
    dbg = eng.train_step(_smp(b), lc, sc, noise=torch.as_tensor(b["noise"]).cuda(), debug=True)
    torch.cuda.synchronize()
    red = eng.reduce_buf[:eng.reduce_floats].cpu()
    N = b["z_vals"].size
    out = dict(red=red, n=eng.n_params, sdf=dbg["sdf"].cpu().numpy(), sdf_grad=dbg["sdf_grad"].cpu().numpy(),
               tot=dbg["tot_loss_mat"].cpu().numpy(),
               grads={k: eng.grad_view(k).cpu().numpy().astype(np.float64) / N for k in eng.slices})
    return out


def _slices(fix):
    from isdf_amd.engine import NetConfig
    g = _fixture(fix)
    H, B, nf = (int(v) for v in g["net"][:3])
    off, out = 0, {}
    for k, shp in NetConfig(hidden=H, blocks=B, n_freqs=nf).param_shapes():
        out[k] = (off, shp)
        off += int(np.prod(shp))
    return out


def _check_gb_scale(eng, N, nf, terms):
    """s_G as the kernel applied it: bit-exact the rule of its own gbar' (a changed spill_gb_shift or window fails here), and its
    gbar' the model's (kernel-scale adjoints at the same outputs)"""
    aux = _pe_aux(eng, N)
    gk, sk = aux[:, 4:7], aux[:, 7]
    want = sm.gb_scale(np.abs(gk.astype(np.float32)).max(-1), nf)
    assert np.array_equal(sk, want), (N, np.flatnonzero(sk != want)[:5], sk[sk != want][:5], want[sk != want][:5])
    assert gu.rel_err(gk, terms["gx"]) < 1e-4, gu.rel_err(gk, terms["gx"])
    assert np.mean(sk != terms["sG"]) <= 0.01, np.mean(sk != terms["sG"])     # (a point whose |gbar'|_inf sits on a binade edge)


def _oargs(g, b, lo):
    return (gu.params_of(g), gu.net_of(g), lo, b["pc"], b["z_vals"], b["depth_sample"], b["dirs_C_sample"], b["T_WC_sample"],
            b["norm_sample"])


def _model(g, b, lo, fmt, bwd, hip, **kw):
    adj = (hip["sdf"], hip["sdf_grad"])
    return sm.loss_and_grads(*_oargs(g, b, lo), noise=b["noise"], fmt=fmt, bwd=bwd, adjoints_from=adj, **kw)


def _rel(got, ref):
    return {k: gu.rel_err(got[k], ref[k]) for k in ref}


def _check_losses(hip, terms, tol, N, lo, so=0.14):
    ls = hip["red"][hip["n"]:hip["n"] + 8].numpy().astype(np.float64)
    assert ls[4] == N
    fl = {"sdf_loss": lo.trunc_weight * so, "grad_loss": 1.0, "eikonal_loss": 1.0}
    fl["total_loss"] = fl["sdf_loss"] + lo.grad_weight + lo.eik_weight
    worst = 0.0
    for i, k in enumerate(("sdf_loss", "grad_loss", "eikonal_loss", "total_loss")):
        want = float(np.asarray(terms[k]).reshape(-1)[0])
        err = abs(ls[i] / N - want) / (abs(want) + fl[k])
        assert err <= tol, (N, k, ls[i] / N, want)
        worst = max(worst, err)
    return worst


def _all(gr):
    return np.concatenate([gr[k].ravel() for k in sorted(gr)])


# ---- 1. coverage matrix -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(CHAIN_CASES), ids=lambda k: "chain<%d,%d,OPER%d,2,BW%d,SP8_%d>" % k)
def test_every_train_instantiation_vs_its_spill_model(kernel):
    fix, fwd, bwd, spill = CHAIN_CASES[kernel]
    g = _fixture(fix)
    lc, lo, sc = _cfgs(g)
    eng = _engine(g, fwd, bwd, spill)
    twin = _engine(g, fwd, bwd, "16bit") if spill != "16bit" else None
    report = []
    for R, S in SIZES:
        R = min(R, g["z_vals"].shape[0])
        b = _batch(g, R, S)
        N = R * S
        hip = _step(eng, b, lc, sc)
        mterms, model = _model(g, b, lo, spill, bwd, hip, want_intermediates=True)
        _check_gb_scale(eng, N, int(g["net"][2]), mterms)
        e_model = _rel(hip["grads"], model)
        model16 = _model(g, b, lo, "16bit", bwd, hip)[1] if spill != "16bit" else model
        eff = _rel(model, model16)
        if twin is not None:
            h16 = _step(twin, b, lc, sc)
            assert np.array_equal(h16["sdf"], hip["sdf"]) and np.array_equal(h16["sdf_grad"], hip["sdf_grad"])
        else:
            h16 = hip
        _, lin = orc.loss_and_grads(*_oargs(g, b, lo), noise=b["noise"], adjoints_from=(h16["sdf"], h16["sdf_grad"]))
        e_twin = _rel(h16["grads"], lin)
        ceil = CEIL[(fwd == "bf16", bwd)]
        for k in e_model:
            bar = TWIN_FACTOR * (e_twin[k] + eff[k]) + TWIN_FLOOR
            assert e_model[k] <= bar, (N, k, e_model[k], e_twin[k], eff[k])
            assert e_twin[k] <= ceil and e_model[k] <= ceil + TWIN_FACTOR * eff[k], (N, k, e_model[k], e_twin[k], eff[k], ceil)
        terms, _ = orc.loss_and_grads(*_oargs(g, b, lo), noise=b["noise"])
        tol_loss = TOL_LOSS_BF16_SMALL if fwd == "bf16" and N < 1000 else TOL_LOSS[fwd]
        e_loss = _check_losses(hip, terms, tol_loss, N, lo, float(g["net"][4]))
        ratio = float("nan")
        if spill != "16bit" and N > 1000:     # the format was applied: HIP moves by about what the model says the format moves
            ratio = np.linalg.norm(_all(hip["grads"]) - _all(h16["grads"])) / np.linalg.norm(_all(model) - _all(model16))
            assert EFFECT_RATIO[0] <= ratio <= EFFECT_RATIO[1], (N, ratio)
        worst = max((v, k) for k, v in e_model.items())
        report.append("N=%d: vs model %.2e (%s), twin vs oracle %.2e, format effect %.2e, losses %.1e of bar, effect ratio %.2f"
                      % (N, worst[0], worst[1], max(e_twin.values()), max(eff.values()), e_loss / tol_loss, ratio))
    print(kernel, fix, fwd, bwd, spill, "|", "; ".join(report))


# ---- 2. invariants across formats ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fix", ["eval_full_ray", "eval_rs_franka", "eval_small_b3_f11"])
def test_formats_change_nothing_but_the_second_order_gradient(fix):
    g = _fixture(fix)
    b = _batch(g, min(111, g["z_vals"].shape[0]), 27)
    nf = int(g["net"][2])
    ep512 = 42 * nf + 3 > 256
    out = {}
    for w, name in ((1.0, "shipped"), (0.0, "no input-gradient terms")):
        lc, lo, sc = _cfgs(g, weight=w)
        res = {s: _step(_engine(g, "fp16x2", "fp16", s), b, lc, sc) for s in ("auto", "16bit", "e4m3", "e4m3_gb")}
        ref = res["16bit"]
        n = ref["n"]
        for s, h in res.items():
            for k in ("sdf", "sdf_grad", "tot"):
                assert np.array_equal(h[k], ref[k]), (name, s, k)
            assert torch.equal(h["red"][n:], ref["red"][n:]), (name, s, "loss sums / frame bins")
        resolved = "e4m3" if nf <= 6 else "16bit"
        assert torch.equal(res["auto"]["red"], res[resolved]["red"]), (name, "auto is not " + resolved)
        if w == 0.0:     # gbar = 0: GB = Ebar = 0 exactly, s_G = 1, the injected term is 0 -- the same MFMAs add the same values
            for s, h in res.items():
                for k, (off, shp) in _slices(fix).items():
                    a, r = h["red"][off:off + int(np.prod(shp))], ref["red"][off:off + int(np.prod(shp))]
                    if ep512 and s.startswith("e4m3") and k in ("in_layer.0.weight", "cat_layer.0.weight"):
                        # the embedding-rebuilding dW units of the e4m3 instantiations at EP = 512 take the run-time octave loop
                        # (dw.hip: straightRef is SP8 == 0 only), whose fill rounds ~15 % of the sine / cosine columns to the other
                        # neighbouring 16-bit value: measured rel-L2 1.1e-6, max 4e-8 absolute -- the same values, not the same bits
                        assert gu.rel_err(a.numpy(), r.numpy()) < 1e-5, (name, s, k)
                    else:
                        assert torch.equal(a, r), (name, s, k)
        out[name] = {s: max(_rel(h["grads"], ref["grads"]).values()) for s, h in res.items()}
    print(fix, "worst gradient tensor vs 16bit:", out)


# ---- 3. direction of the format's effect at BASELINE size --------------------------------------------------------------------
@pytest.mark.parametrize("fix", ["eval_base_680x1200_ray", "eval_rs_franka_offline"])
def test_e4m3_effect_tracks_the_model_at_baseline_size(fix):
    g = _fixture(fix)
    b = _batch(g, g["z_vals"].shape[0], g["z_vals"].shape[1])
    lc, lo, sc = _cfgs(g)
    h = {s: _step(_engine(g, "fp16x2", "fp16", s), b, lc, sc) for s in ("16bit", "e4m3", "e4m3_gb")}
    m = {s: _model(g, b, lo, s, "fp16", h["16bit"])[1] for s in h}
    rows = []
    for s in ("e4m3", "e4m3_gb"):
        for k in m[s]:
            dh = (h[s]["grads"][k] - h["16bit"]["grads"][k]).ravel()
            dm = (m[s][k] - m["16bit"][k]).ravel()
            if np.linalg.norm(dm) < 1e-6 * np.linalg.norm(m["16bit"][k]):
                continue        # (the format does not reach this tensor: out_alpha)
            cos = float(dh @ dm / (np.linalg.norm(dh) * np.linalg.norm(dm)))
            ratio = float(np.linalg.norm(dh) / np.linalg.norm(dm))
            rows.append((s, k, cos, ratio))
    for s, k, cos, ratio in rows:
        print("%s %-8s %-24s cos %.4f  |dHIP|/|dmodel| %.3f" % (fix, s, k, cos, ratio))
    for s, k, cos, ratio in rows:
        assert cos >= DIR_COS and DIR_RATIO[0] <= ratio <= DIR_RATIO[1], (s, k, cos, ratio)


# ---- 4. loss-weight sweep ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fix", ["eval_full_ray", "eval_rs_franka"])
@pytest.mark.parametrize("factor", [2.0 ** -10, 1.0, 2.0 ** 4])
def test_spill_formats_across_loss_weight_magnitudes(fix, factor):
    g = _fixture(fix)
    b = _batch(g, min(111, g["z_vals"].shape[0]), 27)
    lc, lo, sc = _cfgs(g, weight=factor)
    res = {}
    for s in ("16bit", "e4m3", "e4m3_gb"):
        hip = _step(_engine(g, "fp16x2", "fp16", s), b, lc, sc)
        assert all(np.isfinite(v).all() for v in hip["grads"].values()), s
        res[s] = (hip, _rel(hip["grads"], _model(g, b, lo, s, "fp16", hip)[1]))
    _, lin = orc.loss_and_grads(*_oargs(g, b, lo), noise=b["noise"], adjoints_from=(res["16bit"][0]["sdf"], res["16bit"][0]["sdf_grad"]))
    e_twin = _rel(res["16bit"][0]["grads"], lin)
    print(fix, "weights x %g:" % factor, {s: "%.2e" % max(e.values()) for s, (_, e) in res.items()}, "twin %.2e" % max(e_twin.values()))
    m16 = _model(g, b, lo, "16bit", "fp16", res["16bit"][0])[1]
    for s, (hip, e) in res.items():
        eff = _rel(_model(g, b, lo, s, "fp16", hip)[1], m16) if s != "16bit" else {k: 0.0 for k in e}
        for k in e:
            assert e[k] <= TWIN_FACTOR * (e_twin[k] + eff[k]) + TWIN_FLOOR, (s, k, e[k], e_twin[k], eff[k])


# ---- 5. trained weights --------------------------------------------------------------------------------------------------------
TOL_SIGNED, TOL_SIGNED_ALL = 6e-3, 5e-3       # test_gpu_parity.py: test_trained_weights_step_vs_reference
MODEL_OVER_ORACLE = 1.25
# HIP vs the model where the test holds HIP to the model (trained_franka, forced e4m3): measured worst tensor 8.5e-3 (in_layer.0.weight)
HM_TENSOR, HM_ALL = 1.5e-2, 1e-2


@pytest.mark.parametrize("fix,spill", [("trained_default", "16bit"), ("trained_default", "e4m3"), ("trained_franka", "e4m3")])
def test_trained_weights_spill_formats_vs_reference(fix, spill):
    """The signed-projection checks of test_trained_weights_step_vs_reference (a constant-sign bias that rel-L2 misses) per format.
    Where the model says the format costs more than the oracle bar (e4m3 at nine octaves and up), HIP is held to the model and its
    distance to the reference to MODEL_OVER_ORACLE x the model's."""
    g = gu.load(fix)
    lc, lo, sc = _cfgs(g)
    b = _batch(g, g["eval/pc"].shape[0], g["eval/pc"].shape[1], prefix="eval/")
    hip = _step(_engine(g, "fp16x2", "fp16", spill), b, lc, sc)
    names = list(gu.params_of(g))
    ref = gu.trained_eval_grads(g, names)
    _, model = _model(g, b, lo, spill, "fp16", hip)
    allg, allr, allm = [], [], []
    rows = {}
    for k in names:
        got, r, mm = hip["grads"][k].ravel(), ref[k].ravel(), model[k].ravel()
        rows[k] = (gu.rel_err(got, r), gu.signed_projection(got, r), gu.rel_err(mm, r), gu.rel_err(got, mm))
        allg.append(got); allr.append(r); allm.append(mm)
    allg, allr, allm = np.concatenate(allg), np.concatenate(allr), np.concatenate(allm)
    e_all, s_all, m_all = gu.rel_err(allg, allr), gu.signed_projection(allg, allr), gu.rel_err(allm, allr)
    print("%s %s: all rel-L2 %.3e signed %.2e (model vs reference %.3e)" % (fix, spill, e_all, s_all, m_all))
    for k, v in rows.items():
        print("  %-24s rel %.3e signed %+.2e  model vs ref %.3e  HIP vs model %.3e" % ((k,) + v))
    held_to_model = m_all > TOL_DW / 2
    e_hm = gu.rel_err(allg, allm)
    print("  all parameters: HIP vs model %.3e" % e_hm)
    for k, (e, s, em, ehm) in rows.items():
        if k == "out_alpha.bias":       # one number that nearly cancels at a trained state (test_trained_weights_step_vs_reference)
            continue
        assert abs(s) < TOL_SIGNED, (k, s)
        if held_to_model:
            assert e <= MODEL_OVER_ORACLE * em + 1e-3, (k, e, em)
            assert ehm <= HM_TENSOR, (k, ehm)
        else:
            assert e < TOL_DW, (k, e)
    assert abs(s_all) < TOL_SIGNED_ALL, s_all
    assert e_all <= (MODEL_OVER_ORACLE * m_all if held_to_model else TOL_DW), (e_all, m_all)
    if held_to_model:
        assert e_hm <= HM_ALL, e_hm
