"""Float64 model of the training step's spill formats -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

`isdf_net_cfg.spill_operand` (include/isdf_hip.h) decides how the chain kernel parks two tensor families in HBM: P_l = d sdf / d z_l
(first reverse sweep) and GB_l = the adjoint entering layer l in the upward sweep (GB_l = qb_{l-1}, l >= 1; the oracle's `Gb` without
its embedding part).  This module is `oracle.isdf_oracle.loss_and_grads` in float64 with P and GB rounded to the spill format exactly
where the kernels consume the SPILLED copy, and nowhere else:

  * dW kernel (dw.hip), odd stages: P_l^T GB_l for every layer.  P_l is read from the spill for every l (the top layer's P stays
    16-bit in every format: SpillLayout); GB_l is read for l >= 1 (layer 0's Ebar and the embedding columns of the cat layer are
    rebuilt from pe_aux in the 16-bit operand type -- exact here).  An e4m3 tensor is decoded straight to that 16-bit type
    (v_cvt_scalef32_pk_f16_fp8 / _bf16_fp8: e4m3 * scale, then one 16-bit rounding).
  * chain kernel, reverse sweep: the injected term of layer l <= L-2, beta GB_{l+1} P_l (1 - sigma') / sigma', is rebuilt from
    P_l (spill) and GB_{l+1} (spill, decoded to fp32) -- except at l = L-2, whose GB_{L-1} comes back from the copy the adjoint sweep
    parked in LDS in the 16-bit spill type whatever the format.  The top layer's injected term never leaves registers (exact).
  * Everything the sweeps keep on chip -- the 16-bit LDS operand copies of P and GB feeding the next GEMM, A, ZB, the weights -- and
    every other operand stays exact: "HIP vs this model" is then the kernels' own 16-bit operand floor, "this model vs the oracle"
    the cost of the format.

Formats (`fmt`): "exact" (= the oracle), "16bit" (P and GB in the `bwd` type: fp16 or bf16), "e4m3" (P below the top layer and GB
in OCP e4m3fn), "e4m3_gb" (GB only).  e4m3 encodes P / 2^-10 and GB / s_G[point] with
    s_G = 2^(floor(log2 |gbar'|_inf) + 1 + spill_gb_shift(n_freqs)),  spill_gb_shift(n) = n - 7 for n > 6, else -1,
gbar' = the point's loss adjoint of d sdf / dx in x' space (scale_input * R gbar), and s_G = 1 when |gbar'|_inf is 0, below 2^-100
or at least 2^73 (chain.hip's loss stage, fp32 exponent field).  Conversions saturate at +-448 (MODE.FP16_OVFL).

The kernel works on loss SUMS (its gbar / sbar carry no 1 / N; the host divides the reduced gradient), and s_G and every 16-bit
rounding are taken on that scale: the model runs the backward on it too and divides by N at the end.
"""
import numpy as np

import oracle.isdf_oracle as orc

P_SCALE = 2.0 ** -10          # chain.hip / dw.hip kSpillPScale
E4M3_MAX = 448.0
FORMATS = ("exact", "16bit", "e4m3", "e4m3_gb")
_SPEC = {"e4m3": (3, -6, E4M3_MAX), "fp16": (10, -14, 65504.0), "bf16": (7, -126, 3.3895313892515355e38)}


def round_to(x, fmt):
    """x (float64) rounded to `fmt` ("e4m3", "fp16", "bf16"): round to nearest even, gradual underflow, and saturation at the
    largest finite value (the kernel's e4m3 conversion saturates at +-448; the 16-bit ones never get there on this path)."""
    mant, emin, vmax = _SPEC[fmt]
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)                                    # |x| = f 2^e, f in [0.5, 1): floor(log2 |x|) = e - 1
    q = np.ldexp(1.0, np.maximum(e - 1, emin) - mant)     # the quantum at x's binade (subnormal quantum below 2^emin)
    with np.errstate(invalid="ignore"):
        r = np.rint(x / q) * q                            # x / q and r are exact in float64; rint ties to even
    return np.clip(r, -vmax, vmax)


def spill_gb_shift(n_freqs):
    """isdf_common.h spill_gb_shift"""
    return n_freqs - 7 if n_freqs > 6 else -1


def gb_scale(gmax, n_freqs):
    """s_G of points whose |gbar'|_inf (fp32, kernel scale) is `gmax` -> float64 array (chain.hip's loss stage)"""
    g = np.abs(np.asarray(gmax, np.float32)).astype(np.float64)
    _, e = np.frexp(g)
    ok = (g >= 2.0 ** -100) & (g < 2.0 ** 73)
    return np.where(ok, np.ldexp(1.0, e - 1 + 1 + spill_gb_shift(n_freqs)), 1.0)


def gbar_xprime(gbar, cfg):
    """the per-point loss adjoint of d sdf / dx in x' space: scale_input * R gbar ([P,3] -> [P,3])"""
    R = np.eye(3) if cfg.transform is None else np.asarray(cfg.transform, np.float64)[:3, :3]
    return cfg.scale_input * (np.asarray(gbar, np.float64) @ R.T)


class Spill:
    """How one format stores / decodes P and GB.  All arrays are on the kernel's (loss-sum) scale."""

    def __init__(self, fmt, bwd="fp16"):
        assert fmt in FORMATS and bwd in ("fp16", "bf16")
        assert not (fmt.startswith("e4m3") and bwd != "fp16"), "the e4m3 formats go with fp16 second-order sweeps"
        self.fmt, self.bwd = fmt, bwd
        self.p8, self.g8 = fmt == "e4m3", fmt in ("e4m3", "e4m3_gb")

    def r16(self, v):
        return v if self.fmt == "exact" else round_to(v, self.bwd)

    def p_spilled(self, p, top):
        """P as the spill holds it, decoded to fp32"""
        if self.p8 and not top:
            return round_to(p / P_SCALE, "e4m3") * P_SCALE
        return self.r16(p)

    def g_spilled(self, gb, sG):
        if self.g8:
            return round_to(gb / sG[:, None], "e4m3") * sG[:, None]
        return self.r16(gb)

    def p_dw(self, p, top):         # dW operand: the spilled value in the 16-bit operand type
        return self.r16(self.p_spilled(p, top))

    def g_dw(self, gb, sG):
        return self.r16(self.g_spilled(gb, sG))


def loss_and_grads(params, cfg, lc, pc, z_vals, depth_sample, dirs_C_sample, T_WC_sample, norm_sample, noise=None,
                   fmt="e4m3", bwd="fp16", adjoints_from=None, want_intermediates=False):
    """`oracle.isdf_oracle.loss_and_grads` in float64 with the spill format `fmt` (see the module docstring).  Arguments as there;
    returns (terms, grads) with grads divided by N like the oracle's.  want_intermediates adds terms["P"] (per layer, [N,H]),
    terms["GB"] (index l >= 1: GB_l, [N,H]; kernel scale), terms["gx"] (gbar' [N,3], kernel scale), terms["sG"] ([N]) and terms["N"]."""
    sp = Spill(fmt, bwd)
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)
    params = {k: f64(v) for k, v in params.items()}
    cfg = orc.NetCfg(cfg.H, cfg.B, cfg.n_freqs, cfg.scale_input, cfg.scale_output, f64(cfg.transform))
    pc, z_vals, depth_sample, dirs_C_sample, T_WC_sample, norm_sample, noise = map(
        f64, (pc, z_vals, depth_sample, dirs_C_sample, T_WC_sample, norm_sample, noise))
    R, S = z_vals.shape
    N = R * S
    x = pc.reshape(-1, 3)
    L = len(cfg.names)
    so = cfg.scale_output
    do_grad = lc.eik_weight != 0 or lc.grad_weight != 0

    emb, I, Z, A, raw = orc._forward_cache(params, cfg, x)
    if noise is not None:
        raw = raw + noise.reshape(-1)
    sdf = (raw * so).reshape(R, S)
    Q, Pm, S1, Eg = orc._input_grad_cache(params, cfg, x, Z)
    sdf_grad = orc.pe_vjp(x, Eg, cfg.transform, cfg.scale_input, cfg.n_freqs).reshape(R, S, 3) if do_grad else None
    if lc.bounds_method == "ray":
        bounds, grad_vec = orc.bounds_ray(depth_sample, z_vals, dirs_C_sample, T_WC_sample)
    else:
        bounds, grad_vec = orc.bounds_pc(pc, z_vals, depth_sample)
    terms = orc.loss_terms(sdf, sdf_grad, bounds, grad_vec, norm_sample, lc)
    terms.update(sdf=sdf, sdf_grad=sdf_grad, bounds=bounds)
    adj_sdf, adj_grad = sdf, sdf_grad
    if adjoints_from is not None:
        adj_sdf = f64(adjoints_from[0]).reshape(R, S)
        adj_grad = None if adjoints_from[1] is None else f64(adjoints_from[1]).reshape(R, S, 3)
    sbar, gbar = orc.loss_adjoints(adj_sdf, adj_grad if do_grad else np.zeros((R, S, 3)), bounds, grad_vec, norm_sample, lc)
    sbar, gbar = sbar.reshape(-1) * N, gbar.reshape(-1, 3) * N          # the kernel's (loss-sum) scale
    gx = gbar_xprime(gbar, cfg)
    sG = gb_scale(np.abs(gx.astype(np.float32)).max(-1), cfg.n_freqs)

    grads, inj, GB = {}, [None] * L, [None] * L
    W = [params[n + ".weight"] for n in cfg.names]
    d_wout = (sbar * so) @ A[-1]
    if do_grad:
        Eb = orc.pe_jvp(x, gbar, cfg.transform, cfg.scale_input, cfg.n_freqs)
        qb = None
        for li, n in enumerate(cfg.names):
            top = li == L - 1
            if li == 0:
                Gb, Gb_dw = Eb, Eb
            else:
                GB[li] = qb
                g_dw = sp.g_dw(qb, sG)
                Gb = np.concatenate([qb, Eb], -1) if li == cfg.cat else qb
                Gb_dw = np.concatenate([g_dw, Eb], -1) if li == cfg.cat else g_dw
            u = Gb @ W[li].T
            grads[n + ".weight"] = sp.p_dw(Pm[li], top).T @ Gb_dw
            qb = u * S1[li]
            if top:
                inj[li] = u * Q[li] * orc.softplus_d2(Z[li])
            else:
                # beta GB_{l+1} P_l (1 - sigma') / sigma' from the spilled copies (GB_{L-1}: the 16-bit copy parked in LDS)
                g = sp.r16(qb) if li == L - 2 else sp.g_spilled(qb, sG)
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = np.where(S1[li] > 0, (1.0 - S1[li]) / S1[li], 0.0)
                inj[li] = orc.SOFTPLUS_BETA * g * sp.p_spilled(Pm[li], False) * ratio
        d_wout = d_wout + so * qb.sum(0)
    ab = (sbar * so)[:, None] * params["out_alpha.weight"]
    for li in range(L - 1, -1, -1):
        n = cfg.names[li]
        zb = ab * S1[li]
        if inj[li] is not None:
            zb = zb + inj[li]
        gW = zb.T @ I[li]
        grads[n + ".weight"] = grads[n + ".weight"] + gW if n + ".weight" in grads else gW
        grads[n + ".bias"] = zb.sum(0)
        if li > 0:
            ab = (zb @ W[li])[:, :cfg.H]
    grads["out_alpha.weight"] = d_wout[None, :]
    grads["out_alpha.bias"] = np.array([(sbar * so).sum()])
    grads = {k: v / N for k, v in grads.items()}
    if want_intermediates:
        terms.update(P=Pm, GB=GB, gx=gx, sG=sG, N=N)
    return terms, grads


def headroom(P, GB, sG):
    """(max |P_l| / 2^-10 over the layers below the top one, max |GB_l| / s_G over l >= 1): where the e4m3 codes of a batch sit
    against the format's 448"""
    hp = max(float(np.abs(p).max()) for p in P[:-1]) / P_SCALE
    hg = max(float((np.abs(g) / sG[:, None]).max()) for g in GB[1:])
    return hp, hg
