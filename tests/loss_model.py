"""Per-point model of the chain kernel's loss stage (isdf_amd/csrc/chain.hip, `// loss + adjoints`) and of bounds_pc_kernel
(optim.hip) -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.  numpy only, no torch, no GPU.

`point_terms` is `oracle.isdf_oracle.loss_terms` / `loss_adjoints` in float64 ON THE KERNEL'S OWN fp32 INPUTS (its sdf, its d sdf/dx,
its bound, its target), per point, on the kernel's scale (loss SUMS: sbar and gbar carry no 1/N), with gbar' and s_G through
`spill_model.gbar_xprime` / `gb_scale`.  Next to every value it returns the bound on |kernel - model| derived below, and a flag for
the points whose BRANCH may legally differ.  `bounds_pc_f32` restates bounds_pc_kernel's fp32 arithmetic and gives its bounds and
nearest index bit for bit.

Error bounds (U = 2^-24, the unit roundoff of fp32; first order, the whole bound times 1 + 64 U for the higher orders).  chain.hip is
built with floating-point contraction allowed, so a product feeding a sum may or may not be rounded: every product and every sum is
counted as ONE rounding, which covers both forms.  Relative roundings by value, as the code is written:

  bnd   ray method: sqrtf(c0 c0 + c1 c1 + c2 c2) * (depth - z): 3 products + 2 sums = 5 under the root -> 2.5, sqrtf 1, the difference
        1 (relative to the difference: its operands are inputs), the product 1: K_BND = 6 (5.5 rounded up).  When every intermediate
        of every association is representable in fp32 (the hand-made batches) no rounding happens at all: band 0.
        pc method: the bound is an input (bounds_pc_kernel wrote it): band 0.
  gn    sqrtf(gx gx + gy gy + gz gz): 2.5 + 1 -> K_GN = 4;  inv = 1 / gn: 5;  n_i = g_i inv: 6
  v     truncation / free space with m1: sd - bnd: the band of bnd + U |v|.
        free space with m2 = __expf(-5 sd) - 1: E(sd) ex + U |m2|, E below
  sl    L1 |v|: d_v.  L2 v v: 2 |v| d_v + U v^2.  Truncation: times trunc_weight: trunc_weight * that + U sl
  cs    tn = max(sqrtf(t.t), 1e-6f): 4;  h_i = t_i / tn: 5;  g_i h_i: 6;  two sums: 8 U A on A = sum_i |g_i h_i| / gc;
        gc = max(gn, 1e-6f): 4 (or the constant's own rounding, 1), the division 1, one spare: d_cs = 8 U A + 6 U |cs|
  gl    1 - cs: d_cs + U |gl|;   orien_loss: 0 or 1, exact (a point with |cs| <= d_cs is flagged)
  ek    eik_weight |gn - 1|: eik_weight (K_GN U gn + U |gn - 1|) + U ek
  sbar  dsl/dv dv: dv = -5 ex on the exp branch ((E + U) |dv|), else 0 or 1 exactly.  L1: sign(v) dv: d_dv (either sign where
        |v| <= d_v).  L2: 2 v dv: 2 (|dv| d_v + |v| d_dv) + 2 U |sbar|.  Times trunc_weight in truncation, times scale_output: 2 U |sbar|
  tot   sl + grad_weight gl + ek: d_sl + grad_weight d_gl + U grad_weight gl + d_ek + 2 U tot (the terms are >= 0)
  gbar  normal term, gn > 1e-6: -k (h_i - cs n_i), k = grad_weight / gc (6):
            k (5 U |h_i| + d_cs |n_i| + 7 U |cs n_i| + U |h_i - cs n_i|) + 7 U |k (h_i - cs n_i)|
        gn <= 1e-6: -k h_i: 12 U |k h_i|   (at gn = 0: gbar = -(grad_weight / 1e-6) h, what CosineSimilarity(eps=1e-6) gives)
        eikonal term eik_weight sign(gn - 1) n_i: 8 U |term|;  the two accumulations: 2 U (|normal term| + |eikonal term|)
  gbar' si (T_i0 b_0 + T_i1 b_1 + T_i2 b_2): si sum_j |T_ij| d_b_j + 4 U si sum_j |T_ij b_j|
  s_G   an exponent-field rule of the kernel's own gbar': bit for bit (spill_model.gb_scale), no bound

__expf.  The ISA guide this project works from states NO accuracy for v_exp_f32.  For that case the bound is
taken from numpy: EXP_HW_REL = 4 x the worst relative error of numpy's fp32 exp against float64 over the tested range |sd| <= SD_MAX
-- a number NOT measured on the device -- plus the rounding of the scaled argument: -5 sd (1), times log2(e) (1, and the
constant's own 1) = 3 U |5 sd| absolute on the argument, the same relatively on the result:  E(sd) = EXP_HW_REL + 3 U |5 sd|.
exp(-5 * 0) is taken to be exactly 1 (2^0).

Flags (a flagged point may take either branch's value: `alternatives` gives the model at the four corners of the bands):
bnd within its band of trunc_distance or eik_apply_dist; gn within K_GN U gn of 1 or (+ U 1e-6 for the constant) of 1e-6; in free
space |m1 - m2| within the sum of their errors; with orien_loss |cs| <= d_cs.  A band of 0 flags nothing.
"""
import numpy as np

import oracle.isdf_oracle as orc
from tests import spill_model as sm

U32 = 2.0 ** -24
K_BND, K_GN = 6, 4
SD_MAX = 2.0
HIGHER = 1.0 + 64 * U32


def f32(x):
    return np.asarray(x, np.float32)


def f64(x):
    return np.asarray(x, np.float64)


def _repr32(x):
    """x (float64) is an fp32 value"""
    x = f64(x)
    with np.errstate(over="ignore"):
        return x.astype(np.float32).astype(np.float64) == x


def exp_hw_rel():
    """EXP_HW_REL: 4 x numpy's fp32 exp against float64 over |x| <= 5 SD_MAX (see the module docstring; not a device measurement)"""
    global _EXP_HW
    if _EXP_HW is None:
        x = np.linspace(-5 * SD_MAX, 5 * SD_MAX, 1 << 18).astype(np.float32)
        ref = np.exp(x.astype(np.float64))
        _EXP_HW = 4.0 * float(np.max(np.abs(np.exp(x).astype(np.float64) - ref) / ref))
    return _EXP_HW


_EXP_HW = None


def exp_rel(sd):
    return exp_hw_rel() + 3 * U32 * np.abs(5.0 * f64(sd))


def lc32(lc):
    """the loss configuration as the kernel holds it: every float an fp32 value"""
    r = lambda v: float(np.float32(v))
    return orc.LossCfg(lc.bounds_method, lc.loss_type, r(lc.trunc_weight), r(lc.trunc_distance), r(lc.eik_weight),
                       r(lc.eik_apply_dist), r(lc.grad_weight), bool(lc.orien_loss))


def cfg32(cfg):
    T = None if cfg.transform is None else f64(f32(cfg.transform))
    return orc.NetCfg(cfg.H, cfg.B, cfg.n_freqs, float(np.float32(cfg.scale_input)), float(np.float32(cfg.scale_output)), T)


# ---- bounds ----------------------------------------------------------------------------------------------------------------------
def bound_ray_f32(depth, z, dirs_C, lc):
    """bounds_method "ray": |dirs_C| (depth - z) of fp32 inputs -> (bnd fp32 [R,S], band float64 [R,S], near bool [R,S]).
    band: how far the kernel's fp32 value may sit from the float64 one under any legal association / contraction (0 where every
    intermediate is an fp32 value); near: bnd within a non-zero band of trunc_distance or eik_apply_dist."""
    l = lc32(lc)
    c, d, zz = f64(f32(dirs_C)), f64(f32(depth))[:, None], f64(f32(z))
    sq = c * c
    n2 = sq.sum(-1)
    nrm = np.sqrt(n2)
    parts = [sq[:, 0], sq[:, 1], sq[:, 2], sq[:, 0] + sq[:, 1], sq[:, 1] + sq[:, 2], sq[:, 0] + sq[:, 2], n2, nrm]
    with np.errstate(invalid="ignore"):
        ray_exact = np.all([_repr32(p) for p in parts], 0) & (nrm * nrm == n2)
        q = d - zz
        b64 = nrm[:, None] * q
        exact = ray_exact[:, None] & _repr32(q) & _repr32(b64)
        band = np.where(exact, 0.0, K_BND * U32 * np.abs(b64))
        near = (band > 0) & ((np.abs(b64 - l.trunc_distance) <= band) | (np.abs(b64 - l.eik_apply_dist) <= band))
    return b64.astype(np.float32), band, near


def bounds_pc_f32(pc, z, depth, surf=None):
    """bounds_pc_kernel: fp32 squared distances in its operation order ((dx dx + dy dy) + dz dz, every product and sum rounded),
    the FIRST minimum in index order, sqrtf, the sign by z > depth -> (bounds fp32 [R,S], grad_vec float64 [R,S,3], nearest index
    [R,S]).  grad_vec is the float64 unit vector of the fp32 difference to the nearest surface point (NaN where that is 0 / 0):
    the kernel normalises it in contractible fp32, |kernel - this| <= GRAD_VEC_K U per component (norm 2.5 + 1, division 1, one spare)."""
    pc, z, depth = f32(pc), f32(z), f32(depth)
    R, S = z.shape
    sp = pc[:, 0] if surf is None else f32(surf)
    p = pc.reshape(-1, 3)
    best = np.full(p.shape[0], np.inf, np.float32)
    bi = np.zeros(p.shape[0], np.int64)
    with np.errstate(over="ignore"):
        for r0 in range(0, sp.shape[0], 1024):
            blk = sp[r0:r0 + 1024]
            dx = p[:, None, 0] - blk[None, :, 0]
            dy = p[:, None, 1] - blk[None, :, 1]
            dz = p[:, None, 2] - blk[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz                     # float32 arrays: every operation rounds once
            k = d2.argmin(-1)                                      # (first minimum)
            m = d2[np.arange(p.shape[0]), k]
            upd = m < best                                         # strict: an earlier block's equal distance stays
            best[upd], bi[upd] = m[upd], r0 + k[upd]
    dist = np.sqrt(best)                                           # fp32 sqrt, correctly rounded
    behind = (z > depth[:, None]).reshape(-1)
    bounds = np.where(behind, -dist, dist).astype(np.float32)
    g = (p - sp[bi]).astype(np.float64)                            # the fp32 difference, then float64
    with np.errstate(invalid="ignore", divide="ignore"):
        g = g / np.sqrt((g * g).sum(-1))[:, None]
    g = np.where(behind[:, None], -g, g)
    return bounds.reshape(R, S), g.reshape(R, S, 3), bi.reshape(R, S)


GRAD_VEC_K = 6


# ---- the loss stage --------------------------------------------------------------------------------------------------------------
def point_terms(sdf32, grad32, bnd32, target32, normal32, s, lc, cfg, bnd_band=None):
    """sdf32, bnd32 [R,S]; grad32, target32 [R,S,3] (the target of sample 0 is not read); normal32 [R,3]; s [R,S] the sample index
    of each point (must be the column index: the rule `s == 0` is the oracle's `[:, 0]`); lc a LossCfg / LossConfig; cfg the net's
    NetCfg (scale_input, transform, n_freqs); bnd_band: bound_ray_f32's band (None: the bound is an input, band 0).
    -> dict of float64 arrays on the kernel's scale: sl, gl, ek, tot, sbar [R,S]; gbar, gbar_x [R,S,3]; sG [R,S]; label, target_kind
    [R,S] of str; eik_on, flag [R,S] of bool; d_sl, d_gl, d_ek, d_tot, d_sbar [R,S] and d_gbar_x [R,S,3]: the bounds of the module docstring."""
    l, c = lc32(lc), cfg32(cfg)
    sd, g, bnd, nrm = f64(f32(sdf32)), f64(f32(grad32)), f64(f32(bnd32)), f64(f32(normal32))
    tgt = f64(f32(target32))
    R, S = sd.shape
    assert np.array_equal(np.broadcast_to(np.asarray(s), (R, S)), np.broadcast_to(np.arange(S), (R, S)))
    N = R * S
    band = np.zeros((R, S)) if bnd_band is None else f64(bnd_band)
    gv, ns = tgt[:, 1:], nrm          # the oracle's grad_vec [R,S-1,3] / norm_sample: sample 0 and NaN targets take the normal
    with np.errstate(over="ignore", invalid="ignore"):
        t = orc.loss_terms(sd, g, bnd, gv, ns, l)
        sbar, gbar = orc.loss_adjoints(sd, g, bnd, gv, ns, l)
    sbar, gbar = sbar * N, gbar * N
    zero = np.zeros((R, S))
    out = dict(sl=t["sdf_loss_mat"], gl=t.get("grad_loss_mat", zero), ek=t.get("eik_loss_mat", zero), tot=t["tot_loss_mat"],
               sbar=sbar, gbar=gbar)
    out["gbar_x"] = sm.gbar_xprime(gbar.reshape(-1, 3), c).reshape(R, S, 3)
    out["sG"] = sm.gb_scale(np.abs(out["gbar_x"].astype(np.float32)).max(-1), c.n_freqs)

    # ---- classes
    free = t["free"]
    with np.errstate(over="ignore"):
        ex = np.exp(-5.0 * sd)
    m1, m2 = np.maximum(sd - bnd, 0.0), ex - 1.0
    expb = free & ~(m1 >= m2)
    label = np.where(free, np.where(expb, "free:exp", np.where(sd > bnd, "free:sd>bnd", "free:v=0")),
                     np.where(sd < bnd, "trunc:sd<bnd", np.where(sd > bnd, "trunc:sd>bnd", "trunc:sd=bnd")))
    out["label"] = label
    nan_t = np.isnan(tgt[..., 0])
    kind = np.where(nan_t, "normal(nan)", "given")
    kind[:, 0] = "normal"
    out["target_kind"] = kind
    out["eik_on"] = (bnd >= l.eik_apply_dist) if l.eik_weight != 0 else np.zeros((R, S), bool)

    # ---- bounds
    U = U32
    E = exp_rel(sd)
    vabs = np.where(expb, np.abs(m2), np.abs(sd - bnd))
    vabs = np.where(free & ~expb, m1, vabs)
    d_v = np.where(expb, E * ex + U * np.abs(m2), band + U * np.abs(sd - bnd))
    d_raw = d_v if l.loss_type == "L1" else 2 * vabs * d_v + U * vabs * vabs
    d_sl = np.where(free, d_raw, l.trunc_weight * d_raw + U * out["sl"])
    # sbar = dsl/dv dv (so): dv = -5 ex on the exp branch ((E + U) |dv|), else 0 or 1; L1's sign(v) is either sign where |v| <= d_v
    dv_abs = np.where(expb, 5.0 * ex, 1.0)
    d_dv = np.where(expb, (E + U) * 5.0 * ex, 0.0)
    d_sb = d_dv if l.loss_type == "L1" else 2 * (dv_abs * d_v + vabs * d_dv) + 2 * U * np.abs(sbar)
    if l.loss_type == "L1":
        d_sb = np.where((d_v > 0) & (vabs <= d_v), 2 * np.abs(dv_abs) * np.where(free, 1.0, l.trunc_weight), d_sb)
    out["d_sbar"] = (np.where(free, d_sb, l.trunc_weight * d_sb) + 2 * U * np.abs(sbar)) * HIGHER
    gn = np.sqrt((g * g).sum(-1))
    d_gn = K_GN * U * gn
    gc = np.maximum(gn, 1e-6)
    hh = np.concatenate((np.broadcast_to(nrm[:, None, :], (R, 1, 3)), np.where(nan_t[:, 1:, None], nrm[:, None, :], tgt[:, 1:])), 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        h = hh / np.maximum(np.sqrt((hh * hh).sum(-1, keepdims=True)), 1e-6)
        n = np.where(gn[..., None] > 0, g / gn[..., None], 0.0)
    cs = (g * h).sum(-1) / gc
    d_cs = 8 * U * np.abs(g * h).sum(-1) / gc + 6 * U * np.abs(cs)
    d_gl = zero
    if l.grad_weight != 0:
        d_gl = zero if l.orien_loss else d_cs + U * np.abs(out["gl"])
    d_ek = zero
    if l.eik_weight != 0:
        d_ek = np.where(out["eik_on"], l.eik_weight * (d_gn + U * np.abs(gn - 1.0)) + U * out["ek"], 0.0)
    out["d_sl"], out["d_gl"], out["d_ek"] = d_sl * HIGHER, d_gl * HIGHER, d_ek * HIGHER
    out["d_tot"] = (d_sl + l.grad_weight * d_gl + U * l.grad_weight * out["gl"] + d_ek + 2 * U * out["tot"]) * HIGHER
    d_b = np.zeros((R, S, 3))
    a_norm, a_eik = np.zeros((R, S, 3)), np.zeros((R, S, 3))
    if l.grad_weight != 0 and not l.orien_loss:
        k = (l.grad_weight / gc)[..., None]
        w = h - cs[..., None] * n
        big = k * (5 * U * np.abs(h) + d_cs[..., None] * np.abs(n) + 7 * U * np.abs(cs[..., None] * n) + U * np.abs(w)) + 7 * U * np.abs(k * w)
        small = 12 * U * np.abs(k * h)
        d_b = d_b + np.where(gn[..., None] > 1e-6, big, small)
        a_norm = np.where(gn[..., None] > 1e-6, np.abs(k * w), np.abs(k * h))
    if l.eik_weight != 0:
        a_eik = np.where(out["eik_on"][..., None], np.abs(l.eik_weight * n), 0.0)
        d_b = d_b + 8 * U * a_eik
    d_b = d_b + 2 * U * (a_norm + a_eik)
    Rm = np.eye(3) if c.transform is None else c.transform[:3, :3]
    out["d_gbar_x"] = c.scale_input * (d_b @ np.abs(Rm).T + 4 * U * (np.abs(gbar) @ np.abs(Rm).T)) * HIGHER

    # ---- flags
    thr = lambda x, v, b: (b > 0) & (np.abs(x - v) <= b)
    flag = thr(bnd, l.trunc_distance, band)
    if l.eik_weight != 0:
        flag = flag | thr(bnd, l.eik_apply_dist, band) | thr(gn, 1.0, d_gn)
    if l.grad_weight != 0:
        flag = flag | ((d_gn > 0) & (np.abs(gn - 1e-6) <= d_gn + U * 1e-6))
        if l.orien_loss:
            flag = flag | ((d_cs > 0) & (np.abs(cs) <= d_cs))
    d_m1 = band + U * np.abs(sd - bnd)
    d_m1 = np.where(sd - bnd < -d_m1, 0.0, d_m1)              # clamped: m1 is exactly 0
    d_m2 = np.where(sd == 0, 0.0, E * ex + U * np.abs(m2))
    flag = flag | (free & (d_m1 + d_m2 > 0) & (np.abs(m1 - m2) <= d_m1 + d_m2))
    out["flag"] = flag
    return out


def alternatives(sdf32, grad32, bnd32, target32, normal32, s, lc, cfg, bnd_band=None):
    """point_terms at the four corners (bound -+ its band, gradient scaled by 1 -+ 2 K_GN U): a flagged point must agree with
    the model or one of these -- it took the other side of a border its inputs sit on"""
    band = np.zeros(np.shape(bnd32)) if bnd_band is None else f64(bnd_band)
    outs = []
    for sb in (-1.0, 1.0):
        for sg in (-1.0, 1.0):
            b = (f64(f32(bnd32)) + sb * 2 * band).astype(np.float32)
            g = (f64(f32(grad32)) * (1.0 + sg * 2 * K_GN * U32)).astype(np.float32)
            outs.append(point_terms(sdf32, g, b, target32, normal32, s, lc, cfg, bnd_band))
    return outs


def ray_inputs(b, lc):
    """a batch dict (tests/loss_cases.py) under bounds_method "ray" -> (bnd fp32, band, near, target [R,S,3] = -dirs_W)"""
    bnd, band, near = bound_ray_f32(b["depth_sample"], b["z_vals"], b["dirs_C_sample"], lc)
    R, S = b["z_vals"].shape
    return bnd, band, near, np.broadcast_to(-f32(b["dirs_W_sample"])[:, None, :], (R, S, 3))


def sample_index(R, S):
    return np.broadcast_to(np.arange(S), (R, S))
