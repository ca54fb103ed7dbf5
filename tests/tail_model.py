"""Exact models of the step tail (isdf_amd/csrc/optim.hip: finalize_block, frame_avg_block, adamw_update) in numpy.

The bins and the frame averages are integer and fp32 arithmetic with a fixed order, so `bins` and `frame_avg` give the kernels'
values BIT FOR BIT.  `adamw` is the float64 value of torch.optim.AdamW's formula on the fp32 inputs the kernel sees; `adamw_bound`
is the forward-error bound of the kernel's fp32 evaluation of it.  No torch, no GPU.
"""
import re

import numpy as np

U32 = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)


# ---- constants of optim.hip -----------------------------------------------------------------------------------------------------
def kernel_constants(optim_src, common_src):
    """The constants the GPU cases are built from, read from the kernel source; a changed form raises (the CPU test fails)."""
    def one(pat, src, what):
        m = re.search(pat, src)
        if not m:
            raise AssertionError("optim.hip / isdf_common.h changed form: " + what)
        return [int(v) for v in m.groups()]
    c = {}
    c["FIN_CAP"], = one(r"constexpr\s+int\s+FIN_CAP\s*=\s*(\d+)\s*;", optim_src, "FIN_CAP")
    c["LOSS_STRIDE"], = one(r"for\s*\(int64_t\s+t\s*=\s*tid;\s*t\s*<\s*nTiles\s*&&\s*t\s*<\s*maxTiles;\s*t\s*\+=\s*(\d+)\)", optim_src,
                            "block 0's loss-partial loop")
    c["TAIL_THREADS"], = one(r"__launch_bounds__\((\d+)\)\s*void\s+step_tail_kernel", optim_src, "step_tail_kernel's launch bounds")
    c["L1_LOOK"], c["L1_STEP"] = one(r"for\s*\(;\s*t\s*\+\s*(\d+)\s*<\s*nTiles;\s*t\s*\+=\s*(\d+)\)\s*\{\s*//\s*8", optim_src, "first unrolled loop")
    c["L2_LOOK"], c["L2_STEP"] = one(r"for\s*\(;\s*t\s*\+\s*(\d+)\s*<\s*nTiles;\s*t\s*\+=\s*(\d+)\)\s*\{\s*//\s*4", optim_src, "second unrolled loop")
    c["L3_STEP"], = one(r"for\s*\(;\s*t\s*<\s*nTiles;\s*t\s*\+=\s*(\d+)\)\s*\{", optim_src, "remainder loop")
    c["GROUPS"], = one(r"for\s*\(int\s+k\s*=\s*0;\s*k\s*<\s*(\d+);\s*\+\+k\)\s*t\s*\+=\s*sh\[k\]\[pi\]", optim_src, "the group sum")
    c["TILE_PTS"], = one(r"constexpr\s+int\s+TILE_PTS\s*=\s*(\d+)\s*;", common_src, "TILE_PTS")
    c["DW_SPLIT_REG"], c["DW_SPLIT_PE"] = one(r"constexpr\s+int\s+DW_SPLIT_REG\s*=\s*(\d+)\s*,\s*DW_SPLIT_PE\s*=\s*(\d+)", common_src, "DW_SPLIT_*")
    return c


def loop_mix(n_tiles, g, c):
    """(iterations of loop 1, of loop 2, of the remainder loop) that thread group g runs at n_tiles: the vector section's control flow"""
    t, n1, n2, n3 = g, 0, 0, 0
    while t + c["L1_LOOK"] < n_tiles:
        t += c["L1_STEP"]; n1 += 1
    while t + c["L2_LOOK"] < n_tiles:
        t += c["L2_STEP"]; n2 += 1
    while t < n_tiles:
        t += c["L3_STEP"]; n3 += 1
    return n1, n2, n3


def tiles_of_group(n_tiles, g, c):
    """the tiles thread group g must add, whatever the loops: g, g + 16, ..."""
    return list(range(g, n_tiles, c["GROUPS"]))


def vec_chain_length(n_tiles, c):
    """fp32 additions on the longest chain from a tile's partial to a bias / w_out gradient element: per loop-1 iteration the
    three-level tree of 8 loads (3) + the accumulation (1); per loop-2 iteration (2) + 1; one per remainder tile; `s += s2` (w_out has
    two slots) 1; the 16-group sum 16 (it starts from 0.f)."""
    d = 0
    for g in range(c["GROUPS"]):
        n1, n2, n3 = loop_mix(n_tiles, g, c)
        d = max(d, 4 * n1 + 3 * n2 + n3)
    return d + 1 + c["GROUPS"]


def loss_chain_length(n_tiles, c):
    """fp32 additions on the longest chain of block 0's loss sum: ceil(n_tiles / stride) per thread, 6 butterfly stages, 16 waves"""
    return -(-n_tiles // c["LOSS_STRIDE"]) + 6 + c["TAIL_THREADS"] // 64


# ---- bins -----------------------------------------------------------------------------------------------------------------------
def ray_sums(tot):
    """total_loss_mat.sum(-1) as the kernel takes it: sequential fp32 over the S samples"""
    tot = np.asarray(tot, np.float32)
    s = np.zeros(tot.shape[0], np.float32)
    for k in range(tot.shape[1]):
        s = (s + tot[:, k]).astype(np.float32)
    return s


def kept_rays(indices_b, indices_h, indices_w, R, H, W, keep="last"):
    """indices of the rays that survive the duplicate rule: per (frame, h, w) the ray with the HIGHEST index (`keep="first"`: the
    lowest -- a mutant)"""
    b, h, w = (np.asarray(a, np.int64)[:R] for a in (indices_b, indices_h, indices_w))
    key = (b * H + h) * W + w
    if keep == "last":
        _, first = np.unique(key[::-1], return_index=True)
        return np.sort(R - 1 - first)
    _, first = np.unique(key, return_index=True)
    return np.sort(first)


def bins(tot_loss_mat, indices_b, indices_h, indices_w, R, F, H, W, keep="last", count_all=False):
    """(block_loss [F, 64] f32, block_cnt [F, 64] f32) of finalize_block.  `keep` / `count_all` select mutants of the rule."""
    assert H % 8 == 0 and W % 8 == 0, "the reference's view(-1, 8, H // 8, 8, W // 8) needs it as well"
    s = ray_sums(np.asarray(tot_loss_mat, np.float32)[:R])
    fixed = np.rint(s.astype(np.float64) * 4294967296.0).astype(np.int64)          # 32.32 fixed point (llrint)
    b, h, w = (np.asarray(a, np.int64)[:R] for a in (indices_b, indices_h, indices_w))
    kept = kept_rays(b, h, w, R, H, W, keep)
    slot = b * 64 + (h // (H // 8)) * 8 + w // (W // 8)
    acc = np.zeros(F * 64, np.int64)
    np.add.at(acc, slot[kept], fixed[kept])
    cnt = np.zeros(F * 64, np.int64)
    np.add.at(cnt, slot if count_all else slot[kept], 1)
    block_loss = (acc.astype(np.float64) * (1.0 / 4294967296.0)).astype(np.float32)
    return block_loss.reshape(F, 64), cnt.astype(np.float32).reshape(F, 64)


def bins_fp32_ray_order(tot_loss_mat, indices_b, indices_h, indices_w, R, F, H, W):
    """mutant: no fixed point, the kept rays added to their bin in fp32 in ray order"""
    s = ray_sums(np.asarray(tot_loss_mat, np.float32)[:R])
    b, h, w = (np.asarray(a, np.int64)[:R] for a in (indices_b, indices_h, indices_w))
    slot = b * 64 + (h // (H // 8)) * 8 + w // (W // 8)
    acc = np.zeros(F * 64, np.float32)
    cnt = np.zeros(F * 64, np.float32)
    for r in kept_rays(b, h, w, R, H, W):
        acc[slot[r]] = np.float32(acc[slot[r]] + s[r])
        cnt[slot[r]] += 1
    return acc.reshape(F, 64), cnt.reshape(F, 64)


def frame_avg(block_loss, block_cnt):
    """(loss_approx [F, 64] f32, frame average [F] f32) of frame_avg_block / finalize_block's closing lines"""
    bl = np.asarray(block_loss, np.float32).reshape(-1, 64)
    c = np.asarray(block_cnt, np.float32).reshape(-1, 64).copy()
    c[c == 0] = 1
    la = (bl / c).astype(np.float32)                    # fp32 division, correctly rounded
    v = la.copy()
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):                      # v += __shfl_xor(v, m): every lane, so all 64 end with the same sum
        v = (v + v[:, lane ^ m]).astype(np.float32)
    return la, (v[:, 0] / np.float32(64)).astype(np.float32)


def border_pixels(n):
    """0, n - 1 and k * n / 8 - 1, k * n / 8 for k = 1 .. 7"""
    b = n // 8
    return np.array(sorted({0, n - 1} | {k * b - 1 for k in range(1, 8)} | {k * b for k in range(1, 8)}), np.int64)


# ---- AdamW ----------------------------------------------------------------------------------------------------------------------
def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def bias_corrections_f32(beta1, beta2, step):
    """(bc1, sqrt(bc2)) the way the launcher computes them: fp32 powf, fp32 subtraction, fp32 sqrtf"""
    b1, b2, t = np.float32(beta1), np.float32(beta2), np.float32(step)
    with np.errstate(under="ignore"):
        bc1 = np.float32(1) - np.power(b1, t, dtype=np.float32)
        bc2 = np.float32(1) - np.power(b2, t, dtype=np.float32)
    return np.float32(bc1), np.float32(np.sqrt(bc2, dtype=np.float32))


def adamw(p, m, v, g_sum, count, grad_scale, lr, betas, eps, wd, step, bc=None, want_terms=False, exact_state=False):
    """One torch.optim.AdamW step in float64, in torch's order, on the fp32 values of every input.  count: None = no division.
    bc: (bc1, sqrt(bc2)) to use instead of the float64 ones (the GPU test passes the launcher's fp32 values).
    exact_state: take p, m, v and g_sum as the float64 arrays they are (the CPU test carries this function's own output over
    1 000 steps against torch in float64; the hyper-parameters are still their fp32 values)."""
    p, m, v, g = (np.asarray(x, np.float64) for x in (p, m, v, g_sum)) if exact_state else (f32(p), f32(m), f32(v), f32(g_sum))
    lr, b1, b2, eps, wd, gs = (float(np.float32(x)) for x in (lr, betas[0], betas[1], eps, wd, grad_scale))
    if count is not None:
        gs = gs / float(np.float32(count))
    g = g * gs
    bc1, bc2s = (1.0 - b1 ** step, np.sqrt(1.0 - b2 ** step)) if bc is None else (float(bc[0]), float(bc[1]))
    pd = p * (1.0 - lr * wd)
    t_m = (b1 * m, (1.0 - b1) * g)
    m1 = t_m[0] + t_m[1]
    v1 = b2 * v + (1.0 - b2) * g * g
    denom = np.sqrt(v1) / bc2s + eps
    upd = lr / bc1 * (m1 / denom)
    p1 = pd - upd
    if want_terms:
        return p1, m1, v1, dict(A_m=np.abs(t_m[0]) + np.abs(t_m[1]), pd=np.abs(pd), denom=denom, step_size=lr / bc1)
    return p1, m1, v1


# fp32 roundings on the path from the inputs to each value in adamw_update (optim.hip; `fp contract(off)`: no FMA):
#   gi    = gsum * gs,  gs = grad_scale / count (PHASE 0: / float(P))                                   2
#   mi    = b1 * m0 + (1 - b1) * gi:   gi 2, (1 - b1) 1, product 1, sum 1                               5   (the b1 * m0 path: 2)
#   vi    = b2 * v0 + (1 - b2) * gi * gi:   gi twice 4, (1 - b2) 1, two products 2, sum 1               8   (all terms >= 0)
#   denom = sqrtf(vi) / bc2_sqrt + eps:   half of vi's 8 = 4, sqrtf 1, division 1, sum 1                7   (all terms >= 0)
#   upd   = (lr / bc1) * (mi / denom):   mi 5 (on A_m, not on |mi|: its two terms may cancel), denom 7, lr / bc1 1, mi / denom 1, product 1
#   pi    = p * (1 - lr * wd) - upd:   decay path lr * wd 1, 1 - x 1, product 1, final difference 1 = 4;   update path 15 + 1 = 16
K_M, K_V, K_P_DECAY, K_P_UPDATE = 5, 8, 4, 16
POW_ULPS = 2          # the host's powf: allowed 2 ulp (4 unit roundoffs) of its value


def _gamma(k):
    return k * U32 / (1.0 - k * U32)


def adamw_bound(terms, v1, betas, step):
    """per-element bounds (dp, dm, dv) on |kernel - model| from the table above.  The bias corrections add the propagated powf
    allowance: d bc1 / bc1 = 2 ulp * b1^t / bc1, d sqrt(bc2) / sqrt(bc2) = half of 2 ulp * b2^t / bc2.
    Not in the bound: where the host's powf and numpy's really differ, the fp32 roundings of `1 - pow` and of sqrtf differ too, by
    up to 1 ulp of bc1 / sqrt(bc2) each.  The bound is therefore on the tight side (a spurious failure, never a missed bug) on a host
    whose two powf disagree; measured on MI355X hosts the kernel sits at 0.53 .. 0.61 of it at every step, i.e. they agree."""
    b1, b2 = float(np.float32(betas[0])), float(np.float32(betas[1]))
    e_bc1 = POW_ULPS * 2 * U32 * b1 ** step / (1.0 - b1 ** step)
    e_bc2 = 0.5 * POW_ULPS * 2 * U32 * b2 ** step / (1.0 - b2 ** step)
    dm = _gamma(K_M) * terms["A_m"]
    dv = _gamma(K_V) * np.abs(v1)
    dp = _gamma(K_P_DECAY) * terms["pd"] + (_gamma(K_P_UPDATE) + e_bc1 + e_bc2) * terms["step_size"] * terms["A_m"] / terms["denom"]
    return dp, dm, dv


def grad_grid(n, rng, lo=1e-12, hi=1e2, zero_frac=0.05):
    """gradients log-uniform in magnitude over [lo, hi] with random sign, plus exact zeros: the eps-dominated, the mixed and the
    gradient-dominated regimes of AdamW's denominator"""
    g = np.exp(rng.uniform(np.log(lo), np.log(hi), n)) * rng.choice([-1.0, 1.0], n)
    g[rng.uniform(size=n) < zero_frac] = 0.0
    return g.astype(np.float32)
