"""CPU checks of the step-tail models (tests/tail_model.py): the bins and frame averages against the float64 oracle and the REAL
reference `loss.frame_avg`, the AdamW model against torch.optim.AdamW in float64, the kernel constants the GPU cases of
tests/test_step_tail_gpu.py are derived from, and that the duplicate-heavy input tells the obvious wrong rules apart."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

import oracle.isdf_oracle as orc
from tests import tail_model as tm
from tests.test_render_cpu import needs_ref      # the same reference checkout, the same skip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isdf_amd", "csrc")
U = tm.U32


def _consts():
    return tm.kernel_constants(open(os.path.join(CSRC, "optim.hip")).read(), open(os.path.join(CSRC, "isdf_common.h")).read())


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _tot(rng, R, S=4, quantised=True):
    """per-sample losses in [2^-6, 0.25).  quantised: multiples of 2^-20, so a ray's sum over S is exact in fp32 in ANY order (the
    reference's torch.sum and the kernel's sequential loop then feed the bins the same value) while a bin of many rays still needs
    more than 24 bits: the bin summation is the only place the implementations can differ."""
    t = rng.uniform(2.0 ** -6, 0.25, (R, S))
    if quantised:
        t = np.floor(t * 2.0 ** 20) * 2.0 ** -20
    return t.astype(np.float32)


def _cases(quantised=True):
    """name -> (tot [R,S], ib, ih, iw, F, H, W); rays sorted by frame like the sampler's compacted list"""
    rng = np.random.RandomState(17)
    out = {}
    H, W = 680, 1200
    # duplicate-heavy: 4 000 rays of frame 0 on a 16 x 20 pixel patch that straddles a bin corner, frame 1 one pixel hit by every ray,
    # frame 2 duplicate-free
    R0, R1, R2 = 4000, 300, 500
    h0, w0 = H // 8 * 3 - 7, W // 8 * 5 - 9
    ih = np.concatenate([h0 + rng.randint(0, 16, R0), np.full(R1, 401), rng.permutation(H)[:R2]])
    iw = np.concatenate([w0 + rng.randint(0, 20, R0), np.full(R1, 77), rng.permutation(W)[:R2]])
    ib = np.concatenate([np.zeros(R0), np.ones(R1), np.full(R2, 2)]).astype(np.int64)
    out["duplicate_heavy"] = (_tot(rng, len(ib), quantised=quantised), ib, ih, iw, 3, H, W)
    # a frame without rays: first, middle, last
    for name, empty in (("empty_first", 0), ("empty_middle", 1), ("empty_last", 2)):
        fr = [f for f in range(3) if f != empty]
        ib = np.repeat(fr, 200).astype(np.int64)
        out[name] = (_tot(rng, 400, quantised=quantised), ib, rng.randint(0, H, 400), rng.randint(0, W, 400), 3, H, W)
    # all rays in one bin
    out["one_bin"] = (_tot(rng, 900, quantised=quantised), np.zeros(900, np.int64), 85 * 7 + rng.randint(0, 85, 900),
                      150 * 2 + rng.randint(0, 150, 900), 1, H, W)
    # corners and both sides of every bin border, at three rasters (the last: H / 8 and W / 8 odd)
    for H, W in ((680, 1200), (480, 640), (8 * 13, 8 * 21)):
        hs, ws = tm.border_pixels(H), tm.border_pixels(W)
        ih, iw = np.meshgrid(hs, ws, indexing="ij")
        ih, iw = ih.ravel(), iw.ravel()
        perm = rng.permutation(len(ih))
        out["borders_%dx%d" % (H, W)] = (_tot(rng, len(ih), quantised=quantised), np.zeros(len(ih), np.int64), ih[perm], iw[perm], 1, H, W)
    return out


def _kept_per_bin(ib, ih, iw, F, H, W):
    kept = tm.kept_rays(ib, ih, iw, len(ib), H, W)
    n = np.zeros(F * 64, np.int64)
    np.add.at(n, ib[kept] * 64 + (ih[kept] // (H // 8)) * 8 + iw[kept] // (W // 8), 1)
    return n.reshape(F, 64)


# ---- 1. bins and frame averages -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(_cases()))
def test_bins_and_frame_avg_vs_float64_oracle(name):
    """Bar (derived): the model's bin is the EXACT sum of its kept rays (integer accumulation; the inputs sit on the 2^-32 grid)
    rounded once to fp32, the oracle's is the float64 sum: 2^-24 of the value.  loss_approx adds the fp32 division (exact at one ray):
    n_bin * 2^-24, n_bin = rays kept in the bin, covers both.  The frame value adds 6 butterfly stages and the division by 64 (exact)."""
    tot, ib, ih, iw, F, H, W = _cases()[name]
    R = len(ib)
    bl, bc = tm.bins(tot, ib, ih, iw, R, F, H, W)
    la, fa = tm.frame_avg(bl, bc)
    n_bin = _kept_per_bin(ib, ih, iw, F, H, W)
    assert np.array_equal(bc, n_bin.astype(np.float32))
    rs = tm.ray_sums(tot).astype(np.float64)[:, None]
    la64, fa64 = orc.frame_avg(rs, ib, ih, iw, F, H, W)
    la64 = la64.reshape(F, 64)
    sums64 = la64 * np.maximum(n_bin, 1)
    assert np.all(np.abs(bl - sums64) <= U * sums64 * (1 + 1e-12))
    assert np.all(np.abs(la - la64) <= n_bin * U * la64)
    assert np.all(bl[n_bin == 0] == 0) and np.all(la[n_bin == 0] == 0)
    assert np.all(np.abs(fa - fa64) <= (n_bin.max(-1) + 6) * U * fa64)
    for f in range(F):
        if not (ib == f).any():
            assert fa[f] == 0 and not bl[f].any() and not bc[f].any()


@needs_ref
@pytest.mark.parametrize("name", sorted(_cases()))
def test_bins_and_frame_avg_vs_the_real_reference_single_threaded(name):
    """The REAL loss.frame_avg.  Its scatter `full_loss[indices_b, indices_h, indices_w] = ...` is last-wins only single-threaded (with
    torch's default thread count duplicate pixels resolve in an unspecified order), so it runs under torch.set_num_threads(1).
    Bar (derived): the reference sums a bin's kept pixels in fp32 in another order, all terms >= 0: n_bin * 2^-24 of the bin's value.
    The raw bin sums are read from the reference by passing an all-zero mask (every divisor becomes 1)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden as mg
    with contextlib.redirect_stdout(io.StringIO()):
        loss = mg.import_reference()[4]
    tot, ib, ih, iw, F, H, W = _cases()[name]
    R = len(ib)
    bl, bc = tm.bins(tot, ib, ih, iw, R, F, H, W)
    la, fa = tm.frame_avg(bl, bc)
    n_bin = _kept_per_bin(ib, ih, iw, F, H, W)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    prev = torch.get_num_threads()
    try:
        torch.set_num_threads(1)
        depth = torch.zeros(F, H, W)
        mask = torch.zeros(F, H, W)
        mask[t(ib), t(ih), t(iw)] = 1                                      # sample.py:58-61
        sums_ref, _ = loss.frame_avg(t(tot), depth, t(ib), t(ih), t(iw), W, H, 8, torch.zeros(F, H, W))
        la_ref, fa_ref = loss.frame_avg(t(tot), depth, t(ib), t(ih), t(iw), W, H, 8, mask)
    finally:
        torch.set_num_threads(prev)
    sums_ref = sums_ref.numpy().reshape(F, 64).astype(np.float64)
    la_ref, fa_ref = la_ref.numpy().reshape(F, 64).astype(np.float64), fa_ref.numpy().astype(np.float64)
    assert np.array_equal(mask.view(F, 8, H // 8, 8, W // 8).sum(dim=(2, 4)).numpy().reshape(F, 64), bc)
    err = np.abs(bl.astype(np.float64) - sums_ref)
    assert np.all(err <= n_bin * U * sums_ref), (name, float((err / np.maximum(sums_ref, 1e-30)).max()))
    print(name, "worst bin vs reference: %.2e of the largest bin" % (err.max() / max(sums_ref.max(), 1e-30)))
    # loss_approx: each side divides its own fp32 sum (one more rounding each); the frame value: 63 fp32 additions there, 6 here
    assert np.all(np.abs(la - la_ref) <= (n_bin + 2) * U * la_ref)
    assert np.all(np.abs(fa - fa_ref) <= (n_bin.max(-1) + 2 + 63 + 6) * U * fa_ref)


def test_wrong_duplicate_rules_are_told_apart():
    """The GPU test holds the kernel's bins to the model BIT FOR BIT; each of these wrong rules changes the bins of the
    duplicate-heavy input by far more than that, so the input can tell them apart."""
    tot, ib, ih, iw, F, H, W = _cases(quantised=False)["duplicate_heavy"]
    R = len(ib)
    bl, bc = tm.bins(tot, ib, ih, iw, R, F, H, W)
    la, fa = tm.frame_avg(bl, bc)
    first = tm.bins(tot, ib, ih, iw, R, F, H, W, keep="first")
    every = tm.bins(tot, ib, ih, iw, R, F, H, W, count_all=True)
    order = tm.bins_fp32_ray_order(tot, ib, ih, iw, R, F, H, W)
    assert np.array_equal(first[1], bc) and not np.array_equal(first[0].view(np.uint32), bl.view(np.uint32))
    assert np.abs(tm.frame_avg(*first)[0] - la).max() > 1e-3 * la.max()            # another ray's loss: a visible move of loss_approx
    assert not np.array_equal(every[1], bc) and every[1].sum() == R
    assert np.array_equal(order[1], bc) and not np.array_equal(order[0].view(np.uint32), bl.view(np.uint32))
    assert np.abs(order[0] - bl).max() <= bc.max() * U * bl.max()                    # ... and the fp32 variant is only roundings away
    assert bc[0].sum() <= 320 and bc[1].sum() == 1 and bc[2].sum() == 500


# ---- 2. the AdamW model ---------------------------------------------------------------------------------------------------------
HYPER = dict(lr=0.0013, betas=(0.9, 0.999), eps=1e-8)


STEPS = (1, 2, 10, 1000)


def _torch_adamw(p, wd):
    f = lambda x: float(np.float32(x))
    tp = torch.nn.Parameter(torch.from_numpy(np.asarray(p, np.float64).copy()))
    opt = torch.optim.AdamW([tp], lr=f(HYPER["lr"]), betas=(f(HYPER["betas"][0]), f(HYPER["betas"][1])), eps=f(HYPER["eps"]),
                            weight_decay=f(wd), foreach=False)
    return tp, opt


def _agree(got, want, g64, tag):
    """1e-12 relative: of |g| for exp_avg and g^2 for exp_avg_sq (moments built from gradients of one magnitude per element never exceed
    them) and of max(|p|, lr) for the parameter (lr: one step's largest move)"""
    (p, m, v), (tp, tm_, tv) = got, want
    assert np.all(np.abs(m - tm_) <= 1e-12 * np.abs(g64)), tag
    assert np.all(np.abs(v - tv) <= 1e-12 * g64 * g64), tag
    assert np.all(np.abs(p - tp) <= 1e-12 * np.maximum(np.abs(tp), float(np.float32(HYPER["lr"])))), tag


@pytest.mark.parametrize("wd", [0.0, 0.012])
def test_adamw_model_is_torch_adamw_in_float64(wd):
    """tm.adamw ITSELF against torch.optim.AdamW, both float64, on the gradient grid of the GPU test; torch gets the fp32-rounded
    hyper-parameters the model takes.  Two ways, at steps 1, 2, 10 and 1 000:
      * free-running: tm.adamw (exact_state: no fp32 rounding of the carried state) fed its own output for 1 000 steps;
      * one step from torch's state: torch's p, m, v before the step rounded to fp32 and loaded into both -- the entry the GPU test
        uses (fp32 inputs), with non-zero moments and the bias corrections of that step.
    The gradient's sign flips between steps, so b1 * m and (1 - b1) * g also cancel."""
    rng = np.random.RandomState(3)
    n = 6000
    g = tm.grad_grid(n, rng)
    g64 = g.astype(np.float64)
    p0 = (0.05 * rng.standard_normal(n)).astype(np.float32)
    tp, opt = _torch_adamw(p0, wd)
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    kw = dict(count=None, grad_scale=1.0, lr=HYPER["lr"], betas=HYPER["betas"], eps=HYPER["eps"], wd=wd)
    for step in range(1, max(STEPS) + 1):
        sign = -1.0 if step % 3 == 0 else 1.0
        if step in STEPS:                     # one step from torch's current state, rounded to fp32, in both
            st = opt.state[tp] if step > 1 else dict(exp_avg=torch.zeros(n, dtype=torch.float64), exp_avg_sq=torch.zeros(n, dtype=torch.float64))
            s32 = [x.detach().numpy().astype(np.float32) for x in (tp, st["exp_avg"], st["exp_avg_sq"])]
            tq, oq = _torch_adamw(s32[0], wd)
            oq.state[tq] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(s32[1].astype(np.float64)),
                                exp_avg_sq=torch.from_numpy(s32[2].astype(np.float64)))
            tq.grad = torch.from_numpy(sign * g64)
            oq.step()
            assert float(oq.state[tq]["step"]) == step
            got = tm.adamw(s32[0], s32[1], s32[2], (sign * g).astype(np.float32), step=step, **kw)
            _agree(got, (tq.detach().numpy(), oq.state[tq]["exp_avg"].numpy(), oq.state[tq]["exp_avg_sq"].numpy()), g64, ("one step", step))
        tp.grad = torch.from_numpy(sign * g64)
        opt.step()
        p, m, v = tm.adamw(p, m, v, sign * g64, step=step, exact_state=True, **kw)
        if step in STEPS:
            st = opt.state[tp]
            _agree((p, m, v), (tp.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()), g64, ("free-running", step))
    # count and grad_scale: the gradient is g_sum * (grad_scale / count)
    z = np.zeros(n, np.float32)
    a = tm.adamw(p0, z, z, g, step=1, **kw)
    c = tm.adamw(p0, z, z, g * np.float32(8), 16.0, 2.0, HYPER["lr"], HYPER["betas"], HYPER["eps"], wd, 1)
    assert all(np.array_equal(x, y) for x, y in zip(a, c))
    # exact_state changes nothing on inputs that are fp32 already, and the fp32 view is what the default takes
    assert all(np.array_equal(x, y) for x, y in zip(a, tm.adamw(p0, z, z, g, step=1, exact_state=True, **kw)))
    q = p0.astype(np.float64) * (1 + 2.0 ** -30)
    assert all(np.array_equal(x, y) for x, y in zip(a, tm.adamw(q, z, z, g, step=1, **kw)))


def test_fp32_bias_corrections_are_within_the_powf_allowance_of_float64():
    """tm.bias_corrections_f32 -- what the GPU test feeds the model, computed like the launcher (fp32 powf, 1 - x, sqrtf) -- against
    the float64 values at the steps the GPU test uses: the 2 ulp allowed to powf, propagated as tm.adamw_bound propagates them, plus
    the function's own fp32 roundings (1 - x: one; sqrtf: one more on half of bc2's error)."""
    b1, b2 = (float(np.float32(b)) for b in HYPER["betas"])
    for step in (1, 2, 10, 1000, 100000):
        bc1, bc2s = (float(x) for x in tm.bias_corrections_f32(HYPER["betas"][0], HYPER["betas"][1], step))
        w1, w2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        e1 = tm.POW_ULPS * 2 * U * b1 ** step / w1 + U
        e2 = 0.5 * (tm.POW_ULPS * 2 * U * b2 ** step / w2 + U) + U
        assert abs(bc1 - w1) <= e1 * w1, (step, bc1, w1)
        assert abs(bc2s - np.sqrt(w2)) <= e2 * np.sqrt(w2), (step, bc2s, np.sqrt(w2))
    # step 1: powf(b, 1) = b and 1 - b is exact in fp32 for b in [0.5, 1]
    bc1, bc2s = tm.bias_corrections_f32(HYPER["betas"][0], HYPER["betas"][1], 1)
    assert float(bc1) == 1.0 - b1 and float(bc2s) == float(np.sqrt(np.float32(1.0 - b2)))


def test_adamw_bound_sees_a_misplaced_eps_and_a_dropped_bias_correction():
    """The derived per-element bound is far below what the mistakes the GPU test is there for would cost, in every regime they act
    in: eps inside the square root (eps-dominated and mixed elements), no bias correction of the second moment (step 1 .. 1 000)."""
    rng = np.random.RandomState(4)
    n = 4000
    g = tm.grad_grid(n, rng)
    p0 = (0.05 * rng.standard_normal(n)).astype(np.float32)
    z = np.zeros(n, np.float32)
    lr, (b1, b2), eps = (float(np.float32(HYPER["lr"])), [float(np.float32(b)) for b in HYPER["betas"]], float(np.float32(HYPER["eps"])))
    for step in (1, 10, 1000):
        p1, m1, v1, terms = tm.adamw(p0, z, z, g, None, 1.0, HYPER["lr"], HYPER["betas"], HYPER["eps"], 0.012, step, want_terms=True)
        dp, dm, dv = tm.adamw_bound(terms, v1, HYPER["betas"], step)
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        inside = terms["pd"] * np.sign(p0) - lr / bc1 * m1 / np.sqrt(v1 / bc2 + eps)
        nobc2 = terms["pd"] * np.sign(p0) - lr / bc1 * m1 / (np.sqrt(v1) + eps)
        small = (np.abs(g) > 1e-9) & (np.abs(g) < 1e-7)
        assert small.sum() > 100 and np.all(np.abs(inside - p1)[small] > 10 * dp[small]), step
        big = np.abs(g) > 1e-6
        assert big.sum() > 100 and np.all(np.abs(nobc2 - p1)[big] > 10 * dp[big]), step
        assert np.all(dm <= 6 * U * np.abs(g)) and np.all(dv <= 9 * U * g.astype(np.float64) ** 2)


# ---- 3. constants and the GPU file's case tables ----------------------------------------------------------------------------------
def test_kernel_constants_and_derived_gpu_cases():
    c = _consts()
    assert c["LOSS_STRIDE"] == c["TAIL_THREADS"]     # block 0 strides by its own thread count
    assert c["GROUPS"] * 64 == c["TAIL_THREADS"] and c["L3_STEP"] == c["GROUPS"]
    # each unrolled loop must look exactly as far as it reads: `look` = step - GROUPS (its last load is at t + look)
    assert c["L1_LOOK"] == c["L1_STEP"] - c["GROUPS"] and c["L2_LOOK"] == c["L2_STEP"] - c["GROUPS"]
    assert c["FIN_CAP"] * 4 <= 48 * 1024 and c["FIN_CAP"] > c["TAIL_THREADS"]
    from tests import test_step_tail_gpu as tg
    assert tg.C == c
    assert tg.N_MAX == 2 * c["L1_STEP"] + c["L3_STEP"] + 1
    # every mix of the three loops occurs in the sweep 1 .. N_MAX, the first loop with 0, 1 and 2 iterations
    mixes = {tm.loop_mix(n, g, c) for n in range(1, tg.N_MAX + 1) for g in range(c["GROUPS"])}
    per_l3 = c["L2_LOOK"] // c["L3_STEP"]        # the remainder loop runs at most that often after the second
    want = {(a, b, r) for a in (0, 1) for b in (0, 1) for r in range(per_l3 + 1)} - {(0, 0, 0)}
    assert want <= mixes and (2, 0, 0) in mixes and (2, 0, 1) in mixes, sorted(want - mixes)
    # whatever the mix, a group must add exactly its tiles: loop_mix's iterations cover tiles_of_group
    for n in range(1, tg.N_MAX + 1):
        for g in range(c["GROUPS"]):
            n1, n2, n3 = tm.loop_mix(n, g, c)
            assert n1 * (c["L1_STEP"] // c["GROUPS"]) + n2 * (c["L2_STEP"] // c["GROUPS"]) + n3 == len(tm.tiles_of_group(n, g, c))
    # the ragged handful: one tile count per mix boundary
    assert set(tg.RAGGED_TILES) == {c["L2_LOOK"], c["L2_LOOK"] + 1, c["L2_STEP"], c["L2_STEP"] + 1, c["L1_LOOK"] + 1, c["L1_STEP"],
                                    c["L1_STEP"] + 1, c["L1_STEP"] + c["L2_LOOK"] + 1, 2 * c["L1_STEP"] + 1}
    assert tg.FIN_CASES == (c["FIN_CAP"], c["FIN_CAP"] + 1, c["FIN_CAP"] * 3 // 2)
    assert tg.R_CASES == (1, c["TAIL_THREADS"] + 1)
    assert tg.BIG_TILES > 4 * c["LOSS_STRIDE"]
    assert tm.vec_chain_length(1, c) == 1 + 1 + c["GROUPS"] and tm.loss_chain_length(c["LOSS_STRIDE"] + 1, c) == 2 + 6 + 16
