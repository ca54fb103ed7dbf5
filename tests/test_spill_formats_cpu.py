"""CPU checks of the spill formats (`isdf_net_cfg.spill_operand`): the float64 model in tests/spill_model.py against torch's e4m3 and
against the oracle, the s_G rule, where the shipped fixtures' P and GB sit against e4m3's 448, the train-mode instantiation table
that tests/test_spill_formats_gpu.py covers against the built library, and the configurations the library must reject."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import oracle.isdf_oracle as orc
from tests import golden_util as gu
from tests import spill_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isdf_amd", "csrc")


def _e4m3_torch(x):
    return torch.from_numpy(np.asarray(x, np.float64)).to(torch.float8_e4m3fn).to(torch.float64).numpy()


def _finite_codes():
    v = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    return np.unique(v[np.isfinite(v)])


# ---- 1. the e4m3 model -----------------------------------------------------------------------------------------------------------
def test_e4m3_model_is_bit_exact_vs_torch():
    codes = _finite_codes()
    assert len(codes) == 253 and codes.max() == 448.0 and codes[codes > 0].min() == 2.0 ** -9     # 254 finite codes, +-0 one value
    mid = (codes[1:] + codes[:-1]) / 2                       # every tie: round to the even code
    m32 = mid.astype(np.float32)         # (the kernel converts fp32; torch converts through fp32 as well)
    near = np.concatenate([np.nextafter(m32, np.float32(np.inf)), np.nextafter(m32, np.float32(-np.inf))]).astype(np.float64)
    tiny = np.array([2.0 ** -10, 2.0 ** -11, 3 * 2.0 ** -11, 2.0 ** -20, 1e-30, 2.0 ** -1074, 0.0])   # below / at half the smallest subnormal
    rng = np.random.RandomState(5)
    rand = np.ldexp(rng.uniform(0.5, 1.0, 20000), rng.randint(-14, 9, 20000)).astype(np.float32).astype(np.float64)
    x = np.concatenate([codes, mid, near, tiny, rand])
    x = np.concatenate([x, -x])
    x = x[np.abs(x) <= 448.0]
    got, want = sm.round_to(x, "e4m3"), _e4m3_torch(x)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, list(zip(x[bad][:5], got[bad][:5], want[bad][:5]))
    assert np.array_equal(np.signbit(got[x != 0]), np.signbit(x[x != 0]))


def test_e4m3_model_saturates_past_448():
    """Past the largest code the kernel's conversion saturates (MODE.FP16_OVFL, chain.hip); torch's gives NaN past 464 (the
    midpoint to the NaN code), so the model's behaviour there is its own rule, checked by value"""
    x = np.array([448.0, 448.5, 463.9, 464.0, 465.0, 480.0, 1e4, 3e38])
    assert np.all(sm.round_to(x, "e4m3") == 448.0) and np.all(sm.round_to(-x, "e4m3") == -448.0)
    assert np.isnan(_e4m3_torch([480.0, 1e4])).all()


@pytest.mark.parametrize("fmt,tdt", [("fp16", torch.float16), ("bf16", torch.bfloat16)])
def test_16bit_models_match_torch(fmt, tdt):
    rng = np.random.RandomState(7)
    x = np.ldexp(rng.uniform(-1.0, 1.0, 50000), rng.randint(-30, 15, 50000)).astype(np.float32).astype(np.float64)
    want = torch.from_numpy(x.astype(np.float32)).to(tdt).to(torch.float64).numpy()
    assert np.array_equal(sm.round_to(x, fmt), want)


# ---- 2. the s_G rule ---------------------------------------------------------------------------------------------------------------
def test_gb_scale_rule_table():
    below = float(np.nextafter(np.float32(2.0 ** -100), np.float32(0)))
    top = float(np.nextafter(np.float32(2.0 ** 73), np.float32(0)))
    # (|gbar'|_inf, n_freqs, s_G): s_G = 2^(floor(log2 |gbar'|_inf) + 1 + shift), shift = -1 (<= 6 octaves), n_freqs - 7 above
    table = [
        (0.0, 6, 1.0), (0.0, 11, 1.0),
        (1.0, 6, 1.0), (1.0, 9, 8.0), (1.0, 10, 16.0), (1.0, 11, 32.0),         # exact powers of two: the next binade up, shifted
        (0.75, 6, 0.5), (0.75, 9, 4.0), (1.5, 6, 1.0), (2.0 ** 20, 6, 2.0 ** 20), (2.0 ** -20 * 1.99, 11, 2.0 ** -15),
        (1e-40, 6, 1.0),                                                          # subnormal maximum
        (2.0 ** -100, 6, 2.0 ** -100), (below, 6, 1.0), (2.0 ** -100, 11, 2.0 ** -95),
        (top, 6, 2.0 ** 72), (top, 11, 2.0 ** 77), (2.0 ** 73, 6, 1.0), (2.0 ** 73, 11, 1.0), (np.inf, 6, 1.0),
    ]
    for g, nf, want in table:
        got = float(sm.gb_scale(np.float32(g), nf))
        assert got == want, (g, nf, got, want)
    assert [sm.spill_gb_shift(n) for n in (6, 9, 10, 11)] == [-1, 2, 3, 4]


def test_model_constants_are_the_kernels():
    """The model's rules as the kernels state them (a changed shift, P scale or s_G window fails here, on any host)"""
    common = open(os.path.join(CSRC, "isdf_common.h")).read()
    m = re.search(r"spill_gb_shift\(int\s+n_freqs\)\s*\{\s*return\s+n_freqs\s*>\s*(\d+)\s*\?\s*n_freqs\s*-\s*(\d+)\s*:\s*(-?\d+)\s*;\s*\}", common)
    assert m, "spill_gb_shift changed form"
    hdr = lambda n: n - int(m.group(2)) if n > int(m.group(1)) else int(m.group(3))
    assert all(hdr(n) == sm.spill_gb_shift(n) for n in range(1, 16))
    assert re.search(r"kSpillPScale\s*=\s*1\.f\s*/\s*1024\.f\s*;", common) and sm.P_SCALE == 2.0 ** -10
    # (compared with all white space removed: a reformatted line still matches, a changed expression does not)
    flat = lambda t: re.sub(r"\s+", "", t)
    chain = flat(open(os.path.join(CSRC, "chain.hip")).read())
    assert flat("(ge < (27u << 23) || ge >= (200u << 23)) ? 1.f : __uint_as_float(ge + ((uint32_t)(1 + spill_gb_shift(nf)) << 23))") in chain
    assert flat("if (SP8) __builtin_amdgcn_s_setreg(1 | (23 << 6), 1);") in chain      # MODE.FP16_OVFL: saturate
    dw = flat(open(os.path.join(CSRC, "dw.hip")).read())
    assert flat("put8(sb, regA1, kSpillPScale, kSpillPScale, C8{})") in dw and flat("put8(sb + T::TEN, regB1, sG1[0], sG1[1], C8{})") in dw
    assert flat("(tid & 31) * 32 + 28") in dw          # sG1: float 7 of the point's pe_aux row (chain.hip: aux[1].w = sG)


# ---- 3. the model against the oracle -------------------------------------------------------------------------------------------------
def _args(g):
    return (gu.params_of(g), gu.net_of(g), gu.loss_of(g), g["pc"], g["z_vals"], g["depth_sample"], g["dirs_C_sample"], g["T_WC_sample"],
            g["norm_sample"] if gu.with_normals(g) else None)


def _oracle64(params, cfg, lc, *rest, **kw):
    cfg = orc.NetCfg(cfg.H, cfg.B, cfg.n_freqs, cfg.scale_input, cfg.scale_output, None if cfg.transform is None else cfg.transform.astype(np.float64))
    f = lambda a: None if a is None else np.asarray(a, np.float64)
    return orc.loss_and_grads({k: f(v) for k, v in params.items()}, cfg, lc, *map(f, rest), **kw)


@pytest.mark.parametrize("case", ["eval_small_ray", "eval_small_b3_f11"])
def test_model_formats_against_the_oracle(case):
    """'exact' IS the float64 oracle; 16-bit spills cost ~1e-4 at most; e4m3 costs more at eleven octaves than at six, GB-only less
    than P and GB; with eik / grad weights 0 no format changes anything (P^T GB and the injected term vanish)"""
    g = gu.load(case)
    args = _args(g)
    _, ref = _oracle64(*args)
    err = {}
    for fmt in sm.FORMATS:
        _, gm = sm.loss_and_grads(*args, fmt=fmt)
        err[fmt] = max(gu.rel_err(gm[k], ref[k]) for k in ref)
    print(case, err)
    assert err["exact"] < 1e-12 and err["16bit"] < 3e-4
    assert err["e4m3_gb"] < err["e4m3"] < (2e-2 if int(g["net"][2]) > 6 else 5e-3)
    lc0 = copy.copy(args[2]); lc0.eik_weight = 0.0; lc0.grad_weight = 0.0
    a0 = args[:2] + (lc0,) + args[3:]
    _, r0 = _oracle64(*a0)
    for fmt in sm.FORMATS:
        _, g0 = sm.loss_and_grads(*a0, fmt=fmt)
        assert max(gu.rel_err(g0[k], r0[k]) for k in r0) < 1e-12, fmt


# ---- 4. headroom of the fixtures against e4m3's 448 ----------------------------------------------------------------------------
HEADROOM_CASES = ["eval_base_680x1200_ray", "eval_base_480x640_ray", "eval_full_ray", "eval_rs_realsense", "eval_rs_franka",
                  "eval_rs_franka_offline", "eval_small_ray", "eval_small_pc_l2", "eval_small_eikonly", "eval_small_orien",
                  "eval_small_b3_f9", "eval_small_b3_f10", "eval_small_b3_f11", "trained_default", "trained_franka"]
P_MARGIN, G_MARGIN = 2.0, 1.2     # max |P| / 2^-10 <= 448 / P_MARGIN, max |GB| / s_G <= 448 / G_MARGIN


@pytest.mark.parametrize("case", HEADROOM_CASES)
def test_spilled_values_stay_inside_e4m3(case):
    """isdf_common.h's measured assumptions, asserted: |P| <= 0.2 (205 of 448 after the 2^-10 scale) below the top layer, and
    |GB| / s_G inside 448 at the shipped spill_gb_shift (the e4m3 conversion saturates there: a clipped value is a biased gradient)"""
    g = gu.load(case)
    if "eval/pc" in g:
        b = gu.trained_batch(g, "eval/")
        args = (gu.params_of(g), gu.net_of(g), gu.loss_of(g), b["pc"], b["z_vals"], b["depth_sample"], b["dirs_C_sample"],
                b["T_WC_sample"], b["norm_sample"])
        noise = b["noise"]
    else:
        args = _args(g)
        noise = g["draw_noise"].reshape(g["z_vals"].shape[0], -1) * np.float32(g["noise_std"][0])
    terms, _ = sm.loss_and_grads(*args, noise=noise, fmt="exact", want_intermediates=True)
    hp, hg = sm.headroom(terms["P"], terms["GB"], terms["sG"])
    print("%s (n_freqs %d): max |P|/2^-10 = %.1f, max |GB|/s_G = %.1f of 448" % (case, int(g["net"][2]), hp, hg))
    assert hp <= 448.0 / P_MARGIN, hp
    assert hg <= 448.0 / G_MARGIN, hg


# ---- 5. the instantiation table --------------------------------------------------------------------------------------------------
_CHAIN = re.compile(r"chain_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELi(\d+)EE")
_DW = re.compile(r"dw_kernelILi(\d+)ELb([01])ELi(\d+)EE")


def test_train_instantiations_are_the_gpu_tables():
    """Every train-mode chain_kernel<HD, EP, OPER, 2, BW, SP8> and dw_kernel<HD, F16, SP8> in the built library is a case of
    tests/test_spill_formats_gpu.py -- a kernel added without a test fails here, on any host"""
    from isdf_amd import _ffi, build, isa_lint
    if not os.path.exists(os.path.join(isa_lint.LLVM_BIN, "llvm-readelf")):
        pytest.skip("no llvm-readelf on this host")
    from tests import test_spill_formats_gpu as G
    build.build(verbose=False)
    names = list(isa_lint.kernel_resources(_ffi.LIB_PATH))
    chain, dw = set(), set()
    for n in names:
        m = _CHAIN.search(n)
        if m and int(m.group(4)) == 2:
            hd, ep, op, _, bw, sp8 = map(int, m.groups())
            chain.add((hd, ep, op, bw, sp8))
        m = _DW.search(n)
        if m:
            dw.add(tuple(map(int, m.groups())))
    assert len(chain) == 27 and len(dw) == 6, (len(chain), len(dw))
    assert chain == set(G.CHAIN_CASES), (chain ^ set(G.CHAIN_CASES))
    assert dw == set(G.DW_KERNELS), (dw ^ set(G.DW_KERNELS))


def test_gpu_table_cases_reach_their_kernels():
    """Each case's (fixture net, fwd, bwd, spill) resolves to its kernel's template arguments.  This is a RESTATEMENT of make_layout's
    rules (isdf_common.h) and of the launch dispatch (chain.hip launch_one / launch_oper, dw.hip launch_dw), not a query of the
    library, which exposes no layout: that each case launches its listed instantiation was checked once with a kernel trace of the
    coverage matrix."""
    from tests import test_spill_formats_gpu as G
    for (hd, ep, op, bw, sp8), (fix, fwd, bwd, spill) in G.CHAIN_CASES.items():
        H, B, nf = (int(v) for v in np.load(os.path.join(gu.GOLDEN_DIR, fix + ".npz"))["net"][:3])
        E = 42 * nf + 3
        HD = 256 if H <= 256 else 512
        assert (HD, max(-(-E // 256) * 256, HD)) == (hd, ep), fix
        assert G.OPERS.index(fwd) == op and (bwd == "fp16") == bool(bw) and G.SPILL_SP8[spill] == sp8, (fix, fwd, bwd, spill)


# ---- 6. rejections and copies ----------------------------------------------------------------------------------------------------
def test_spill_operand_rejections():
    from isdf_amd import _ffi
    from isdf_amd.engine import NetConfig
    lib = _ffi.lib()
    chk = lambda **kw: lib.isdf_check_net(C.byref(NetConfig(**kw).to_c()))
    for s in ("e4m3", "e4m3_gb"):
        assert chk(hidden=300, n_freqs=10, spill_operand=s) == -2        # ISDF_EUNSUPPORTED: instantiated for the 256-wide tiles
        assert chk(hidden=512, blocks=3, n_freqs=10, spill_operand=s) == -2
        assert chk(spill_operand=s, bwd_operand="bf16") == -1            # ISDF_EINVAL: e4m3 goes with fp16 second-order sweeps
        assert chk(spill_operand=s, fwd_operand="bf16") == -1
        assert chk(spill_operand=s) == 0 and chk(n_freqs=11, blocks=3, spill_operand=s) == 0
    for s in (None, "auto", "16bit"):
        assert chk(hidden=512, n_freqs=10, spill_operand=s) == 0 and chk(bwd_operand="bf16", spill_operand=s) == 0
    for bad in (-1, 4, 99):
        c = NetConfig().to_c()
        c.spill_operand = bad
        assert lib.isdf_check_net(C.byref(c)) == -1, bad                 # ISDF_EINVAL
    with pytest.raises(ValueError):
        NetConfig(spill_operand="fp8").to_c()


@pytest.mark.parametrize("spill", [None, "auto", "16bit", "e4m3", "e4m3_gb"])
def test_deepcopy_keeps_the_spill_format(spill):
    """copy.deepcopy(SDFMapHIP) (trainer.py:576; modules.py __deepcopy__) builds its snapshot's engine with the same format"""
    from isdf_amd.modules import SDFMapHIP
    from tests.fake_engine import FakeEngine

    class PE(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.n_freqs, self.scale, self.transform, self.embedding_size = 6, 0.05937489, None, 42 * 6 + 3

    m = SDFMapHIP(PE(), 256, 2, 0.14, device="cpu", spill_operand=spill, engine_factory=lambda net, dev: FakeEngine(net, dev))
    c = copy.deepcopy(m)
    assert c.engine.net.spill_operand == spill and c.engine.net == m.engine.net
    assert c.engine is not m.engine and torch.equal(c.engine.params, m.engine.params)
