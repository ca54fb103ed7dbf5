"""The forward-only `sdf_eval` (no input gradient: launch_chain mode 0) against a float64 reference, on every kernel it can reach.

Mode 0 builds the mesh volume of `get_sdf_grid` for every shipped config.  It runs on `fwd_pair.hip` for the <256, 256> six-octave
cat-3 net (replicaCAD / scanNet) in the bf16 / fp16 / fp16x2 operand modes and on `chain_kernel<HD, EP, OPER, MODE = 0>` for every
other net and for fp16x2_full.  References: `oracle.torch_port.PortNet` in float64 on the device, and the reference fixtures'
`sdf_nonoise` where they exist.  Bars are the ones tests/test_gpu_parity.py holds the same nets / operands to with the input gradient.

  * coverage matrix: one case per forward-only instantiation; ragged sizes; the `noise` argument; mode 0 bit-identical to mode 1 on
    the chain kernel (one template, `if (MODE == 0) return;` after the sdf store)
  * the C ABI: no store past `n_points` in either kernel, with and without the gradient output; `n_points = 0` is a no-op
  * the 200^3 mesh grid of the trained fixtures: all 8 M points elementwise, chunking and permutation invariance, the mesh
  * the hardware sine (`__sinf` -> v_sin_f32, no range reduction) over 8x the largest positional-encoding angle a shipped config
    reaches on its fixture's grid box
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import oracle.isdf_oracle as orc
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

TOL_SDF = 1e-3
TOL_SDF_GRAD = 2e-3
# sdf rel-L2 bar per forward operand (test_gpu_parity.py: TOL_SDF, SDF_BAR, test_forward_sdf's 8e-3 for bf16); the max error on the
# output scale (`_scaled_err`) is held to twice that, fp16x2_full to 1e-4 (test_base_size_forward_and_input_gradient_vs_reference)
REL_BAR = {"fp16x2": TOL_SDF, "fp16": 2e-3, "bf16": 8e-3, "fp16x2_full": 2e-5}
SCALED_BAR = {"fp16x2": 2 * TOL_SDF, "fp16": 4e-3, "bf16": 1.6e-2, "fp16x2_full": 1e-4}
# pair-tile forward vs the one-tile chain forward (test_pair_tile_forward_kernel_agrees_with_the_one_tile_forward)
PAIR_VS_CHAIN = {"fp16x2": 5e-5, "fp16": 1e-4, "bf16": 5e-4}
RAGGED = (1, 63, 64, 65, 127, 128, 129, 4133)     # 4133 = 64 full tiles + 37 points (32 full pairs + a half pair + 37 points)


def _load(name):
    # np.load, not gu.load: the forward needs no keyframes (gu.load regenerates the BASELINE-size ones)
    return dict(np.load(os.path.join(gu.GOLDEN_DIR, name + ".npz"), allow_pickle=False))


def _around(x, n, seed):
    """n points near the rows of x (a fixture's samples: 2.6 k .. 15 k points), for sizes past the fixture's own"""
    rng = np.random.RandomState(seed)
    xs = x.cpu().numpy()
    pick = xs[rng.randint(0, xs.shape[0], n)] + rng.normal(0.0, 0.05, (n, 3)) * xs.std(0)
    return torch.from_numpy(pick.astype(np.float32)).cuda()


def _has_T(g):
    return int(g["has_transform"][0]) if "has_transform" in g else 1


def _scaled_err(got, ref, floor):
    """max |got - ref| on the scale of the output (max |ref|, never below `floor`: 0.14 = scale_output for sdf), float64."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double().to(torch.as_tensor(got).device)
    return float((got - ref).abs().max() / max(float(ref.abs().max()), floor))


def _rel(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double().to(torch.as_tensor(got).device)
    return float((got - ref).norm() / max(float(ref.norm()), 1e-30))


class Net:
    """One network: the HIP engine, its float64 port on the device, and what the kernel dispatch will pick for it."""

    def __init__(self, hidden, blocks, n_freqs, scale_input, params, transform, fwd_operand="fp16x2", scale_output=0.14):
        from isdf_amd.engine import Engine, NetConfig
        from oracle.torch_port import PortNet
        self.eng = Engine(NetConfig(hidden=hidden, blocks=blocks, n_freqs=n_freqs, scale_input=scale_input,
                                    scale_output=scale_output, transform=transform, fwd_operand=fwd_operand), "cuda")
        self.eng.load_params(params)
        port = PortNet(hidden, blocks, n_freqs, scale_input, scale_output, transform=transform)
        port.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
        self.port = port.to(device="cuda", dtype=torch.float64).eval()
        self.operand, self.params = fwd_operand, params
        self.cfg = orc.NetCfg(hidden, blocks, n_freqs, scale_input, scale_output, transform)
        HD = 256 if hidden <= 256 else 512
        E = 2 * 21 * n_freqs + 3                  # 21 icosahedron directions (embedding.py)
        EP = max(-(-E // 256) * 256, HD)
        self.pair = (HD, EP) == (256, 256) and 2 * blocks + 2 == 6 and n_freqs == 6 and fwd_operand != "fp16x2_full"
        oper = {"bf16": 0, "fp16": 1, "fp16x2": 2, "fp16x2_full": 3}[fwd_operand]
        self.kernel = ("fwd_pair_kernel<OPER %d>" % oper) if self.pair else ("chain_kernel<%d, %d, OPER %d, MODE 0>" % (HD, EP, oper))

    @classmethod
    def of_fixture(cls, g, fwd_operand="fp16x2"):
        H, B, nf, si, so = g["net"]
        return cls(int(H), int(B), int(nf), float(si), gu.params_of(g), g["bounds_T"] if _has_T(g) else None, fwd_operand, float(so))

    def ref(self, x, noise=None, want_grad=False, chunk=1 << 18):
        """float64 PortNet on the device, chunked (a few GB at most), -> sdf [n] (and d sdf / dx [n, 3]) float64"""
        outs, grads = [], []
        for i in range(0, x.shape[0], chunk):
            xc = x[i:i + chunk].to(device="cuda", dtype=torch.float64)
            nc = None if noise is None else noise[i:i + chunk].to(device="cuda", dtype=torch.float64)
            if want_grad:
                xc.requires_grad_(True)
                with torch.enable_grad():
                    y = self.port(xc, nc)
                    g, = torch.autograd.grad(y.sum(), xc)
                outs.append(y.detach()); grads.append(g)
            else:
                with torch.no_grad():
                    outs.append(self.port(xc, nc))
        return (torch.cat(outs), torch.cat(grads)) if want_grad else torch.cat(outs)


# ---- 1. coverage matrix: one case per forward-only instantiation ----------------------------------------------------------------
# (id, fixture or random-init shape (hidden, blocks, n_freqs), forward operand); the comment names the kernel the dispatch picks
MODE0_CASES = [
    ("default", "eval_full_ray", "fp16x2"),                  # fwd_pair<2>: replicaCAD / scanNet
    ("default-fp16", "eval_full_ray", "fp16"),               # fwd_pair<1>
    ("default-bf16", "eval_full_ray", "bf16"),               # fwd_pair<0>
    ("default-fp16x2_full", "eval_full_ray", "fp16x2_full"),  # chain<256, 256, 3>
    ("h128", "eval_h128", "fp16x2"),                         # fwd_pair<2>, zero-padded to 256
    ("b1_256", "eval_b1_256", "fp16x2"),                     # chain<256, 256, 2>: four hidden layers
    ("b1_256-fp16", "eval_b1_256", "fp16"),                  # chain<256, 256, 1>
    ("b1_256-bf16", "eval_b1_256", "bf16"),                  # chain<256, 256, 0>
    ("odd96", (96, 3, 4), "fp16x2"),                         # chain<256, 256, 2>, zero-padded width and embedding
    ("rs_realsense", "eval_rs_realsense", "fp16x2"),         # chain<256, 512, 2>: realsense.json
    ("rs_franka", "eval_rs_franka", "fp16x2"),               # chain<256, 512, 2>: realsense_franka.json
    ("rs_franka-fp16", "eval_rs_franka", "fp16"),            # chain<256, 512, 1>
    ("rs_franka-bf16", "eval_rs_franka", "bf16"),            # chain<256, 512, 0>
    ("rs_franka_offline", "eval_rs_franka_offline", "fp16x2"),  # chain<256, 512, 2>: eleven octaves, three blocks
    ("wide_512", "eval_wide_512", "fp16x2"),                 # chain<512, 512, 2>
    ("wide_512-fp16", "eval_wide_512", "fp16"),              # chain<512, 512, 1>
    ("wide_512-bf16", "eval_wide_512", "bf16"),              # chain<512, 512, 0>
    ("h300_f10", "eval_h300_f10", "fp16x2"),                 # chain<512, 512, 2>, zero-padded
    ("odd300", (300, 2, 6), "fp16x2"),                       # chain<512, 512, 2>, zero-padded
]
# test_forward_sdf holds the default net's fp16 fast mode to the north star itself.  bf16 on the four-hidden-layer net sits on its
# operand floor above test_forward_sdf's 8e-3 (the numpy model of bf16 operands is as far from the reference; DESIGN 5 gives 1.1e-2 for
# the model at BASELINE size): the kernel is held to the model instead, as every case is
FIXTURE_REL_BAR = {("eval_full_ray", "fp16"): TOL_SDF, ("eval_b1_256", "bf16"): 1.1e-2}
# the kernel against the numpy model of its own operand rounding (tests/precision_model.py): accumulation order and the hardware
# transcendentals only (test_base_size_forward_and_input_gradient_vs_reference's bars).  bf16: an operand rounding that flips between
# kernel and model moves a value by a bf16 step, 8x an fp16 one (measured 2.1e-4 .. 1.2e-3)
MODEL_BAR = {"fp16x2": 6e-4, "fp16": 6e-4, "bf16": 2e-3, "fp16x2_full": 2e-5}


def _case(src, fwd_operand):
    """-> (Net, points [n, 3] float32 on the device, the reference's sdf_nonoise or None)"""
    if isinstance(src, tuple):      # random-init odd widths of test_odd_hidden_widths_match_oracle, on the default fixture's points
        hidden, blocks, n_freqs = src
        g = _load("eval_full_ray")
        params = orc.init_params(hidden, blocks, n_freqs, np.random.RandomState(hidden + n_freqs))
        net = Net(hidden, blocks, n_freqs, 0.05937489, params, g["bounds_T"], fwd_operand)
        return net, torch.from_numpy(g["pc"].reshape(-1, 3)).cuda(), None
    g = _load(src)
    return Net.of_fixture(g, fwd_operand), torch.from_numpy(g["pc"].reshape(-1, 3)).cuda(), g["sdf_nonoise"].reshape(-1)


@pytest.mark.parametrize("cid,src,fwd_operand", MODE0_CASES, ids=[c[0] for c in MODE0_CASES])
def test_forward_only_matches_float64_reference(cid, src, fwd_operand):
    net, x, fixture = _case(src, fwd_operand)
    eng = net.eng
    rel_bar = FIXTURE_REL_BAR.get((src, fwd_operand), REL_BAR[fwd_operand])
    scaled_bar = SCALED_BAR[fwd_operand]

    # (a) the fixture's points: against the float64 port and against the reference's own output
    sdf = eng.sdf_eval(x)
    ref = net.ref(x)
    e_port, m_port = _rel(sdf, ref), _scaled_err(sdf, ref, 0.14)
    msg = "%s on %s: n %d, vs float64 port rel-L2 %.3e max/scale %.3e" % (cid, net.kernel, x.shape[0], e_port, m_port)
    if fixture is not None:
        e_fix, m_fix = _rel(sdf.cpu(), fixture), _scaled_err(sdf.cpu(), fixture, 0.14)
        msg += ", vs reference fixture rel-L2 %.3e max/scale %.3e" % (e_fix, m_fix)
    from tests import precision_model as pm
    model = pm.forward(net.params, net.cfg, x.cpu().numpy(), fwd_operand)
    e_model, floor = _rel(sdf.cpu(), model), _rel(torch.from_numpy(model), ref.cpu())
    msg += ", vs operand model rel-L2 %.3e (model vs port %.3e)" % (e_model, floor)
    print(msg)
    assert e_model < MODEL_BAR[fwd_operand], msg
    assert m_port < scaled_bar, msg
    if fixture is not None:        # (random-init nets: test_odd_hidden_widths_match_oracle holds them to the max error alone)
        assert e_port < rel_bar and e_fix < rel_bar and m_fix < scaled_bar, msg

    # (b) mode 0 against mode 1 (chain: the same template up to `if (MODE == 0) return;` after the sdf store -- same instructions
    # in front of it, so the same bits; pair tile: a different kernel, held to its existing bar against the one-tile forward)
    sdf1, _ = eng.sdf_eval(x, want_grad=True)
    if net.pair:
        d = float((sdf - sdf1).abs().max())
        assert d <= PAIR_VS_CHAIN[fwd_operand], (cid, d)
    else:
        assert torch.equal(sdf, sdf1), (cid, float((sdf - sdf1).abs().max()))

    # (c) ragged sizes: partial tiles, partial pairs, a partial last tile behind 64 full ones
    xr = _around(x, max(RAGGED), 3)
    full, refr = eng.sdf_eval(xr), net.ref(xr)
    for n in RAGGED:
        a = eng.sdf_eval(xr[:n])
        r = refr[:n]
        assert a.shape == (n,) and bool(torch.isfinite(a).all()), (cid, n)
        assert torch.equal(a, full[:n]), (cid, n)               # per point, independent of the batch it sits in
        assert _scaled_err(a, r, 0.14) < scaled_bar, (cid, n, _scaled_err(a, r, 0.14))
        if n >= 64 and fixture is not None:
            assert _rel(a, r) < rel_bar, (cid, n, _rel(a, r))
        b, _ = eng.sdf_eval(xr[:n], want_grad=True)
        if net.pair:
            assert float((a - b).abs().max()) <= PAIR_VS_CHAIN[fwd_operand], (cid, n)
        else:
            assert torch.equal(a, b), (cid, n)

    # (d) the noise argument: raw + noise before * scale_output (fc_map.py:104-109)
    nz = torch.from_numpy(np.random.RandomState(11).standard_normal(x.shape[0]).astype(np.float32) * np.float32(0.08)).cuda()
    a = eng.sdf_eval(x, noise=nz)
    r = net.ref(x, noise=nz)
    e_n, m_n = _rel(a, r), _scaled_err(a, r, 0.14)
    print("%s with noise: vs float64 port rel-L2 %.3e max/scale %.3e" % (cid, e_n, m_n))
    assert m_n < scaled_bar and (fixture is None or e_n < rel_bar), (cid, e_n, m_n)
    b, _ = eng.sdf_eval(x, noise=nz, want_grad=True)
    if net.pair:
        assert float((a - b).abs().max()) <= PAIR_VS_CHAIN[fwd_operand], cid
    else:
        assert torch.equal(a, b), cid


def test_coverage_matrix_names_every_forward_only_instantiation():
    """launch_mode<0> reaches chain_kernel<256, 256, OPER 0..3>, <256, 512, OPER 0..2>, <512, 512, OPER 0..2> (OPER 3 exists for
    <256, 256> only); launch_fwd_pair reaches OPER 0..2.  Each is named by at least one case above."""
    got = set()
    for cid, src, op in MODE0_CASES:
        if isinstance(src, tuple):
            H, B, nf = src
        else:
            H, B, nf = [int(v) for v in _load(src)["net"][:3]]
        HD = 256 if H <= 256 else 512
        EP = max(-(-(42 * nf + 3) // 256) * 256, HD)
        oper = {"bf16": 0, "fp16": 1, "fp16x2": 2, "fp16x2_full": 3}[op]
        pair = (HD, EP, B, nf) == (256, 256, 2, 6) and oper != 3
        got.add(("pair", oper) if pair else (HD, EP, oper))
    want = {("pair", o) for o in range(3)} | {(256, 256, o) for o in range(4)} | {(hd, ep, o) for hd, ep in ((256, 512), (512, 512))
                                                                                  for o in range(3)}
    assert got == want, (sorted(map(str, want - got)), sorted(map(str, got - want)))


# ---- 2. the C ABI: nothing stored past n_points, n_points = 0 is a no-op -----------------------------------------------------------
PAD = 300      # more than a pair of 64-point tiles


@pytest.mark.parametrize("want_grad", [False, True], ids=["sdf", "sdf+grad"])
@pytest.mark.parametrize("src", ["eval_full_ray", "eval_rs_franka", "eval_wide_512"])
def test_c_abi_stores_nothing_past_n_points(src, want_grad):
    from isdf_amd import _ffi
    net = Net.of_fixture(_load(src))
    eng = net.eng
    assert net.pair == (src == "eval_full_ray")
    x_all = _around(torch.from_numpy(_load(src)["pc"].reshape(-1, 3)), 4133, 8)

    def call(n):
        sdf = torch.full((n + PAD,), float("nan"), device="cuda")
        grad = torch.full((n + PAD, 3), float("nan"), device="cuda") if want_grad else None
        ws = eng.workspace(max(n, 1), False) if want_grad else None
        torch.cuda.synchronize()
        rc = eng.lib.isdf_sdf_eval(C.byref(eng.cnet), _ffi.ptr(eng.params), _ffi.ptr(eng.shadow), _ffi.ptr(x_all), n, None,
                                   _ffi.ptr(sdf), _ffi.ptr(grad), _ffi.ptr(ws), 0 if ws is None else ws.numel(), None)
        torch.cuda.synchronize()
        return rc, sdf, grad

    for n in (1, 63, 65, 129, 4133):
        rc, sdf, grad = call(n)
        assert rc == 0, (n, rc)
        assert bool(torch.isnan(sdf[n:]).all()), (src, n, int((~torch.isnan(sdf[n:])).sum()))
        assert bool(torch.isfinite(sdf[:n]).all()), (src, n)
        ref = eng.sdf_eval(x_all[:n], want_grad=want_grad)
        assert torch.equal(sdf[:n], ref[0] if want_grad else ref), (src, n)
        if want_grad:
            assert bool(torch.isnan(grad[n:]).all()) and bool(torch.isfinite(grad[:n]).all()), (src, n)
            assert torch.equal(grad[:n], ref[1]), (src, n)
    rc, sdf, grad = call(0)
    assert rc == 0 and bool(torch.isnan(sdf).all()) and (grad is None or bool(torch.isnan(grad).all()))


# ---- 3. the 200^3 mesh grid of the trained fixtures, elementwise --------------------------------------------------------------------
@pytest.mark.parametrize("case", ["trained_default", "trained_franka"])
def test_mesh_grid_elementwise_chunking_and_permutation(case):
    from tests.test_mesh_gpu import _bounds_grid, _vertex_to_mesh_distance
    from isdf_amd.mesh import grid_index_to_world
    g = _load(case)
    net = Net.of_fixture(g)
    eng = net.eng
    assert net.kernel == ("fwd_pair_kernel<OPER 2>" if case == "trained_default" else "chain_kernel<256, 512, OPER 2, MODE 0>")
    dim = 200
    pts, scale, T_bounds = _bounds_grid(g, dim)
    pts = pts.cuda()
    N = pts.shape[0]
    vol = eng.sdf_eval(pts)                                 # get_sdf_grid: one launch over all grid_dim^3 points
    ref = net.ref(pts)
    err = (vol.double() - ref).abs()
    worst = int(err.argmax())
    e_rel, e_max = _rel(vol, ref), _scaled_err(vol, ref, 0.14)
    print("%s (%s): %d points, rel-L2 %.3e, max |err| %.3e = %.3e of the output scale, worst point %d at %s (hip %.6f, ref %.6f)"
          % (case, net.kernel, N, e_rel, float(err.max()), e_max, worst, pts[worst].tolist(), float(vol[worst]), float(ref[worst])))
    assert bool(torch.isfinite(vol).all())
    assert e_rel < TOL_SDF and e_max < 2 * TOL_SDF, (e_rel, e_max, worst)
    # chunking: the reference's fc_map.chunks (100 000 points per call) -- tile and pair boundaries all move
    chunks = torch.cat([eng.sdf_eval(pts[i:i + 100000]) for i in range(0, N, 100000)])
    assert torch.equal(vol, chunks), int((vol != chunks).sum())
    # permutation: a point's output depends on its own row only
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5)).cuda()
    pv = eng.sdf_eval(pts[perm])
    assert torch.equal(pv, vol[perm]), int((pv != vol[perm]).sum())
    # the mesh of the HIP volume is within a voxel of the float64 volume's
    A = grid_index_to_world(dim, scale, T_bounds)
    v, f, _ = eng.marching_cubes(vol.view(dim, dim, dim), 0.0, A)
    rv, rf, _ = eng.marching_cubes(ref.float().view(dim, dim, dim), 0.0, A)
    voxel = float(np.min(np.linalg.norm(A[:, :3], axis=0)))
    dist = _vertex_to_mesh_distance(v.cpu().numpy(), rv.cpu().numpy())
    print("%s: %d / %d faces, vertex-to-mesh distance %.3e (voxel %.3e)" % (case, f.shape[0], rf.shape[0], dist, voxel))
    assert f.shape[0] > 10000 and abs(f.shape[0] - rf.shape[0]) < 0.01 * rf.shape[0]
    assert dist < voxel


# ---- 4. the hardware sine over the positional-encoding angles the shipped configs reach -----------------------------------------
# (n_freqs, scale_input, hidden_layers_block, fixture whose grid box sets the reachable angle): replicaCAD / scanNet, realsense_franka,
# realsense, realsense_franka_offline
PE_SETTINGS = [(6, 0.05937489, 2, "trained_default"), (9, 0.4, 2, "trained_franka"), (9, 0.04, 2, "eval_rs_realsense"),
               (11, 0.04, 3, "eval_rs_franka_offline")]


def _largest_top_angle(g, n_freqs, scale_input):
    """largest |x' . dir| 2^(n_freqs - 1) over the fixture's mesh-grid box (test_mesh_gpu._bounds_grid's box: corners are extreme)"""
    T_bounds = np.linalg.inv(g["bounds_T"].astype(np.float64))
    pc = (g["eval/pc"] if "eval/pc" in g else g["pc"]).reshape(-1, 3).astype(np.float64)
    local = (pc - T_bounds[:3, 3]) @ T_bounds[:3, :3]
    scale = 2 * np.abs(local).max(0) / (2 * 0.9)
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * scale
    world = corners @ T_bounds[:3, :3].T + T_bounds[:3, 3]
    pe_in = world @ g["bounds_T"][:3, :3].T.astype(np.float64) + g["bounds_T"][:3, 3] if _has_T(g) else world
    proj = (pe_in * scale_input) @ np.asarray(orc.ICO_DIRS, np.float64)
    return float(np.abs(proj).max()) * 2.0 ** (n_freqs - 1)


@pytest.mark.parametrize("n_freqs,scale_input,blocks,fixture", PE_SETTINGS, ids=["f%d_s%g" % s[:2] for s in PE_SETTINGS])
def test_pe_sine_over_eight_times_the_reachable_angle(n_freqs, scale_input, blocks, fixture):
    """v_sin_f32 / v_cos_f32 take revolutions and have no range reduction; the kernels feed them proj 2^f (chain.hip's PE fill and
    d/dx stages, fwd_pair.hip's octaves f % 3 == 0).  Measured on MI355X: the error grows with the angle as the fp32 rounding of
    x / 2pi does (~ 2^-24 |x|), with no cliff at 256 revolutions, up to 4096 revolutions.  Points on two lines through the origin
    (identity transform) sweep the top-octave angle from 0 to 8x the largest the config reaches on its fixture's grid box."""
    A = _largest_top_angle(_load(fixture), n_freqs, scale_input)
    params = orc.init_params(256, blocks, n_freqs, np.random.RandomState(40 + n_freqs))
    net = Net(256, blocks, n_freqs, scale_input, params, None)
    eng = net.eng
    dirs = np.asarray(orc.ICO_DIRS, np.float64)
    u0 = dirs[:, 0] / np.linalg.norm(dirs[:, 0])
    u1 = np.random.RandomState(2).standard_normal(3)
    u1 /= np.linalg.norm(u1)
    n = 8192
    rows, theta = [], []
    for u in (u0, u1):
        top = np.abs(u @ dirs).max() * scale_input * 2.0 ** (n_freqs - 1)      # top-octave angle per unit of t
        t = np.linspace(0.0, 8.0 * A / top, n)
        rows.append(t[:, None] * u[None, :]); theta.append(t * top)
    x = torch.from_numpy(np.concatenate(rows).astype(np.float32)).cuda()
    theta = np.concatenate(theta)
    sdf0 = eng.sdf_eval(x)
    sdf1, grad1 = eng.sdf_eval(x, want_grad=True)
    ref, refg = net.ref(x, want_grad=True)
    assert torch.equal(sdf0, sdf1) or net.pair
    print("n_freqs %d, scale_input %g (%s): reachable top-octave angle %.1f rad = %.1f revolutions; swept to %.1f revolutions"
          % (n_freqs, scale_input, net.kernel, A, A / (2 * np.pi), theta.max() / (2 * np.pi)))
    for lo, hi in ((0.0, 1.0), (1.0, 2.0), (2.0, 4.0), (4.0, 8.01)):
        m = torch.from_numpy((theta >= lo * A) & (theta <= hi * A)).cuda()
        e0, e1 = _scaled_err(sdf0[m], ref[m], 0.14), _scaled_err(sdf1[m], ref[m], 0.14)
        eg = _scaled_err(grad1[m], refg[m], 1.0)
        print("  top angle in [%.0f, %.0f] x reachable (up to %6.1f revolutions): sdf max/scale mode 0 %.3e mode 1 %.3e, d sdf/dx %.3e"
              % (lo, hi, hi * A / (2 * np.pi), e0, e1, eg))
        assert e0 < 2 * TOL_SDF and e1 < 2 * TOL_SDF and eg < 2 * TOL_SDF_GRAD, (lo, hi, e0, e1, eg)
