"""The step tail (isdf_amd/csrc/optim.hip: step_tail_kernel<0|1|2>, finalize_block, frame_avg_kernel, adamw_kernel) against the exact
models of tests/tail_model.py.  Needs a real MI355X: `pytest -m gpu`.

  a. bins, loss_approx and frame averages BIT FOR BIT: duplicate pixels, frames without a valid ray, image corners and bin borders,
     frames at / past FIN_CAP rays (the unstaged key scan), R = 1 and one more ray than the tail has threads
  b. every route (fused tail with a device / inline index list, isdf_frame_avg, isdf_train_step_finish) writes the same averages,
     where the index list says and nowhere else; hand-made bins
  c. the gradient and loss reductions at every tile count 1 .. N_MAX (every mix of the vector section's three unrolled loops) and past
     1 024 / 4 096 tiles, against float64 sums of small runs that use the plain remainder loop only
  d. AdamW against the float64 model on a gradient grid over 1e-12 .. 1e2, held to the forward-error bound of adamw_update; the three
     routes bit-identical; empty batches change nothing
The pixel lists go in through the sampler's injected draws on synthetic keyframes; `dbg["tot_loss_mat"]` is the value the chain kernel
also stores for the tail, so the models read what the tail read.  tests/test_step_tail_cpu.py checks the models and that the case
tables below follow optim.hip's constants.
"""
import ctypes as ct
import os

import numpy as np
import pytest
import torch

from tests import tail_model as tm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isdf_amd", "csrc")
C = tm.kernel_constants(open(os.path.join(CSRC, "optim.hip")).read(), open(os.path.join(CSRC, "isdf_common.h")).read())
U = tm.U32

# ---- case tables, all from optim.hip's constants (tests/test_step_tail_cpu.py::test_kernel_constants_and_derived_gpu_cases) --------
N_MAX = 2 * C["L1_STEP"] + C["L3_STEP"] + 1            # every mix of the three loops occurs in 1 .. N_MAX, the first loop's twice
RAGGED_TILES = sorted({C["L2_LOOK"], C["L2_LOOK"] + 1, C["L2_STEP"], C["L2_STEP"] + 1, C["L1_LOOK"] + 1, C["L1_STEP"], C["L1_STEP"] + 1,
                       C["L1_STEP"] + C["L2_LOOK"] + 1, 2 * C["L1_STEP"] + 1})
FIN_CASES = (C["FIN_CAP"], C["FIN_CAP"] + 1, C["FIN_CAP"] * 3 // 2)
R_CASES = (1, C["TAIL_THREADS"] + 1)
BIG_FRAMES, BIG_RAYS, BIG_S = 5, 2000, 27
BIG_TILES = -(-BIG_FRAMES * BIG_RAYS * BIG_S // C["TILE_PTS"])          # 4 219 > 4 x 1 024
BASE_RAYS = 1000                                                         # BASELINE size: 5 keyframes x 200 rays (x 27 samples = 422 tiles)
CHUNK_TILES = C["L3_STEP"] - 1                                           # 15: only the remainder loop runs, one addition per group

ODD_CAM = dict(H=8 * 13, W=8 * 21, fx=84.0, fy=84.0, cx=83.5, cy=51.5)   # H / 8 and W / 8 odd
OPT0 = dict(lr=0.0, weight_decay=0.0)                                    # the fused tail with an update of exactly zero


def _cams():
    from isdf_amd import synthetic
    return {"680x1200": dict(synthetic.REPLICA_CAM), "480x640": dict(synthetic.SCANNET_CAM), "104x168": dict(ODD_CAM)}


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


_KF = {}


def _kf(F, cam):
    """F synthetic keyframes WITHOUT invalid pixels (the cases decide which rays are valid) and without NaN normals"""
    from isdf_amd import synthetic
    key = (cam["H"], cam["W"])
    if key not in _KF or _KF[key][0].shape[0] < F:
        T = synthetic.trajectory(F * 40)[::40][:F]
        depth = np.stack([synthetic.render_depth(T[i], cam, rng=None) for i in range(F)])
        assert np.isfinite(depth).all() and (depth > 0).all()
        normal = np.stack([synthetic.estimate_normals(depth[i], cam) for i in range(F)])
        normal[~np.isfinite(normal).all(-1)] = (0.0, 0.0, -1.0)
        _KF[key] = (depth, normal, T)
    d, n, T = _KF[key]
    return d[:F].copy(), n[:F], T[:F]


def _engine(hidden=256, blocks=2, n_freqs=6, seed=0):
    from isdf_amd.engine import Engine, NetConfig
    from isdf_amd import synthetic
    eng = Engine(NetConfig(hidden=hidden, blocks=blocks, n_freqs=n_freqs, transform=synthetic.bounds_transform()), "cuda")
    g = torch.Generator().manual_seed(seed)
    eng.params.copy_((0.05 * torch.randn(eng.n_params, generator=g)).cuda())
    eng.pack()
    return eng


def _sc(cam, n_rays, n_strat=19, n_surf=8):
    from isdf_amd.engine import SampleConfig
    return SampleConfig(n_rays=n_rays, n_strat=n_strat, n_surf=n_surf, **cam)


def _sample(eng, kf, sc, ih, iw, seed=0, U_rows=None):
    depth, normal, T = kf
    F = depth.shape[0]
    R0 = F * sc.n_rays
    assert len(ih) == len(iw) == R0 and ih.min() >= 0 and ih.max() < sc.H and iw.min() >= 0 and iw.max() < sc.W
    rng = np.random.RandomState(seed)
    Udraw = rng.uniform(size=(R0, sc.n_strat)).astype(np.float32) if U_rows is None else U_rows
    draws = dict(indices_h=_dev(ih.astype(np.int64)), indices_w=_dev(iw.astype(np.int64)), U=_dev(Udraw))
    if sc.n_surf > 1:
        draws["N_off"] = _dev((0.1 * rng.standard_normal((R0, sc.n_surf - 1))).astype(np.float32))
    idx = torch.arange(F, dtype=torch.int32, device="cuda")
    return eng.sample(_dev(depth), _dev(T), _dev(normal), idx, idx, sc, draws=draws)


def _step(eng, s, sc, optim=None, split_event=None):
    from isdf_amd.engine import LossConfig
    dbg = eng.train_step(s, LossConfig(), sc, debug=True, optim=None if optim is None else dict(optim), split_event=split_event)
    torch.cuda.synchronize()
    return dbg


def _red(eng, F):
    P = eng.n_params
    red = eng.reduce_buf.cpu().numpy()
    return dict(grad=red[:P], ls=red[P:P + 8], bl=red[P + 8:P + 8 + 64 * F].reshape(F, 64),
                bc=red[P + 8 + 64 * F:P + 8 + 128 * F].reshape(F, 64))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _model(s, dbg, sc, F):
    R = int(s["n_valid"].item())
    tot = dbg["tot_loss_mat"][:R].cpu().numpy()
    assert np.isfinite(tot).all() and (tot >= 0).all()
    ib, ih, iw = (s[k][:R].cpu().numpy() for k in ("indices_b", "indices_h", "indices_w"))
    assert np.all(np.diff(ib) >= 0)
    bl, bc = tm.bins(tot, ib, ih, iw, R, F, sc.H, sc.W)
    la, fa = tm.frame_avg(bl, bc)
    return dict(R=R, tot=tot, ib=ib, ih=ih, iw=iw, bl=bl, bc=bc, la=la, fa=fa)


def _check_all_routes(eng, s, sc, F, tag):
    """two-call form + isdf_frame_avg, then the fused tail (update exactly zero): bins, counts, loss_approx and the averages equal
    the model bit for bit.  Returns the model."""
    before = eng.params.clone()
    dbg = _step(eng, s, sc)
    m = _model(s, dbg, sc, F)
    r = _red(eng, F)
    assert np.array_equal(r["bc"], m["bc"]), (tag, "block_cnt")
    assert np.array_equal(_bits(r["bl"]), _bits(m["bl"])), (tag, "block_loss", np.abs(r["bl"] - m["bl"]).max())
    la, fa = eng.frame_avg(F)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(la.cpu().numpy().reshape(F, 64)), _bits(m["la"])), (tag, "loss_approx (isdf_frame_avg)")
    assert np.array_equal(_bits(fa.cpu().numpy()), _bits(m["fa"])), (tag, "frame_avg (isdf_frame_avg)")
    store = torch.full((F,), -7.0, device="cuda")
    dbg2 = _step(eng, s, sc, optim=dict(OPT0, frame_avg_out=store, frame_avg_index=torch.arange(F, dtype=torch.int32, device="cuda")))
    r2 = _red(eng, F)
    assert torch.equal(dbg2["tot_loss_mat"], dbg["tot_loss_mat"]) and torch.equal(eng.params, before), tag
    assert np.array_equal(r2["bc"], m["bc"]) and np.array_equal(_bits(r2["bl"]), _bits(m["bl"])), (tag, "fused bins")
    assert np.array_equal(_bits(dbg2["loss_approx"].cpu().numpy().reshape(F, 64)), _bits(m["la"])), (tag, "loss_approx (fused)")
    assert np.array_equal(_bits(store.cpu().numpy()), _bits(m["fa"])), (tag, "frame_avg (fused)")
    assert r["ls"][4] == r2["ls"][4] == m["R"] * s["S"]
    return m


# ---- a. bins, bit for bit ---------------------------------------------------------------------------------------------------------
def test_duplicate_pixels_last_ray_wins_and_counts_once():
    cam = _cams()["680x1200"]
    H, W = cam["H"], cam["W"]
    F, n = 3, 4000
    rng = np.random.RandomState(5)
    h0, w0 = H // 8 * 3 - 7, W // 8 * 5 - 9              # a 16 x 20 patch across a bin corner
    free = rng.choice(H * W, n, replace=False)
    ih = np.concatenate([h0 + rng.randint(0, 16, n), np.full(n, 401), free // W])
    iw = np.concatenate([w0 + rng.randint(0, 20, n), np.full(n, 77), free % W])
    eng = _engine()
    sc = _sc(cam, n, n_strat=3, n_surf=2)
    m = _check_all_routes(eng, _sample(eng, _kf(F, cam), sc, ih, iw), sc, F, "duplicates")
    assert m["R"] == F * n and m["bc"][0].sum() <= 320 and m["bc"][1].sum() == 1 and m["bc"][2].sum() == n
    # the inputs tell the wrong rules apart (tests/test_step_tail_cpu.py::test_wrong_duplicate_rules_are_told_apart, on this step's values)
    first = tm.bins(m["tot"], m["ib"], m["ih"], m["iw"], m["R"], F, H, W, keep="first")[0]
    assert not np.array_equal(_bits(first[:2]), _bits(m["bl"][:2]))
    print("duplicates: kept %d of %d rays; first-wins would move loss_approx by %.1e of its maximum"
          % (int(m["bc"].sum()), m["R"], np.abs(tm.frame_avg(first, m["bc"])[0] - m["la"]).max() / m["la"].max()))


@pytest.mark.parametrize("empty", [0, 1, 2])
def test_frame_without_a_valid_ray_has_exactly_zero_bins(empty):
    cam = _cams()["680x1200"]
    F, n = 3, 200
    depth, normal, T = _kf(F, cam)
    depth[empty] = 0.0
    rng = np.random.RandomState(6 + empty)
    eng = _engine()
    sc = _sc(cam, n)
    m = _check_all_routes(eng, _sample(eng, (depth, normal, T), sc, rng.randint(0, cam["H"], F * n), rng.randint(0, cam["W"], F * n)),
                          sc, F, "empty frame %d" % empty)
    assert m["R"] == (F - 1) * n
    assert not m["bl"][empty].any() and not m["bc"][empty].any() and not m["la"][empty].any() and m["fa"][empty] == 0
    assert all(m["fa"][f] > 0 for f in range(F) if f != empty)


@pytest.mark.parametrize("raster", ["680x1200", "480x640", "104x168"])
def test_image_corners_and_both_sides_of_every_bin_border(raster):
    cam = _cams()[raster]
    H, W = cam["H"], cam["W"]
    F = 3
    hs, ws = np.meshgrid(tm.border_pixels(H), tm.border_pixels(W), indexing="ij")
    hs, ws = hs.ravel(), ws.ravel()
    n = len(hs)
    rng = np.random.RandomState(8)
    perms = [rng.permutation(n) for _ in range(F)]
    ih, iw = np.concatenate([hs[p] for p in perms]), np.concatenate([ws[p] for p in perms])
    eng = _engine()
    sc = _sc(cam, n)
    m = _check_all_routes(eng, _sample(eng, _kf(F, cam), sc, ih, iw), sc, F, "borders " + raster)
    assert m["R"] == F * n and np.all(m["bc"] == 4)              # 16 x 16 pixels: every bin holds its four corners


@pytest.mark.parametrize("F", [1, 2])
def test_frames_at_and_past_fin_cap_staged_and_unstaged_scan_agree(F):
    """One frame with exactly FIN_CAP, FIN_CAP + 1 and 1.5 FIN_CAP valid rays (F = 2: the long frame second, ten valid rays before it)
    drawn from 10 000 pixels, so most pixels repeat, with pairs placed on both sides of ray index FIN_CAP.  Then the FIN_CAP-ray frame
    (staged keys) again with one more ray PREPENDED on ray 0's pixel: FIN_CAP + 1 rays (keys from global memory), the new ray loses to
    ray 0's, every surviving ray has the pixel and the draws it had -- the two scans must give the same bins bit for bit."""
    cam = _cams()["480x640"]
    H, W = cam["H"], cam["W"]
    cap = C["FIN_CAP"]
    depth, normal, T = _kf(F, cam)
    if F == 2:
        depth[0, 8:, :] = 0.0                                     # frame 0: valid on its first 8 rows only
    eng = _engine()
    res = {}
    for n in FIN_CASES + ("prepended",):
        rng = np.random.RandomState(9)
        nn = cap if n == "prepended" else n
        pix = rng.randint(0, 10000, nn)
        k = np.arange(min(64, nn - cap + 64))
        pix[nn - 1 - k] = pix[50 + k]                              # the last rays repeat early ones: across index FIN_CAP when nn > FIN_CAP
        if nn > cap + 64:
            pix[cap + k] = pix[cap - 1 - k]                        # ... and pairs right at the index
        Urows = rng.uniform(size=(nn, 2)).astype(np.float32)
        if n == "prepended":
            pix, Urows, nn = np.concatenate([pix[:1], pix]), np.concatenate([rng.uniform(size=(1, 2)).astype(np.float32), Urows]), nn + 1
        ih, iw = 100 + pix // 100, 200 + pix % 100
        if F == 2:     # frame 0's slots: ten rays on its valid rows, the rest on invalid pixels; U is consumed per VALID ray
            ih = np.concatenate([np.arange(nn) % 8 * (np.arange(nn) < 10) + 300 * (np.arange(nn) >= 10), ih])
            iw = np.concatenate([np.arange(nn) * 7 % W, iw])
            Urows = np.concatenate([rng.uniform(size=(10, 2)).astype(np.float32), Urows, np.zeros((nn - 10, 2), np.float32)])
        sc = _sc(cam, nn, n_strat=2, n_surf=1)
        s = _sample(eng, (depth, normal, T), sc, ih, iw, U_rows=Urows)
        m = _check_all_routes(eng, s, sc, F, "FIN_CAP case %s, F = %d" % (n, F))
        assert m["R"] == nn + (10 if F == 2 else 0) and m["bc"][F - 1].sum() < 10000
        res[n] = m
    a, b = res[cap], res["prepended"]
    f = F - 1
    assert np.array_equal(_bits(a["bl"][f]), _bits(b["bl"][f])) and np.array_equal(a["bc"][f], b["bc"][f])
    assert np.array_equal(_bits(a["fa"][f]), _bits(b["fa"][f]))


@pytest.mark.parametrize("R", R_CASES)
def test_one_ray_and_one_more_than_the_tail_has_threads(R):
    cam = _cams()["480x640"]
    F = 3
    depth, normal, T = _kf(F, cam)
    rng = np.random.RandomState(10)
    if R == 1:
        n = 1
        depth[0] = 0.0; depth[2] = 0.0
        ih, iw = np.array([5, 239, 7]), np.array([9, 320, 11])
    else:
        n = -(-R // F)
        ih, iw = rng.randint(1, cam["H"], F * n), rng.randint(1, cam["W"], F * n)
        drop = F * n - R                                          # that many rays of frame 1 land on an invalid pixel
        depth[1, 0, 0] = 0.0
        ih[n:n + drop] = 0; iw[n:n + drop] = 0
    eng = _engine()
    sc = _sc(cam, n)
    m = _check_all_routes(eng, _sample(eng, (depth, normal, T), sc, ih, iw), sc, F, "R = %d" % R)
    assert m["R"] == R


# ---- b. every route writes the same averages, where the index says -------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 5, 8, 9])
def test_every_route_writes_the_same_frame_averages_where_the_index_says(F):
    from isdf_amd import _ffi
    cam = _cams()["104x168"]
    n = 150
    rng = np.random.RandomState(20 + F)
    eng = _engine()
    sc = _sc(cam, n)
    s = _sample(eng, _kf(F, cam), sc, rng.randint(0, cam["H"], F * n), rng.randint(0, cam["W"], F * n))
    m = _check_all_routes(eng, s, sc, F, "routes F = %d" % F)
    slots = (rng.permutation(F) * 2 + 1).astype(np.int32)         # permuted and non-contiguous
    size = 2 * F + 3
    want = np.full(size, -7.0, np.float32)
    want[slots] = m["fa"]
    dev_idx = torch.as_tensor(slots, device="cuda")

    def canary():
        return torch.full((size,), -7.0, device="cuda")
    routes = {}
    # fused tail, device index array
    st = canary()
    dbg = _step(eng, s, sc, optim=dict(OPT0, frame_avg_out=st, frame_avg_index=dev_idx))
    routes["fused, device index"] = (st, dbg["loss_approx"])
    if F <= _ffi.MAX_INLINE_FRAMES:
        st = canary()
        dbg = _step(eng, s, sc, optim=dict(OPT0, frame_avg_out=st, frame_avg_index=tuple(int(v) for v in slots)))
        routes["fused, inline index"] = (st, dbg["loss_approx"])
    # (F = 9: an inline list holds at most eight frames, the device array is the only form)
    # isdf_train_step + isdf_frame_avg
    _step(eng, s, sc)
    st = canary()
    la, _ = eng.frame_avg(F, out=st, index=dev_idx)
    routes["isdf_frame_avg"] = (st, la)
    # isdf_train_step + isdf_train_step_finish
    _step(eng, s, sc)
    st = canary()
    dbg = eng.train_step_finish(F, dict(OPT0, frame_avg_out=st, frame_avg_index=dev_idx))
    routes["isdf_train_step_finish"] = (st, dbg["loss_approx"])
    torch.cuda.synchronize()
    for name, (st, la) in routes.items():
        assert np.array_equal(_bits(st.cpu().numpy()), _bits(want)), (name, st.cpu().numpy(), want)
        assert np.array_equal(_bits(la.cpu().numpy().reshape(F, 64)), _bits(m["la"])), name


def test_inline_index_list_is_rewritten_on_the_cached_plan_path():
    """The trainer's form: Philox sampling into the reused buffer set, no debug outputs, so Engine.train_step's SECOND call on the set
    reuses its argument structs and only rewrites the inline index list.  Same batch, another list: the averages (from a debug run of
    the same batch, update exactly zero throughout) land where the new list says, the old slots keep the canary."""
    from isdf_amd.engine import LossConfig
    F, n = 5, 150
    cam = _cams()["104x168"]
    depth, normal, T = (_dev(a) for a in _kf(F, cam))
    eng = _engine()
    sc, lc = _sc(cam, n), LossConfig()
    win = tuple(range(F))
    s = eng.sample(depth, T, normal, win, win, sc, seed=11, offset=3, reuse=True)
    assert s.get("_slot") is not None
    m = _model(s, _step(eng, s, sc, optim=OPT0), sc, F)                 # (debug: never the cached plan)
    size = 2 * F + 3
    store = torch.empty(size, device="cuda")
    la_ptr = None
    for call, slots in enumerate([(1, 3, 5, 7, 9), (8, 0, 6, 2, 12), (4, 5, 6, 7, 8)]):
        store.fill_(-7.0)
        cached = eng._step_plans.get(s["_slot"])
        dbg = eng.train_step(s, lc, sc, optim=dict(OPT0, frame_avg_out=store, frame_avg_index=slots))
        torch.cuda.synchronize()
        if call == 0:
            assert cached is None
            la_ptr = dbg["loss_approx"].data_ptr()
        else:     # the plan of the previous call was taken: same structs, same loss_approx buffer
            assert cached is not None and eng._step_plans[s["_slot"]] is cached and dbg["loss_approx"].data_ptr() == la_ptr
        want = np.full(size, -7.0, np.float32)
        want[list(slots)] = m["fa"]
        assert np.array_equal(_bits(store.cpu().numpy()), _bits(want)), (call, slots, store.cpu().numpy(), want)
        assert np.array_equal(_bits(dbg["loss_approx"].cpu().numpy().reshape(F, 64)), _bits(m["la"])), call


def test_frame_avg_routes_on_hand_made_bins():
    """isdf_frame_avg and isdf_train_step_finish fed bins written by hand (no chain kernel): counts 0, 1 and large, sums 0, tiny and
    large, in every combination across the 64 bins of each frame"""
    F = 4
    cam = _cams()["104x168"]
    eng = _engine()
    sc = _sc(cam, 20)
    rng = np.random.RandomState(30)
    s = _sample(eng, _kf(F, cam), sc, rng.randint(0, cam["H"], F * 20), rng.randint(0, cam["W"], F * 20))
    _step(eng, s, sc)                                             # sizes reduce_buf and the mailbox
    counts = np.array([0, 1, 3, 1000, C["FIN_CAP"], 2.0 ** 24], np.float32)
    sums = np.array([0, 2.0 ** -32, 1e-30, 3e-7, 1.0, 1e4, 3e38 / 64], np.float32)
    bc = counts[rng.randint(0, len(counts), (F, 64))]
    bl = sums[rng.randint(0, len(sums) - 1, (F, 64))] * rng.uniform(0.5, 1.0, (F, 64)).astype(np.float32)
    bl[0] = 0; bc[1] = 0; bl[2, :32] = sums[-1]                   # a frame of zero sums, one of zero counts, one near overflow of the sum
    la, fa = tm.frame_avg(bl, bc)
    P = eng.n_params
    eng.reduce_buf[P:P + 8] = 0                                   # count 0: isdf_train_step_finish skips the update
    eng.reduce_buf[P + 8:P + 8 + 64 * F] = _dev(bl.ravel())
    eng.reduce_buf[P + 8 + 64 * F:P + 8 + 128 * F] = _dev(bc.ravel())
    before = eng.params.clone()
    got = [eng.frame_avg(F)]
    st = torch.full((F,), -7.0, device="cuda")
    got.append((eng.train_step_finish(F, dict(OPT0, frame_avg_out=st))["loss_approx"], st))
    torch.cuda.synchronize()
    with np.errstate(over="ignore"):
        for g_la, g_fa in got:
            assert np.array_equal(_bits(g_la.cpu().numpy().reshape(F, 64)), _bits(la))
            assert np.array_equal(_bits(g_fa.cpu().numpy()), _bits(fa))
    assert torch.equal(eng.params, before)


# ---- c. reductions at every tile count ---------------------------------------------------------------------------------------------
# d = fp32 additions on the longest chain to one output element, from the constants:
#   biases / w_out / b_out   tm.vec_chain_length(tiles): per group 4 per first-loop pass (tree of 8 + accumulate), 3 per second-loop pass,
#                            1 per remainder tile; s += s2; the 16-group sum
#   weight matrices          a K-split slab takes every DW_SPLIT-th tile: ceil(tiles / DW_SPLIT_REG) tiles x TILE_PTS / 16 MFMAs (K = 16)
#                            accumulate into it, then at most DW_SPLIT_PE slabs are added
#   loss sums                the chain kernel adds a tile's TILE_PTS points (at most TILE_PTS - 1 additions in any order), then block 0:
#                            tm.loss_chain_length(tiles) = ceil(tiles / 1 024) + 6 butterfly stages + 16 waves
def _d_vec(t):
    return tm.vec_chain_length(t, C)


def _d_w(t):
    return -(-t // C["DW_SPLIT_REG"]) * (C["TILE_PTS"] // 16) + C["DW_SPLIT_PE"]


def _d_loss(t):
    return C["TILE_PTS"] - 1 + tm.loss_chain_length(t, C)


def _d_small(name, is_weight):
    """roundings inside a SINGLE-TILE run's own value (the aligned sweep's parts).  Bias / b_out: 0 -- the run's gradient is the
    tile's partial row plus zeros.  w_out: 1, its `s += s2` of the two slots.  Weight matrices: the tile's TILE_PTS / 16 MFMAs
    accumulate into ONE slab (in the full run they continue a running accumulator instead), the other slabs are zero slabs."""
    if is_weight:
        return C["TILE_PTS"] // 16
    return 1 if name == "out_alpha.weight" else 0


def _sub_smp(s, lo, hi, F):
    keys = ("pc", "z_vals", "depth_sample", "dirs_C_sample", "dirs_W_sample", "norm_sample", "indices_b", "indices_h", "indices_w")
    d = {k: (None if s.get(k) is None else s[k][lo:hi].clone().contiguous()) for k in keys}
    d.update(n_valid=torch.tensor([hi - lo], dtype=torch.int32, device="cuda"), max_rays=hi - lo, S=s["S"], n_frames=F)
    return d


FORMS = ("two-call", "two-call, split event", "fused, zero update")


def _run_form(eng, s, sc, form):
    if form == "fused, zero update":
        return _step(eng, s, sc, optim=OPT0)
    from isdf_amd import dp
    return _step(eng, s, sc, split_event=dp.new_split_event(eng.device) if form.endswith("split event") else None)


def _check_reduction(eng, tag, full, want, A, tiles, d_extra_tiles, tot64, n_points, worst):
    """full: this run's reduce_buf; want / A: float64 sum and sum of absolute values of the small runs' reduce_bufs"""
    P = eng.n_params
    ls = full[P:P + 8].double()
    assert float(ls[4]) == n_points, (tag, float(ls[4]), n_points)
    dl = _d_loss(tiles)
    e = abs(float(ls[3]) - tot64) / tot64
    worst["loss"] = max(worst.get("loss", 0), e / (dl * U))
    assert e <= dl * U, (tag, "loss_sums[3] vs the float64 sum of tot_loss_mat", e, dl * U)
    # (i) test_gpu_parity.py::test_full_size_step_batch_split_invariance_and_determinism's bars for the same property
    assert torch.allclose(want[P:P + 3], ls[:3], rtol=1e-5, atol=0), (tag, want[P:P + 3], ls[:3])
    g, gs = full[:P].double(), want[:P]
    e = float((g - gs).norm() / g.norm())
    worst["all"] = max(worst.get("all", 0), e / 1e-5)
    assert e < 1e-5, (tag, "gradient vs the sum of the small runs", e)
    # (ii) per tensor: |full - sum|_2 <= d 2^-24 |A|_2
    for k, (off, shp) in eng.slices.items():
        cnt = int(np.prod(shp))
        is_w = k.endswith(".weight") and not k.startswith("out_alpha")
        d = _d_w(tiles) if is_w else _d_vec(tiles)
        if d_extra_tiles:            # the small runs are chunks of several tiles with chains of their own
            d += _d_w(d_extra_tiles) if is_w else _d_vec(d_extra_tiles)
        else:                        # single-tile runs (_d_small): only their own roundings, every other addend is an exact zero
            d += _d_small(k, is_w)
        err = float((g[off:off + cnt] - gs[off:off + cnt]).norm())
        bar = d * U * float(A[off:off + cnt].norm())
        worst[k] = max(worst.get(k, 0), err / bar if bar > 0 else 0.0)
        assert err <= bar, (tag, k, err, bar, d)


@pytest.mark.parametrize("form", FORMS)
def test_reductions_at_every_tile_count(form):
    """ONE batch of N_MAX tiles, S = 16 (four rays per tile), run at n = 1 .. N_MAX tiles by overwriting the device n_valid with 4 n.
    Each tile also runs alone (its four rays at the front of a second buffer set): there its bias / w_out gradient IS the tile's
    partial row and only the remainder loop runs, so the float64 prefix sums of those runs are the expected value at every n and a
    dropped or doubled tile is |part_k| itself against a bound of a few 1e-6 |A|.  No noise: the in-kernel noise is keyed by the
    point's position in the batch.  Here d = d(n) + _d_small: a single-tile run adds nothing to a bias element (its own partial
    row plus exact zeros), 1 to w_out and TILE_PTS / 16 to a weight element."""
    cam = _cams()["480x640"]
    F, n_rays = 4, N_MAX
    assert C["TILE_PTS"] % 16 == 0
    rays_per_tile = C["TILE_PTS"] // 16
    rng = np.random.RandomState(40)
    eng = _engine()
    sc = _sc(cam, n_rays * rays_per_tile // 4, n_strat=8, n_surf=8)
    s = _sample(eng, _kf(F, cam), sc, rng.randint(0, cam["H"], F * sc.n_rays), rng.randint(0, cam["W"], F * sc.n_rays))
    assert int(s["n_valid"].item()) == N_MAX * rays_per_tile
    before = eng.params.clone()
    ref = _run_form(eng, s, sc, form)
    ref = {k: ref[k].clone() for k in ("sdf", "sdf_grad", "tot_loss_mat")}
    nred = eng.reduce_buf.numel()
    parts = torch.empty(N_MAX, nred, dtype=torch.float32, device="cuda")
    for k in range(N_MAX):
        lo = k * rays_per_tile
        dbg = _step(eng, _sub_smp(s, lo, lo + rays_per_tile, F), sc)
        parts[k] = eng.reduce_buf
        for key in ref:                                          # per-point outputs do not depend on the batch: bit for bit
            assert torch.equal(dbg[key][:rays_per_tile], ref[key][lo:lo + rays_per_tile]), (k, key)
    want = torch.zeros(nred, dtype=torch.float64, device="cuda")
    A = torch.zeros(nred, dtype=torch.float64, device="cuda")
    tot64 = ref["tot_loss_mat"].double().sum(-1).cumsum(0)
    worst = {}
    for n in range(1, N_MAX + 1):
        want += parts[n - 1].double()
        A += parts[n - 1].double().abs()
        s["n_valid"].fill_(n * rays_per_tile)
        dbg = _run_form(eng, s, sc, form)
        R = n * rays_per_tile
        for key in ref:
            assert torch.equal(dbg[key][:R], ref[key][:R]), (n, key)
        _check_reduction(eng, "%s, %d tiles" % (form, n), eng.reduce_buf.clone(), want, A, n, 0, float(tot64[R - 1]), R * 16, worst)
        assert torch.equal(eng.params, before), n               # every run saw the same weights
    print(form, "aligned sweep 1 .. %d tiles, worst share of each bar:" % N_MAX, {k: "%.2f" % v for k, v in worst.items()})


def _chunked(eng, s, sc, F, R, chunk_rays):
    nred = eng.reduce_buf.numel()
    want = torch.zeros(nred, dtype=torch.float64, device="cuda")
    A = torch.zeros(nred, dtype=torch.float64, device="cuda")
    outs = []
    for lo in range(0, R, chunk_rays):
        hi = min(R, lo + chunk_rays)
        dbg = _step(eng, _sub_smp(s, lo, hi, F), sc)
        want += eng.reduce_buf.double()
        A += eng.reduce_buf.double().abs()
        outs.append({k: dbg[k][:hi - lo].clone() for k in ("sdf", "sdf_grad", "tot_loss_mat")})
    return want, A, {k: torch.cat([o[k] for o in outs]) for k in outs[0]}


@pytest.mark.parametrize("form", FORMS)
def test_reductions_with_rays_across_tiles_and_a_ragged_last_tile(form):
    """S = 27: rays straddle tiles, the last tile is ragged.  One tile count per boundary of the loop mix, against ray-wise chunks of at
    most CHUNK_TILES tiles (remainder loop only).  The chunks are runs of their own, so their chains count as well:
    d = d(tiles) + d(CHUNK_TILES).  Caveat: A is the sum of |chunk result|, not of |tile partial|; a chunk's own rounding error is
    bounded by its TILES' absolute sums, which are at least |chunk result|, so d(CHUNK_TILES) * 2^-24 * |A| is slightly TIGHTER than
    what can strictly be derived for that share (it can only fail spuriously; measured: at most 0.25 of the bar).  The aligned
    sweep above, where every part is one tile, is the strictly derived one."""
    cam = _cams()["480x640"]
    F, S = 4, 27
    Rmax = max(RAGGED_TILES) * C["TILE_PTS"] // S
    n_rays = -(-Rmax // F)
    rng = np.random.RandomState(41)
    eng = _engine()
    sc = _sc(cam, n_rays)
    s = _sample(eng, _kf(F, cam), sc, rng.randint(0, cam["H"], F * n_rays), rng.randint(0, cam["W"], F * n_rays))
    before = eng.params.clone()
    chunk_rays = CHUNK_TILES * C["TILE_PTS"] // S
    worst = {}
    for t in RAGGED_TILES:
        R = t * C["TILE_PTS"] // S
        assert -(-R * S // C["TILE_PTS"]) == t and R <= F * n_rays
        s["n_valid"].fill_(R)
        dbg = _run_form(eng, s, sc, form)
        full = eng.reduce_buf.clone()
        want, A, outs = _chunked(eng, s, sc, F, R, chunk_rays)
        for key in outs:
            assert torch.equal(dbg[key][:R], outs[key]), (t, key)
        tot64 = float(dbg["tot_loss_mat"][:R].double().sum())
        _check_reduction(eng, "%s, %d tiles (ragged)" % (form, t), full, want, A, t, CHUNK_TILES, tot64, R * S, worst)
        assert torch.equal(eng.params, before)
    print(form, "ragged tile counts", RAGGED_TILES, "worst share of each bar:", {k: "%.2f" % v for k, v in worst.items()})


@pytest.mark.parametrize("net", ["default", "<256, 512>"])
def test_reductions_past_four_thousand_tiles(net):
    """5 frames x 2 000 rays x 27 samples = BIG_TILES tiles (block 0's loss loop passes five times, the first vector loop 33 times)
    against chunks of the BASELINE size; d = d(BIG_TILES) + d(chunk tiles), with the caveat on A of the ragged test.  All three forms."""
    cam = _cams()["480x640"]
    F, n, S = BIG_FRAMES, BIG_RAYS, BIG_S
    rng = np.random.RandomState(42)
    eng = _engine() if net == "default" else _engine(hidden=128, blocks=1, n_freqs=9)
    sc = _sc(cam, n)
    s = _sample(eng, _kf(F, cam), sc, rng.randint(0, cam["H"], F * n), rng.randint(0, cam["W"], F * n))
    R = int(s["n_valid"].item())
    assert R == F * n and -(-R * S // C["TILE_PTS"]) == BIG_TILES
    before = eng.params.clone()
    fulls = {}
    for form in FORMS:
        dbg = _run_form(eng, s, sc, form)
        fulls[form] = (eng.reduce_buf.clone(), {k: dbg[k].clone() for k in ("sdf", "sdf_grad", "tot_loss_mat")})
    want, A, outs = _chunked(eng, s, sc, F, R, BASE_RAYS)
    chunk_tiles = -(-BASE_RAYS * S // C["TILE_PTS"])
    for form, (full, dbg) in fulls.items():
        worst = {}
        for key in outs:
            assert torch.equal(dbg[key][:R], outs[key]), (form, key)
        _check_reduction(eng, "%s, %d tiles" % (form, BIG_TILES), full, want, A, BIG_TILES, chunk_tiles,
                         float(dbg["tot_loss_mat"].double().sum()), R * S, worst)
        print(net, form, "%d tiles, share of each bar:" % BIG_TILES, {k: "%.2f" % v for k, v in worst.items()})
    assert torch.equal(eng.params, before)
    assert torch.equal(fulls[FORMS[0]][0], fulls[FORMS[1]][0]) and torch.equal(fulls[FORMS[0]][0], fulls[FORMS[2]][0])


# ---- d. AdamW --------------------------------------------------------------------------------------------------------------------
NETS = {"default": dict(), "hidden 96 (zero-padded)": dict(hidden=96, blocks=3, n_freqs=4), "512 wide": dict(hidden=512, blocks=3, n_freqs=10)}
HYPER = dict(lr=0.0013, betas=(0.9, 0.999), eps=1e-8)
COUNT = 1728.0          # 1e-12 * 0.37 / 1 728 = 2e-16: (1 - beta2) g^2 = 4.6e-35 stays in fp32's normal range (above 1e-37)


def _adamw_call(eng, route, use_count, grad_scale, wd):
    from isdf_amd import _ffi
    from isdf_amd.engine import _stream
    if route == "shadow":                                         # step_tail_kernel<2>
        eng.adamw(weight_decay=wd, grad_scale=grad_scale, use_device_count=use_count, **HYPER)
        return
    eng.opt_step += 1                                             # shadow == NULL: adamw_kernel
    cnt = eng.reduce_buf[eng.n_params + _ffi.LS_COUNT:] if use_count else None
    _ffi.check(eng.lib.isdf_adamw(ct.byref(eng.cnet), _ffi.ptr(eng.params), _ffi.ptr(eng.exp_avg), _ffi.ptr(eng.exp_avg_sq),
                                  _ffi.ptr(eng.reduce_buf), _ffi.ptr(cnt), float(grad_scale), float(HYPER["lr"]), float(HYPER["betas"][0]),
                                  float(HYPER["betas"][1]), float(HYPER["eps"]), float(wd), int(eng.opt_step), None,
                                  _stream(eng.device)), "isdf_adamw")


@pytest.mark.parametrize("net", sorted(NETS))
def test_adamw_vs_float64_model_on_a_gradient_grid(net):
    """Every element of every parameter tensor against tm.adamw, within tm.adamw_bound (the forward-error bound counted from
    adamw_update, tests/tail_model.py).  Gradients log-uniform over 1e-12 .. 1e2 with random sign and exact zeros (eps-dominated, mixed
    and gradient-dominated denominators in every tensor of more than a few elements), steps 1, 2, 10, 1 000 and 100 000 with the
    moments carried from the model, weight decay on and off, grad_scale 1 and 0.37, with and without the device count.  Both
    stand-alone routes (with the operand copies: tail phase 2; without: adamw_kernel) must agree bit for bit."""
    eng = _engine(**NETS[net])
    n = eng.n_params
    nred = int(eng.lib.isdf_reduce_floats(ct.byref(eng.cnet), 1))
    eng.reduce_buf = torch.zeros(nred, device="cuda")
    eng.reduce_buf[n + 4] = COUNT
    rng = np.random.RandomState(50)
    p_init = eng.params.cpu().numpy()
    worst = dict(p=0.0, m=0.0, v=0.0)
    for wd in (0.0, 0.012):
        for gs in (1.0, 0.37):
            for use_count in (False, True):
                p, m, v = p_init.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
                for step in (1, 2, 10, 1000, 100000):
                    g = tm.grad_grid(n, rng)
                    eng.reduce_buf[:n] = _dev(g)
                    bc = tm.bias_corrections_f32(HYPER["betas"][0], HYPER["betas"][1], step)
                    p1, m1, v1, terms = tm.adamw(p, m, v, g, COUNT if use_count else None, gs, HYPER["lr"], HYPER["betas"], HYPER["eps"],
                                                 wd, step, bc=bc, want_terms=True)
                    dp, dm, dv = tm.adamw_bound(terms, v1, HYPER["betas"], step)
                    got = {}
                    for route in ("shadow", "plain"):
                        eng.params.copy_(_dev(p)); eng.exp_avg.copy_(_dev(m)); eng.exp_avg_sq.copy_(_dev(v))
                        eng.opt_step = step - 1
                        _adamw_call(eng, route, use_count, gs, wd)
                        torch.cuda.synchronize()
                        got[route] = tuple(t.cpu().numpy() for t in (eng.params, eng.exp_avg, eng.exp_avg_sq))
                        if route == "shadow" and step in (1, 1000):      # the operand copies are the updated parameters' (padding units stay 0)
                            kept = eng.shadow.clone()
                            eng.pack()
                            torch.cuda.synchronize()
                            assert torch.equal(kept, eng.shadow), (net, step, "shadow != pack(params)")
                    tag = (net, wd, gs, use_count, step)
                    for a, b in zip(got["shadow"], got["plain"]):
                        assert np.array_equal(_bits(a), _bits(b)), tag
                    for name, a, want, bound in (("p", got["plain"][0], p1, dp), ("m", got["plain"][1], m1, dm), ("v", got["plain"][2], v1, dv)):
                        err = np.abs(a.astype(np.float64) - want)
                        share = float(np.max(err / np.maximum(bound, 1e-300)))
                        worst[name] = max(worst[name], share)
                        bad = np.flatnonzero(err > bound)
                        assert bad.size == 0, (tag, name, bad[:5], a[bad[:5]], want[bad[:5]], bound[bad[:5]], g[bad[:5]])
                    p, m, v = (x.astype(np.float32) for x in (p1, m1, v1))
    print(net, "AdamW worst share of the derived bound:", {k: "%.3f" % x for k, x in worst.items()})


def _real_step_state(eng, F=3, n=150, seed=60):
    cam = _cams()["104x168"]
    rng = np.random.RandomState(seed)
    sc = _sc(cam, n)
    s = _sample(eng, _kf(F, cam), sc, rng.randint(0, cam["H"], F * n), rng.randint(0, cam["W"], F * n))
    return s, sc


@pytest.mark.parametrize("net", sorted(NETS))
def test_three_adamw_routes_leave_identical_state_on_a_real_gradient(net):
    """The fused step (tail phase 0), isdf_train_step + isdf_adamw with the operand copies (phase 2) and without (adamw_kernel), from
    the same state on the same batch: bit-identical parameters and moments; the two that keep operand copies keep identical ones,
    equal to a fresh pack of the updated parameters.  The update itself is held to the float64 model within its bound."""
    opt = dict(weight_decay=0.012, grad_scale=0.37, **HYPER)
    states = {}
    for route in ("fused", "shadow", "plain"):
        eng = _engine(**NETS[net])
        g = torch.Generator().manual_seed(3)
        eng.exp_avg.copy_((1e-3 * torch.randn(eng.n_params, generator=g)).cuda())
        eng.exp_avg_sq.copy_((1e-6 * torch.rand(eng.n_params, generator=g)).cuda())
        eng.opt_step = 7
        start = tuple(t.cpu().numpy() for t in (eng.params, eng.exp_avg, eng.exp_avg_sq))
        s, sc = _real_step_state(eng)
        if route == "fused":
            _step(eng, s, sc, optim=opt)
        else:
            _step(eng, s, sc)
            _adamw_call(eng, route, True, opt["grad_scale"], opt["weight_decay"])
        torch.cuda.synchronize()
        assert eng.opt_step == 8
        states[route] = dict(p=eng.params.clone(), m=eng.exp_avg.clone(), v=eng.exp_avg_sq.clone(), red=eng.reduce_buf.clone())
        if route != "plain":
            states[route]["shadow"] = eng.shadow.clone()
            eng.pack()
            torch.cuda.synchronize()
            assert torch.equal(states[route]["shadow"], eng.shadow), (route, "shadow != pack(params)")
    for k in ("p", "m", "v", "red"):
        for route in ("shadow", "plain"):
            a, b = states["fused"][k], states[route][k]
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (net, route, k, int((a != b).sum()))
    assert torch.equal(states["fused"]["shadow"], states["shadow"]["shadow"])
    n = eng.n_params
    red = states["fused"]["red"].cpu().numpy()
    bc = tm.bias_corrections_f32(HYPER["betas"][0], HYPER["betas"][1], 8)
    p1, m1, v1, terms = tm.adamw(*start, red[:n], red[n + 4], opt["grad_scale"], HYPER["lr"], HYPER["betas"], HYPER["eps"], opt["weight_decay"],
                                 8, bc=bc, want_terms=True)
    for name, got, want, bound in zip("pmv", (states["fused"][k].cpu().numpy() for k in "pmv"), (p1, m1, v1), tm.adamw_bound(terms, v1, HYPER["betas"], 8)):
        err = np.abs(got.astype(np.float64) - want)
        assert np.all(err <= bound), (net, name, float(np.max(err / np.maximum(bound, 1e-300))))
    g = np.abs(red[:n] / red[n + 4])
    print(net, "mean gradient of a real step: median |g| %.1e, 1st percentile %.1e" % (np.median(g), np.percentile(g, 1)))


@pytest.mark.parametrize("net", ["default", "hidden 96 (zero-padded)"])
def test_empty_batch_and_zero_count_change_nothing_on_any_route(net):
    """A batch without a valid ray (every depth 0) and a reduced count of 0: parameters, both moments AND the operand copies are
    unchanged bit for bit on the fused tail, isdf_adamw with and without the operand copies and isdf_train_step_finish; the bins,
    loss_approx, the frame averages and the loss sums are exactly 0."""
    cam = _cams()["104x168"]
    F, n = 3, 50
    depth, normal, T = _kf(F, cam)
    depth[:] = 0.0
    eng = _engine(**NETS[net])
    g = torch.Generator().manual_seed(4)
    eng.exp_avg.copy_((1e-3 * torch.randn(eng.n_params, generator=g)).cuda())
    eng.exp_avg_sq.copy_((1e-6 * torch.rand(eng.n_params, generator=g)).cuda())
    keep = [t.clone() for t in (eng.params, eng.exp_avg, eng.exp_avg_sq, eng.shadow)]
    rng = np.random.RandomState(61)
    sc = _sc(cam, n)
    s = _sample(eng, (depth, normal, T), sc, rng.randint(0, cam["H"], F * n), rng.randint(0, cam["W"], F * n))
    assert int(s["n_valid"].item()) == 0
    opt = dict(weight_decay=0.012, **HYPER)

    def unchanged(tag):
        torch.cuda.synchronize()
        for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "shadow"), keep, (eng.params, eng.exp_avg, eng.exp_avg_sq, eng.shadow)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (tag, name)
        r = _red(eng, F)
        assert not r["ls"].any() and not r["bl"].any() and not r["bc"].any(), tag
    st = torch.full((F,), -7.0, device="cuda")
    dbg = _step(eng, s, sc, optim=dict(opt, frame_avg_out=st))
    unchanged("fused")
    assert not st.cpu().numpy().any() and not dbg["loss_approx"].cpu().numpy().any()
    _step(eng, s, sc)
    eng.reduce_buf[:eng.n_params] = 1.0                            # a gradient that WOULD move everything
    for route in ("shadow", "plain"):
        _adamw_call(eng, route, True, 1.0, 0.012)
        unchanged(route)
    st = torch.full((F,), -7.0, device="cuda")
    dbg = eng.train_step_finish(F, dict(opt, frame_avg_out=st))
    eng.reduce_buf[:eng.n_params] = 0.0
    unchanged("isdf_train_step_finish")
    assert not st.cpu().numpy().any() and not dbg["loss_approx"].cpu().numpy().any()
    la, fa = eng.frame_avg(F)
    torch.cuda.synchronize()
    assert not la.cpu().numpy().any() and not fa.cpu().numpy().any()
