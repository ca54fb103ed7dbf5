"""The step kernels request memory BEFORE they know how many points are valid (chain.hip: the tile's points, layer 0's weights and
bias next to n_valid; dw.hip: a K-split's first tile and its pe_aux rows).  Nothing at or beyond the valid points may reach a result.
Needs a real MI355X: `pytest -m gpu`.

Each case runs one fused training step (sampler -> chain -> dW -> step tail with AdamW and the frame averages) twice from the same
state on the default net: once with the engine workspace (spill tiles, pe_aux, partials, slabs) and both of the sampler's point
buffers zero-filled BEFORE the sampler runs, once with the same bytes set to 0xFF -- a NaN in fp32, fp16 and e4m3 alike.  Whatever
the step does not write itself keeps that fill, so a value picked up from beyond the valid points shows as a NaN or as a changed bit.
Required: loss sums, the whole reduce_buf, parameters, both AdamW moments and the frame averages are finite and BITWISE equal between
the two runs.

Shapes (27 samples per ray, 64-point tiles): the smallest at which the early requests can go wrong --
  1 x 3 rays    81 points, 2 tiles: a partly filled last tile; every dW unit has more K-splits than tiles (exact zero slabs)
  2 x 40 rays   2 160 points, 34 tiles: K-splits with two tiles and with one, PE units with empty splits
  2 x 40, half  depth zeroed on half of each image: whole trailing workgroups beyond the valid points, capacity unchanged
  all depth 0   n_valid = 0: no update, count 0
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CAM = dict(H=8 * 13, W=8 * 21, fx=84.0, fy=84.0, cx=83.5, cy=51.5)
TILE = 64
OPT = dict(lr=0.0013, weight_decay=0.012)
_KF = {}


def _kf(F):
    """F synthetic keyframes without invalid pixels (the cases decide what is valid)"""
    from isdf_amd import synthetic
    if "kf" not in _KF:
        T = synthetic.trajectory(2 * 40)[::40][:2]
        depth = np.stack([synthetic.render_depth(T[i], CAM, rng=None) for i in range(2)])
        assert np.isfinite(depth).all() and (depth > 0).all()
        normal = np.stack([synthetic.estimate_normals(depth[i], CAM) for i in range(2)])
        normal[~np.isfinite(normal).all(-1)] = (0.0, 0.0, -1.0)
        _KF["kf"] = (depth, normal, T)
    d, n, T = _KF["kf"]
    return d[:F].copy(), n[:F], T[:F]


def _run(kf, n_rays, fill):
    """one fused step on a fresh engine whose workspace and sampler point buffers were filled with byte `fill` beforehand"""
    from isdf_amd.engine import Engine, NetConfig, LossConfig, SampleConfig
    from isdf_amd import synthetic
    depth, normal, T = (torch.as_tensor(np.ascontiguousarray(a)).cuda() for a in kf)
    F = depth.shape[0]
    eng = Engine(NetConfig(transform=synthetic.bounds_transform()), "cuda")
    g = torch.Generator().manual_seed(0)
    eng.params.copy_((0.05 * torch.randn(eng.n_params, generator=g)).cuda())
    eng.exp_avg.copy_((1e-3 * torch.randn(eng.n_params, generator=g)).cuda())
    eng.exp_avg_sq.copy_((1e-6 * torch.rand(eng.n_params, generator=g)).cuda())
    eng.pack()
    before = eng.params.clone()
    sc = SampleConfig(n_rays=n_rays, n_strat=19, n_surf=8, **CAM)
    ws = eng.workspace(F * n_rays * sc.S, True)
    ws.fill_(fill)
    idx = torch.arange(F, dtype=torch.int32, device="cuda")
    sample = lambda: eng.sample(depth, T, normal, idx, idx, sc, seed=1, offset=0, reuse=True)
    sample(); sample()                                    # both buffer sets of the sampler's ring exist now
    torch.cuda.synchronize()
    for bufs in eng._smp_ring[1]:
        bufs["pc"].view(torch.uint8).fill_(fill)
    s = sample()                                          # the run's own sampler call writes the valid points only
    store = torch.full((F,), -7.0, device="cuda")
    eng.train_step(s, LossConfig(), sc, optim=dict(OPT, frame_avg_out=store, frame_avg_index=idx))
    torch.cuda.synchronize()
    assert eng._ws.data_ptr() == ws.data_ptr()
    R = int(s["n_valid"].item())
    out = dict(loss_sums=eng.loss_sums(), reduce_buf=eng.reduce_buf, params=eng.params, exp_avg=eng.exp_avg,
               exp_avg_sq=eng.exp_avg_sq, frame_avg_losses=store)
    return R, sc.S, {k: v.cpu().numpy().copy() for k, v in out.items()}, before.cpu().numpy()


def _both(kf, n_rays):
    Rc, S, clean, before = _run(kf, n_rays, 0x00)
    Rp, _, poisoned, _ = _run(kf, n_rays, 0xFF)
    assert Rc == Rp
    for k in clean:
        assert np.isfinite(clean[k]).all(), ("clean", k)
        assert np.isfinite(poisoned[k]).all(), ("poisoned", k, int((~np.isfinite(poisoned[k])).sum()))
        a, b = clean[k].view(np.uint32), poisoned[k].view(np.uint32)
        assert np.array_equal(a, b), (k, int((a != b).sum()))
    return Rc, S, clean, before


def test_partly_filled_last_tile_and_zero_slabs():
    R, S, out, before = _both(_kf(1), 3)
    assert R == 3 and -(-R * S // TILE) == 2 and out["loss_sums"][4] == R * S
    assert not np.array_equal(out["params"], before)


def test_splits_with_two_tiles_one_tile_and_none():
    R, S, out, before = _both(_kf(2), 40)
    assert R == 80 and -(-R * S // TILE) == 34 and out["loss_sums"][4] == R * S
    assert not np.array_equal(out["params"], before)


def test_trailing_workgroups_beyond_the_valid_points():
    depth, normal, T = _kf(2)
    depth[:, :, CAM["W"] // 2:] = 0.0
    R, S, out, before = _both((depth, normal, T), 40)
    assert 16 <= R <= 64, R                               # about half of the 80 rays: whole tiles of the 34 lie beyond the valid points
    assert out["loss_sums"][4] == R * S
    assert not np.array_equal(out["params"], before)


def test_no_valid_ray():
    depth, normal, T = _kf(2)
    depth[:] = 0.0
    R, S, out, before = _both((depth, normal, T), 40)
    assert R == 0 and not out["loss_sums"].any()          # count 0 reported ...
    assert np.array_equal(out["params"].view(np.uint32), before.view(np.uint32))      # ... and the update skipped
