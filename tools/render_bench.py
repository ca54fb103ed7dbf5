#!/usr/bin/env python3
"""Rendered-view timing on the trained default net (fixture `trained_default`): the eager path the reference's render methods
ran around SDFMapHIP before they were bound (restated from trainer.py:1055-1147,1225-1280 -- per keyframe a host resize and an
upload, sample_along_rays as torch ops, one forward, sdf_render_depth's ops, an autograd pass for the input gradient, a 3x3
inverse and the rotation) against the bound path (one isdf_render_views call per pass).  The two alternate within one process;
device-synchronised wall time per call, medians over --reps.

    python tools/render_bench.py [--reps 10] [--out profiles/render_bench.json]

Sizes: frames_vis (render_depth_vis + render_normals_vis) at K = 5, 20, 60 keyframes of 680 x 1200 depth (vis raster 42 x 75,
19 samples); latest_frame_vis's render (20 samples at 42 x 75, upsample, 12 at 85 x 150, normals); one full-resolution view
(680 x 1200 rays, 19 samples, normals).  The host resize of the eager path is the numpy INTER_LINEAR restatement
(tests/render_oracle.py; cv2 is not a dependency here)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import golden_util as gu            # noqa: E402
from tests import render_oracle as ro          # noqa: E402

H, W = 680, 1200
FX, FY, CX, CY = 600.0, 600.0, 599.5, 339.5
MFMA_PEAK_FP16 = 2.5e15          # dense fp16 MFMA FLOP/s of an MI355X


def dirs(h, w, f):
    c, r = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    d = np.stack([(c - np.float32(CX / f)) / np.float32(FX / f), (r - np.float32(CY / f)) / np.float32(FY / f), np.ones_like(c)], -1)
    return torch.from_numpy(d.reshape(-1, 3)).cuda()


# ---- the eager path (pre-PR): the reference's chain around SDFMapHIP --------------------------------------------------------
def eager_samples(T, lo, hi, S, dC, U):
    R_WC = T[:, :3, :3]
    dW = (R_WC * dC[..., None, :]).sum(-1).view(-1, 3)
    o = T[:, :3, -1].view(-1, 3)
    if torch.is_tensor(hi):
        rng = (hi - lo)[:, None]
        lim = torch.linspace(0, 1, S + 1, device=dW.device)[None, :].repeat(dW.shape[0], 1) * rng + (lo[:, None] if torch.is_tensor(lo) else lo)
        blen = rng / S
    else:
        lim = torch.linspace(lo, hi, S + 1, device=dW.device)[None, :]
        blen = (hi - lo) / S
    z = lim[..., :-1] + U * blen
    return o[:, None, :] + dW[:, None, :] * z[:, :, None], z


def eager_render_depth(z, sdf):
    n = sdf.size(1)
    mx = ((sdf < 0) * torch.arange(n, 0, -1, device=sdf.device)).argmax(dim=1)
    ar = torch.arange(z.size(0), device=z.device)
    d = z[ar, mx] + sdf[ar, mx]
    d[mx == n - 1] = 0.
    return d


def eager_normals(sdf_map, T, depth, dC):
    dW = (T[:, :3, :3] * dC[..., None, :]).sum(-1).view(-1, 3)
    pc = (T[:, :3, -1].view(-1, 3) + dW * depth.flatten()[:, None]).detach().requires_grad_()
    with torch.enable_grad():
        sdf = sdf_map(pc)
        g, = torch.autograd.grad(sdf, pc, torch.ones_like(sdf))
    nW = -g / (g.norm(dim=1, keepdim=True) + 1e-4)
    R_CW = T[:, :3, :3].inverse()
    return (R_CW * nW[..., None, :]).sum(-1)


def eager_frames_vis(sdf_map, Ts, depth_np, dC, hv, wv, S, U):
    ds = []
    with torch.no_grad():
        for b in range(Ts.shape[0]):
            rs = torch.from_numpy(ro.cv_resize_linear(depth_np[b], wv, hv)).cuda()
            pc, z = eager_samples(Ts[b:b + 1], 0.07, (rs + 0.8).flatten(), S, dC, U[b])
            ds.append(eager_render_depth(z, sdf_map(pc)).view(hv, wv))
    ds = torch.stack(ds)
    ns = torch.stack([eager_normals(sdf_map, Ts[b:b + 1], ds[b], dC) for b in range(Ts.shape[0])])
    return ds, ns


def eager_latest(sdf_map, T, dC, dCu, hv, wv, hu, wu, Uc, Uf):
    with torch.no_grad():
        pc, z = eager_samples(T, 0.07, 12.0, 20, dC, Uc)
        d = eager_render_depth(z, sdf_map(pc))
        up = torch.nn.functional.interpolate(d.view(1, 1, hv, wv), size=[hu, wu], mode="bilinear", align_corners=True).view(-1)
        pc, z = eager_samples(T, up - 0.1, up + 0.1, 12, dCu, Uf)
        d = eager_render_depth(z, sdf_map(pc))
    n = eager_normals(sdf_map, T, d[None], dCu)
    return d, n


# ---- the bound path ---------------------------------------------------------------------------------------------------------
def bound_frames_vis(eng, Ts, depth_dev, dC, hv, wv, S, U):
    d, _ = eng.render_views(Ts, dC, hv, wv, S, depth_images=depth_dev, min_depth=0.07, depth_offset=0.8, draws=U)
    _, n = eng.render_views(Ts, dC, hv, wv, depth=d)
    return d.view(-1, hv, wv), n


def bound_latest(eng, T, dC, dCu, hv, wv, hu, wu, Uc, Uf):
    c, _ = eng.render_views(T, dC, hv, wv, 20, scalar_range=(0.07, 12.0), draws=Uc)
    return eng.render_views(T, dCu, hu, wu, 12, upsample=c.view(1, hv, wv), depth_offset=0.1, draws=Uf, want_normals=True)


def timed(fn, reps):
    out, res = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out)) * 1e3, res


def count_launches(fn):
    """kernel launches of one call (torch profiler, device activity)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as p:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in p.events() if e.device_type.name == "CUDA" and "Memcpy" not in e.name and "Memset" not in e.name)


def compare(d_e, n_e, d_b, n_b):
    d_e, d_b = d_e.reshape(-1), d_b.reshape(-1)
    close = (d_e - d_b).abs() <= 1e-3
    return dict(depth_same_crossing_frac=float(close.float().mean()),
                depth_max_abs_diff_where_same=float((d_e - d_b).abs()[close].max()) if bool(close.any()) else None,
                normals_rel_l2=float((n_e.reshape(-1, 3) - n_b.reshape(-1, 3)).norm() / n_e.norm()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ks", type=int, nargs="+", default=[5, 20, 60])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from isdf_amd.modules import PositionalEncodingHIP, SDFMapHIP
    g = gu.load("trained_default")
    net = g["net"]
    pe = PositionalEncodingHIP(min_deg=0, max_deg=int(net[2]) - 1, scale=float(net[3]),
                               transform=torch.from_numpy(g["bounds_T"].astype(np.float32)))
    sdf_map = SDFMapHIP(pe, hidden_size=int(net[0]), hidden_layers_block=int(net[1]), scale_output=float(net[4]), device="cuda")
    sdf_map.load_state_dict({k: torch.from_numpy(v) for k, v in gu.params_of(g).items()})
    eng = sdf_map.engine
    hv, wv, hu, wu = H // 16, W // 16, H // 8, W // 8
    dC, dCu = dirs(hv, wv, 16), dirs(hu, wu, 8)
    Kmax = max(a.ks)
    depth_np, _, _ = gu.synth_frames(np.random.RandomState(1), Kmax, H, W, FX, FY, CX, CY)
    T_all = torch.from_numpy(np.repeat(g["T_WC_batch"].astype(np.float32), -(-Kmax // 5), 0)[:Kmax]).cuda()
    depth_dev = torch.from_numpy(depth_np).cuda()
    gen = torch.Generator(device="cuda").manual_seed(0)
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, timing="device-synchronised wall time per call, median",
               note="eager = the reference's per-keyframe chain around SDFMapHIP (pre-PR), bound = isdf_render_views", cases={})
    for K in a.ks:
        S = 19
        U = torch.rand(K, hv * wv, S, device="cuda", generator=gen)
        Ts, dd = T_all[:K], depth_dev[:K]
        fe = lambda: eager_frames_vis(sdf_map, Ts, depth_np[:K], dC, hv, wv, S, U)
        fb = lambda: bound_frames_vis(eng, Ts, dd, dC, hv, wv, S, U)
        fe(); fb()
        te, tb = [], []
        for _ in range(a.reps):      # alternate the two paths
            te.append(timed(fe, 1)[0]); tb.append(timed(fb, 1)[0])
        (de, ne), (db, nb) = fe(), fb()
        res["cases"]["frames_vis_K%d" % K] = dict(
            eager_ms=float(np.median(te)), bound_ms=float(np.median(tb)), speedup=float(np.median(te) / np.median(tb)),
            launches_eager=count_launches(fe), launches_bound=count_launches(fb),
            host_syncs_eager="%d (one host resize + upload per keyframe)" % K, host_syncs_bound=0,
            points=K * hv * wv * (S + 1), bytes_samples_bound=K * hv * wv * S * 20 + K * hv * wv * 32,
            outputs=compare(de, ne, db, nb))
        print(json.dumps({k: v for k, v in res["cases"]["frames_vis_K%d" % K].items() if k != "outputs"}), flush=True)
    T1 = T_all[:1]
    Uc = torch.rand(1, hv * wv, 20, device="cuda", generator=gen)
    Uf = torch.rand(1, hu * wu, 12, device="cuda", generator=gen)
    fe = lambda: eager_latest(sdf_map, T1, dC, dCu, hv, wv, hu, wu, Uc[0], Uf[0])
    fb = lambda: bound_latest(eng, T1, dC, dCu, hv, wv, hu, wu, Uc, Uf)
    fe(); fb()
    te, tb = [], []
    for _ in range(a.reps):
        te.append(timed(fe, 1)[0]); tb.append(timed(fb, 1)[0])
    (de, ne), (db, nb) = fe(), fb()
    res["cases"]["latest_frame_vis_render"] = dict(eager_ms=float(np.median(te)), bound_ms=float(np.median(tb)),
                                                    speedup=float(np.median(te) / np.median(tb)),
                                                    launches_eager=count_launches(fe), launches_bound=count_launches(fb),
                                                    host_syncs_bound=0, outputs=compare(de, ne, db, nb))
    print(json.dumps({k: v for k, v in res["cases"]["latest_frame_vis_render"].items() if k != "outputs"}), flush=True)
    # one full-resolution view: 680 x 1200 rays, 19 samples, normals
    dF = dirs(H, W, 1)
    U = torch.rand(1, H * W, 19, device="cuda", generator=gen)
    fb = lambda: eng.render_views(T1, dF, H, W, 19, depth_images=depth_dev[:1], min_depth=0.07, depth_offset=0.8, draws=U,
                                  want_normals=True)
    fb()
    tb, _ = timed(fb, a.reps)
    pts = H * W * 19
    flop = 2 * 460033 * pts + 6 * 460033 * H * W          # forward per sample point, forward + input-gradient sweep per ray
    res["cases"]["full_view_680x1200_S19_normals"] = dict(bound_ms=tb, points_per_s=pts / (tb * 1e-3),
                                                           mfma_peak_share=flop / (tb * 1e-3) / MFMA_PEAK_FP16,
                                                           launches_bound=count_launches(fb), eager_ms="not measured")
    print(json.dumps(res["cases"]["full_view_680x1200_S19_normals"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
