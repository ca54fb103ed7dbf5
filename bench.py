#!/usr/bin/env python3
"""Benchmark of the iSDF training hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is one pass of `Trainer.step`'s hot path (sampler -> fused PE+MLP chain
-> dW -> reductions -> [RCCL all-reduce] -> AdamW -> frame averages) over one
batch of synthetic posed-depth keyframes.  Workload (BASELINE.json configs[1],
read as SURVEY 0 explains): replicaCAD.json defaults = 5 keyframes x 200 rays x
27 samples = 27 000 points per rank-step, 680x1200 depth, 6x256 Softplus MLP
with 255-wide icosahedron PE, eikonal + normal terms on, bounds "ray".  With N
ranks every rank draws its own 1000 rays (rays shard over ranks, weak scaling:
N x 27k points per optimiser step) and ONE RCCL all-reduce carries the flat
[grad | loss sums | bins] buffer.  Prints one JSON line on rank 0.

A plain run sets up, warms up, times the K steps and prints the headline figures.  `--full` adds everything else the line
has carried (pipelined and windowed rates, per-kernel times and rooflines, the CPU / eager-GPU baselines, the accuracy leg,
the fp16 fast mode); `--dump-outputs DIR` writes what the last timed step computed as .npy files.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

M_MAC = 255 * 256 + 4 * 256 * 256 + (256 + 255) * 256 + 256      # 458 496 MAC/point
MFMA_PEAK = 2.5e15                                                # dense bf16/f16 MFMA peak, gfx950


class HipEvents:
    """hipEvent_t via ctypes on the HIP runtime (events live on the stream the kernels use)."""

    def __init__(self, n):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.ev = (ctypes.c_void_p * n)()
        for i in range(n):
            e = ctypes.c_void_p()
            assert self.hip.hipEventCreate(ctypes.byref(e)) == 0
            self.ev[i] = e

    def prime(self, stream):
        """record every event once, outside any timed region: an event's FIRST record allocates (seen as a 30-80 us step)"""
        for e in self.ev:
            assert self.hip.hipEventRecord(ctypes.c_void_p(e), ctypes.c_void_p(stream)) == 0

    def group(self, i, k=4):
        return ctypes.cast(ctypes.byref(self.ev, i * k * ctypes.sizeof(ctypes.c_void_p)),
                           ctypes.POINTER(ctypes.c_void_p))

    def ms(self, a, b):
        out = ctypes.c_float()
        rc = self.hip.hipEventElapsedTime(ctypes.byref(out), ctypes.c_void_p(self.ev[a]), ctypes.c_void_p(self.ev[b]))
        assert rc == 0, rc
        return out.value


def latest_profile(suffix):
    """newest committed profiles/rNN_<suffix> (PMC passes cannot run inside the timed region: bench.py quotes the committed
    rocprofv3 --pmc measurement of this same command)"""
    for r in range(9, 0, -1):
        p = os.path.join(ROOT, "profiles", "r%02d_%s" % (r, suffix))
        if os.path.exists(p):
            return p
    return None


def reference_config():
    """replicaCAD.json defaults (isdf/train/configs/replicaCAD.json) for the hot path."""
    return {
        "dataset": {"camera": {"w": 1200, "h": 680, "fx": 600.0, "fy": 600.0, "cx": 599.5, "cy": 339.5}},
        "optimiser": {"lr": 0.0013, "weight_decay": 0.012},
        "sample": {"n_rays": 200, "n_rays_is_kf": 400, "n_strat_samples": 19, "n_surf_samples": 8,
                   "depth_range": [0.07, 12.0], "dist_behind_surf": 0.1},
        "model": {"do_active": 0, "frac_time_perception": 1.0, "scale_output": 0.14, "noise_std": 0.25,
                  "noise_kf": 0.08, "noise_frame": 0.04, "window_size": 5, "hidden_layers_block": 2,
                  "hidden_feature_size": 256, "iters_per_kf": 60, "iters_per_frame": 10,
                  "kf_dist_th": 0.1, "kf_pixel_ratio": 0.65,
                  "embedding": {"scale_input": 0.05937489, "n_embed_funcs": 5}},
        "loss": {"bounds_method": "ray", "loss_type": "L1", "trunc_weight": 5.38344020,
                 "trunc_distance": 0.29365022, "eik_weight": 0.268, "eik_apply_dist": 0.1,
                 "grad_weight": 0.018, "orien_loss": 0},
    }


def make_keyframes(cam, n, seed=1):
    from isdf_amd import synthetic
    cache = "/tmp/isdf_bench_kf_%dx%d_%d_%d.npz" % (cam["H"], cam["W"], n, seed)
    if os.path.exists(cache):
        try:
            z = np.load(cache)
            return z["depth"], z["normal"], z["T"]
        except Exception:
            pass
    d, nrm, T = synthetic.keyframes(n, cam, seed=seed, noise_std=0.01)
    try:
        tmp = cache + ".%d.tmp.npz" % os.getpid()
        np.savez(tmp, depth=d, normal=nrm, T=T)
        os.replace(tmp, cache)
    except Exception:
        pass
    return d, nrm, T


def _cpu_baseline_child(threads, ftz, budget_s, rays_per_frame, min_steps=1):
    """One configuration of the CPU baseline in its OWN process: flush-to-zero is a per-thread mode that the intra-op worker
    threads inherit when they are created, so it has to be set before the first parallel region and cannot be switched inside
    one process (round 3 measured "as shipped" with workers that still flushed)."""
    torch.set_flush_denormal(bool(ftz))
    torch.set_num_threads(threads)
    from oracle import torch_port as tp
    from isdf_amd import synthetic
    cfg = reference_config()
    cam = dict(synthetic.REPLICA_CAM)
    depth, normal, T = make_keyframes(cam, cfg["model"]["window_size"])
    sc = dict(n_rays=rays_per_frame, n_strat=19, n_surf=8, min_depth=0.07, dist_behind_surf=0.1)
    lc = dict(trunc_distance=cfg["loss"]["trunc_distance"], loss_type="L1", trunc_weight=cfg["loss"]["trunc_weight"],
              eik_apply_dist=0.1, eik_weight=cfg["loss"]["eik_weight"], grad_weight=cfg["loss"]["grad_weight"])
    d, n, Tt = torch.from_numpy(depth), torch.from_numpy(normal), torch.from_numpy(T)
    torch.manual_seed(1)
    net = tp.PortNet(256, 2, 6, 0.05937489, 0.14, None)
    opt = torch.optim.AdamW(net.parameters(), lr=0.0013, weight_decay=0.012)
    gen = torch.Generator().manual_seed(1)
    tp.train_step(net, opt, d, Tt, n, cam, sc, lc, 0.25, gen)           # warm-up
    t0 = time.perf_counter(); k = 0
    while True:
        tp.train_step(net, opt, d, Tt, n, cam, sc, lc, 0.25, gen); k += 1
        el = time.perf_counter() - t0
        if (el > budget_s and k >= min_steps) or k >= 40:
            break
    print(json.dumps({"steps_per_s": k / el, "steps": k, "seconds": el, "threads": threads, "ftz": bool(ftz)}), flush=True)


def cpu_baseline(cfg, threads_list=None, budget_s=26.0):
    """The reference's CPU PyTorch path (torch port, oracle/torch_port.py) on the host cores of this box, bounded sample of
    the same workload.  SURVEY 8d: all host cores, stated; time both flush-denormal settings and "use the faster as the
    denominator".  So: the thread count is SWEPT with denormals flushed (more threads are not faster for 27k x 256 GEMMs: 16 of 256
    logical CPUs beat all of them), the two fastest thread counts are re-run as shipped (denormals not flushed), and the FASTEST
    of all these settings -- whichever it is on this box -- is then timed for >= 10 steps and becomes the denominator.  Every
    configuration runs in its own process (see _cpu_baseline_child)."""
    import subprocess
    cores = os.cpu_count() or 1
    cands = sorted({t for t in (threads_list or [8, 16, 32, 64, 128, cores]) if 1 <= t <= cores}) or [cores]
    per = max(2.0, 0.45 * budget_s / len(cands))

    def child(th, ftz, b, min_steps=1):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-child", str(th), str(int(ftz)), str(b),
                              str(cfg["sample"]["n_rays"]), str(min_steps)], capture_output=True, text=True, timeout=600)
        return json.loads(out.stdout.strip().splitlines()[-1])
    sweep = [child(th, True, per) for th in cands]
    top2 = sorted(sweep, key=lambda r: -r["steps_per_s"])[:2]
    shipped = [child(r["threads"], False, per) for r in top2]
    pick = max(sweep + shipped, key=lambda r: r["steps_per_s"])
    final = child(pick["threads"], pick["ftz"], 0.25 * budget_s, min_steps=10)      # the denominator: >= 10 timed steps
    best_ftz = max(sweep, key=lambda r: r["steps_per_s"])
    best_shipped = max(shipped, key=lambda r: r["steps_per_s"])
    label = "flush-denormal ON (the reference ships with it off)" if final["ftz"] else "as shipped: denormals NOT flushed"
    return {"value": round(final["steps_per_s"], 4), "unit": "train-steps/s", "cores": final["threads"], "kind": "port",
            "flush_denormal": bool(final["ftz"]),
            "sample": "%d steps of the same 27k-point workload in %.1f s, torch %s CPU, %d threads, %s -- the fastest of a sweep over "
                      "thread counts (denormals flushed: %s) and, at its two fastest thread counts, the as-shipped setting (%s); %d logical CPUs"
                      % (final["steps"], final["seconds"], torch.__version__, final["threads"], label,
                         {r["threads"]: round(r["steps_per_s"], 3) for r in sweep},
                         {r["threads"]: round(r["steps_per_s"], 3) for r in shipped}, cores),
            "thread_sweep_steps_per_s": {str(r["threads"]): round(r["steps_per_s"], 4) for r in sweep},
            "as_shipped_steps_per_s": {str(r["threads"]): round(r["steps_per_s"], 4) for r in shipped},
            "best_flush_denormal_value": round(best_ftz["steps_per_s"], 4), "as_shipped_value": round(best_shipped["steps_per_s"], 4),
            "logical_cpus": cores,
            "as_shipped_sample": "%d steps in %.1f s at %d threads, denormals NOT flushed (own process, so the worker threads "
                                 "do not flush either; SURVEY 6.1: sub-normal Softplus(beta=100) tails are handled in microcode on x86)"
                                 % (best_shipped["steps"], best_shipped["seconds"], best_shipped["threads"])}


def gpu_eager_baseline(depth, normal, T, cam, cfg, device, budget_s=8.0):
    """SURVEY 8d's informative second baseline: the reference's op chain as PyTorch-ROCm EAGER ops + autograd on this
    MI355X (oracle/torch_port.py on device "cuda": what the unmodified reference does when handed a HIP device), same
    27k-point workload, device-synchronised per step as metrics.start_timing/end_timing do.  Not the target."""
    from oracle import torch_port as tp
    sc = dict(n_rays=cfg["sample"]["n_rays"], n_strat=19, n_surf=8, min_depth=0.07, dist_behind_surf=0.1)
    lc = dict(trunc_distance=cfg["loss"]["trunc_distance"], loss_type="L1", trunc_weight=cfg["loss"]["trunc_weight"],
              eik_apply_dist=0.1, eik_weight=cfg["loss"]["eik_weight"], grad_weight=cfg["loss"]["grad_weight"])
    d, n, Tt = (torch.from_numpy(a).to(device) for a in (depth, normal, T))
    torch.manual_seed(1)
    net = tp.PortNet(256, 2, 6, 0.05937489, 0.14, None).to(device)
    opt = torch.optim.AdamW(net.parameters(), lr=0.0013, weight_decay=0.012)
    gen = torch.Generator().manual_seed(1)
    for _ in range(5):
        tp.train_step(net, opt, d, Tt, n, cam, sc, lc, 0.25, gen)
    torch.cuda.synchronize()
    t0 = time.perf_counter(); k = 0
    while True:
        tp.train_step(net, opt, d, Tt, n, cam, sc, lc, 0.25, gen)
        torch.cuda.synchronize(); k += 1
        el = time.perf_counter() - t0
        if el > budget_s or k >= 300:
            break
    return {"value": round(k / el, 2), "unit": "train-steps/s", "kind": "port on device", "device": torch.cuda.get_device_name(device),
            "sample": "%d device-synchronised steps of the same 27k-point workload in %.1f s, torch %s eager + autograd "
                      "(fp32), the reference's op chain (oracle/torch_port.py)" % (k, el, torch.__version__)}


def accuracy_leg(local, seeds=(1, 2), n_kf=24, steps_per_kf=100):
    """The metric's second half, SDF L1 vs GT (eval_pts.py:332-400, trainer.py:1819-1866: mean |sdf_pred - sdf_GT| over points sampled one
    per ray along rays of all frames seen): a short PINNED schedule on the synthetic analytic room (closed-form GT; the ReplicaCAD /
    ScanNet sequences are download-only) -- 24 keyframes x 100 steps, 480x640, replicaCAD.json settings -- run by the HIP path and by
    the fp32-eager CONTROL (the reference's op chain as PyTorch-ROCm eager on this same GPU) on the same seeds, initial networks and
    torch random streams (paired draws).  Band: BASELINE.md 1 / SURVEY 6.2: final visible-region L1 of the authors' runs 3-7 cm, sd 0.5 cm."""
    import tests.accuracy_experiment as ax
    from isdf_amd import synthetic
    cam = dict(synthetic.SCANNET_CAM)
    t0 = time.perf_counter()
    load = ax.prepare_keyframes(list(seeds), n_kf)
    ax.PAIRED, ax.DEVICE, ax.FWD_OPERAND, ax.BWD_OPERAND = True, "cuda:%d" % local, "fp16x2", None
    out = {"hip": [], "control": [], "hip_surface": [], "control_surface": []}
    for sd in seeds:
        depth, normal, T = load(sd)
        pts, surf = ax.eval_points(depth, T, cam, np.random.RandomState(1000 + sd), n_per_frame=200000 // n_kf)
        gt, gts = synthetic.gt_sdf(pts), synthetic.gt_sdf(surf)
        for name, runner in (("hip", ax.run_hip), ("control", ax.run_port)):
            fn, _, _ = runner(sd, depth, normal, T, cam, steps_per_kf)
            with torch.no_grad():
                out[name].append(float(np.mean(np.abs(fn(pts).reshape(-1) - gt))))
                out[name + "_surface"].append(float(np.mean(np.abs(fn(surf).reshape(-1) - gts))))
    cm = lambda v: round(100.0 * float(np.mean(v)), 3)
    return {"value": cm(out["hip"]), "unit": "cm (visible-region L1, mean over seeds)", "control_fp32_eager": cm(out["control"]),
            "hip_minus_control": round(cm(out["hip"]) - cm(out["control"]), 3),
            "per_seed_cm": {"seeds": list(seeds), "hip": [round(100 * v, 3) for v in out["hip"]], "control": [round(100 * v, 3) for v in out["control"]]},
            "surface_l1_cm": {"hip": cm(out["hip_surface"]), "control": cm(out["control_surface"])},
            "band_cm": [3.0, 7.0], "band_source": "BASELINE.md 1: final rays.vis.av_l1 of the authors' 12 sequences x 10 runs (0.031-0.074 m, sd ~0.5 cm)",
            "schedule": "%d keyframes x %d steps, 480x640 synthetic room, 200k evaluation rays, paired draws (same initial network, same torch streams)" % (n_kf, steps_per_kf),
            "seconds": round(time.perf_counter() - t0, 1),
            "note": "two seeds of a chaotic trajectory have a standard error of ~0.6 cm; the 100-paired-seed control on round 6's final "
                    "tree (profiles/r06_accuracy_gap.txt) measured HIP - control = -0.12 +- 0.09 cm (round 5, 120 seeds: +0.09 +- 0.09)"}


def sampler_scale(args, tr, eng, cam, rank):
    """The sampler as a streaming kernel: 5 x RAYS_PER_FRAME rays per launch (in-kernel Philox draws), HIP-event timed.
    Algorithmic bytes per ray: 16 read (depth 4 + normal 12) + 496 written (pc 324, z_vals 108,
    indices 24, depth_sample 4, dirs_C 12, dirs_W 12, norm_sample 12) = 512."""
    from isdf_amd.engine import SampleConfig
    from isdf_amd import dp
    F = tr.frames.depth_batch.shape[0]
    sc = SampleConfig(n_rays=args.sampler_scale, **cam)
    fidx = torch.arange(F, dtype=torch.int32, device=tr.device)
    run = lambda i: eng.sample(tr.frames.depth_batch, tr.frames.T_WC_batch, tr.frames.normal_batch, fidx, fidx, sc,
                               seed=dp.rank_seed(1, rank), offset=i)
    for i in range(5):
        s = run(i)
    torch.cuda.synchronize()
    K = max(args.steps // 10, 10)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(K):
        s = run(10 + i)
    e1.record(); torch.cuda.synchronize()
    t = e0.elapsed_time(e1) / K * 1e-3
    rays = F * args.sampler_scale
    R = int(s["n_valid"].item())
    alg = 16.0 * rays + 496.0 * R
    traffic, src = None, None
    tpath = latest_profile("hbm_traffic.json")
    if tpath:
        with open(tpath) as f:
            tj = json.load(f)
        if tj.get("sampler_scale", {}).get("rays") == rays:
            traffic, src = tj["sampler_scale"]["hbm_bytes"], tj["source"]
    res = {"metric": "sampler rays/s (sample_pixels + get_batch_data + sample_along_rays, one launch)", "value": round(rays / t, 1),
           "unit": "rays/s", "n_gpus": 1, "steps": K, "warmup": 5, "ms_per_step": round(t * 1e3, 4), "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": "f32 + int64 indices", "data": "synthetic",
           "config": {"workload": "%d keyframes x %d rays (680x1200 synthetic room depth + normals), 27 samples per ray" % (F, args.sampler_scale)},
           "valid_rays": R,
           "roofline": {"bound": "hbm", "kernel": "sample_rays_kernel", "achieved": round(alg / t / 1e9, 1), "peak": 8000.0,
                        "unit": "GB/s", "frac": round(alg / t / 8e12, 4), "traffic": traffic, "traffic_source": src,
                        "algorithmic_bytes_per_launch": alg,
                        "note": "16 B read per drawn ray are two RANDOM gathers (4 B depth + 12 B normal); HBM serves them as "
                                "whole sectors, which is the traffic/algorithmic gap on the read side"}}
    if rank == 0:
        print(json.dumps(res), flush=True)


def infer_bench(args, tr, eng, rank):
    """the inference forward at meshing / slice sizes (`fc_map.chunks`, fc_map.py:25-48, feeding
    `SDFMap.forward`; trainer.py:1426-1444 evaluates 256^3-class grids): one isdf_sdf_eval call over N points (the kernel
    has no chunking need), and the same with d sdf / d x (render.render_normals, render.py:39-47).  MFMA-bound: 2 M FLOP
    per point forward, 4 M with the input gradient (M = 458 496 MAC for the default net)."""
    N = args.infer_points
    g = torch.Generator(device="cpu"); g.manual_seed(5)
    pts = ((torch.rand(N, 3, generator=g) - 0.5) * torch.tensor([6.0, 3.0, 5.0])).to(tr.device)   # the synthetic room's extent
    M = 458496   # MAC per point and pass of the default net (E*Hd + 2B*Hd^2 + (Hd+E)*Hd + Hd)
    out = {}
    from isdf_amd.engine import Engine, NetConfig
    import dataclasses
    engines = {eng.net.fwd_operand: eng}
    if eng.net.fwd_operand == "fp16x2":      # the plain-fp16 fast mode beside the default (same weights)
        e2 = Engine(dataclasses.replace(eng.net, fwd_operand="fp16"), tr.device)
        e2.params.copy_(eng.params); e2.pack()
        engines["fp16"] = e2
        e3 = Engine(dataclasses.replace(eng.net, fwd_operand="fp16x2_full"), tr.device)   # exact-forward instrument (one workgroup per CU)
        e3.params.copy_(eng.params); e3.pack()
        engines["fp16x2_full"] = e3
    for op, en in engines.items():
        for name, wg, flop in (("forward", False, 2.0 * M), ("forward_with_input_gradient", True, 4.0 * M)):
            n = N if not wg else max(N // 4, 1)
            x = pts[:n]
            for _ in range(3):
                en.sdf_eval(x, want_grad=wg)
            torch.cuda.synchronize()
            K = max(args.steps // 30, 5)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(K):
                r = en.sdf_eval(x, want_grad=wg)
            e1.record(); torch.cuda.synchronize()
            t = e0.elapsed_time(e1) / K * 1e-3
            key = name if op == eng.net.fwd_operand else name + "[fwd_operand=%s]" % op
            out[key] = {"points": n, "ms": round(t * 1e3, 4), "points_per_s": round(n / t, 1), "fwd_operand": op,
                        "TFLOPs": round(flop * n / t / 1e12, 1), "frac_of_mfma_peak": round(flop * n / t / MFMA_PEAK, 4)}
    issue_port, ipath = None, latest_profile("issue_port.json")
    if ipath:
        with open(ipath) as fh:
            ij = json.load(fh)
        if "fwd_pair_kernel" in ij:
            ck = ij["fwd_pair_kernel"]
            issue_port = {"utilisation": ck["issue_port_utilisation"], "matrix_pipe_utilisation_at_clock": ck["matrix_pipe_utilisation"],
                          "valu_instructions_per_mfma": ck["valu_instructions_per_mfma"], "source": os.path.relpath(ipath, ROOT),
                          "what": "fp16 operands, 2 M points (tools/pmc_issue_mix.sh); model: " + ij.get("model", "")}
    f = out["forward"]
    res = {"metric": "inference points/s (SDFMap.forward on the fused kernel, one call)", "value": f["points_per_s"], "unit": "points/s",
           "n_gpus": 1, "steps": max(args.steps // 30, 5), "warmup": 3, "ms_per_step": f["ms"], "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": "f16 MFMA operands (%s), f32 accumulate" % eng.net.fwd_operand, "data": "synthetic",
           "config": {"workload": "%d uniform points in the synthetic room, default 6x256 net (meshing / slice grid size)" % N},
           "modes": out,
           "roofline": {"bound": "mfma", "kernel": "fwd_pair_kernel (PE + MLP forward, two 64-point halves per workgroup; csrc/fwd_pair.hip)", "achieved": f["TFLOPs"], "peak": MFMA_PEAK / 1e12,
                        "unit": "TFLOP/s", "frac": f["frac_of_mfma_peak"], "traffic": None,
                        "algorithmic_flop_per_launch": 2.0 * M * N, "issue_port": issue_port}}
    if rank == 0:
        print(json.dumps(res), flush=True)


def ingest_bench(args, tr, eng, cam, rank):
    """per-frame ingest = depth -> camera-frame normals (transform.py:169-196,215-270) as ONE stencil
    kernel.  HBM-bound by construction: 4 B read + 12 B written per pixel (neighbour depths come from L1/L2)."""
    from isdf_amd.engine import SampleConfig
    sc = SampleConfig(n_rays=200, **cam)
    d = tr.frames.depth_batch[0].contiguous()
    H, W = d.shape
    for _ in range(5):
        eng.estimate_normals(d, sc)
    torch.cuda.synchronize()
    K = max(args.steps, 100)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(K):
        n = eng.estimate_normals(d, sc)
    e1.record(); torch.cuda.synchronize()
    t = e0.elapsed_time(e1) / K * 1e-3
    alg = 16.0 * H * W
    res = {"metric": "ingest frames/s (depth -> normals stencil, one launch per frame incl. the output allocation)", "value": round(1.0 / t, 1),
           "unit": "frames/s", "n_gpus": 1, "steps": K, "warmup": 5, "ms_per_step": round(t * 1e3, 4), "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": "%dx%d synthetic room depth frame" % (H, W)},
           "roofline": {"bound": "hbm", "kernel": "normals_kernel", "achieved": round(alg / t / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
                        "frac": round(alg / t / 8e12, 4), "traffic": None, "algorithmic_bytes_per_launch": alg,
                        "note": "13 MB per 680x1200 frame is ~2.5 us of HBM time; the kernel itself (rocprofv3: 13.5 us) is VALU-bound: ~600 instructions per pixel (8 correctly rounded sqrt, 5 IEEE divisions, argmin with the reference's NaN rule); the rest of this figure is the per-call output allocation and launch"}}
    if rank == 0:
        print(json.dumps(res), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--cpu-baseline-child":
        return _cpu_baseline_child(int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4]), int(sys.argv[5]),
                                   int(sys.argv[6]) if len(sys.argv) > 6 else 1)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rays-per-frame", type=int, default=200)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--stream", default="680x1200", choices=["680x1200", "480x640"],
                    help="depth stream the keyframes come from: 680x1200 = replicaCAD.json's camera (the metric's configuration, default); "
                         "480x640 = the north star's synthetic 640x480 stream (scanNet.json's camera): same 5 x 200 rays x 27 samples per step")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="N > 1: weak = every rank draws the full 5 x 200 rays (N x 27k points per optimiser step, the reported "
                         "line); strong = the 27k-point batch is SPLIT over the ranks (200 / N rays per keyframe and rank; SURVEY 8e: "
                         "reported, not tuned for)")
    ap.add_argument("--overlap-allreduce", action="store_true",
                    help="N > 1: the step tail in two launches and the all-reduce in two parts, the first on a side stream while the "
                         "second launch runs (hot_path.graft(overlap_allreduce=True)); same parameters bit for bit at world size 2")
    ap.add_argument("--cpu-threads", type=int, nargs="*", default=None,
                    help="thread counts of the CPU-baseline sweep (default: 8 16 32 64 128 and all logical CPUs, capped at the box)")
    ap.add_argument("--fwd-operand", default="fp16x2", choices=["fp16x2", "fp16", "bf16", "fp16x2_full"])
    ap.add_argument("--bwd-operand", default=None, choices=["fp16", "bf16"],
                    help="operand / spill type of the second-order sweeps and the dW contraction (default: fp16 with an fp16-family forward)")
    ap.add_argument("--spill-operand", default=None, choices=["auto", "16bit", "e4m3", "e4m3_gb"],
                    help="storage of the spilled P / GB tensors (default auto: e4m3 bytes for nets of up to six octaves with fp16 sweeps)")
    ap.add_argument("--ramp-seconds", type=float, default=1.3,
                    help="untimed clock-ramp phase before the W warm-up steps (a fresh box runs the first ~100 ms at idle "
                         "clocks: 25 cold steps measured 13 %% slower than steady state in round 1); reported in the JSON line")
    ap.add_argument("--sampler-scale", type=int, default=0, metavar="RAYS_PER_FRAME",
                    help="instead of the training bench: the sampler alone at 5 x RAYS_PER_FRAME rays (>= 1e6 total rays is "
                         "where it is a streaming kernel, SURVEY 8d) with its HBM roofline")
    ap.add_argument("--infer-points", type=int, default=0, metavar="N",
                    help="time the inference forward (and forward + input gradient) on N points instead of the training step")
    ap.add_argument("--ingest", action="store_true", help="time the per-frame ingest stencil (depth -> normals) instead")
    ap.add_argument("--dry-run", action="store_true", help="launch path only: rendezvous + one collective + the JSON line, no device work")
    ap.add_argument("--no-accuracy", action="store_true", help="skip the sdf_l1_vs_gt leg (a pinned 24-keyframe x 100-step schedule, HIP and fp32-eager control)")
    ap.add_argument("--wide", action="store_true",
                    help="BASELINE configs[4] instead of the metric's configuration: hidden 512, 3 blocks (8 hidden layers), "
                         "n_freqs 10, 8000 rays = 216k points per GPU-step (not the reported bench line)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: pipelined and windowed rates, per-kernel times and rooflines, the CPU and eager-GPU "
                         "baselines, the accuracy leg and the fp16 fast mode (minutes); a plain run times the K steps and stops")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (its losses, the parameters and AdamW moments "
                         "it left, the keyframes' average losses) as DIR/<name>.npy")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` launches itself: one process per GPU under torch.distributed.run, as the contract's own command
        # does (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* then come from the launcher); rank 0's JSON line stays the last line of stdout
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        import subprocess
        sys.exit(subprocess.call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
                                  "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit("--gpus %d under a launcher with WORLD_SIZE=%d" % (args.gpus, world))
    if args.dry_run:
        # the launch path alone (CPU test of `--gpus N`): rendezvous, one barrier, the MAX all-reduce of the timing protocol, rank 0's
        # JSON line -- no device, no kernels
        backend = os.environ.get("ISDF_BENCH_BACKEND", "nccl")
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29533")
            torch.distributed.init_process_group(backend, rank=rank, world_size=world)
            torch.distributed.barrier()
            t = torch.tensor([float(rank + 1)], dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            assert float(t.item()) == world
            torch.distributed.destroy_process_group()
        if rank == 0:
            print(json.dumps({"dry_run": True, "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "backend": backend}), flush=True)
        return
    # ISDF_BENCH_BACKEND=gloo: functional test of the N>1 path on a box with fewer GPUs than ranks
    # (ranks share devices; RCCL refuses duplicate devices).  Never used for reported numbers.
    backend = os.environ.get("ISDF_BENCH_BACKEND", "nccl")
    local = local % max(torch.cuda.device_count(), 1) if backend != "nccl" else local
    torch.cuda.set_device(local)
    group = None
    # ISDF_BENCH_FORCE_DP=1: run the data-parallel step sequence (two-call form + all-reduce) with a one-rank
    # process group, to exercise the N>1 code path end to end on a single-GPU box.  Not the N=1 bench line.
    force_dp = world == 1 and os.environ.get("ISDF_BENCH_FORCE_DP") == "1"
    if world > 1 or force_dp:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        kw = dict(rank=rank, world_size=world)
        if backend == "nccl":
            torch.distributed.init_process_group("nccl", device_id=torch.device("cuda", local), **kw)
        else:
            torch.distributed.init_process_group(backend, **kw)
        group = torch.distributed.group.WORLD

    import __graft_entry__
    __graft_entry__.build(verbose=False)
    from bench_support.standin_trainer import HipTrainer, FrameData
    from isdf_amd import synthetic, dp

    cfg = reference_config()
    if args.scaling == "strong" and world > 1:
        if args.rays_per_frame % world:
            sys.exit("--scaling strong: %d rays per keyframe do not split over %d ranks" % (args.rays_per_frame, world))
        args.rays_per_frame //= world         # the SAME global batch, split: 200 / N rays per keyframe on every rank
    cfg["sample"]["n_rays"] = args.rays_per_frame
    m_mac = M_MAC
    if args.wide:
        cfg["model"].update(hidden_feature_size=512, hidden_layers_block=3)
        cfg["model"]["embedding"]["n_embed_funcs"] = 9          # n_freqs 10 -> E = 423
        if args.rays_per_frame == 200:
            cfg["sample"]["n_rays"] = args.rays_per_frame = 1600
        E, H = 423, 512
        m_mac = E * H + 6 * H * H + (H + E) * H + H             # 2 268 672 MAC/point
    cam = dict(synthetic.REPLICA_CAM if args.stream == "680x1200" else synthetic.SCANNET_CAM)
    cfg["dataset"]["camera"] = {"w": cam["W"], "h": cam["H"], "fx": cam["fx"], "fy": cam["fy"], "cx": cam["cx"], "cy": cam["cy"]}
    F = cfg["model"]["window_size"]
    depth, normal, T = make_keyframes(cam, F)

    torch.manual_seed(1)
    np.random.seed(1)
    tr = HipTrainer("cuda:%d" % local, cfg, incremental=True, inv_bounds_transform=synthetic.bounds_transform(),
                    rng="philox", seed=1, dist_group=group, fwd_operand=args.fwd_operand, bwd_operand=args.bwd_operand,
                    overlap_allreduce=args.overlap_allreduce, spill_operand=args.spill_operand)
    dev = tr.device       # (replicated weights: graft() broadcasts rank 0's at construction)
    tr.frames = FrameData(frame_id=np.arange(F), depth_batch=torch.from_numpy(depth).to(dev),
                          T_WC_batch=torch.from_numpy(T).to(dev), normal_batch=torch.from_numpy(normal).to(dev),
                          frame_avg_losses=torch.zeros(F, device=dev))
    eng = tr.engine
    sc = tr._sample_cfg()
    lc = tr._loss_cfg()
    S = sc.S
    fidx = tuple(range(F))      # the window inline (kernel arguments), as HipTrainer.step passes it
    max_rays = F * sc.n_rays
    K, W = args.steps, args.warmup
    # per-kernel HIP events ride on every PROF_EVERY-th timed step: four event records between the launches cost ~2 us of
    # stream time each (a step with them measured 305 us, without 296 us), and the other steps take the engine's cached call plan
    # (--full only: a plain run times the steps alone)
    PROF_EVERY = 4
    KP = max(K // PROF_EVERY, 1)             # on the LAST step of every group of four (never the first step behind the barrier)
    events = HipEvents(4 * KP) if args.full else None

    overlap = group is not None and args.overlap_allreduce
    split_ev, side = (dp.new_split_event(dev), torch.cuda.Stream(dev)) if overlap else (None, None)

    def one_step(i, ev=None, tr=tr, eng=eng):
        s = eng.sample(tr.frames.depth_batch, tr.frames.T_WC_batch, tr.frames.normal_batch, fidx, fidx, sc,
                       seed=dp.rank_seed(1, rank), offset=i, reuse=True)
        og = tr.optimiser.param_groups[0]
        fused = None if group is not None else dict(lr=og["lr"], weight_decay=og["weight_decay"], betas=og["betas"],
                                                    eps=og["eps"], frame_avg_out=tr.frames.frame_avg_losses,
                                                    frame_avg_index=fidx)   # trainer.py:979 inside the tail
        eng.train_step(s, lc, sc, prof_events=ev, noise_std=tr.noise_std, noise_seed=1 + rank,
                       noise_offset=i, optim=fused, split_event=split_ev)   # in-kernel N(0,1)*noise_std (fc_map.py:106-108)
        if group is not None:   # data parallel (exactly what HipTrainer.step issues): ONE all-reduce of the flat buffer (or its
            if overlap:         # two parts, the first beside the closing reduction's second launch), then
                dp.allreduce_split_(eng.reduce_buf, eng.reduce_split, split_ev, side, group)
            else:
                dp.allreduce_(eng.reduce_buf, group)      # ONE closing launch: AdamW + repack + frame averages (trainer.py:979-982)
            eng.train_step_finish(F, dict(lr=og["lr"], weight_decay=og["weight_decay"], betas=og["betas"], eps=og["eps"],
                                          frame_avg_out=tr.frames.frame_avg_losses, frame_avg_index=fidx))
        return s

    if args.sampler_scale:
        return sampler_scale(args, tr, eng, cam, rank)
    if args.infer_points:
        return infer_bench(args, tr, eng, rank)
    if args.ingest:
        return ingest_bench(args, tr, eng, cam, rank)
    # ---- untimed clock ramp: the driver's `--steps 20 --warmup 5` is 8 ms of GPU work in a fresh process, i.e. measured
    # at idle clocks with first-touch allocations inside the timed region (BENCH_r01: chain 223 us vs 197 us steady); and the
    # FIRST process on a freshly booted box stalls one step for ~35-40 ms about half a second into its run (seen three times in
    # round 3, never in a second process) -- the ramp is longer than that
    tr.noise_std = tr.noise_kf
    # the ramp trains too, for a number of steps that depends on the box: its steps are undone afterwards (the trainer's own
    # checkpoint / resume, exact), so that the warm-up and timed steps start from the seeded initial state on every run
    initial_state = tr.state_dict()
    ramp_steps, t_r = 0, time.perf_counter()
    if group is None:
        while time.perf_counter() - t_r < args.ramp_seconds:
            for _ in range(20):
                tr.step(); ramp_steps += 1
    else:   # every rank must issue the SAME number of collectives: a fixed count instead of a time budget
        for _ in range(int(1000 * args.ramp_seconds)):
            tr.step(); ramp_steps += 1
    torch.cuda.synchronize()
    tr.load_state_dict(initial_state)
    del initial_state
    if events is not None:
        events.prime(torch.cuda.current_stream(dev).cuda_stream)
    for i in range(W):
        tr.step()
    torch.cuda.synchronize()
    if group is not None:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    # ---- THE timed region: K calls of Trainer.step() -- each device-synchronised and timed exactly as the reference's
    # metrics.start_timing / end_timing bracket it (metrics.py:13-38; SURVEY 8d's definition of the metric) -- between two barriers
    per_step = np.empty(K)
    t0 = time.perf_counter()
    for i in range(K):
        if events is not None and (i % PROF_EVERY == PROF_EVERY - 1 or K < PROF_EVERY and i == K - 1) and i // PROF_EVERY < KP:
            tr._hip.prof_events = events.group(i // PROF_EVERY)       # HIP events around this step's kernels, on the launch stream
        t_a = time.perf_counter()
        last = tr.step()
        per_step[i] = time.perf_counter() - t_a
    torch.cuda.synchronize()
    if group is not None:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    elapsed = my_elapsed = time.perf_counter() - t0
    if group is not None:
        t = torch.tensor([elapsed], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())
    sync_step_ms = 1e3 * elapsed / K
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, tr, last[0])

    batches = world if (args.scaling == "weak" or world == 1) else 1
    res = {
        "metric": "train-steps/sec: device-synchronised Trainer.step() on 27k-point ray batches, timed as metrics.start_timing / end_timing bracket it (SURVEY 8d); whole job.  SDF L1 vs GT: sdf_l1_vs_gt",
        # weak: N x 27k points per optimiser step = N batches; strong: ONE 27k-point batch per optimiser step whatever N
        "value": round(batches * K / elapsed, 2),
        "unit": "train-steps/s",
        "n_gpus": world, "steps": K, "warmup": W,
        "ms_per_step": round(1e3 * elapsed / K, 4),
        "higher_is_better": True,
        "scaling": args.scaling if world > 1 else "weak",
        "vs_baseline": None,
        "distributed": {"world_size": torch.distributed.get_world_size() if group is not None else 1,
                        "backend": torch.distributed.get_backend() if group is not None else None,
                        "collectives_per_step": 0 if group is None else (2 if overlap else 1),
                        "overlap_allreduce": bool(overlap), "collective": getattr(tr._hip, "collective", None)},
        "dtype": {"fp16x2": "f16 MFMA operands (compensated forward: hi+lo operands past the cat layer), f32 accumulate; ",
                  "fp16x2_full": "f16 MFMA operands (exact-forward instrument: hi+lo operands in every forward layer), f32 accumulate; ",
                  "fp16": "f16 MFMA operands, f32 accumulate; ", "bf16": "bf16 MFMA operands, f32 accumulate; "}[args.fwd_operand]
                 + "second-order sweeps and dW operands %s" % (eng.net.bwd_operand or ("bf16" if args.fwd_operand == "bf16" else "fp16")),
        "fwd_operand": args.fwd_operand, "bwd_operand": eng.net.bwd_operand or ("bf16" if args.fwd_operand == "bf16" else "fp16"),
        "data": "synthetic",
        "config": {"workload": ("replicaCAD.json defaults: 5 keyframes x %d rays x 27 samples = %d points per "
                                "rank-step, STREAM synthetic room depth, 6x256 Softplus MLP + 255-wide "
                                "icosahedron PE (460033 params), eik+normal loss, bounds=ray, AdamW"
                                if not args.wide else
                                "BASELINE configs[4] (wide): 5 keyframes x %d rays x 27 samples = %d points per "
                                "rank-step, STREAM synthetic room depth, 8x512 Softplus MLP + 423-wide "
                                "icosahedron PE (2272769 params), eik+normal loss, bounds=ray, AdamW")
                               .replace("STREAM", "%dx%d" % (cam["H"], cam["W"])) % (sc.n_rays, max_rays * S),
                   "stream": "%dx%d" % (cam["H"], cam["W"]),
                   "global_points_per_step": int(world * max_rays * S),
                   "scaling_mode": ("weak: every rank draws the full 5 x 200 rays" if args.scaling == "weak" or world == 1 else
                                    "strong: the 27k-point batch split over %d ranks (%d rays per keyframe and rank)" % (world, sc.n_rays)),
                   "parallelism": "dp%d (rays sharded, one %s all-reduce of %d floats)"
                                  % (world, "RCCL" if backend == "nccl" else backend, eng.reduce_buf.numel())
                   if world > 1 else "single GPU"},
        "clock_ramp": {"untimed_steps_before_warmup": ramp_steps, "seconds": args.ramp_seconds},
    }
    if not args.full:
        return finish(res, group, rank)

    # ---- informational: the same step PIPELINED (K2 steps between two synchronisations, the engine called directly: no timing
    # bracket, no loss dict) -- what the device can do when the host never waits; rounds 1-5 reported this as `value`
    K2 = max(K, 100) if group is None else K
    for i in range(10):
        one_step(i)
    torch.cuda.synchronize()
    if group is not None:
        torch.distributed.barrier()
    t_p = time.perf_counter()
    for i in range(K2):
        one_step(W + i)
    torch.cuda.synchronize()
    if group is not None:
        torch.distributed.barrier()
    pipe_elapsed = time.perf_counter() - t_p
    if group is not None:
        t = torch.tensor([pipe_elapsed], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        pipe_elapsed = float(t.item())

    # ---- SURVEY 8d asks for >= 200 timed steps after >= 20 warm-up steps: the same synchronised step() over 200 more steps
    # (the driver's K = 20 is what `value` is made of; this is the low-noise figure beside it)
    n_sync, n_warm = 200, ramp_steps + W
    per200 = np.empty(n_sync)
    ts = time.perf_counter()
    for i in range(n_sync):
        t_a = time.perf_counter()
        tr.step()
        per200[i] = time.perf_counter() - t_a
    sync200_ms = (time.perf_counter() - ts) / n_sync * 1e3

    # ---- the same synchronised step() once the keyframe set has outgrown the window (K = 8 > window_size = 5): the regime
    # every real run is in after the first few seconds -- `select_keyframes` (trainer.py:652-674, the reference's own code: two
    # device ops + a .cpu()) draws a new window on the host EVERY step; the window travels inline as kernel arguments
    windowed_ms, transport_ab, losses_ab = None, None, None
    if group is None and not args.wide:
        K8 = 8
        d8, n8, T8 = (torch.cat([t, t[:K8 - F]]) for t in (tr.frames.depth_batch, tr.frames.normal_batch, tr.frames.T_WC_batch))
        saved = tr.frames
        def frames_k8(losses):
            return FrameData(frame_id=np.arange(K8), depth_batch=d8, T_WC_batch=T8, normal_batch=n8, frame_avg_losses=losses,
                             host_losses=not losses.is_cuda)       # (a device tensor stays on the device: the A/B's other arm)
        # where the K frame-average losses live once K > window_size: pinned host memory (isdf_amd.frame_store moves them there: the
        # closing launch writes them zero-copy, select_keyframes runs on the host) or the device (the reference's own FrameData)
        frames8 = frames_k8(torch.full((K8,), 0.1).pin_memory())
        frames8_dev = frames_k8(torch.full((K8,), 0.1, device=dev))

        def timed_steps(n=n_sync, warm=60):
            for _ in range(warm):
                tr.step()
            t_a = time.perf_counter()
            for _ in range(n):
                tr.step()
            return (time.perf_counter() - t_a) / n * 1e3
        transport_ab = {}
        for label, inline in (("inline_kernel_arguments", True), ("device_tensors", False)):   # A/B of the window's transport
            tr._hip.inline_window = inline
            tr.frames = saved
            fixed = timed_steps()
            tr.frames = frames8
            transport_ab[label] = {"sync_step_ms_K5": round(fixed, 4), "sync_step_ms_K8_windowed": round(timed_steps(), 4)}
        tr._hip.inline_window = True
        tr.frames = frames8_dev
        losses_ab = {"pinned_host (isdf_amd.frame_store)": transport_ab["inline_kernel_arguments"]["sync_step_ms_K8_windowed"],
                     "device (the reference's FrameData)": round(timed_steps(), 4)}
        tr.frames = saved
        windowed_ms = transport_ab["inline_kernel_arguments"]["sync_step_ms_K8_windowed"]

    # ---- per-kernel timing from the HIP events recorded inside the timed region
    chain_us = np.array([events.ms(4 * i, 4 * i + 1) for i in range(KP)]) * 1e3
    t_chain = np.mean([events.ms(4 * i, 4 * i + 1) for i in range(KP)]) * 1e-3
    t_dw = np.mean([events.ms(4 * i + 1, 4 * i + 2) for i in range(KP)]) * 1e-3
    t_red = np.mean([events.ms(4 * i + 2, 4 * i + 3) for i in range(KP)]) * 1e-3
    # valid points per launch: replay the same Philox draws (sampler only) and read n_valid
    nv = []
    for i in range(min(K, 50)):
        s = eng.sample(tr.frames.depth_batch, tr.frames.T_WC_batch, tr.frames.normal_batch, fidx, fidx, sc,
                       seed=dp.rank_seed(1, rank), offset=W + i)
        nv.append(int(s["n_valid"].item()))
    P = float(np.mean(nv)) * S
    ls = eng.loss_sums().cpu().numpy()
    final_loss = float(ls[3] / max(ls[4], 1))

    traffic, traffic_src, traffic_commit, step_traffic = None, None, None, None
    tpath = latest_profile("hbm_traffic.json")
    if tpath and args.rays_per_frame == 200 and not args.wide:     # PMC passes cannot run inside the timed region:
        with open(tpath) as f:                                    # the committed rocprofv3 --pmc measurement of this
            tj = json.load(f)                                     # command (FETCH_SIZE x2 gfx950 correction + WRITE_SIZE)
        traffic, traffic_src = tj["chain_kernel"]["hbm_bytes"], tj["source"]
        traffic_commit = tj.get("commit")          # the tree the PMC passes were taken on (tools/round_records.sh stamps it)
        step_traffic = sum(v["hbm_bytes"] for k, v in tj.items() if isinstance(v, dict) and "hbm_bytes" in v and k != "sampler_scale")
    # the SIMD issue-port model of the kernel (tools/issue_model.py on a committed rocprofv3 --pmc summary, like `traffic`): on this chip
    # a VALU wave-instruction next to MFMAs costs ~4 issue cycles of its SIMD (transcendental 8, MFMA 8 of the 32 it executes for):
    # with ~11 VALU instructions per MFMA the tile kernels run out of issue slots long before they run out of matrix pipe
    issue_port, ipath = None, latest_profile("issue_port.json")
    if ipath and args.rays_per_frame == 200 and not args.wide:
        with open(ipath) as f:
            ij = json.load(f)
        if "chain_kernel" in ij:
            ck = ij["chain_kernel"]
            issue_port = {"utilisation": ck["issue_port_utilisation"], "matrix_pipe_utilisation_at_clock": ck["matrix_pipe_utilisation"],
                          "valu_instructions_per_mfma": ck["valu_instructions_per_mfma"],
                          "valu_cycles_per_instruction": ck["valu_cycles_per_instruction"],
                          "source": os.path.relpath(ipath, ROOT), "model": ij.get("model")}
    per_rank_chain_us, per_rank_elapsed = [round(t_chain * 1e6, 1)], [round(my_elapsed, 4)]
    if group is not None:      # every rank's own chain-kernel time and wall clock in the line (rank 0 prints)
        slots = torch.zeros(2 * world, dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        slots[2 * rank], slots[2 * rank + 1] = t_chain * 1e6, my_elapsed
        torch.distributed.all_reduce(slots)
        per_rank_chain_us = [round(float(v), 1) for v in slots[0::2]]
        per_rank_elapsed = [round(float(v), 4) for v in slots[1::2]]
    if rank == 0:
        flops_chain = 8.0 * m_mac * P      # fwd 2M + input-grad 2M + its adjoint 2M + reverse sweep 2M
        res["distributed"].update(per_rank_chain_us=per_rank_chain_us, per_rank_elapsed_s=per_rank_elapsed)
        res.update({
            "points_per_s": round(world * P * K / elapsed, 1),
            "valid_points_per_step": round(P, 1),
            "final_total_loss": round(final_loss, 5),
            # `value` is SURVEY 8d's metric: K device-synchronised Trainer.step() calls between two barriers (rounds 1-5 put the
            # PIPELINED rate there -- the engine called directly, K steps between two synchronisations -- which is this extra key)
            "pipelined": {"steps_per_s": round(batches * K2 / pipe_elapsed, 2), "ms_per_step": round(1e3 * pipe_elapsed / K2, 4), "steps": K2,
                          "what": "sampler + step kernels launched back to back through the engine, no per-step synchronisation, no "
                                  "timing bracket, no loss dict: the device-side rate"},
            "synchronised_step": {"steps_per_s": round(1e3 / sync200_ms, 2), "ms_per_step": round(sync200_ms, 4),
                                  "median_ms": round(float(np.median(per200)) * 1e3, 4),
                                  "p90_ms": round(float(np.percentile(per200, 90)) * 1e3, 4),
                                  "slowest": [[int(i), round(float(per200[i]) * 1e3, 3)] for i in np.argsort(per200)[::-1][:5]],
                                  "n": n_sync, "warmup": n_warm,
                                  "timed_region": {"median_ms": round(float(np.median(per_step)) * 1e3, 4),
                                                   "slowest": [[int(i), round(float(per_step[i]) * 1e3, 3)] for i in np.argsort(per_step)[::-1][:3]]},
                                  "what": "the same HipTrainer.step() as `value`, over 200 more steps (SURVEY 8d: >= 200 timed steps): sync + "
                                  "event, sampler, step kernels (AdamW, frame averages and the loss sums' host copy inside the last launch), sync"},
            "trainer_step_sync_ms": round(sync_step_ms, 4),
            "synchronised_step_windowed": None if windowed_ms is None else {
                "ms_per_step": round(windowed_ms, 4), "steps_per_s": round(1e3 / windowed_ms, 2), "keyframes": 8, "window": F,
                "what": "HipTrainer.step() with K = 8 keyframes > window_size: the reference's select_keyframes draws a new window "
                        "on the host every step from frames.frame_avg_losses -- in pinned host memory with isdf_amd.frame_store (the "
                        "closing launch writes it zero-copy), on the device with the reference's FrameData (two device ops + a "
                        "synchronising copy per step); the window goes to the kernels inline",
                "frame_avg_losses_placement_ab": losses_ab,
                "window_transport_ab": transport_ab},
            "chain_us_per_step": {"first5": [round(float(v), 1) for v in chain_us[:5]], "min": round(float(chain_us.min()), 1),
                                  "median": round(float(np.median(chain_us)), 1), "max": round(float(chain_us.max()), 1),
                                  "launches_timed": int(KP), "what": "HIP events around the chain kernel on every %d-th timed step" % PROF_EVERY},
            "kernel_ms": {"chain": round(t_chain * 1e3, 4), "dw": round(t_dw * 1e3, 4),
                          "tail(reduce,adamw,pack,finalize)" if group is None else "reduce+finalize": round(t_red * 1e3, 4)},
            # The dominant kernel against BOTH roofs.  SURVEY 8d declares rows a10-a12 / a19 MFMA-bound and gives the algorithmic
            # figure for that roof (8 M FLOP per point in this kernel), so `achieved` / `frac` are that; `hbm` is what the counters say:
            # the kernel's measured traffic over its measured duration against 8 TB/s.  `bound` names the roof the kernel sits
            # nearer to -- it is a chain of 31 dependent GEMM -> barrier -> epilogue phases per tile and saturates neither.
            "roofline": {"bound": "mfma" if traffic is None or flops_chain / t_chain / MFMA_PEAK >= traffic / t_chain / 8e12 else "hbm",
                         "kernel": "chain_kernel (fused PE+MLP fwd / input-grad / adjoint / reverse)",
                         "achieved": round(flops_chain / t_chain / 1e12, 3), "peak": MFMA_PEAK / 1e12,
                         "unit": "TFLOP/s", "frac": round(flops_chain / t_chain / MFMA_PEAK, 5), "traffic": traffic,
                         "traffic_unit": "bytes per launch on the L2's fabric side (rocprofv3 --pmc FETCH_SIZE x 2 + WRITE_SIZE, separate passes): requests that "
                                         "leave an XCD's L2, answered by the Infinity Cache or by HBM -- the counters cannot tell which; with the default cache "
                                         "policy of round 6 the chain kernel's re-reads are mostly Infinity-Cache hits (DESIGN 6)", "traffic_source": traffic_src,
                         "traffic_commit": traffic_commit,
                         "hbm": None if traffic is None else {"achieved": round(traffic / t_chain / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
                                                              "frac": round(traffic / t_chain / 8e12, 4),
                                                              "frac_of_achievable_6300": round(traffic / t_chain / 6.3e12, 4),
                                                              "what": "counter traffic of this kernel / its HIP-event duration (the kernel's algorithmic "
                                                                      "bytes are ~3 MB: points in, sdf / loss sums out, 2.4 MB of packed weights)"},
                         "step_traffic": step_traffic,
                         "algorithmic_flop_per_launch": flops_chain,
                         "issue_port": issue_port,
                         "whole_step_frac_of_mfma_peak": round(12.0 * m_mac * P * K / elapsed / MFMA_PEAK, 5)},
        })
        if world == 1 and not args.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline(cfg, args.cpu_threads)
            res["speedup_vs_cpu_baseline"] = round(res["value"] / res["cpu_baseline"]["value"], 1)
            try:      # informative second baseline: the same op chain as eager PyTorch-ROCm on this GPU
                res["gpu_eager_baseline"] = gpu_eager_baseline(depth, normal, T, cam, cfg, dev)
            except Exception as e:   # never lose the bench line to the baseline
                res["gpu_eager_baseline"] = {"error": repr(e)[:200]}
        if world == 1 and not args.no_accuracy and not args.wide and args.rays_per_frame == 200:
            try:
                res["sdf_l1_vs_gt"] = accuracy_leg(local)
            except Exception as e:   # never lose the bench line to the accuracy leg
                res["sdf_l1_vs_gt"] = {"error": repr(e)[:300]}
        if world == 1 and args.fwd_operand == "fp16x2":
            # the plain-fp16 FAST mode on the same box, same workload (not the default: its sdf sits at 0.9e-3 .. 1.5e-3 of the
            # reference at BASELINE size, tests/test_gpu_parity.py) -- reported so the cost of the compensated forward is visible
            tr2 = HipTrainer("cuda:%d" % local, cfg, incremental=True, inv_bounds_transform=synthetic.bounds_transform(),
                             rng="philox", seed=1, fwd_operand="fp16")
            tr2.frames = tr.frames
            K2 = min(max(K, 100), 200)
            KP2 = (K2 + PROF_EVERY - 1) // PROF_EVERY
            ev2 = HipEvents(4 * KP2)
            for i in range(max(W, 20)):
                one_step(i, tr=tr2, eng=tr2.engine)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            for i in range(K2):
                one_step(W + i, ev2.group(i // PROF_EVERY) if i % PROF_EVERY == 0 else None, tr=tr2, eng=tr2.engine)
            torch.cuda.synchronize()
            el2 = time.perf_counter() - t2
            c2 = float(np.mean([ev2.ms(4 * i, 4 * i + 1) for i in range(KP2)])) * 1e-3
            res["fast_mode_fp16"] = {"steps_per_s": round(K2 / el2, 2), "ms_per_step": round(1e3 * el2 / K2, 4), "steps": K2,
                                     "chain_ms": round(c2 * 1e3, 4), "chain_frac_of_mfma_peak": round(flops_chain / c2 / MFMA_PEAK, 5),
                                     "what": "fwd_operand=fp16 (no compensation GEMMs); parity: sdf rel-L2 0.9e-3 .. 1.5e-3 vs the "
                                             "reference at BASELINE size, i.e. NOT within the north star's 1e-3 on every fixture"}
    finish(res, group, rank)


def dump_outputs(d, tr, losses):
    """What the last timed step computed, as a caller of Trainer.step() receives it: the returned losses (float64) and the state the
    step's update left behind -- network parameters, AdamW moments, the keyframes' average losses (float32, flat)."""
    os.makedirs(d, exist_ok=True)
    eng = tr.engine
    out = {k: np.array([float(v)], dtype=np.float64) for k, v in losses.items()}
    for k, t in (("params", eng.params), ("exp_avg", eng.exp_avg), ("exp_avg_sq", eng.exp_avg_sq),
                 ("frame_avg_losses", tr.frames.frame_avg_losses)):
        out[k] = t.detach().reshape(-1).float().cpu().numpy()
    for k, v in out.items():
        np.save(os.path.join(d, k + ".npy"), v)


def finish(res, group, rank):
    if group is not None:
        torch.distributed.destroy_process_group()
    try:      # RCCL prints its version banner through C stdio, which is flushed at exit when stdout is a pipe:
        ctypes.CDLL(None).fflush(None)          # push it out now so that the JSON line is the LAST line of stdout
    except Exception:
        pass
    if rank == 0:
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
