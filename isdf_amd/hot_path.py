"""The drop-in boundary on the Python side: `graft(trainer)` re-binds the three hot-path methods of a
reference `isdf.modules.trainer.Trainer` INSTANCE to the HIP kernels behind the C ABI
(include/isdf_hip.h), in place:

    Trainer.step                trainer.py:951-1016
    Trainer.sample_points       trainer.py:683-766
    Trainer.sdf_eval_and_loss   trainer.py:768-868   (+ total_loss.backward(), trainer.py:981)
    Trainer.is_keyframe         trainer.py:586-620   (fused sampler -> frozen net -> depth render)
    Trainer.get_data            trainer.py:530-562   (the reference's own method runs; its two geometry calls -- depth -> point cloud ->
                                                      8-neighbour normals, transform.py:169-196,215-270 -- are ONE stencil launch)
    Trainer.get_sdf_grid        trainer.py:1426-1443 (one isdf_sdf_eval over grid_pc instead of 100k-point chunks)
    Trainer.mesh_rec            trainer.py:1500-1542 (marching cubes in HIP, world affine in-kernel, one copy to the host;
                                                      write_mesh / eval_mesh follow through it)
    Trainer.render_depth_vis    trainer.py:1225-1262 (all keyframes in ONE isdf_render_views pass; the depth resize in-kernel)
    Trainer.render_normals_vis  trainer.py:1264-1280 (all keyframes in one pass at the given depths; frames_vis follows)
    Trainer.latest_frame_vis    trainer.py:1055-1147 (coarse pass, upsample, fine pass and normals on the device, one copy back)
    Trainer.eval_sdf            trainer.py:1819-1866 (ground-truth lookup, mask, L1, bins and CHOMP differences: ONE isdf_sdf_metrics
                                                      pass over the device copy of gt_sdf_interp's grid, one copy of 24 doubles)
    Trainer.eval_sdf_visible    trainer.py:1868-1905 (the cached sequence stays resident on the device; only new frames are uploaded)
    Trainer.eval_object_sdf     trainer.py:1955-2008 (resident frames; per visible object one isdf_sdf_metrics call)
    Trainer.eval_traj_cost      trainer.py:2010-2052 (validity count and both CHOMP sums from one record)
    Trainer.eval_mesh           trainer.py:2054-2064 (accuracy / completion by isdf_nn_distance instead of two host KD-trees)
    Trainer.eval_fixed          trainer.py:2080-2088 (eval_pts.fixed_pts_eval, eval_pts.py:96-299: resident frames, ONE sampler launch
                                                      for both point sets, one isdf_region_metrics pass per leg -- region masks,
                                                      central-difference ground-truth gradient, cosine distance --, one copy back)
    Trainer.compute_slices      trainer.py:1558-1707 (all slices in one forward launch; colours, ground truth and CHOMP cost fields in
                                                      ONE isdf_slice_images pass, one copy back; write_slices / slices_vis follow)
    Trainer.obj_slices_vis      trainer.py:1775-1815 (per object one forward launch and one isdf_slice_images pass)
    Trainer.get_sdf_grid_pc     trainer.py:1446-1481 (ground truth by the device lookup, the near-point-cloud mask by
                                                      isdf_nn_distance instead of a host KD-tree; view_sdf follows)

ONE object owns the state: every attribute the reference's drivers and its own remaining methods read or
write -- `tot_step_time`, `steps_since_frame`, `optim_frames`, `last_is_keyframe`, `noise_std`, `frames`,
`active_idxs`, `active_pixels`, `frozen_sdf_map`, `sdf_map`, `optimiser` (train.py:102-136,
trainer.py:574-650,1011-1014) -- stays on the `Trainer` instance; the methods here only use `self.<name>`
with the reference's names.  `trainer.sdf_map` becomes an `SDFMapHIP` (a real nn.Module with the
reference's state_dict keys whose parameters are views of one flat buffer), `trainer.optimiser` a facade
with the `torch.optim.AdamW` surface, `trainer.frames` an `isdf_amd.frame_store.FrameData` (the reference's fields and
`add_frame_data` contract on geometrically growing buffers instead of one `torch.cat` of the whole keyframe set per frame,
data_util.py:84-102; the existing keyframes migrate).  Everything else (`add_frame`, `add_data`,
`check_keyframe_latest`, `select_keyframes`, `eval_sdf_volume`, the remaining visualisation)
keeps running as the reference's own code on the same object.

Where the reference is not importable (the GPU box, bench.py), `bench_support/standin_trainer.py` (test / bench infrastructure, outside
this package) restates the driver-side methods; its `HipTrainer` is `graft()` applied to that stand-in -- the same code path.

There is no CPU fallback: without the HIP library or a HIP device `graft` raises.
"""
import copy
import ctypes
import os
import sys
import types
import warnings

import numpy as np
import torch

from . import _ffi, dp, frame_store
from .engine import LossConfig, NetConfig, SampleConfig
from .modules import PositionalEncodingHIP, SDFMapHIP


class FlatAdamW:
    """Facade with the `torch.optim.AdamW` surface the drivers touch
    (`state_dict()`, `param_groups`, `step()`; trainer.py:435-439, train.py:213);
    the update itself is the fused flat HIP kernel."""

    def __init__(self, sdf_map, lr, weight_decay, betas=(0.9, 0.999), eps=1e-8):
        self.sdf_map = sdf_map
        self.param_groups = [dict(params=list(sdf_map.parameters()), lr=lr, betas=betas, eps=eps,
                                  weight_decay=weight_decay, amsgrad=False)]

    def step(self):
        g = self.param_groups[0]
        self.sdf_map.engine.adamw(lr=g["lr"], weight_decay=g["weight_decay"], betas=g["betas"], eps=g["eps"])

    def zero_grad(self, set_to_none=True):
        pass   # gradients never live on the parameters (they are sums in the engine's reduce buffer)

    def state_dict(self):
        eng = self.sdf_map.engine
        state = {}
        if eng.opt_step > 0:
            for i, (k, (off, shp)) in enumerate(eng.slices.items()):
                n = int(np.prod(shp))
                state[i] = dict(step=torch.tensor(float(eng.opt_step)),
                                exp_avg=eng.exp_avg[off:off + n].view(*shp).clone(),
                                exp_avg_sq=eng.exp_avg_sq[off:off + n].view(*shp).clone())
        g = dict(self.param_groups[0])
        g["params"] = list(range(len(eng.slices)))
        return dict(state=state, param_groups=[g])

    def load_state_dict(self, sd):
        eng = self.sdf_map.engine
        if not sd["state"]:          # a checkpoint taken before the first step: fresh moments
            eng.exp_avg.zero_(); eng.exp_avg_sq.zero_(); eng.opt_step = 0
        for i, (k, (off, shp)) in enumerate(eng.slices.items()):
            if i in sd["state"]:
                n = int(np.prod(shp))
                eng.exp_avg[off:off + n].copy_(sd["state"][i]["exp_avg"].reshape(-1))
                eng.exp_avg_sq[off:off + n].copy_(sd["state"][i]["exp_avg_sq"].reshape(-1))
                eng.opt_step = int(float(sd["state"][i]["step"]))
        for k in ("lr", "weight_decay", "betas", "eps"):
            if sd.get("param_groups") and k in sd["param_groups"][0]:
                self.param_groups[0][k] = sd["param_groups"][0][k]


_CUDA_GET_DEVICE = getattr(torch._C, "_cuda_getDevice", None)       # the current device index without torch.cuda's Python layers


class StepLosses(dict):
    """`losses` of `Trainer.step`: keys sdf_loss / grad_loss / eikonal_loss (floats) and total_loss (0-d tensor;
    callers use '{:.6f}'.format and .item(), train.py:138,215).  Built from ONE 8-float device->host copy that
    rides on the step's closing synchronisation instead of the reference's three `.item()` syncs
    (loss.py:187-200); the values are snapshotted at construction, so a later step cannot change them."""

    def __init__(self, loss_sums_host, has_grad, has_eik):
        ls = loss_sums_host.tolist()        # (iterating a tensor goes through unbind(): ~20 us)
        n = max(ls[_ffi.LS_COUNT], 1.0)
        super().__init__()
        self["sdf_loss"] = ls[_ffi.LS_SDF] / n
        if has_grad:
            self["grad_loss"] = ls[_ffi.LS_GRAD] / n
        if has_eik:
            self["eikonal_loss"] = ls[_ffi.LS_EIK] / n
        self["total_loss"] = torch.scalar_tensor(ls[_ffi.LS_TOTAL] / n)   # (0-d fp32 like torch.tensor(float), at half its cost)


class _LazyCut(dict):
    """`self.active_pixels` (trainer.py:970-974, read by keyframe_vis :1162-1175): the sampler's index tensors
    cut to the valid-ray count on first access, so `step()` itself never waits for the count."""

    def __init__(self, raw):
        super().__init__()
        self._raw = raw

    def _fill(self):
        if self._raw is not None:
            R = int(self._raw["n_valid"].item())
            for k in ("indices_b", "indices_h", "indices_w"):
                dict.__setitem__(self, k, self._raw[k][:R])
            self._raw = None

    def __getitem__(self, k):
        self._fill(); return dict.__getitem__(self, k)

    def keys(self):
        self._fill(); return dict.keys(self)

    def items(self):
        self._fill(); return dict.items(self)

    def values(self):
        self._fill(); return dict.values(self)

    def __iter__(self):
        self._fill(); return dict.__iter__(self)

    def __len__(self):
        return 3

    def __contains__(self, k):
        return k in ("indices_b", "indices_h", "indices_w")


class _BackwardDone(torch.autograd.Function):
    """`total_loss` of `sdf_eval_and_loss`: the reference returns a graph-attached scalar and the caller runs
    `total_loss.backward(); self.optimiser.step()` (trainer.py:981-982).  Here the backward pass has already
    run inside the native call (gradient sums sit in the engine's reduce buffer), so `.backward()` is a no-op
    and the same two caller lines keep working."""

    @staticmethod
    def forward(ctx, value, anchor):
        return value.clone()

    @staticmethod
    def backward(ctx, g):
        return None, None


class HotPath:
    """Mix-in holding the replaced methods.  `self` is the Trainer (reference or stand-in)."""

    # ------------------------------------------------------------------ helpers
    def _loss_cfg(self):
        return LossConfig(self.bounds_method, self.loss_type, self.trunc_weight, self.trunc_distance,
                          self.eik_weight, self.eik_apply_dist, self.grad_weight, bool(self.orien_loss))

    def _sample_cfg(self, n_rays=None, dist_behind_surf=None, n_strat=None, n_surf=None):
        return SampleConfig(n_rays=self.n_rays if n_rays is None else n_rays,
                            n_strat=self.n_strat_samples if n_strat is None else n_strat,
                            n_surf=self.n_surf_samples if n_surf is None else n_surf,
                            min_depth=self.min_depth,
                            dist_behind_surf=self.dist_behind_surf if dist_behind_surf is None else dist_behind_surf,
                            H=self.H, W=self.W, fx=self.fx, fy=self.fy, cx=self.cx, cy=self.cy)

    @property
    def engine(self):
        return self.sdf_map.engine

    def _rank(self):
        g = self._hip.dist_group
        return 0 if g is None else torch.distributed.get_rank(g)

    # ------------------------------------------------------------------ sampling (trainer.py:683-766)
    def _draws_torch(self, F, sc, n_valid_fn):
        """Reference draw order / shapes / devices: randint(h), randint(w) on the training device,
        rand(R, n_strat) on the device, normal(0, 0.1, (R, n_surf-1)) on the CPU generator
        (sample.py:15-16,123,160-162)."""
        dev = self._hip.device
        total = sc.n_rays * F
        ih = torch.randint(0, sc.H, (total,), device=dev)
        iw = torch.randint(0, sc.W, (total,), device=dev)
        R = n_valid_fn(ih, iw)
        U = torch.rand(R, sc.n_strat, device=dev)
        N_off = torch.normal(torch.zeros(R, max(sc.n_surf - 1, 0)), 0.1).to(dev)
        return dict(indices_h=ih, indices_w=iw, U=U, N_off=N_off)

    def _sample_raw(self, depth_batch, T_WC_batch, norm_batch, frame_idx, normal_idx, sc, want_T, shared_key=False,
                    reuse=False):
        """sampler launch; returns the engine's capacity-sized output dict (rows >= n_valid are undefined).
        shared_key: use the rank-INDEPENDENT Philox key (keyframe test under data parallelism: every rank
        must reach the same decision)."""
        eng, hip = self.engine, self._hip
        if hip.rng == "torch":
            as_t = lambda ix: torch.as_tensor(list(ix), dtype=torch.long, device=hip.device) if isinstance(ix, (tuple, list)) else ix.long()
            fi_t, ni_t = as_t(frame_idx), (None if normal_idx is None else as_t(normal_idx))

            def n_valid(ih, iw):   # the reference learns R from its boolean-mask compaction (a sync)
                ib = torch.arange(fi_t.numel(), device=ih.device).repeat_interleave(sc.n_rays)
                d = depth_batch[fi_t[ib], ih, iw]
                ok = d != 0
                if norm_batch is not None:
                    ok &= ~torch.isnan(norm_batch[ni_t[ib], ih, iw, 0])
                return int(ok.sum().item())
            draws = self._draws_torch(fi_t.numel(), sc, n_valid)
            return eng.sample(depth_batch, T_WC_batch, norm_batch, frame_idx, normal_idx, sc, draws=draws,
                              want_T=want_T, reuse=reuse)
        hip.draw_count += 1
        seed = hip.seed if shared_key else dp.rank_seed(hip.seed, self._rank())
        return eng.sample(depth_batch, T_WC_batch, norm_batch, frame_idx, normal_idx, sc,
                          seed=seed, offset=hip.draw_count, want_T=want_T, reuse=reuse)

    def sample_points(self, depth_batch, T_WC_batch, norm_batch=None, active_loss_approx=None, n_rays=None,
                      dist_behind_surf=None, n_strat_samples=None, n_surf_samples=None, _shared_key=False):
        """Same 11 named tensors as the reference (trainer.py:753-766), cut to the R valid rays (one host
        sync for R, exactly where the reference's boolean-mask compaction has one, sample.py:39-55).
        `binary_masks` is None: the dense [F,H,W] mask image is never materialised (sample.py:58-61)."""
        if active_loss_approx is not None:
            raise Exception('Active sampling not currently supported.')
        sc = self._sample_cfg(n_rays, dist_behind_surf, n_strat_samples, n_surf_samples)
        dev = self._hip.device
        ar = torch.arange(depth_batch.shape[0], dtype=torch.int32, device=dev)
        s = self._sample_raw(depth_batch.contiguous(), T_WC_batch.contiguous(),
                             None if norm_batch is None else norm_batch.contiguous(), ar,
                             None if norm_batch is None else ar, sc, want_T=True, shared_key=_shared_key)
        R = int(s["n_valid"].item())

        def cut(t):
            return None if t is None else t[:R]
        return {
            "depth_batch": depth_batch, "pc": cut(s["pc"]), "z_vals": cut(s["z_vals"]),
            "indices_b": cut(s["indices_b"]), "indices_h": cut(s["indices_h"]), "indices_w": cut(s["indices_w"]),
            "dirs_C_sample": cut(s["dirs_C_sample"]), "depth_sample": cut(s["depth_sample"]),
            "T_WC_sample": cut(s["T_WC_sample"]), "norm_sample": cut(s["norm_sample"]),
            "binary_masks": None,
            "_raw": s, "_sc": sc,
        }

    # ------------------------------------------------------------------ loss + backward (trainer.py:768-868, 981)
    def _raw_from_public(self, sample):
        """A `sample` dict that did not come from our sample_points (a caller assembled the reference's 11
        tensors itself): rebuild what the step kernel needs."""
        dev = self._hip.device
        pc = sample["pc"].detach().to(dev, torch.float32).contiguous()
        R, S = pc.shape[0], pc.shape[1]
        T = sample["T_WC_sample"].to(dev, torch.float32)
        dC = sample["dirs_C_sample"].to(dev, torch.float32).contiguous()
        dW = (T[:, :3, :3] * dC[:, None, :]).sum(-1).contiguous()          # transform.py:36-41
        i64 = lambda t: t.to(dev, torch.int64).contiguous()
        F = int(sample["depth_batch"].shape[0])
        s = dict(n_valid=torch.tensor([R], dtype=torch.int32, device=dev), pc=pc,
                 z_vals=sample["z_vals"].to(dev, torch.float32).contiguous(),
                 depth_sample=sample["depth_sample"].to(dev, torch.float32).contiguous(),
                 dirs_C_sample=dC, dirs_W_sample=dW,
                 norm_sample=None if sample.get("norm_sample") is None else sample["norm_sample"].to(dev, torch.float32).contiguous(),
                 indices_b=i64(sample["indices_b"]), indices_h=i64(sample["indices_h"]), indices_w=i64(sample["indices_w"]),
                 max_rays=R, S=S, n_frames=F)
        sc = self._sample_cfg(n_strat=S - self.n_surf_samples)
        return s, sc

    def _optim_kw(self, **extra):
        """the engine's `optim` dict from the optimiser's (only) parameter group, plus `extra`"""
        g = self.optimiser.param_groups[0]
        return dict(lr=g["lr"], weight_decay=g["weight_decay"], betas=g["betas"], eps=g["eps"], **extra)

    def _step_kernels(self, s, sc, fused_optim, frame_avg_dst):
        """sampler outputs -> reduce buffer (+ optimiser when fused).  Returns (loss_approx, frame_avg_loss)."""
        hip, eng = self._hip, self.engine
        noise, kw = None, {}
        if self.noise_std is not None:   # fc_map.py:106-108 (drawn even for 0)
            if hip.rng == "torch":
                R = int(s["n_valid"].item())
                noise = torch.randn(R, s["S"], device=hip.device) * self.noise_std
            else:                        # philox mode: drawn inside the kernel
                hip.noise_count += 1
                kw = dict(noise_std=self.noise_std, noise_seed=dp.rank_seed(hip.seed, self._rank()),
                          noise_offset=hip.noise_count)
        if fused_optim:
            kw["optim"] = self._optim_kw()
            if frame_avg_dst is not None:   # frames.frame_avg_losses[idxs] = ... inside the launch
                kw["optim"].update(frame_avg_out=frame_avg_dst[0], frame_avg_index=frame_avg_dst[1])
        if hip.dist_group is not None and self.bounds_method == "pc":
            kw["surf_group"] = hip.dist_group
        if hip.clock_slots:              # this rank's previous step time rides in the message's tail (one slot per rank)
            kw.update(extra_slot=hip.rank, extra_value=hip.prev_step_ms)
        if hip.prof_events is not None:  # bench.py: HIP events around this step's kernels (a ctypes array of four hipEvent_t), once
            kw["prof_events"], hip.prof_events = hip.prof_events, None
        split = hip.dist_group is not None and hip.overlap_allreduce and not fused_optim
        if split:
            if hip.split_event is None:
                hip.split_event, hip.comm_stream = dp.new_split_event(hip.device), torch.cuda.Stream(hip.device)
            kw["split_event"] = hip.split_event
        dbg = eng.train_step(s, self._loss_cfg(), sc, noise=noise, **kw)
        if split:                        # the message in two parts, the first one beside the closing reduction's second launch
            dp.allreduce_split_(eng.reduce_buf, eng.reduce_split, hip.split_event, hip.comm_stream, hip.dist_group)
        elif hip.dist_group is not None:   # sums over ranks; AdamW divides by the reduced count
            if hip.rccl is not None:       # THE collective of the step: RCCL on the step's own stream, enqueued by the C library
                eng.allreduce_direct(hip.rccl)
            else:                          # (gloo / a torch without the communicator handle: the framework's side-stream form)
                dp.allreduce_(eng.reduce_buf, hip.dist_group)
        return dbg

    def sdf_eval_and_loss(self, sample, do_avg_loss=True):
        """(total_loss, losses, loss_approx, frame_avg_loss) as the reference.  The backward pass has already
        run when this returns (gradient sums are in the engine's reduce buffer): the caller's
        `total_loss.backward()` is a no-op and `self.optimiser.step()` applies the update."""
        if "_raw" in sample:
            s, sc = sample["_raw"], sample["_sc"]
        else:
            s, sc = self._raw_from_public(sample)
        self._step_kernels(s, sc, fused_optim=False, frame_avg_dst=None)
        eng = self.engine
        ls = eng.loss_sums().detach().cpu()
        losses = StepLosses(ls, self.grad_weight != 0, self.eik_weight != 0)
        anchor = next(iter(self.sdf_map.parameters()))
        total_loss = _BackwardDone.apply((eng.loss_sums()[_ffi.LS_TOTAL] / eng.loss_sums()[_ffi.LS_COUNT]).detach(), anchor)
        loss_approx = frame_avg_loss = None
        if do_avg_loss:
            loss_approx, frame_avg_loss = eng.frame_avg(s["n_frames"])
        return total_loss, losses, loss_approx, frame_avg_loss

    # ------------------------------------------------------------------ step (trainer.py:951-1016)
    def _timing_start(self, st):
        """metrics.start_timing (metrics.py:13-22): device-synchronised, CUDA(HIP) events.  `st` is the stream all of
        the step's work is launched on; synchronising it is the reference's device synchronisation for this path
        (torch.cuda.synchronize() itself costs ~5 us of host time per call in index / env lookups)."""
        if st is not None:
            st.synchronize()
            ev = self._hip.timing_events          # ONE pair of events re-recorded every step: no event creation on the step path
            if ev is None:
                ev = self._hip.timing_events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record(st)
            return ev
        import time
        return time.perf_counter(), None

    def _timing_end(self, st, start, end):
        """metrics.end_timing (metrics.py:25-38), milliseconds.  The reference synchronises, records `end`, synchronises again;
        here `end` is recorded IN STREAM ORDER behind the step's last launch and the stream is synchronised once: the same
        interval on the device (start of the step's first kernel's queue slot to the end of its last kernel) without the host's
        wake-up latency of the first synchronisation inside it, and one device round trip less per step."""
        if st is not None:
            end.record(st)
            st.synchronize()
            return start.elapsed_time(end)
        import time
        return (time.perf_counter() - start) * 1000.0

    def step(self):
        dev = self._hip.device
        if dev.type != "cuda":
            return self._step(None)
        from .engine import pinned_stream
        if _CUDA_GET_DEVICE is not None and dev.index is not None and _CUDA_GET_DEVICE() == dev.index:
            with pinned_stream(dev.index) as st:      # already the current device: no device switch around the step (~3 us of host time)
                return self._step(st)
        with torch.cuda.device(dev), pinned_stream(dev) as st:
            return self._step(st)

    def _step(self, st):
        hip = self._hip
        start, end = self._timing_start(st)

        K = self.frames.T_WC_batch.shape[0]
        if len(self.frames) > self.window_size and self.incremental:
            # from here on select_keyframes reads frames.frame_avg_losses EVERY step: a store that can keep them in pinned host
            # memory (isdf_amd.frame_store; not the reference's FrameData) is asked to, once -- the closing launch then writes
            # them zero-copy and the draw below never touches the device
            if hip.device.type == "cuda" and self.frames.frame_avg_losses.device.type == "cuda":
                to_host = getattr(self.frames, "losses_to_host", None)
                if to_host is not None:
                    to_host()
            idxs = self._select_window()               # the reference's select_keyframes; replicated under data parallelism
        else:
            idxs = np.arange(K)
        self.active_idxs = idxs
        # The window: up to 8 keyframes travel INLINE as kernel arguments (sampler, step tail) -- select_keyframes re-draws it on
        # the host every step once K > window_size, and a device copy per step (two H2D copies + new call plans) cost ~80 us of
        # the synchronised step in that regime.  Longer windows (non-incremental runs over many frames) use cached device tensors.
        if hip.inline_window and len(idxs) <= _ffi.MAX_INLINE_FRAMES:
            fidx = tuple(idxs.tolist()) if isinstance(idxs, np.ndarray) else tuple(int(i) for i in idxs)   # (ndarray.tolist(): Python ints, 0.2 us)
            # reference quirk q4: normals are read from the UN-windowed normal_batch with
            # window-local indices (trainer.py:956,969); fix_normal_window=True uses idxs.
            nidx = fidx if hip.fix_normal_window else tuple(range(len(fidx)))
        else:
            key = (tuple(int(i) for i in idxs), bool(hip.fix_normal_window))
            if hip.idx_cache is None or hip.idx_cache[0] != key:
                fidx = torch.as_tensor(np.asarray(idxs), dtype=torch.int32, device=hip.device)
                nidx = fidx if hip.fix_normal_window else torch.arange(len(idxs), dtype=torch.int32, device=hip.device)
                hip.idx_cache = (key, fidx, nidx)
            _, fidx, nidx = hip.idx_cache
        norm_batch = self.frames.normal_batch if self.do_normal else None
        sc = self._sample_cfg()
        # no depth_batch[idxs] copy (trainer.py:965: 16 MB at 680x1200x5): the sampler takes the window indices
        s = self._sample_raw(self.frames.depth_batch, self.frames.T_WC_batch, norm_batch, fidx,
                             nidx if norm_batch is not None else None, sc, want_T=False, reuse=True)
        self.active_pixels = _LazyCut(s)

        fal = self.frames.frame_avg_losses
        fused = hip.dist_group is None and hip.fuse_optimiser
        # the kernels write the window's averages straight into the keyframe store: a device tensor (the reference's FrameData), or
        # pinned host memory (isdf_amd.frame_store: select_keyframes then never touches the device)
        direct = fal.is_contiguous() and fal.dtype == torch.float32 and (fal.device == hip.device or self._pinned(fal))
        dbg = self._step_kernels(s, sc, fused, (fal, fidx) if direct else None)
        eng = self.engine
        if not fused and direct and hip.fuse_optimiser:
            # two-call / data-parallel form: ONE closing launch = AdamW on the (all-reduced) gradient sums + operand
            # repack + `frames.frame_avg_losses[idxs] = frame_avg_loss` from the reduced bins (trainer.py:979-982)
            eng.train_step_finish(len(idxs), self._optim_kw(frame_avg_out=fal, frame_avg_index=fidx))
        else:
            if not fused or not direct:                # separate launches (caller-owned frame_avg_losses layout, or
                if direct:                             # fuse_optimiser=False: the reference's call sequence)
                    eng.frame_avg(len(idxs), out=fal, index=fidx)
                else:
                    _, fa = eng.frame_avg(len(idxs))
                    self.frames.frame_avg_losses[[int(i) for i in idxs]] = fa      # trainer.py:979
            if not fused:
                self.optimiser.step()                  # AdamW on the (all-reduced) gradient sums
        # `losses`: the step's last launch stored the (reduced) loss sums -- and, data parallel, the ranks' step times -- in
        # pinned host memory (eng.mailbox); they are valid after the closing synchronisation below.  No copy command.
        if getattr(eng, "mailbox", None) is None:      # engines without a host mailbox (tests' CPU stand-in)
            hip.loss_host.copy_(eng.loss_sums(), non_blocking=True)
            mailbox = hip.loss_host
        else:
            mailbox = eng.mailbox
            if hip.dist_group is not None and not (not fused and direct and hip.fuse_optimiser):
                # reference call sequence (separate AdamW launch): the reduced sums were not mirrored by a closing launch
                mailbox[:8].copy_(eng.loss_sums(), non_blocking=True)
                if hip.clock_slots:
                    mailbox[8:].copy_(eng.reduce_buf[eng.reduce_floats:], non_blocking=True)

        step_time = self._timing_end(st, start, end)
        clock_ms = step_time
        if hip.virtual_step_ms is not None:            # pinned schedule (parity / accuracy runs)
            clock_ms = step_time = float(hip.virtual_step_ms)
        elif hip.clock_slots:
            # ONE virtual clock for all ranks (the frame schedule is a function of it) WITHOUT a second collective: every
            # rank's time of the PREVIOUS step came back in the tail of this step's all-reduce message; the clock advances
            # by the slowest rank's, one step late (step 0 advances it by 0).  This step's own time goes out with the next.
            clock_ms = float(mailbox[8:8 + hip.clock_slots].max()) if mailbox.numel() >= 8 + hip.clock_slots else \
                float(eng.reduce_buf[eng.reduce_floats:].max())
            hip.prev_step_ms = float(np.float32(step_time))
        losses = StepLosses(mailbox, self.grad_weight != 0, self.eik_weight != 0)   # (reads the first 8 floats; a slice is 1.7 us)
        hip.step_count += 1
        self.tot_step_time += (1 / self.frac_time_perception) * (clock_ms / 1000.0)
        self.steps_since_frame += 1
        return losses, step_time

    def _pinned(self, t):
        """t is a pinned host tensor the HIP device can write (is_pinned() is a driver query: asked once per buffer)"""
        hip = self._hip
        if t.device.type != "cpu" or hip.device.type != "cuda":
            return False
        key = (t.data_ptr(), t.numel())
        if getattr(hip, "pinned_key", None) != key:
            hip.pinned_key, hip.pinned_ok = key, bool(t.is_pinned())
        return hip.pinned_ok

    def _select_window(self):
        """The reference's window draw (`select_keyframes`, trainer.py:652-674) runs unchanged.  Under data parallelism
        every rank must pick the SAME window, and it does without a collective: the inputs are bit-identical on every rank
        (`frames.frame_avg_losses` comes from the all-reduced bins) and `np.random.choice` draws from a private stream
        that graft() seeded identically everywhere -- swapped in for the call, so nothing else that touches numpy's
        global generator on one rank can de-synchronise it."""
        hip = self._hip
        if hip.dist_group is None:
            return self.select_keyframes()
        saved = np.random.get_state()
        np.random.set_state(hip.window_rng_state)
        try:
            return self.select_keyframes()
        finally:
            hip.window_rng_state = np.random.get_state()
            np.random.set_state(saved)

    # ------------------------------------------------------------------ keyframe test (trainer.py:586-620)
    def is_keyframe(self, T_WC, depth_gt):
        """sampler (n_rays_is_kf rays, 0.8 m behind the surface) -> frozen net forward -> per-ray z sort +
        first-zero-crossing depth render + below-threshold count, all in HIP kernels; the decision and the
        printed line are the reference's.  Rank-independent draws under data parallelism."""
        hip = self._hip
        sample_pts = self.sample_points(depth_gt, T_WC, n_rays=self.n_rays_is_kf, dist_behind_surf=0.8,
                                        _shared_key=hip.dist_group is not None)
        s = sample_pts["_raw"]
        pc = s["pc"]
        n = int(sample_pts["pc"].shape[0])           # R valid rays (sample_points already synchronised on it)
        noise = None
        if self.noise_std is not None:               # drawn on the CUT tensor like upstream (trainer.py:594-595,
            noise = torch.zeros(pc.shape[:-1], device=hip.device)     # fc_map.py:106): the generator advances by R x S
            noise[:n] = torch.randn(n, pc.shape[1], device=hip.device) * self.noise_std
        sdf = self.frozen_sdf_map.engine.sdf_eval(pc, noise=noise)           # frozen net, no grad (trainer.py:594-595)
        view, below = self.engine.render_depth(s["z_vals"], sdf, s["depth_sample"], self.kf_dist_th,
                                               n_valid=s["n_valid"])
        # no valid ray: upstream divides 0 by 0 -> NaN -> `NaN < ratio` is False (trainer.py:606-609)
        below_th_prop = float(below.item()) / n if n > 0 else float("nan")
        is_keyframe = below_th_prop < self.kf_pixel_ratio
        print("Proportion of loss below threshold", below_th_prop, "for KF should be less than",
              self.kf_pixel_ratio, " ---> is keyframe:", is_keyframe)
        return is_keyframe

    # ------------------------------------------------------------------ per-frame ingest (trainer.py:530-562)
    def get_data(self, idxs):
        """The reference's `get_data` runs unchanged (dataset access, host twins, `T_WC_gt`, its own `FrameData` per frame); for the
        duration of the call its two geometry functions are answered by the stencil kernel: `pointcloud_from_depth_torch`
        (transform.py:169-196) hands over the depth image, `estimate_pointcloud_normals` (transform.py:215-270: eight shifted
        cross products through a 70 MB index tensor, ~10 eager kernels) becomes ONE launch of `isdf_estimate_normals` -- same
        camera-frame normals, NaN where the reference leaves NaN (fixture `ingest_small`).  With a 0.3 ms step and
        iters_per_frame = 10 a frame arrives every ~3 ms of stepping: the eager chain was a visible share of that."""
        geo = self._hip.geometry_transform
        if not self.do_normal or geo is None:      # (no normals wanted, or not the reference's trainer module)
            return super().get_data(idxs)
        eng, hip = self.engine, self._hip

        class _DepthAsPointCloud:          # what the first call hands to the second
            def __init__(self, depth, fx, fy, cx, cy):
                self.depth, self.k = depth, (fx, fy, cx, cy)

        def pointcloud_from_depth(depth, fx, fy, cx, cy):
            return _DepthAsPointCloud(depth, fx, fy, cx, cy)

        def estimate_normals(pc):
            if not isinstance(pc, _DepthAsPointCloud):      # some other caller's point cloud: the reference's own arithmetic
                return saved[1](pc)
            fx, fy, cx, cy = pc.k
            hip.ingest_launches += 1
            return eng.estimate_normals(pc.depth, SampleConfig(H=int(pc.depth.shape[0]), W=int(pc.depth.shape[1]),
                                                               fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy)))
        saved = (geo.pointcloud_from_depth_torch, geo.estimate_pointcloud_normals)
        geo.pointcloud_from_depth_torch, geo.estimate_pointcloud_normals = pointcloud_from_depth, estimate_normals
        try:
            return super().get_data(idxs)
        finally:
            geo.pointcloud_from_depth_torch, geo.estimate_pointcloud_normals = saved

    # ------------------------------------------------------------------ mesh reconstruction (trainer.py:1426-1443,1500-1542)
    def get_sdf_grid(self):
        """The network on the cached `grid_pc` as a [grid_dim]^3 volume: ONE forward launch over all grid_dim^3 points (the
        reference's fc_map.chunks makes one per 100 000; the kernel's result per point does not depend on the chunking)."""
        d = self.grid_dim
        with torch.no_grad():
            return self.engine.sdf_eval(self.grid_pc).view(d, d, d)

    def _vis_pointcloud(self):
        """world-frame point cloud of the keyframes at visualisation resolution (update_vis_vars + backproject + draw_pc)"""
        ref = self._hip.ref_module
        self.update_vis_vars()
        pcs_cam = ref.geometry.transform.backproject_pointclouds(self.gt_depth_vis, self.fx_vis, self.fy_vis, self.cx_vis,
                                                                 self.cy_vis)
        pc, _ = ref.draw3D.draw_pc(len(self.frames), pcs_cam, self.frames.T_WC_batch_np)
        return pc

    def mesh_rec(self, crop_mesh_with_pc=True):
        """The reconstructed mesh as a trimesh.Trimesh in world coordinates, what the reference's mesh_rec returns.

        Contract kept: a trainer without a GT scene that runs incrementally first re-derives its scene bounds from the keyframes'
        point cloud (set_scene_properties); with crop_mesh_with_pc, faces none of whose vertices lie within crop_dist of that
        point cloud are dropped (a KDTree query on the host) together with the vertices left unreferenced; a pending grid size
        (new_grid_dim / new_grid_pc) is swapped in at the end.  The point cloud is only built when one of the two needs it.

        The mesh itself: get_sdf_grid, then Engine.marching_cubes with draw_mesh's index -> world chain as the kernel's affine
        (isdf_amd.mesh.grid_index_to_world), so vertices and normals come out in world coordinates; ONE device -> host copy;
        flat grey face colours as draw_mesh(..., color_by="none") sets them."""
        from .mesh import grid_index_to_world
        ref = self._hip.ref_module
        if ref is None or not hasattr(ref, "trimesh"):
            raise _ffi.IsdfError("mesh_rec needs the reference's trainer module (trimesh, KDTree, draw3D)")
        rescale = self.gt_scene is False and self.incremental
        pc = self._vis_pointcloud() if (crop_mesh_with_pc or rescale) else None
        if rescale:
            self.set_scene_properties(ref.trimesh.PointCloud(pc))
        sdf = self.get_sdf_grid()
        A = grid_index_to_world(self.grid_dim, self.scene_scale_np, self.bounds_transform_np)
        verts, faces, normals = self.engine.marching_cubes(sdf, 0.0, A)
        nv, nf = verts.shape[0], faces.shape[0]
        flat = torch.cat([verts.reshape(-1), normals.reshape(-1), faces.reshape(-1).view(torch.float32)]).cpu().numpy()
        verts_h = flat[:3 * nv].reshape(nv, 3)
        normals_h = flat[3 * nv:6 * nv].reshape(nv, 3)
        faces_h = flat[6 * nv:].view(np.int32).reshape(nf, 3)
        if crop_mesh_with_pc:
            near = ref.KDTree(pc).query(verts_h, k=1)[0] < self.crop_dist
            faces_h = faces_h[near[faces_h].any(axis=1)]
            used = np.zeros(nv, bool)
            used[faces_h.reshape(-1)] = True
            remap = np.cumsum(used) - 1
            verts_h, normals_h, faces_h = verts_h[used], normals_h[used], remap[faces_h].astype(np.int32)
        mesh = ref.trimesh.Trimesh(vertices=verts_h, vertex_normals=normals_h, faces=faces_h)
        mesh.visual.face_colors = [160, 160, 160, 255]
        if self.new_grid_dim is not None:
            self.grid_dim, self.grid_pc = self.new_grid_dim, self.new_grid_pc
            self.new_grid_dim = self.new_grid_pc = None
        return mesh

    # ------------------------------------------------------------------ rendered views (trainer.py:1055-1147,1225-1280)
    def _render_rng(self, B, R, S):
        """uniforms of one render pass: rng "torch" draws torch.rand(R, S) per view on the trainer's device, in the reference's
        order (sample.py:123) -> dict(draws=[B, R, S]); "philox" advances the render counter (visualisation only: not part of
        hip_state_dict) and leaves the torch generator alone"""
        hip = self._hip
        if hip.rng == "torch":
            return dict(draws=torch.stack([torch.rand(R, S, device=self.device) for _ in range(B)]))
        hip.render_count = getattr(hip, "render_count", 0) + 1
        return dict(seed=hip.seed, counter=hip.render_count)

    def _vis_poses(self):
        T_WC_batch = self.frames.T_WC_batch
        if self.frames.T_WC_track:                 # trainer.py:1229-1231 (a truthy track: a list of [4, 4] poses or a one-pose tensor)
            T_WC_batch = self.frames.T_WC_track
        if isinstance(T_WC_batch, (list, tuple)):
            T_WC_batch = torch.stack([torch.as_tensor(t).reshape(4, 4) for t in T_WC_batch])
        return T_WC_batch

    def render_depth_vis(self):
        """[K, H_vis, W_vis] depth of every keyframe from the map, on the device: ONE isdf_render_views pass over the K poses, the
        depth range [min_depth, cv2.resize(depth, INTER_LINEAR) + 0.8] read from the device depth_batch (no host resize, no
        upload), n_strat_samples stratified samples, first crossing.  No host synchronisation."""
        K, H, W, S = len(self.frames), self.H_vis, self.W_vis, self.n_strat_samples
        T = self._vis_poses()[:K]
        rng = self._render_rng(K, H * W, S)
        with torch.no_grad():
            depth, _ = self.engine.render_views(T, self.dirs_C_vis[0], H, W, S, depth_images=self.frames.depth_batch[:K],
                                                min_depth=self.min_depth, depth_offset=0.8, **rng)
        return depth.view(K, H, W)

    def render_normals_vis(self, view_depths):
        """[K, H_vis, W_vis, 3] camera-frame normals at the given depths (render.render_normals per keyframe, render.py:38-57):
        one pass of points, forward with input gradient and rotation by the inverse of each pose's 3x3 block."""
        K, H, W = len(self.frames), self.H_vis, self.W_vis
        T = self._vis_poses()[:K]
        with torch.no_grad():
            _, normals = self.engine.render_views(T, self.dirs_C_vis[0], H, W, depth=view_depths.reshape(K, H * W))
        return normals.view(K, H, W, 3)

    def latest_frame_vis(self, do_render=True):
        """The reference's (rgbd_vis, render_vis, T_WC_np) and timing line.  The renders run on the device: a coarse pass of 20
        samples over [min_depth, max_depth] on dirs_C_vis, the align-corners upsample and a fine pass of 12 samples over
        d +- 0.1 on dirs_C_vis_up (in-kernel), normals at the fine depth; depth and normal image come back in one copy.
        The host image work (cv2.resize, imgviz.depth2rgb, hstack) is the reference module's own.  do_render=False is the
        reference's path."""
        if not do_render:
            return super().latest_frame_vis(do_render=False)
        ref = self._hip.ref_module
        start, end = ref.start_timing()
        if self.live:
            data = self.scene_dataset[0]
            image, depth, T_WC_np = data['image'], data['depth'], data['T']
        else:
            image = self.frames.im_batch_np[-1]
            depth = self.frames.depth_batch_np[-1]
            T_WC_np = self.frames.T_WC_batch_np[-1]
        w, h = self.W_vis_up * 2, self.H_vis_up * 2
        image = ref.cv2.resize(image, (w, h))
        depth = ref.cv2.resize(depth, (w, h))
        depth_viz = ref.imgviz.depth2rgb(depth, min_value=self.min_depth, max_value=self.max_depth)
        rgbd_vis = np.hstack((image, depth_viz))

        T_WC = torch.FloatTensor(T_WC_np).to(self.device)[None, ...]
        Hc, Wc, Hu, Wu = self.H_vis, self.W_vis, self.H_vis_up, self.W_vis_up
        rng_c = self._render_rng(1, Hc * Wc, 20)
        rng_f = self._render_rng(1, Hu * Wu, 12)
        eng = self.engine
        with torch.no_grad():
            coarse, _ = eng.render_views(T_WC, self.dirs_C_vis, Hc, Wc, 20, scalar_range=(self.min_depth, self.max_depth),
                                         **rng_c)
            fine, normals = eng.render_views(T_WC, self.dirs_C_vis_up, Hu, Wu, 12, upsample=coarse.view(1, Hc, Wc),
                                             depth_offset=0.1, want_normals=True, **rng_f)
            normals = torch.clip((-normals + 1.0) / 2.0, 0., 1.)
            host = torch.cat([fine.reshape(-1), normals.reshape(-1)]).cpu().numpy()
        render_depth = host[:Hu * Wu].reshape(Hu, Wu)
        render_depth_viz = ref.imgviz.depth2rgb(render_depth, min_value=self.min_depth, max_value=self.max_depth)
        normals_viz = (host[Hu * Wu:].reshape(Hu, Wu, 3) * 255).astype(np.uint8)
        render_vis = np.hstack((normals_viz, render_depth_viz))
        render_vis = ref.cv2.resize(render_vis, (int(render_vis.shape[1] * 2), int(render_vis.shape[0] * 2)))
        elapsed = ref.end_timing(start, end)
        print("Time for depth and normal render", elapsed)
        return rgbd_vis, render_vis, T_WC_np

    # ------------------------------------------------------------------ evaluation against ground truth (trainer.py:1819-2064)
    def _gt_volume(self):
        """`self.gt_sdf_interp`'s grid on the device (isdf_amd.metrics.GtVolume), uploaded once and re-made only if the attribute is
        replaced; the interpolator itself is never called"""
        from .metrics import GtVolume
        hip, itp = self._hip, self.gt_sdf_interp
        if itp is None:
            raise _ffi.IsdfError("evaluation needs trainer.gt_sdf_interp (a ground-truth SDF grid)")
        c = getattr(hip, "gt_volume", None)
        if c is None or c[0] is not itp:
            c = hip.gt_volume = (itp, GtVolume.from_interpolator(itp, hip.device))
        return c[1]

    def _eval_frames(self, upto=None):
        """(depth_batch [F,H,W], T_WC_batch [F,4,4]) of the cached sequence up to the virtual clock, as eval_sdf_visible and
        eval_object_sdf build them (trainer.py:1869-1875,1968-1974) -- but RESIDENT: the reference converts and uploads the whole
        sequence on every call (2 GB at 600 frames of 680 x 1200); here only the frames not yet on the device are read from
        `self.cached_dataset` and copied.  Incremental runs ask for arange(int(tot_step_time * fps)), which only grows; the
        non-incremental get_all() is uploaded once.  The cache lives on self._hip (not in hip_state_dict); drop_eval_cache()
        releases it; a clock that went backwards or another dataset object starts it afresh.
        upto: the frames of cached_dataset[arange(upto)] instead of the clock's (eval_fixed: its timestamp is normally behind the
        clock, so this is a prefix of what is held; frames beyond what is held are uploaded, once)."""
        hip = self._hip
        ds = self.cached_dataset
        c = getattr(hip, "eval_cache", None)
        mode = "incremental" if self.incremental else "all"
        want = int(self.tot_step_time * self.fps) if self.incremental else 0
        if c is None or c.dataset is not ds or c.mode != mode or (upto is None and want < c.clock):
            c = hip.eval_cache = types.SimpleNamespace(dataset=ds, mode=mode, asked=0, clock=0, held=0, depth=None, T=None,
                                                       uploaded_frames=0, uploaded_bytes=0)
        if upto is None:
            c.clock = want
        else:
            want = int(upto)
        if mode == "all":
            if c.depth is None:
                sample = ds.get_all()
                self._eval_cache_append(c, sample["depth"], sample["T"])
        elif want > c.asked:
            sample = ds[np.arange(c.asked, want)]
            self._eval_cache_append(c, sample["depth"], sample["T"])
            c.asked = want
        if c.depth is None:                      # no frame yet: the reference's empty batch (its rays_per_frame then divides by 0)
            return (torch.zeros(0, self.H, self.W, device=hip.device), torch.zeros(0, 4, 4, device=hip.device))
        held = c.held
        if (mode == "all" and upto is not None) or (mode != "all" and want < c.asked):
            # a prefix: the frames with an index below `want` (SceneCache.__getitem__ keeps those in keep_ixs, dataset.py:251-257)
            keep = getattr(ds, "keep_ixs", None)
            k = int(np.searchsorted(np.asarray(keep), want)) if keep is not None else min(want, len(ds))
            held = min(k, c.held)
        return c.depth[:held], c.T[:held]

    def _eval_cache_append(self, c, depth, T):
        """new frames -> the resident buffers (capacity grows by half, never beyond the dataset's length when it has one)"""
        dev = self._hip.device
        depth = torch.as_tensor(np.asarray(depth, np.float32))
        T = torch.as_tensor(np.asarray(T, np.float32)).reshape(-1, 4, 4)
        k = int(depth.shape[0])
        if k == 0:
            return
        need = c.held + k
        if c.depth is None or need > c.depth.shape[0]:
            cap = need if c.mode == "all" else max(need, (c.held * 3) // 2, 32)
            try:
                cap = max(need, min(cap, len(c.dataset)))
            except TypeError:
                pass
            nd = torch.empty((cap,) + tuple(depth.shape[1:]), dtype=torch.float32, device=dev)
            nT = torch.empty(cap, 4, 4, dtype=torch.float32, device=dev)
            if c.held:
                nd[:c.held].copy_(c.depth[:c.held]); nT[:c.held].copy_(c.T[:c.held])
            c.depth, c.T = nd, nT
        c.depth[c.held:need].copy_(depth)
        c.T[c.held:need].copy_(T)
        c.held = need
        c.uploaded_frames += k
        c.uploaded_bytes += depth.numel() * 4 + T.numel() * 4

    def drop_eval_cache(self):
        """release the resident evaluation frames and the ground-truth volume (the next evaluation uploads them again)"""
        self._hip.eval_cache = None
        self._hip.gt_volume = None

    def eval_sdf(self, samples=200000, visible_region=True):
        """The reference's dict (av_l1, binned_l1 [6], l1_chomp_costs [3]; trainer.py:1819-1866).  The points come from
        eval_sdf_visible (bound below) or the reference's own eval_sdf_volume; ground-truth interpolation, mask, L1, the six bins
        and the CHOMP differences are ONE isdf_sdf_metrics pass and one copy of 24 doubles -- no point leaves the device."""
        from . import metrics
        if visible_region:
            sdf, eval_pts = self.eval_sdf_visible(samples)
        else:
            sdf, eval_pts = self.eval_sdf_volume(samples)
        return metrics.sdf_metrics(self.engine, self._gt_volume(), eval_pts, sdf, exclude_zero_gt=True).as_dict()

    def eval_sdf_visible(self, samples=20000):
        """(sdf [n], eval_pts [n,3]) of one sample per ray over the cached sequence (trainer.py:1868-1905): the same
        sample_points call and the same noise_std=0 forward, so the generators advance as in the reference; the frames come
        from the resident cache (_eval_frames).  The reference's ScanNet line (`dist_behind_surf == 0`, a comparison) has no effect."""
        depth_batch, T_WC_batch = self._eval_frames()
        rays_per_frame = samples // depth_batch.shape[0]
        sample_pts = self.sample_points(depth_batch, T_WC_batch, n_rays=rays_per_frame, dist_behind_surf=self.dist_behind_surf,
                                        n_strat_samples=1, n_surf_samples=0)
        pc = sample_pts["pc"]
        with torch.set_grad_enabled(False):
            sdf = self.sdf_map(pc, noise_std=0)
        return sdf.flatten(), pc.squeeze()

    def eval_object_sdf(self, samples=10000):
        """Per object the mean |sdf - gt| in a box around it, NaN while it is not visible (trainer.py:1955-2008).  The visibility
        test is the reference's (100 random offsets per object, frustum.is_visible_torch) on the resident frames; per visible
        object one isdf_sdf_metrics call that keeps zero-valued ground truth; the records come back in one copy."""
        errors = None
        if self.obj_bounds_file is not None:
            ref = self._hip.ref_module
            obj_bounds = ref.metrics.get_obj_eval_bounds(self.obj_bounds_file, self.up_ix)
            obj_bounds = torch.FloatTensor(obj_bounds).to(self.device)
            offsets = torch.rand(100, 3).to(self.device)
            extents = obj_bounds[:, 1] - obj_bounds[:, 0]
            pts = obj_bounds[:, 0] + offsets[:, None] * extents
            depth_batch, T_WC_batch = self._eval_frames()
            visible = ref.geometry.frustum.is_visible_torch(pts.view(-1, 3), T_WC_batch, depth_batch, self.H, self.W, self.fx,
                                                            self.fy, self.cx, self.cy, trunc=0.05)
            visible = visible.detach().cpu().numpy().sum(axis=0) > 0
            visible = visible.reshape(100, len(obj_bounds))
            visible = visible.sum(axis=0) / 100 > 0.5
            vol, records = self._gt_volume(), []
            for i in range(len(obj_bounds)):
                if visible[i]:
                    offsets = torch.rand(samples, 3).to(self.device)
                    bounds = obj_bounds[i]
                    pts = bounds[0] + offsets * (bounds[1] - bounds[0])[None, :]
                    with torch.set_grad_enabled(False):
                        sdf = torch.squeeze(self.sdf_map(pts))
                    records.append(self.engine.sdf_metrics(vol, pts, sdf, exclude_zero_gt=False)[0])
            host = torch.stack(records).cpu().numpy() if records else np.zeros((0, _ffi.METRICS_RECORD))
            errors, k = [], 0
            for i in range(len(obj_bounds)):
                if visible[i]:
                    with np.errstate(divide="ignore", invalid="ignore"):
                        errors.append(np.float64(host[k, 2]) / np.float64(host[k, 0]))
                    k += 1
                else:
                    errors.append(np.nan)
        return errors

    def eval_traj_cost(self, t_ahead=5.):
        """(pred_chomp_costs [3], gt_chomp_costs [3]) summed along the next t_ahead seconds of the trajectory, or (nan, nan) when
        fewer than 90 % of its points have a valid non-zero ground truth or the section is shorter than 30 poses
        (trainer.py:2010-2052).  Network forward, then one isdf_sdf_metrics call: the validity count and both sets of sums
        are fields of its record."""
        from . import metrics
        if self.traj_file:
            traj = np.loadtxt(self.traj_file)
            traj_start_ix = self.tot_step_time * 30
            traj_end_ix = min(len(traj) - 1, (self.tot_step_time + t_ahead) * 30)
            traj_section = traj[int(traj_start_ix): int(traj_end_ix)]
            if len(traj_section) < 30:
                return np.nan, np.nan
            eval_pts = torch.from_numpy(np.ascontiguousarray(traj_section[:, [3, 7, 11]]))
            with torch.set_grad_enabled(False):
                sdf = self.sdf_map(eval_pts.float().to(self.device)).squeeze()
            m = metrics.sdf_metrics(self.engine, self._gt_volume(), eval_pts, sdf, exclude_zero_gt=True)
            if m.n_valid < 0.9 * len(traj_section):
                return np.nan, np.nan
            return m.pred_chomp_sums, m.gt_chomp_sums

    def eval_mesh(self, samples=200000):
        """(accuracy, completion) of the reconstructed mesh against the ground-truth scene mesh (trainer.py:2054-2064,
        metrics.py:62-73): mesh_rec() and the two trimesh surface samplings are the reference's; the two nearest-neighbour
        passes run on the device (isdf_nn_distance) instead of two host KD-trees."""
        from . import metrics
        ref = self._hip.ref_module
        if ref is None or not hasattr(ref, "trimesh"):
            raise _ffi.IsdfError("eval_mesh needs the reference's trainer module (trimesh)")
        mesh_gt = ref.trimesh.load(self.scene_file)
        sdf_mesh = self.mesh_rec()
        rec_pc = ref.trimesh.sample.sample_surface(sdf_mesh, samples)
        gt_pc = ref.trimesh.sample.sample_surface(mesh_gt, samples)
        return metrics.accuracy_completion(self.engine, gt_pc[0], rec_pc[0])

    # ------------------------------------------------------------------ fixed-point evaluation (trainer.py:2080-2088)
    @staticmethod
    def _region_flags(valid_gt_sdf, valid_vox_sdf, valid_gt_grad=None):
        """flag byte per drawn point (_ffi.FLAG_*) from the mask files of one point set, eval_pts.py:130-152 written out:
        A = valid_gt_sdf [N] selects the vis sdf set, valid_vox_sdf [A.sum()] the vox subset of it; G = valid_gt_grad [N] the vis
        gradient set, and the vox gradient set is A & B & G with B scattered back to the N points."""
        A = np.asarray(valid_gt_sdf, bool).reshape(-1)
        B = np.zeros(A.shape[0], bool)
        B[A] = np.asarray(valid_vox_sdf, bool).reshape(-1)
        flags = A * np.uint8(_ffi.FLAG_VIS_SDF) + (A & B) * np.uint8(_ffi.FLAG_VOX_SDF)
        if valid_gt_grad is not None:
            G = np.asarray(valid_gt_grad, bool).reshape(-1)
            flags = flags + G * np.uint8(_ffi.FLAG_VIS_GRAD) + (A & B & G) * np.uint8(_ffi.FLAG_VOX_GRAD)
        return flags.astype(np.uint8)

    def eval_fixed(self):
        """The reference's nested dict (eval_pts.fixed_pts_eval, eval_pts.py:96-299) at the next timestamp of `self.eval_times`.
        Frames from the resident cache; the pixels and the one stratified draw on the torch CPU generator exactly as
        eval_pts.sample_rays draws them (the mask files are aligned index for index with these draws), whatever graft(rng=...)
        says; ONE sampler launch gives both point sets (column 0 of pc: sample_surface's, column 1: sample_visible_region's); one
        forward-with-gradient launch for the visible region, one forward for surface, objects and volume together; one
        isdf_region_metrics pass per leg into one records tensor, ONE copy back.  Two host synchronisations: the sampler's
        n_valid and that copy.  The Philox counter does not advance; afterwards the torch CPU generator and numpy's global one are
        where the reference leaves them.  Deviations: the visible region's sdf comes from the gradient-returning
        kernel; a mask-selected point outside the ground-truth grid is left out (the reference averages its 1e99 fill value in)
        with one warning; the object points are rounded to fp32 before the ground-truth lookup."""
        from . import metrics
        if self.dataset_format not in ("replicaCAD", "ScanNet"):       # the reference's own method (it fails there too)
            return super().eval_fixed()
        t = self.eval_times.pop(0)
        t_str = f"{t:.3f}"
        pts_dir = os.path.join(self.eval_pts_dir, t_str)
        masks_dir = self.eval_pts_dir + t_str
        surf_valid_gt_sdf = np.load(masks_dir + "/surf_valid_gt_sdf.npy")
        surf_valid_vox_sdf = np.load(masks_dir + "/surf_valid_vox_sdf.npy")
        vis_valid_gt_sdf = np.load(masks_dir + "/vis_valid_gt_sdf.npy")
        vis_valid_vox_sdf = np.load(masks_dir + "/vis_valid_vox_sdf.npy")
        vis_valid_gt_grad = np.load(masks_dir + "/vis_valid_gt_grad.npy")
        vis_valid_vox_grad = np.load(masks_dir + "/vis_valid_vox_grad.npy")
        assert surf_valid_gt_sdf.sum() == surf_valid_vox_sdf.shape[0]
        assert vis_valid_gt_sdf.sum() == vis_valid_vox_sdf.shape[0]
        assert vis_valid_gt_grad.sum() == vis_valid_vox_grad.shape[0]

        eng, dev = self.engine, self._hip.device
        upto = int(min(np.floor(t * 30), len(self.scene_dataset)))
        depth_batch, T_WC_batch = self._eval_frames(upto)
        F, H, W = (int(v) for v in depth_batch.shape)

        # eval_pts.sample_rays' draws (eval_pts.py:354-393): seed, randint h, randint w, rand(n_valid, 1)
        torch.manual_seed(float(t_str) * 1e3)
        rays_per_frame = 200000 // F
        ih = torch.randint(0, H, (rays_per_frame * F,))
        iw = torch.randint(0, W, (rays_per_frame * F,))
        after_pixels = torch.get_rng_state()      # where sample_surface, the reference's last seeded call, leaves the generator
        ih_d, iw_d = ih.to(dev), iw.to(dev)
        ib_d = torch.arange(F, device=dev).repeat_interleave(rays_per_frame)
        R = int((depth_batch[ib_d, ih_d, iw_d] != 0).sum().item())           # host synchronisation 1 of 2
        U = torch.rand(R, 1)
        torch.set_rng_state(after_pixels)
        sc = self._sample_cfg(n_rays=rays_per_frame, dist_behind_surf=0. if self.dataset_format == "ScanNet" else 0.1,
                              n_strat=1, n_surf=1)
        sc.min_depth, sc.H, sc.W = 0.1, H, W
        s = eng.sample(depth_batch.contiguous(), T_WC_batch.contiguous(), None,
                       torch.arange(F, dtype=torch.int32, device=dev), None, sc,
                       draws=dict(indices_h=ih_d, indices_w=iw_d, U=U, N_off=torch.zeros(R, 0)), want_T=False)
        pc = s["pc"][:R]
        surf_pts, vis_pts = pc[:, 0], pc[:, 1]
        if vis_valid_gt_sdf.shape[0] != R or vis_valid_gt_grad.shape[0] != R or surf_valid_gt_sdf.shape[0] != R:
            raise IndexError("eval_fixed: the mask files of %s hold %d / %d / %d entries for %d drawn points"
                             % (masks_dir, vis_valid_gt_sdf.shape[0], vis_valid_gt_grad.shape[0], surf_valid_gt_sdf.shape[0], R))
        vis_flags = self._region_flags(vis_valid_gt_sdf, vis_valid_vox_sdf, vis_valid_gt_grad)
        surf_flags = self._region_flags(surf_valid_gt_sdf, surf_valid_vox_sdf)

        # objects (eval_pts.py:204-258): 10000 seeded points per box, only where the timestamp directory has files for it
        obj_legs = None
        obj_bounds_file = self.seq_dir + '/obj_bounds.txt'
        if os.path.exists(obj_bounds_file):
            obj_bounds = np.loadtxt(obj_bounds_file).reshape(-1, 2, 3)          # eval_pts.load_obj_bounds
            obj_bounds[:, 1] += 0.08
            obj_bounds[:, 0, 0] -= 0.08
            obj_bounds[:, 0, 2] -= 0.08
            obj_legs = []
            listing = os.listdir(pts_dir)
            for i, bounds in enumerate(obj_bounds):
                if len([x for x in listing if f'obj{i}' in x]) == 0:
                    continue
                valid_gt_sdf = np.load(masks_dir + f"/obj{i}_valid_gt_sdf.npy")
                valid_vox_sdf = np.load(masks_dir + f"/obj{i}_valid_vox_sdf.npy")
                np.random.seed(0)                                                # eval_pts.object_eval_pts
                offsets = np.random.rand(10000, 3)
                pts = (bounds[0] + offsets * (bounds[1] - bounds[0])[None, :])[valid_gt_sdf]
                fl = np.uint8(_ffi.FLAG_VIS_SDF) + np.asarray(valid_vox_sdf, bool) * np.uint8(_ffi.FLAG_VOX_SDF)
                obj_legs.append((torch.from_numpy(pts.astype(np.float32)), torch.from_numpy(fl.astype(np.uint8))))

        # full volume (eval_pts.py:260-297)
        seq = [x for x in self.seq_dir.split('/') if x != ""][-1]
        if self.dataset_format == "replicaCAD":
            vol_pts_file = self.eval_pts_root + "full_vol/replicaCAD.npy"
        else:
            vol_pts_file = self.eval_pts_root + f"full_vol/{seq}.npy"
        gt_sdf_file = self.eval_pts_root + f"full_vol/gt_{seq}.npy"
        vol_pts = torch.from_numpy(np.load(vol_pts_file).astype(np.float32)).reshape(-1, 3)
        vol_gt = torch.from_numpy(np.load(gt_sdf_file).astype(np.float64)).reshape(-1)

        # network: one forward-with-gradient launch (visible region), one forward launch for everything else
        vis_sdf, vis_grad = eng.sdf_eval(vis_pts, want_grad=True)
        parts = [surf_pts] + [p.to(dev) for p, _ in (obj_legs or [])] + [vol_pts.to(dev)]
        rest_pts = torch.cat(parts)
        rest_sdf = eng.sdf_eval(rest_pts)
        bounds_ix = np.cumsum([0] + [int(p.shape[0]) for p in parts])

        # metrics: one isdf_region_metrics call per leg into one records tensor, one copy back
        vol = self._gt_volume()
        n_obj = len(obj_legs or [])
        records = torch.empty(3 + n_obj, 2, _ffi.REGION_RECORD, dtype=torch.float64, device=dev)
        eng.region_metrics(vis_pts, vis_sdf, volume=vol, sdf_grad=vis_grad, flags=torch.from_numpy(vis_flags), delta=0.01,
                           out=records[0])
        eng.region_metrics(surf_pts, rest_sdf[:R], volume=vol, flags=torch.from_numpy(surf_flags), out=records[1])
        selected = [[int((vis_flags & 1).sum()), int(((vis_flags >> 1) & 1).sum())],
                    [int((surf_flags & 1).sum()), int(((surf_flags >> 1) & 1).sum())]]
        for k, (p, fl) in enumerate(obj_legs or []):
            a, b = bounds_ix[1 + k], bounds_ix[2 + k]
            eng.region_metrics(rest_pts[a:b], rest_sdf[a:b], volume=vol, flags=fl, out=records[2 + k])
            selected.append([int(p.shape[0]), int(((fl.numpy() >> 1) & 1).sum())])
        eng.region_metrics(rest_pts[bounds_ix[-2]:], rest_sdf[bounds_ix[-2]:], gt=vol_gt, out=records[2 + n_obj])
        host = records.cpu().numpy()                                             # host synchronisation 2 of 2

        n_out = int(sum(sel[j] - host[k, j, 0] for k, sel in enumerate(selected) for j in (0, 1)))
        if n_out:
            warnings.warn("eval_fixed(t=%s): the mask files select %d points outside the ground-truth grid; they are left out "
                          "(the reference averages its 1e99 fill value into the result)" % (t_str, n_out))
        res = {"time": t}
        res["rays"] = {"vis": metrics.RegionMetrics(host[0, 0]).as_dict(cossim=True),
                       "vox": metrics.RegionMetrics(host[0, 1]).as_dict(cossim=True)}
        res["visible_surf"] = {"vis": metrics.RegionMetrics(host[1, 0]).as_dict(),
                               "vox": metrics.RegionMetrics(host[1, 1]).as_dict()}
        if obj_legs is not None:
            res["objects"] = [{"vis": {"av_l1": metrics.RegionMetrics(host[2 + k, 0]).sdf.av_l1},
                               "vox": {"av_l1": metrics.RegionMetrics(host[2 + k, 1]).sdf.av_l1}} for k in range(n_obj)]
        res["vol"] = metrics.RegionMetrics(host[2 + n_obj, 0]).as_dict()
        return res

    # ------------------------------------------------------------------ SDF slices (trainer.py:1446-1481,1558-1815)
    def _slice_colormap(self, mappable):
        """the reference's ScalarMappable as an isdf_amd.slices.Colormap, made (and uploaded) once per distinct table"""
        from .slices import Colormap
        hip = self._hip
        cm = Colormap.from_scalar_mappable(mappable)
        cache = getattr(hip, "slice_cmaps", None)
        if cache is None:
            cache = hip.slice_cmaps = {}
        return cache.setdefault(cm.key(), cm)

    @staticmethod
    def _to_host(*tensors):
        """device tensors of any dtype -> numpy arrays, through ONE copy (None stays None)"""
        order = sorted((k for k, t in enumerate(tensors) if t is not None), key=lambda k: -tensors[k].element_size())
        out = [None] * len(tensors)
        if not order:
            return out
        # widest elements first: every array then starts at a multiple of its element size
        flat = torch.cat([tensors[k].contiguous().reshape(-1).view(torch.uint8) for k in order]).cpu().numpy()
        off = 0
        for k in order:
            t = tensors[k]
            nb = t.numel() * t.element_size()
            dt = np.dtype(str(t.dtype).replace("torch.", ""))
            out[k] = flat[off:off + nb].view(dt).reshape(tuple(t.shape))
            off += nb
        return out

    def compute_slices(self, z_ixs=None, n_slices=6, include_gt=False, include_diff=False, include_chomp=False,
                       draw_cams=False, sdf_range=[-2, 2]):
        """The reference's dict of lists of uint8 images (pred_sdf, and gt_sdf / pred_cost / gt_cost / diff where asked for;
        trainer.py:1558-1707).  The slices are selected from grid_pc on the device as the reference selects them; ONE forward
        launch over all of them and ONE isdf_slice_images pass give the colours of the prediction and of the ground truth (the
        device copy of gt_sdf_interp's grid, fill 0 outside it) and both CHOMP cost fields; one copy to the host.  The colour map
        is the reference module's own sdf_util.get_colormap (which edits `sdf_range` in place, as there); cv2.resize,
        imgviz.depth2rgb and the camera markers are the reference module's own calls on the host.  `diff` is the all-white image
        the reference returns (it discards the difference it computes, trainer.py:1647-1671): nothing is computed for it."""
        from . import slices as sl
        ref = self._hip.ref_module
        if ref is None or not hasattr(ref, "sdf_util"):
            raise _ffi.IsdfError("compute_slices needs the reference's trainer module (sdf_util.get_colormap, cv2, imgviz)")
        if z_ixs is None:
            z_ixs = torch.linspace(30, self.grid_dim - 30, n_slices)
            z_ixs = torch.round(z_ixs).long()
        z_ixs = z_ixs.to(self.device)
        pc = self.grid_pc.reshape(self.grid_dim, self.grid_dim, self.grid_dim, 3)
        pc = torch.index_select(pc, self.up_ix, z_ixs)
        if not self.up_aligned:
            indices = np.arange(len(z_ixs))[::-1]
            indices = torch.from_numpy(indices.copy()).to(self.device)
            pc = torch.index_select(pc, self.up_ix, indices)
        cmap = self._slice_colormap(ref.sdf_util.get_colormap(sdf_range=sdf_range))
        grid_shape = tuple(pc.shape[:-1])
        n_slices = grid_shape[self.up_ix]
        scales = torch.cat([self.scene_scale[:self.up_ix], self.scene_scale[self.up_ix + 1:]])
        im_size = 256 * scales / scales.min()
        im_size = im_size.int().cpu().numpy()

        res = sl.slice_images(self.engine, pc, cmap, gt_volume=self._gt_volume() if include_gt else None,
                              chomp_eps=2. if include_chomp else None, oob_fill=0.)
        pred_rgb, gt_rgb, pred_cost, gt_cost = self._to_host(res.pred_rgb, res.gt_rgb, res.pred_cost, res.gt_cost)

        def resized(viz):
            return [ref.cv2.resize(np.take(viz, i, self.up_ix), im_size[::-1]) for i in range(n_slices)]

        def cost_images(cost):
            viz = ref.imgviz.depth2rgb(cost.reshape(self.grid_dim, -1), min_value=0., max_value=1.5)
            return resized(viz.reshape(*grid_shape, 3))
        slices = {"pred_sdf": resized(pred_rgb)}
        if include_chomp:
            slices["pred_cost"] = cost_images(pred_cost)
        if include_gt:
            slices["gt_sdf"] = resized(gt_rgb)
            if include_chomp:
                slices["gt_cost"] = cost_images(gt_cost.astype(np.float64))      # the reference's ground truth is float64
        if include_diff:
            if not include_gt:       # the reference reads its gt_sdf here, which only include_gt assigns (trainer.py:1643)
                raise UnboundLocalError("local variable 'gt_sdf' referenced before assignment")
            slices["diff"] = resized(np.full(grid_shape + (3,), 255, dtype=np.uint8))

        if draw_cams:       # the reference's markers (trainer.py:1673-1705), its own draw / cv2 calls
            cam_xyz = self.frames.T_WC_batch[:, :3, 3].cpu()
            cam_td = self.to_topdown(cam_xyz, im_size)
            cam_rots = self.frames.T_WC_batch[:, :3, :3].cpu().numpy()
            angs = [np.arctan2(rot[0, 2], rot[0, 0]) for rot in cam_rots]
            for i, im in enumerate(slices["pred_sdf"]):
                if self.incremental:
                    trajectory_gt = self.frames.T_WC_batch_np[:, :3, 3]
                    if self.frames.T_WC_gt is not None:
                        trajectory_gt = self.frames.T_WC_gt[:, :3, 3]
                    traj_td = self.to_topdown(trajectory_gt, im_size)
                    for j in range(len(traj_td) - 1):
                        if not (traj_td[j] == traj_td[j + 1]).all():
                            im = im.astype(np.uint8) / 255
                            im = ref.cv2.line(im, traj_td[j][::-1], traj_td[j + 1][::-1], [1., 0., 0.], 2)
                            im = (im * 255).astype(np.uint8)
                for (p, ang) in zip(cam_td, angs):
                    ref.draw.draw_agent(im, p, agent_rotation=ang, agent_radius_px=12)
                slices["pred_sdf"][i] = im
        return slices

    def obj_slices_vis(self, n_slices=6):
        """The reference's stacked image (per object the predicted slices over the ground-truth ones), or None without an
        obj_bounds_file (trainer.py:1775-1815): per object the reference's own 256 x n_slices x 256 points, one forward launch
        and one isdf_slice_images pass (colours of both, map [-0.5, 0.5]); the two images come back in one copy."""
        from . import slices as sl
        if self.obj_bounds_file is None:
            return None
        ref = self._hip.ref_module
        if ref is None or not hasattr(ref, "sdf_util"):
            raise _ffi.IsdfError("obj_slices_vis needs the reference's trainer module (sdf_util.get_colormap, metrics)")
        up_ix = 1
        obj_bounds = ref.metrics.get_obj_eval_bounds(self.obj_bounds_file, up_ix)
        cmap = self._slice_colormap(ref.sdf_util.get_colormap(sdf_range=[-0.5, 0.5]))
        vol = self._gt_volume()
        all_slices = []
        for bounds in obj_bounds:
            dims = [256, 256, 256]
            dims[up_ix] = n_slices
            x = torch.linspace(bounds[0, 0], bounds[1, 0], dims[0])
            y = torch.linspace(bounds[0, 1], bounds[1, 1], dims[1])
            z = torch.linspace(bounds[0, 2], bounds[1, 2], dims[2])
            xx, yy, zz = torch.meshgrid(x, y, z, indexing="ij")
            pc = torch.cat((xx[..., None], yy[..., None], zz[..., None]), dim=3).to(self.device)
            res = sl.slice_images(self.engine, pc, cmap, gt_volume=vol, oob_fill=0.)
            col, gt_col = self._to_host(res.pred_rgb, res.gt_rgb)
            col = np.hstack([col[:, i] for i in range(n_slices)])
            gt_col = np.hstack([gt_col[:, i] for i in range(n_slices)])
            all_slices.append(np.vstack((col, gt_col)))
        return np.vstack((all_slices))

    def get_sdf_grid_pc(self, include_gt=False, mask_near_pc=False):
        """(sdf_grid_pc, keep_mask) of the reference (trainer.py:1446-1481): grid_pc with the network's value as a float32
        [d, d, d, 4] array -- with include_gt (and a ground-truth grid) float64 [d, d, d, 5], the last column the ground truth with
        0 outside its volume, from the device lookup --, and with mask_near_pc the boolean [.., .., ..] mask of the grid points
        whose every-tenth representative lies within crop_dist of the keyframes' point cloud (Engine.nn_distance instead of a
        host KD-tree), repeated as the reference repeats it; else None.  One forward launch, one copy to the host."""
        d = self.grid_dim
        sdf_grid = self.get_sdf_grid()
        grid_pc = self.grid_pc.reshape(d, d, d, 3)
        sdf_grid_pc = torch.cat((grid_pc, sdf_grid[..., None]), dim=-1)
        with_gt = include_gt and self.gt_sdf_interp is not None
        if with_gt:
            gt = self.engine.slice_images(self.grid_pc, None, None, self._gt_volume(), None, oob_fill=0.)[1]
            sdf_grid_pc = torch.cat((sdf_grid_pc, gt.view(d, d, d, 1)), dim=-1)
            self.gt_sdf_interp.fill_value = 0.0           # the state the reference leaves its interpolator in (trainer.py:1454-1461)
            self.gt_sdf_interp.bounds_error = True
        near = None
        if mask_near_pc:
            pc = np.ascontiguousarray(self._vis_pointcloud(), dtype=np.float32)
            sparse = sdf_grid_pc[::10, ::10, ::10, :3]
            dist, _, _ = self.engine.nn_distance(sparse.reshape(-1, 3), torch.from_numpy(pc).reshape(-1, 3).to(self.device))
            near = (dist.double() < self.crop_dist).view(sparse.shape[:-1])
        sdf_grid_pc, keep_mask = self._to_host(sdf_grid_pc.detach(), near)
        if with_gt:
            sdf_grid_pc = sdf_grid_pc.astype(np.float64)
        if keep_mask is not None:
            keep_mask = keep_mask.repeat(10, axis=0).repeat(10, axis=1).repeat(10, axis=2)
        return sdf_grid_pc, keep_mask

    # ------------------------------------------------------------------ data parallel
    def check_keyframe_latest(self):
        """The reference's decision logic (trainer.py:622-650) runs unchanged; under data parallelism rank 0's
        outcome is broadcast so the keyframe sets (and with them the all-reduce message size) cannot diverge."""
        add_new_frame = super().check_keyframe_latest()
        hip = self._hip
        if hip.dist_group is not None:
            v = dp.broadcast_floats([float(add_new_frame), float(self.last_is_keyframe), float(self.optim_frames),
                                     -1.0 if self.noise_std is None else float(self.noise_std)], hip.dist_group, hip.device)
            add_new_frame, self.last_is_keyframe, self.optim_frames = bool(v[0]), bool(v[1]), int(v[2])
            self.noise_std = None if v[3] < 0 else v[3]
        return add_new_frame

    def add_frame(self, frame_data):
        """New frame: under data parallelism rank 0's depth / pose / normals are broadcast once per FRAME
        (1.2-3.3 MB depth + 3.7-9.8 MB normals), then the reference's add_frame runs."""
        hip = self._hip
        if hip.dist_group is not None:
            for k in ("depth_batch", "T_WC_batch", "normal_batch"):
                t = getattr(frame_data, k, None)
                if torch.is_tensor(t):
                    torch.distributed.broadcast(t, dp.src_rank(hip.dist_group), group=hip.dist_group)
        return super().add_frame(frame_data)

    # ------------------------------------------------------------------ checkpoint / resume
    def hip_state_dict(self):
        """Everything needed for a true resume.  The reference saves only model + optimiser
        (train.py:207-219) and restores only the model (trainer.py:441-444); keyframes, RNG
        position, the frozen keyframe-test network and the virtual clock are lost there."""
        fr, hip = self.frames, self._hip
        frozen = getattr(self, "frozen_sdf_map", None)
        return {
            "model_state_dict": {k: v.detach().clone() for k, v in self.sdf_map.state_dict().items()},
            "optimizer_state_dict": self.optimiser.state_dict(),
            "frozen_state_dict": None if frozen is None else {k: v.detach().clone() for k, v in frozen.state_dict().items()},
            # EVERY field of the keyframe store (data_util.py:11-43): the device batches the hot path reads AND the host
            # twins / tracked / ground-truth poses / frame count the reference's visualisation and evaluation index
            # (trainer.py:1021-1067,1152-1157,1228-1231) -- a resumed run appends to all of them consistently
            "frames": {k: (None if getattr(fr, k, None) is None else
                           (getattr(fr, k).copy() if isinstance(getattr(fr, k), np.ndarray) else
                            (getattr(fr, k).clone() if torch.is_tensor(getattr(fr, k)) else copy.deepcopy(getattr(fr, k)))))
                       for k in FRAME_FIELDS if hasattr(fr, k)},
            "clock": dict(tot_step_time=self.tot_step_time, steps_since_frame=self.steps_since_frame,
                          last_is_keyframe=self.last_is_keyframe, optim_frames=self.optim_frames,
                          noise_std=self.noise_std, step_count=hip.step_count,
                          prev_step_ms=hip.prev_step_ms),     # data parallel: the step time still to be added to the clock
            "rng": dict(draw_count=hip.draw_count, noise_count=hip.noise_count, seed=hip.seed,
                        window=getattr(hip, "window_rng_state", None),
                        numpy=np.random.get_state(), torch=torch.get_rng_state(),
                        torch_cuda=torch.cuda.get_rng_state(hip.device) if hip.device.type == "cuda" else None),
        }

    def load_hip_state_dict(self, sd):
        hip = self._hip
        self.sdf_map.load_state_dict(sd["model_state_dict"])
        self.optimiser.load_state_dict(sd["optimizer_state_dict"])
        if sd.get("frozen_state_dict") is not None:
            self.frozen_sdf_map = copy.deepcopy(self.sdf_map)
            self.frozen_sdf_map.load_state_dict(sd["frozen_state_dict"])
        f = sd["frames"]
        fr = type(self.frames)()
        for k, v in f.items():
            setattr(fr, k, v)
        # checkpoints written before the host twins were saved: rebuild them from the device batches so that the next
        # add_frame_data appends at the right length
        for twin, src in (("im_batch_np", "im_batch"), ("depth_batch_np", "depth_batch"), ("T_WC_batch_np", "T_WC_batch")):
            if twin not in f and getattr(fr, src, None) is not None and hasattr(fr, twin):
                t = getattr(fr, src).detach()
                if twin == "im_batch_np":     # the host twin is the raw 0..255 image, the device batch is float in [0, 1]
                    t = (t * 255).round().to(torch.uint8)          # (trainer.py:536-547)
                setattr(fr, twin, t.cpu().numpy())
        fal = getattr(fr, "frame_avg_losses", None)
        if fal is not None and fal.device.type == "cpu" and hip.device.type == "cuda" and not fal.is_pinned():
            fr.frame_avg_losses = fal.pin_memory()      # the ring store keeps them in pinned host memory (frame_store.py)
        self.frames = fr
        c = sd["clock"]
        self.tot_step_time, self.steps_since_frame = c["tot_step_time"], c["steps_since_frame"]
        self.last_is_keyframe, self.optim_frames = c["last_is_keyframe"], c["optim_frames"]
        self.noise_std, hip.step_count = c["noise_std"], c["step_count"]
        hip.prev_step_ms = float(c.get("prev_step_ms", 0.0))
        r = sd["rng"]
        hip.draw_count, hip.noise_count, hip.seed = r["draw_count"], r["noise_count"], r["seed"]
        hip.idx_cache = None
        if r.get("window") is not None:
            hip.window_rng_state = r["window"]
        np.random.set_state(r["numpy"]); torch.set_rng_state(r["torch"])
        if r.get("torch_cuda") is not None:
            torch.cuda.set_rng_state(r["torch_cuda"], hip.device)


# data_util.FrameData's fields (isdf/datasets/data_util.py:11-43) incl. the reference's frame counter
FRAME_FIELDS = ("frame_id", "im_batch", "im_batch_np", "depth_batch", "depth_batch_np", "T_WC_batch", "T_WC_batch_np",
                "normal_batch", "frame_avg_losses", "T_WC_track", "T_WC_gt", "count")

ENGINE_FACTORY = None      # host-logic tests on GPU-less machines install an oracle-backed stand-in here; never set by the product


UNSUPPORTED_HINT = ("isdf_amd hot path: %s (the reference's own Python path is the CPU / fallback path; "
                    "this build ships no second implementation)")


def unsupported_reason(trainer):
    """None, or why the kernels cannot take this trainer's CONFIGURATION (such configs keep running on the reference's
    own Python path -- `can_graft` says no, nothing raises): `bounds_method="normal"` (loss.py:29), `do_active` (trainer.py:718), a
    loss_type other than L1 / L2 (loss.py:104), a network shape the tile kernels are not instantiated for (`isdf_check_net`)."""
    if getattr(trainer, "bounds_method", "ray") not in ("ray", "pc"):
        return "bounds_method %r (only 'ray' and 'pc' can run upstream, loss.py:29)" % (trainer.bounds_method,)
    if getattr(trainer, "do_active", False):
        return "active sampling (rejected by the reference itself, trainer.py:718)"
    if getattr(trainer, "loss_type", "L1") not in ("L1", "L2"):
        return "loss_type %r (loss.py:104)" % (trainer.loss_type,)
    net = getattr(trainer, "sdf_map", None)
    if net is not None and not isinstance(net, SDFMapHIP) and ENGINE_FACTORY is None and os.path.exists(_ffi.LIB_PATH):
        try:
            pe = net.positional_encoding
            c = NetConfig(hidden=net.out_alpha.in_features, blocks=len(net.mid1), n_freqs=int(pe.n_freqs)).to_c()
        except AttributeError:
            return "trainer.sdf_map is not an isdf.modules.fc_map.SDFMap"
        rc = _ffi.lib().isdf_check_net(ctypes.byref(c))
        if rc != 0:
            return "network shape (hidden %d, %d blocks, %d octaves): %s" % (c.hidden, c.blocks, c.n_freqs,
                                                                              _ffi.lib().isdf_error_string(int(rc)).decode())
    return None


def can_graft(trainer):
    """True when `graft(trainer)` can bind the kernels: the trainer sits on a HIP device, libisdf_hip.so is built and the
    configuration is one the kernels take (`unsupported_reason`).  The guard INTEGRATION.md puts in front of graft(): wherever it says
    no -- a CPU-only host (BASELINE configs[0]), `bounds_method="normal"`, `do_active`, an uninstantiated network shape -- the
    reference's own Python path keeps running; this package ships no second implementation, and graft() itself raises there."""
    if unsupported_reason(trainer) is not None:
        return False
    if ENGINE_FACTORY is not None:          # host-logic tests with a stand-in engine
        return True
    return torch.device(trainer.device).type == "cuda" and torch.cuda.is_available() and os.path.exists(_ffi.LIB_PATH)


def graft(trainer, rng="philox", seed=1, dist_group=None, fix_normal_window=False, fwd_operand="fp16x2",
          fuse_optimiser=True, virtual_step_ms=None, engine_factory=None, overlap_allreduce=False, bwd_operand=None, spill_operand=None, migrate_frames=True):
    """Re-bind the hot path of `trainer` (an `isdf.modules.trainer.Trainer` or a `StandinTrainer`) to the HIP
    kernels, IN PLACE, and return it.

    rng: "philox" (in-kernel draws, no host sync inside step) or "torch" (draw with torch in the reference's
         order, shapes and devices: parity mode, one host sync per step like the reference).
    dist_group: torch.distributed process group for ray-sharded data parallelism (one all-reduce per step);
         weights are broadcast from rank 0 here so every rank starts from the same network.
    virtual_step_ms: if set, the virtual clock advances by this much per step instead of the measured step time
         (the frame schedule is a function of measured time, trainer.py:100-101,1011-1013; pin it to compare runs).
    bwd_operand: "fp16" | "bf16" | None (default for the forward mode): operand / spill type of the second-order sweeps and dW.
    spill_operand: None (auto) | "16bit" | "e4m3" | "e4m3_gb": storage of the spilled P / GB tensors (engine.NetConfig.spill_operand;
         "e4m3_gb": GB in e4m3, P in 16 bits; the e4m3 formats need hidden <= 256 and fp16 second-order sweeps).
    overlap_allreduce: data parallel only -- the closing reduction in two launches and the all-reduce in two parts, the first
         one on a side stream beside the second launch (dp.allreduce_split_); two collectives per step instead of one.
    migrate_frames: replace `trainer.frames` (the reference's FrameData: one torch.cat of the whole keyframe set per frame,
         data_util.py:84-102) by an `isdf_amd.frame_store.FrameData` holding the same keyframes (False: keep the caller's store).
    engine_factory: tests only (a stand-in engine for hosts without a GPU)."""
    if isinstance(trainer, HotPath) and getattr(trainer, "_hip", None) is not None:
        return trainer
    if engine_factory is None:
        engine_factory = ENGINE_FACTORY
    dev = torch.device(trainer.device)
    if dev.type == "cuda" and dev.index is None and torch.cuda.is_available():
        # "cuda" names the current device; tensors on it report "cuda:N", and `frames.frame_avg_losses.device == hip.device` decides
        # whether the step's closing launch writes the keyframe losses in place (else: a separate launch and a blocking index_put)
        dev = torch.device("cuda", torch.cuda.current_device())
    if engine_factory is None and dev.type != "cuda":
        raise _ffi.IsdfError(UNSUPPORTED_HINT % ("device %r is not a HIP device" % (trainer.device,)))
    why = unsupported_reason(trainer)
    if why is not None:                # (can_graft() is the non-raising form: the reference's path then stays in place)
        raise _ffi.IsdfError(UNSUPPORTED_HINT % why)
    if rng not in ("philox", "torch"):
        raise ValueError("rng must be 'philox' or 'torch'")

    old = getattr(trainer, "sdf_map", None)
    if old is not None and not isinstance(old, SDFMapHIP):
        pe_old = old.positional_encoding
        pe = PositionalEncodingHIP(min_deg=pe_old.min_deg, max_deg=pe_old.max_deg, scale=pe_old.scale,
                                   transform=pe_old.transform)
        n_block = len(old.mid1)
        hidden = old.out_alpha.in_features
        with torch.random.fork_rng(devices=[]):    # grafting mid-run must not advance the caller's generator: the initial
            new = SDFMapHIP(pe, hidden_size=hidden, hidden_layers_block=n_block, scale_output=old.scale_output,   # weights
                            device=dev, fwd_operand=fwd_operand, engine_factory=engine_factory,    # are overwritten below
                            bwd_operand=bwd_operand, spill_operand=spill_operand)
        new.load_state_dict({k: v.detach() for k, v in old.state_dict().items()})
        new.train(old.training)
        trainer.sdf_map = new
        og = trainer.optimiser.param_groups[0]
        old_state = trainer.optimiser.state_dict()
        trainer.optimiser = FlatAdamW(new, lr=og["lr"], weight_decay=og["weight_decay"], betas=tuple(og["betas"]),
                                      eps=og["eps"])
        if old_state.get("state"):     # a trainer that has already stepped (or loaded optimiser state): keep exp_avg /
            trainer.optimiser.load_state_dict(old_state)    # exp_avg_sq / step; parameter order = named_parameters() order
        if getattr(trainer, "frozen_sdf_map", None) is not None:
            fz = copy.deepcopy(new)
            fz.load_state_dict({k: v.detach() for k, v in trainer.frozen_sdf_map.state_dict().items()})
            trainer.frozen_sdf_map = fz
    elif old is None:
        raise ValueError("graft() needs a trainer whose load_networks() has run")

    hip = types.SimpleNamespace(rng=rng, seed=int(seed), dist_group=dist_group, fix_normal_window=bool(fix_normal_window),
                                fuse_optimiser=bool(fuse_optimiser), device=dev, draw_count=0, noise_count=0,
                                step_count=0, idx_cache=None, timing_events=None, prof_events=None,
                                inline_window=True,      # bench.py flips it for the A/B of the window's transport
                                overlap_allreduce=bool(overlap_allreduce) and dist_group is not None, split_event=None,
                                comm_stream=None,
                                virtual_step_ms=None if virtual_step_ms is None else float(virtual_step_ms),
                                loss_host=torch.zeros(8, dtype=torch.float32,
                                                      pin_memory=(dev.type == "cuda")))
    # the module whose two geometry functions get_data() redirects: `geometry.transform` as the reference's trainer module sees it
    geo = getattr(getattr(sys.modules.get(trainer.__class__.__module__), "geometry", None), "transform", None)
    hip.geometry_transform = geo if (geo is not None and hasattr(geo, "pointcloud_from_depth_torch")
                                     and hasattr(geo, "estimate_pointcloud_normals")) else None
    hip.ingest_launches = 0
    # the module whose trimesh / KDTree / draw3D / geometry the bound mesh_rec uses: the trainer class's own module
    hip.ref_module = sys.modules.get(trainer.__class__.__module__)
    if migrate_frames and getattr(trainer, "frames", None) is not None and not isinstance(trainer.frames, frame_store.FrameData):
        trainer.frames = frame_store.FrameData.from_reference(trainer.frames)     # same fields, the existing keyframes carried over
    trainer._hip = hip
    base = trainer.__class__
    if not issubclass(base, HotPath):
        trainer.__class__ = type("Hip" + base.__name__, (HotPath, base), {"__module__": HotPath.__module__})
    hip.clock_slots, hip.prev_step_ms, hip.rank, hip.rccl, hip.collective = 0, 0.0, 0, None, None
    if dist_group is not None:                           # replicated weights / moments
        eng = trainer.sdf_map.engine
        for t in (eng.params, eng.exp_avg, eng.exp_avg_sq):
            torch.distributed.broadcast(t, dp.src_rank(dist_group), group=dist_group)
        eng.pack()
        hip.rank, hip.world = torch.distributed.get_rank(dist_group), torch.distributed.get_world_size(dist_group)
        hip.window_rng_state = np.random.RandomState(hip.seed + 104729).get_state()   # replicated select_keyframes stream
        if hip.virtual_step_ms is None:                  # per-rank step-time slots in the tail of the all-reduce message
            hip.clock_slots = eng.reduce_extra = hip.world
        if hasattr(eng, "allreduce_direct") and hip.device.type == "cuda":      # (the CPU tests' stand-in engine has no C library behind it)
            from .engine import _stream
            hip.rccl = dp.rccl_agree(eng.lib, dp.rccl_direct(dist_group, hip.device), dist_group, hip.device, _stream(hip.device))
        hip.collective = "rccl on the step's stream (isdf_allreduce_sum_f32)" if hip.rccl is not None else "torch.distributed.all_reduce"
    return trainer
