"""Tensor-level host API over the C ABI (include/isdf_hip.h).

`Engine` owns the torch-allocated device buffers the kernels borrow -- one flat
fp32 parameter buffer (+ AdamW moments), the packed 16-bit MFMA-operand copies,
the step workspace and the flat reduction buffer -- and exposes the four
kernel groups: sampler, fused inference, training step, AdamW.  torch is used
for memory and streams only; every numeric operation on the hot path runs in
the HIP kernels.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from . import _ffi

N_DIRS = 21
FWD_OPERANDS = ("bf16", "fp16", "fp16x2", "fp16x2_full")   # isdf_net_cfg.fwd_operand = index
ADAMW_LR, ADAMW_WEIGHT_DECAY, ADAMW_BETAS, ADAMW_EPS = 0.0013, 0.012, (0.9, 0.999), 1e-8   # what an `optim` dict leaves out


@dataclass
class NetConfig:
    """SDFMap + PostionalEncoding hyper-parameters (replicaCAD.json `model`)."""
    hidden: int = 256            # model.hidden_feature_size
    blocks: int = 2              # model.hidden_layers_block
    n_freqs: int = 6             # model.embedding.n_embed_funcs + 1 (embedding.py:36)
    scale_input: float = 0.05937489
    scale_output: float = 0.14
    transform: Optional[np.ndarray] = None   # 4x4 inv_bounds_transform or None
    # MFMA operand type of the forward / first-backward GEMMs (include/isdf_hip.h `fwd_operand`):
    #   "fp16x2" (default) fp16 with the compensated forward of layers >= cat -- sdf within 1e-3 of the reference
    #   "fp16"   plain fp16 operands (fast mode: sdf 0.9e-3 .. 1.5e-3 at BASELINE size);  "bf16" plain bf16 (1.1e-2)
    #   "fp16x2_full"  every forward layer compensated (exact-forward instrument: sdf ~1e-6, d sdf/dx < 1e-3 of the reference;
    #            hidden 256 / n_freqs <= 6 nets only, one workgroup per CU: slower)
    fwd_operand: str = "fp16x2"
    # MFMA operand / spill type of the second-order sweeps and the dW contraction (include/isdf_hip.h `bwd_operand`):
    #   "fp16" (default with an fp16-family forward) or "bf16" (range-safe for any loss-adjoint magnitude; the only choice with
    #   fwd_operand "bf16").  None = the default for the forward mode.
    bwd_operand: Optional[str] = None
    # storage of the spilled P / GB tensors (include/isdf_hip.h `spill_operand`): None = auto (e4m3 bytes when n_freqs <= 6 with fp16
    # second-order sweeps, i.e. replicaCAD.json / scanNet.json; 16-bit otherwise), "16bit", "e4m3" (forced) or "e4m3_gb" (GB only)
    spill_operand: Optional[str] = None

    @property
    def emb(self):
        return 2 * N_DIRS * self.n_freqs + 3

    def layer_names(self):
        B = self.blocks
        return (["in_layer.0"] + ["mid1.%d.0" % i for i in range(B)] + ["cat_layer.0"]
                + ["mid2.%d.0" % i for i in range(B)])

    def param_shapes(self):
        """[(state_dict key, shape)] in the reference's named_parameters() order."""
        H, E, B = self.hidden, self.emb, self.blocks
        fan_in = [E] + [H] * B + [H + E] + [H] * B
        out = []
        for n, k in zip(self.layer_names(), fan_in):
            out += [(n + ".weight", (H, k)), (n + ".bias", (H,))]
        out += [("out_alpha.weight", (1, H)), ("out_alpha.bias", (1,))]
        return out

    def to_c(self):
        c = _ffi.NetCfg()
        c.hidden, c.blocks, c.n_freqs = self.hidden, self.blocks, self.n_freqs
        c.has_transform = 0 if self.transform is None else 1
        c.scale_input, c.scale_output = self.scale_input, self.scale_output
        T = np.eye(4, dtype=np.float32) if self.transform is None else np.asarray(self.transform, np.float32)
        for i in range(12):
            c.bounds_T[i] = float(T[i // 4, i % 4])
        if self.fwd_operand not in FWD_OPERANDS:
            raise ValueError("fwd_operand must be one of %s" % (FWD_OPERANDS,))
        c.fwd_operand = FWD_OPERANDS.index(self.fwd_operand)
        bwd = self.bwd_operand or ("bf16" if self.fwd_operand == "bf16" else "fp16")
        if bwd not in ("bf16", "fp16") or (bwd == "fp16" and self.fwd_operand == "bf16"):
            raise ValueError("bwd_operand must be 'bf16' or 'fp16' (fp16 needs an fp16-family fwd_operand)")
        c.bwd_operand = 1 if bwd == "fp16" else 0
        if self.spill_operand not in (None, "auto", "16bit", "e4m3", "e4m3_gb"):
            raise ValueError("spill_operand must be None / 'auto', '16bit', 'e4m3' or 'e4m3_gb'")
        c.spill_operand = {None: 0, "auto": 0, "16bit": 1, "e4m3": 2, "e4m3_gb": 3}[self.spill_operand]
        return c


@dataclass
class LossConfig:
    """replicaCAD.json `loss` block (trainer.py:301-318)."""
    bounds_method: str = "ray"
    loss_type: str = "L1"
    trunc_weight: float = 5.38344020
    trunc_distance: float = 0.29365022
    eik_weight: float = 0.268
    eik_apply_dist: float = 0.1
    grad_weight: float = 0.018
    orien_loss: bool = False

    def to_c(self):
        if self.bounds_method not in ("ray", "pc"):
            # "normal" cannot run in the reference either (loss.py:29 calls bounds_ray with 3 of 5 args)
            raise ValueError("bounds_method must be 'ray' or 'pc'")
        if self.loss_type not in ("L1", "L2"):
            raise ValueError("Must be L1 or L2")
        c = _ffi.LossCfg()
        c.bounds_method = 0 if self.bounds_method == "ray" else 1
        c.loss_type = 0 if self.loss_type == "L1" else 1
        c.trunc_weight, c.trunc_distance = self.trunc_weight, self.trunc_distance
        c.eik_weight, c.eik_apply_dist = self.eik_weight, self.eik_apply_dist
        c.grad_weight, c.orien_loss = self.grad_weight, int(self.orien_loss)
        return c


@dataclass
class SampleConfig:
    """replicaCAD.json `sample` block + camera."""
    n_rays: int = 200
    n_strat: int = 19
    n_surf: int = 8
    min_depth: float = 0.07
    dist_behind_surf: float = 0.1
    H: int = 680
    W: int = 1200
    fx: float = 600.0
    fy: float = 600.0
    cx: float = 599.5
    cy: float = 339.5

    @property
    def S(self):
        return self.n_strat + self.n_surf


_PINNED = {}      # device index -> (torch.cuda.Stream, c_void_p) while a caller has pinned that device's launch stream


def _stream(device=None):
    """hipStream_t of torch's current stream ON `device` (an Engine passes its own device: a trainer on cuda:1 must not
    launch on cuda:0's stream because that happens to be the current device).  `torch.cuda.current_stream()` costs ~5 us
    of host time per call, which sits in front of every launch of a device-synchronised step: `pinned_stream()` looks it
    up once per step instead."""
    idx = torch.cuda.current_device() if device is None or device.index is None else device.index
    p = _PINNED.get(idx)
    if p is not None:
        return p[1]
    return C.c_void_p(torch.cuda.current_stream(idx).cuda_stream)


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)     # hipStream_t of a device's current stream as an int, ~0.2 us
_STREAM_OBJ = {}  # device index -> (torch.cuda.Stream, c_void_p, raw handle): torch.cuda.current_stream() builds a new object per call (~3 us)


class pinned_stream:
    """with pinned_stream(device) as st: every Engine call on that device inside launches on `st` (torch's current
    stream of the device at entry).  Keyed per device, so trainers on different devices do not overwrite each other.
    The Stream object is cached per device and re-used while the device's current RAW stream is the one it wraps
    (a caller's `torch.cuda.stream(...)` context changes the raw handle and is honoured)."""

    def __init__(self, device=None):
        if isinstance(device, int):
            self.idx = device
        else:
            self.idx = torch.cuda.current_device() if device is None or torch.device(device).index is None else torch.device(device).index

    def __enter__(self):
        self.prev = _PINNED.get(self.idx)
        c = _STREAM_OBJ.get(self.idx)
        if c is None or _RAW_STREAM is None or _RAW_STREAM(self.idx) != c[2]:
            st = torch.cuda.current_stream(self.idx)
            c = _STREAM_OBJ[self.idx] = (st, C.c_void_p(st.cuda_stream), st.cuda_stream)
        _PINNED[self.idx] = c
        return c[0]

    def __exit__(self, *exc):
        if self.prev is None:
            _PINNED.pop(self.idx, None)
        else:
            _PINNED[self.idx] = self.prev


def to_host(*tensors):
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


def host_array(x, dtype=None):
    """a tensor (of any device) or array-like as a numpy array on the host, of `dtype` if one is given"""
    return np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=dtype)


def _addr(t):
    """the address of a tensor, NULL for an absent or an empty one: an empty tensor has none to hand over, and the call reads or
    writes nothing of it then"""
    return t.data_ptr() if t is not None and t.numel() else None


def morton_codes(p):
    """int64 [n]: the 30-bit Morton code of every point of `p` [n,3] on a 1024^3 grid over the box of the finite points; 2^30 for a
    point with a non-finite coordinate, so that a sort puts those last.  torch ops on p's device, no host synchronisation."""
    p = p.reshape(-1, 3).to(torch.float32)
    if p.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int64, device=p.device)
    finite = torch.isfinite(p).all(1)
    q = torch.where(finite[:, None], p, p.new_tensor(float("inf")))
    lo = torch.where(finite.any(), q.amin(0), p.new_zeros(3))
    q = torch.where(finite[:, None], p, lo[None, :])
    ext = (q.amax(0) - lo).clamp_min(1e-30)
    g = ((q - lo[None, :]) / ext[None, :] * 1023.0).clamp(0.0, 1023.0).to(torch.int64)
    g = (g | (g << 16)) & 0x030000FF
    g = (g | (g << 8)) & 0x0300F00F
    g = (g | (g << 4)) & 0x030C30C3
    g = (g | (g << 2)) & 0x09249249
    code = g[:, 0] | (g[:, 1] << 1) | (g[:, 2] << 2)
    return torch.where(finite, code, torch.full_like(code, 1 << 30))


def morton_order(p):
    """int32 [n]: the indices of the points of `p` [n,3] in Morton order (a stable sort of morton_codes), non-finite points last:
    runs of consecutive entries are spatially compact.  No host synchronisation."""
    return torch.sort(morton_codes(p), stable=True)[1].to(torch.int32)


class Engine:
    def __init__(self, net: NetConfig, device="cuda"):
        self.lib = _ffi.lib()
        self.net = net
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _ffi.IsdfError("isdf_amd kernels need a HIP device (got %s); there is no CPU path" % device)
        self.cnet = net.to_c()
        # fail where the network is built (trainer.py:419-439), not at the first step
        _ffi.check(self.lib.isdf_check_net(C.byref(self.cnet)),
                   "isdf_check_net(hidden=%d, blocks=%d, n_freqs=%d)" % (net.hidden, net.blocks, net.n_freqs))
        n = self.lib.isdf_param_count(C.byref(self.cnet))
        _ffi.check(min(n, 0), "isdf_param_count")
        self.n_params = int(n)
        self.params = torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        sb = self.lib.isdf_shadow_bytes(C.byref(self.cnet))
        self.shadow = torch.zeros(int(sb), dtype=torch.uint8, device=self.device)
        self._ws = None
        self._ws_key = None
        self._scan_ws = None      # sampler look-back state (zero on first use, self re-arming afterwards)
        self._scan_ptr = None     # ... and its address as the launches take it
        self._smp_ring = None     # [key, two sampler buffer sets, current slot, their two call plans] of sample(reuse=True)
        self._ws_ptr = self._params_ptr = self._shadow_ptr = None    # addresses train_step last set up for _launch_step
        self._fa_index_cache = {}     # host-side window -> its int32 device tensor (frame_avg)
        self._mesher = None       # marching-cubes workspace, count pair and output capacity (isdf_amd.mesh.Mesher)
        self._band = None         # narrow-band workspace and count table (isdf_amd.mesh.BandSelector)
        self._renderer = None     # rendered-view workspace (isdf_amd.render.Renderer)
        self._scratch_bufs = {}   # call name -> its grow-only uint8 workspace (_scratch)
        self.reduce_buf = None
        self.reduce_extra = 0
        self.reduce_floats = 0
        self.mailbox = None           # pinned host mirror of [loss sums (8) | reduced tail (reduce_extra)]
        self._step_plans = {}
        self.opt_step = 0
        self.reduce_split = int(self.lib.isdf_reduce_split_floats(C.byref(self.cnet)))   # first float of the message's early-final suffix
        self.slices = {}
        off = 0
        for k, shp in net.param_shapes():
            cnt = int(np.prod(shp))
            self.slices[k] = (off, shp)
            off += cnt
        assert off == self.n_params

    # ---- parameters ---------------------------------------------------------
    def param_view(self, key):
        off, shp = self.slices[key]
        return self.params[off:off + int(np.prod(shp))].view(*shp)

    def load_params(self, state):
        """state: dict key -> array/tensor (reference state_dict layout)."""
        for k, (off, shp) in self.slices.items():
            v = torch.as_tensor(host_array(state[k]), dtype=torch.float32).reshape(-1)
            self.params[off:off + v.numel()].copy_(v)
        self.pack()

    def pack(self):
        _ffi.check(self.lib.isdf_pack_weights(C.byref(self.cnet), _ffi.ptr(self.params),
                                              _ffi.ptr(self.shadow), _stream(self.device)), "isdf_pack_weights")

    def workspace(self, max_points, train):
        key = (int(max_points), bool(train))
        if self._ws is None or self._ws_key[0] < key[0] or (key[1] and not self._ws_key[1]):
            nb = self.lib.isdf_workspace_bytes(C.byref(self.cnet), int(max_points), int(train))
            _ffi.check(min(nb, 0), "isdf_workspace_bytes")
            self._ws = torch.empty(int(nb), dtype=torch.uint8, device=self.device)
            self._ws_key = key
        return self._ws

    # ---- K1 sampler ---------------------------------------------------------
    def sample(self, depth_batch, T_WC_batch, normal_batch, frame_idx, normal_idx, sc: SampleConfig,
               draws=None, seed=0, offset=0, want_T=False, reuse=False):
        """The sampler (one launch).  draws: dict(indices_h, indices_w, U, N_off)
        of device tensors in the reference's shapes (parity mode) or None (Philox).
        frame_idx / normal_idx: int32 device tensors [F], or -- the step loop's form -- tuples of <= 8 Python ints, which
        travel as kernel arguments (isdf_sample_args.n_inline): a window that `select_keyframes` re-draws on the host every
        step then costs no device copy and no new call plan."""
        dev = self.device
        inline = isinstance(frame_idx, (tuple, list))
        if inline and (len(frame_idx) > _ffi.MAX_INLINE_FRAMES or
                       (normal_batch is not None and (normal_idx is None or len(normal_idx) != len(frame_idx)))):
            raise ValueError("inline windows hold up to %d keyframes (with one normal index each)" % _ffi.MAX_INLINE_FRAMES)
        F = len(frame_idx) if inline else int(frame_idx.numel())
        R0 = F * sc.n_rays
        S = sc.S
        key = (R0, S, bool(want_T), normal_batch is not None)
        slot = None
        if reuse:   # the step loop's fast path: ten torch.empty calls sit in front of the first launch otherwise.
            ring = self._smp_ring                        # TWO alternating buffer sets: the previous step's outputs
            if ring is None or ring[0] != key:           # (trainer.active_pixels) stay intact for one more step
                ring = self._smp_ring = [key, [None, None], 0, [None, None]]
                # the cached step plans hold raw pointers into the buffer sets just dropped: a later ring of the same shape may
                # get `pc` back at its old address while the small tensors land elsewhere (clear_keyframes: F 5 -> 1 -> 5)
                self._step_plans.clear()
            ring[2] ^= 1
            slot = ring[2]
            # ... and the call's ctypes structs are kept with the buffer set: a device-synchronised step() has ~40 us of
            # Python between its opening synchronisation and the chain kernel's launch; rebuilding two 20-field structs
            # per step was a third of it.  Valid while the same input tensors / configuration come back.
            plan = ring[3][slot]
            pkey = (depth_batch.data_ptr(), T_WC_batch.data_ptr(), 0 if normal_batch is None else normal_batch.data_ptr(),
                    -1 if inline else frame_idx.data_ptr(),
                    -1 if inline else (0 if normal_idx is None else normal_idx.data_ptr()), sc.n_rays, sc.H, sc.W,
                    sc.fx, sc.fy, sc.cx, sc.cy, sc.n_strat, sc.n_surf, sc.min_depth, sc.dist_behind_surf)
            if draws is None and plan is not None and plan[0] == pkey:
                _, a, o, out = plan
                a.seed, a.offset = int(seed), int(offset)
                if inline:
                    a.frame_idx_inline[:F] = frame_idx
                    if normal_idx is not None:
                        a.normal_idx_inline[:F] = normal_idx
                _ffi.check(self.lib.isdf_sample_rays(C.byref(a), C.byref(o), self._scan_ptr, self._scan_ws.numel(),
                                                     _stream(self.device)), "isdf_sample_rays")
                return dict(out)
        a = _ffi.SampleArgs()
        a.depth_batch, a.T_WC_batch = depth_batch.data_ptr(), T_WC_batch.data_ptr()
        a.normal_batch = None if normal_batch is None else normal_batch.data_ptr()
        if inline:
            a.n_inline = F
            a.frame_idx_inline[:F] = [int(v) for v in frame_idx]
            if normal_idx is not None:
                a.normal_idx_inline[:F] = [int(v) for v in normal_idx]
        else:
            a.frame_idx = frame_idx.data_ptr()
            a.normal_idx = None if normal_idx is None else normal_idx.data_ptr()
        a.n_frames, a.n_rays, a.H, a.W = F, sc.n_rays, sc.H, sc.W
        a.fx, a.fy, a.cx, a.cy = sc.fx, sc.fy, sc.cx, sc.cy
        a.n_strat, a.n_surf = sc.n_strat, sc.n_surf
        a.min_depth, a.dist_behind_surf = sc.min_depth, sc.dist_behind_surf
        keep = []
        if draws is not None:
            a.rng_mode = 0
            for name, dkey, dt in (("draw_h", "indices_h", torch.int64), ("draw_w", "indices_w", torch.int64),
                                   ("draw_u", "U", torch.float32), ("draw_n", "N_off", torch.float32)):
                t = draws.get(dkey)
                if t is not None:
                    t = t.to(device=dev, dtype=dt).contiguous()
                    keep.append(t)
                    setattr(a, name, t.data_ptr())
        else:
            a.rng_mode = 1
            a.seed, a.offset = int(seed), int(offset)
        out = self._smp_ring[1][slot] if slot is not None else None
        if out is None:
            e = lambda *shape, dt=torch.float32: torch.empty(*shape, dtype=dt, device=dev)
            out = dict(
                n_valid=e(1, dt=torch.int32),   # always written by the sampler (no fill launch)
                indices_b=e(R0, dt=torch.int64), indices_h=e(R0, dt=torch.int64), indices_w=e(R0, dt=torch.int64),
                depth_sample=e(R0), dirs_C_sample=e(R0, 3),
                norm_sample=None if normal_batch is None else e(R0, 3),
                T_WC_sample=e(R0, 4, 4) if want_T else None,
                dirs_W_sample=e(R0, 3), z_vals=e(R0, S), pc=e(R0, S, 3))
            if slot is not None:
                self._smp_ring[1][slot] = out
        out = dict(out)
        o = _ffi.SampleOut()
        for k, v in out.items():
            setattr(o, k, None if v is None else v.data_ptr())
        need = int(self.lib.isdf_sample_scan_bytes(R0))
        if self._scan_ws is None or self._scan_ws.numel() < need:
            self._scan_ws = torch.zeros(max(need, 4096), dtype=torch.uint8, device=dev)
            if self._smp_ring is not None:
                self._smp_ring[3] = [None, None]
        self._scan_ptr = _ffi.ptr(self._scan_ws)
        _ffi.check(self.lib.isdf_sample_rays(C.byref(a), C.byref(o), self._scan_ptr, self._scan_ws.numel(),
                                             _stream(self.device)), "isdf_sample_rays")
        out["max_rays"] = R0
        out["S"] = S
        out["n_frames"] = F
        out["_keep"] = keep
        if slot is not None and draws is None:
            out["_slot"] = slot
            self._smp_ring[3][slot] = (pkey, a, o, dict(out))
        return out

    # ---- fused inference ------------------------------------------------------
    def sdf_eval(self, pts, noise=None, want_grad=False):
        """pts [..., 3] -> sdf [...] (and sdf_grad [..., 3]); SDFMap.forward /
        fc_map.gradient (fc_map.py:94-111, 12-22)."""
        shp = pts.shape[:-1]
        x = pts.reshape(-1, 3).to(device=self.device, dtype=torch.float32).contiguous()
        n = x.shape[0]
        sdf = torch.empty(n, dtype=torch.float32, device=self.device)
        grad = torch.empty(n, 3, dtype=torch.float32, device=self.device) if want_grad else None
        ws = self.workspace(n, False) if want_grad else None
        nz = None if noise is None else noise.reshape(-1).to(device=self.device, dtype=torch.float32).contiguous()
        _ffi.check(self.lib.isdf_sdf_eval(C.byref(self.cnet), _ffi.ptr(self.params), _ffi.ptr(self.shadow),
                                          _ffi.ptr(x), n, _ffi.ptr(nz), _ffi.ptr(sdf), _ffi.ptr(grad),
                                          _ffi.ptr(ws), 0 if ws is None else ws.numel(), _stream(self.device)),
                   "isdf_sdf_eval")
        if want_grad:
            return sdf.view(*shp), grad.view(*shp, 3)
        return sdf.view(*shp)

    # ---- training step ----------------------------------------------------------
    def train_step(self, smp, lc: LossConfig, sc: SampleConfig, noise=None, debug=False, prof_events=None,
                   noise_std=0.0, noise_seed=0, noise_offset=0, optim=None, surf_group=None, extra_slot=0, extra_value=0.0,
                   split_event=None):
        """Everything between sampling and the optimiser.  Fills self.reduce_buf with
        [grad sums | loss sums(8) | block_loss | block_cnt]; returns debug tensors.

        optim: None, or a dict(lr, weight_decay, betas, eps, grad_scale) -> the single-GPU fused form
        (isdf_train_step_adamw): the AdamW update and the operand repack happen inside the same call.
        surf_group: process group; with bounds_method "pc" the nearest-surface search then runs against the
        all-gathered surface samples of every rank.
        extra_slot / extra_value: with `self.reduce_extra` caller-owned floats behind the reduction message, the step writes
        extra_value into slot extra_slot and 0 into the others (data parallel: this rank's previous step time).
        split_event: torch.cuda.Event (two-call form only): the closing reduction runs as two launches with this event recorded
        between them; `self.reduce_buf[self.reduce_split:]` is final at the event (dp.allreduce_split_ overlaps its all-reduce
        with the second launch).
        The loss sums also land in `self.mailbox[:8]` (pinned host memory), valid after the next stream synchronisation."""
        dev = self.device
        F, R0, S = smp["n_frames"], smp["max_rays"], smp["S"]
        # fast path of the step loop: same sampler buffer set, same configuration -> the ctypes structs of the previous
        # call on this set are reused and only the per-step scalars change
        plan_key = None
        if (smp.get("_slot") is not None and noise is None and not debug and surf_group is None
                and lc.bounds_method == "ray"):
            fo = None if optim is None else optim.get("frame_avg_out")
            fi = None if optim is None else optim.get("frame_avg_index")
            fi_inline = isinstance(fi, (tuple, list))
            ns = smp.get("norm_sample")
            plan_key = (smp["_slot"], smp["pc"].data_ptr(), smp["n_valid"].data_ptr(), smp["indices_b"].data_ptr(),
                        smp["z_vals"].data_ptr(), 0 if ns is None else ns.data_ptr(),
                        R0, S, F, sc.H, sc.W, lc.loss_type, lc.trunc_weight, lc.trunc_distance,
                        lc.eik_weight, lc.eik_apply_dist, lc.grad_weight, lc.orien_loss, optim is None,
                        0 if fo is None else fo.data_ptr(), 0 if fi is None else (-1 if fi_inline else fi.data_ptr()), self.reduce_extra,
                        0 if split_event is None else split_event.cuda_event,
                        None if self.reduce_buf is None else self.reduce_buf.data_ptr(), None if self._ws is None else self._ws.data_ptr())
            plan = self._step_plans.get(smp["_slot"])
            if plan is not None and plan[0] == plan_key:
                _, closs, a, o, q, ws, dbg = plan
                a.noise_std, a.noise_seed, a.noise_offset = float(noise_std), int(noise_seed), int(noise_offset)
                a.extra_slot, a.extra_value = int(extra_slot), float(extra_value)
                o.prof_events = prof_events          # (bench.py: four hipEvent_t around the step's kernels on some steps; None otherwise)
                if q is not None:
                    self._step_scalars(q, optim, F, fi if fi_inline else None)
                self._launch_step(closs, a, o, q, ws)
                return dict(dbg)      # a fresh dict per call; its `loss_approx` tensor is the plan's reused buffer (overwritten by
                                      # the next step on this buffer set, two steps later)
        # [isdf_reduce_floats | reduce_extra caller-owned floats]: the kernels write the first part; the tail belongs to the
        # host protocol (data parallel: per-rank step-time slots riding in the same all-reduce message, hot_path.py)
        nred = int(self.lib.isdf_reduce_floats(C.byref(self.cnet), F))
        if self.reduce_buf is None or self.reduce_buf.numel() != nred + self.reduce_extra:
            self.reduce_buf = torch.zeros(nred + self.reduce_extra, dtype=torch.float32, device=dev)
        self.reduce_floats = nred
        if self.mailbox is None or self.mailbox.numel() != 8 + self.reduce_extra:
            # pinned HOST memory the step's last launch writes the loss sums (+ the reduced tail) into: no D2H copy command
            self.mailbox = torch.zeros(8 + self.reduce_extra, dtype=torch.float32, pin_memory=True)
        ws = self.workspace(R0 * S, True)
        self._ws_ptr, self._params_ptr, self._shadow_ptr = _ffi.ptr(ws), _ffi.ptr(self.params), _ffi.ptr(self.shadow)
        closs = lc.to_c()
        a = _ffi.StepArgs()
        a.n_valid = smp["n_valid"].data_ptr()
        a.max_rays, a.S, a.n_frames, a.H, a.W = R0, S, F, sc.H, sc.W
        for k in ("pc", "z_vals", "depth_sample", "dirs_C_sample", "dirs_W_sample", "indices_b",
                  "indices_h", "indices_w"):
            setattr(a, k, smp[k].data_ptr())
        a.norm_sample = None if smp.get("norm_sample") is None else smp["norm_sample"].data_ptr()
        keep = []
        a.noise_std, a.noise_seed, a.noise_offset = float(noise_std), int(noise_seed), int(noise_offset)
        a.extra_floats, a.extra_slot, a.extra_value = int(self.reduce_extra), int(extra_slot), float(extra_value)
        if noise is not None:
            if (noise.numel() == R0 * S and noise.dtype == torch.float32 and noise.device == dev
                    and noise.is_contiguous()):
                nz = noise                       # already one value per (ray slot, sample): borrow it
            else:                                # per-valid-ray noise: pad to the slot count
                nz = torch.zeros(R0 * S, dtype=torch.float32, device=dev)
                nn_ = noise.reshape(-1).to(device=dev, dtype=torch.float32)
                nz[:nn_.numel()] = nn_
            keep.append(nz)
            a.noise = nz.data_ptr()
        if lc.bounds_method == "pc":
            pb = torch.empty(R0 * S, dtype=torch.float32, device=dev)
            pg = torch.empty(R0 * S, 3, dtype=torch.float32, device=dev)
            surf = None
            if surf_group is not None:   # data parallel: the surface set is every rank's surface samples
                from . import dp
                surf = dp.gather_surface_points(smp["pc"], smp["n_valid"], surf_group)
                keep.append(surf)
            _ffi.check(self.lib.isdf_bounds_pc(_ffi.ptr(smp["n_valid"]), R0, S, _ffi.ptr(smp["pc"]),
                                               _ffi.ptr(smp["z_vals"]), _ffi.ptr(smp["depth_sample"]),
                                               _ffi.ptr(surf), 0 if surf is None else surf.shape[0],
                                               _ffi.ptr(pb), _ffi.ptr(pg), _stream(self.device)), "isdf_bounds_pc")
            a.pc_bounds, a.pc_grad_vec = pb.data_ptr(), pg.data_ptr()
            keep += [pb, pg]
        o = _ffi.StepOut()
        o.reduce_buf = self.reduce_buf.data_ptr()
        o.host_mailbox = self.mailbox.data_ptr()
        if prof_events is not None:   # ctypes array of 4 hipEvent_t (bench.py)
            o.prof_events = prof_events
        if split_event is not None:
            if optim is not None:
                raise ValueError("split_event belongs to the two-call (data-parallel) form")
            o.split_event = split_event.cuda_event
        dbg = {}
        if debug:
            dbg = dict(sdf=torch.zeros(R0, S, device=dev), sdf_grad=torch.zeros(R0, S, 3, device=dev),
                       tot_loss_mat=torch.zeros(R0, S, device=dev))
            o.sdf, o.sdf_grad, o.tot_loss_mat = (dbg["sdf"].data_ptr(), dbg["sdf_grad"].data_ptr(),
                                                 dbg["tot_loss_mat"].data_ptr())
            if lc.bounds_method == "pc":
                dbg["pc_bounds"], dbg["pc_grad_vec"] = keep[-2].view(R0, S), keep[-1].view(R0, S, 3)
        q = None if optim is None else self._optim_args(optim, F, dbg, keep)
        self._launch_step(closs, a, o, q, ws)
        dbg["_keep"] = keep
        if plan_key is not None:
            # re-key with the buffers this call may have (re)allocated
            plan_key = plan_key[:-2] + (self.reduce_buf.data_ptr(), self._ws.data_ptr())
            self._step_plans[smp["_slot"]] = (plan_key, closs, a, o, q, ws, dbg)
        return dbg

    def _launch_step(self, closs, a, o, q, ws):
        """isdf_train_step_adamw with the isdf_optim_args `q`, isdf_train_step with q None, on the buffers train_step last set up"""
        if q is not None:
            _ffi.check(self.lib.isdf_train_step_adamw(C.byref(self.cnet), C.byref(closs), C.byref(a), C.byref(o),
                                                      C.byref(q), self._ws_ptr, ws.numel(), _stream(self.device)),
                       "isdf_train_step_adamw")
        else:
            _ffi.check(self.lib.isdf_train_step(C.byref(self.cnet), C.byref(closs), self._params_ptr, self._shadow_ptr,
                                                C.byref(a), C.byref(o), self._ws_ptr, ws.numel(), _stream(self.device)),
                       "isdf_train_step")

    def _step_scalars(self, q, optim, F, inline_idx=None):
        """advances the optimiser step; writes lr .. step and, window inline, its F frame-average indices (Python ints) into `q`"""
        self.opt_step += 1
        betas = optim.get("betas", ADAMW_BETAS)
        q.lr, q.weight_decay = float(optim.get("lr", ADAMW_LR)), float(optim.get("weight_decay", ADAMW_WEIGHT_DECAY))
        q.beta1, q.beta2, q.eps = float(betas[0]), float(betas[1]), float(optim.get("eps", ADAMW_EPS))
        q.grad_scale, q.step = float(optim.get("grad_scale", 1.0)), int(self.opt_step)
        if inline_idx is not None:
            q.frame_avg_index_inline[:F] = inline_idx

    def _optim_args(self, optim, F, dbg, keep):
        """isdf_optim_args of this engine's buffers; advances the optimiser step.  optim: dict(lr, weight_decay, betas,
        eps, grad_scale[, frame_avg_out, frame_avg_index])"""
        q = _ffi.OptimArgs()
        q.params, q.exp_avg, q.exp_avg_sq = self.params.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()
        q.shadow = self.shadow.data_ptr()
        inline_idx = None
        if optim.get("frame_avg_out") is not None:   # loss.frame_avg fused into the same launch
            la = torch.empty(F, 8, 8, dtype=torch.float32, device=self.device)
            fa_out, fa_idx = optim["frame_avg_out"], optim.get("frame_avg_index")
            assert fa_out.dtype == torch.float32 and fa_out.is_contiguous()
            q.loss_approx, q.frame_avg = la.data_ptr(), fa_out.data_ptr()
            if isinstance(fa_idx, (tuple, list)):     # the window as kernel arguments (isdf_optim_args.frame_avg_index_inline)
                assert len(fa_idx) == F <= _ffi.MAX_INLINE_FRAMES
                q.frame_avg_inline_n = F
                inline_idx = [int(v) for v in fa_idx]
            else:
                assert fa_idx is None or (fa_idx.dtype == torch.int32 and fa_idx.numel() == F)
                q.frame_avg_index = None if fa_idx is None else fa_idx.data_ptr()
            dbg["loss_approx"] = la
            keep += [fa_out, fa_idx]
        self._step_scalars(q, optim, F, inline_idx)
        return q

    def allreduce_direct(self, rccl):
        """THE collective of the data-parallel step on the step's own stream (isdf_allreduce_sum_f32): in-place sum of the
        whole message -- reduce_buf incl. its caller-owned tail -- over the ranks of `rccl` = dp.rccl_direct(group, device)."""
        fn, comm = rccl
        _ffi.check(self.lib.isdf_allreduce_sum_f32(fn, comm, _ffi.ptr(self.reduce_buf), int(self.reduce_buf.numel()),
                                                   _stream(self.device)), "isdf_allreduce_sum_f32")

    def train_step_finish(self, n_frames, optim):
        """Second half of the data-parallel step (isdf_train_step_finish): AdamW on the all-reduced gradient sums,
        operand repack and -- with optim["frame_avg_out"] -- loss.frame_avg from the reduced bins, ONE launch."""
        dbg, keep = {}, []
        fo, fi = optim.get("frame_avg_out"), optim.get("frame_avg_index")
        fi_inline = isinstance(fi, (tuple, list))
        fkey = (n_frames, 0 if fo is None else fo.data_ptr(), 0 if fi is None else (-1 if fi_inline else fi.data_ptr()),
                self.reduce_buf.data_ptr(), self.mailbox.data_ptr(), self.reduce_extra)
        plan = self._step_plans.get("finish")
        if plan is not None and plan[0] == fkey:      # same buffers as the last call: reuse the struct, bump the scalars
            _, q, dbg = plan
            self._step_scalars(q, optim, n_frames, fi if fi_inline else None)
        else:
            q = self._optim_args(optim, n_frames, dbg, keep)
            self._step_plans["finish"] = (fkey, q, dbg)
        _ffi.check(self.lib.isdf_train_step_finish(C.byref(self.cnet), C.byref(q), _ffi.ptr(self.reduce_buf), int(n_frames),
                                                   int(self.reduce_extra), _ffi.ptr(self.mailbox), _stream(self.device)),
                   "isdf_train_step_finish")
        dbg["_keep"] = keep
        return dbg

    def grad_view(self, key):
        off, shp = self.slices[key]
        return self.reduce_buf[off:off + int(np.prod(shp))].view(*shp)

    def loss_sums(self):
        return self.reduce_buf[self.n_params:self.n_params + 8]

    def frame_avg(self, n_frames, out=None, index=None):
        """loss.frame_avg from the (reduced) bins.  out/index: write frame f's average to out[index[f]] (the
        keyframe store's frame_avg_losses and the window's keyframe ids) instead of a fresh [F] tensor.
        A tuple / list index (the host-side window) is converted once per distinct window and cached."""
        if isinstance(index, (tuple, list)):
            key = tuple(int(v) for v in index)
            cache = self._fa_index_cache
            if key not in cache:
                if len(cache) > 64:
                    cache.clear()
                cache[key] = torch.as_tensor(key, dtype=torch.int32, device=self.device)
            index = cache[key]
        la = torch.empty(n_frames, 8, 8, dtype=torch.float32, device=self.device)
        if out is None:
            fa = torch.empty(n_frames, dtype=torch.float32, device=self.device)
        else:
            assert out.dtype == torch.float32 and out.is_contiguous()
            assert index is None or (index.dtype == torch.int32 and index.numel() == n_frames)
            fa = out
        _ffi.check(self.lib.isdf_frame_avg(_ffi.ptr(self.reduce_buf), self.n_params, n_frames, _ffi.ptr(la),
                                           _ffi.ptr(fa), _ffi.ptr(index), _stream(self.device)), "isdf_frame_avg")
        return la, fa

    # ---- per-frame ingest / keyframe test -------------------------------
    def estimate_normals(self, depth, sc: "SampleConfig"):
        """depth [H,W] -> camera-frame normals [H,W,3] (trainer.py:553-557)."""
        d = depth.to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty(d.shape[0], d.shape[1], 3, dtype=torch.float32, device=self.device)
        _ffi.check(self.lib.isdf_estimate_normals(_ffi.ptr(d), d.shape[0], d.shape[1], sc.fx, sc.fy, sc.cx, sc.cy,
                                                  _ffi.ptr(out), _stream(self.device)), "isdf_estimate_normals")
        return out

    def render_depth(self, z_vals, sdf, depth_sample=None, kf_dist_th=0.1, n_valid=None):
        """(view_depth [R], below_count int32[1]) of Trainer.is_keyframe (trainer.py:597-609)."""
        R, S = z_vals.shape
        view = torch.zeros(R, dtype=torch.float32, device=self.device)
        below = torch.zeros(1, dtype=torch.int32, device=self.device)
        _ffi.check(self.lib.isdf_render_depth(_ffi.ptr(n_valid), R, R, S, _ffi.ptr(z_vals.contiguous()),
                                              _ffi.ptr(sdf.contiguous()), _ffi.ptr(depth_sample), float(kf_dist_th),
                                              _ffi.ptr(view), _ffi.ptr(below), _stream(self.device)), "isdf_render_depth")
        return view, below

    # ---- mesh reconstruction ----------------------------------------------------------
    def marching_cubes(self, volume, level=0.0, index_to_world=None):
        """(verts [V,3] f32, faces [F,3] i32, normals [V,3] f32) on the device: isdf_marching_cubes of a [D0,D1,D2] volume, the
        isosurface step of Trainer.mesh_rec (draw3D.py:111-160).  One launch at the cached capacity, one sync to read the counts,
        one re-launch only on overflow; workspace and capacity are kept across calls (isdf_amd.mesh.Mesher)."""
        if self._mesher is None:
            from .mesh import Mesher
            self._mesher = Mesher(self.device)
        return self._mesher(volume, level, index_to_world)

    def band_volume(self, dims, index_to_world=None, points=None, level=0.0, slack=None, coarse=8, field=None):
        """(volume [D0,D1,D2] f32, stats): `field` evaluated only in a narrow band around its `level` set, NaN elsewhere, so that
        `marching_cubes(volume, level, index_to_world)` is the mesh of the dense grid (the isdf_band_* calls, include/isdf_hip.h:
        coarse to fine over strides coarse .. 2, a cell kept iff a corner is not finite, its corners straddle level or all lie
        within slack x its world diagonal of it).  With an L-Lipschitz field and slack >= L the mesh equals the dense one bit
        for bit; `stats["leaks"]` > 0 says the surface left the band (isdf_amd.mesh.extract_surface then widens).

        dims: D or (D0, D1, D2).  index_to_world: [3, 4] affine, measures the cells and (without `points`) makes the positions;
        points: [D0*D1*D2, 3] device tensor to gather the positions from instead (a trainer's grid_pc).  field: callable, device
        points [n, 3] -> values [n]; default `self.sdf_eval`.  slack: None = isdf_amd.mesh.DEFAULT_SLACK.
        stats: levels = [dict(stride, candidates, kept, evaluated) per stride, dict(stride=1, evaluated) for the closing fill],
        evaluated, dense (= D0*D1*D2), fraction, leaks, slack, coarse.  One small device -> host read per level."""
        if self._band is None:
            from .mesh import BandSelector
            self._band = BandSelector(self.device)
        return self._band(self.sdf_eval if field is None else field, dims, index_to_world, points, level, slack, coarse)

    # ---- rendered views ----------------------------------------------------------
    def render_views(self, T_WC, dirs_C, H, W, n_samples=0, **kw):
        """(depth [B, H*W] or None, normals [B, H*W, 3] or None) on the device for the B poses of T_WC: isdf_render_views, the
        renders of Trainer.render_depth_vis / render_normals_vis / latest_frame_vis (trainer.py:1055-1147,1225-1280) in one
        pass; the options are isdf_amd.render.Renderer's.  The workspace is kept across calls."""
        if self._renderer is None:
            from .render import Renderer
            self._renderer = Renderer(self)
        return self._renderer(T_WC, dirs_C, H, W, n_samples, **kw)

    # ---- evaluation against ground truth -----------------------------------------------
    def _flat(self, t, dtype, width=None):
        """`t` on this engine's device as contiguous `dtype`, flat or (width given) as rows of `width`"""
        t = t.detach().reshape(-1) if width is None else t.detach().reshape(-1, width)
        return t.to(device=self.device, dtype=dtype).contiguous()

    def _check_device(self, name, what, t):
        """`t` lies on this engine's device"""
        if t.device.type != self.device.type or (self.device.index is not None and t.device.index != self.device.index):
            raise ValueError("%s: %s is on %s, the engine on %s" % (name, what, t.device, self.device))

    def _scratch(self, name, nbytes):
        """the uint8 workspace the calls named `name` share: kept across calls, replaced by a larger one when `nbytes` asks for it"""
        ws = self._scratch_bufs.get(name)
        if ws is None or ws.numel() < nbytes:
            ws = self._scratch_bufs[name] = None            # release before growing: the two never need to coexist
            ws = self._scratch_bufs[name] = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return ws

    @property
    def _nn_ws(self):
        """the workspace isdf_nn_distance last used: it begins with the keys (include/isdf_hip.h), which the tests compare"""
        return self._scratch_bufs.get("nn_distance")

    def _record_out(self, name, out, rows, width, on=None):
        """a fresh float64 [rows, width] record tensor, or the caller's `out` checked to be one (and, `on` given, on that device)"""
        if out is None:
            return torch.empty(rows, width, dtype=torch.float64, device=self.device)
        if out.dtype != torch.float64 or out.numel() != rows * width or not out.is_contiguous() or (on is not None and out.device != on):
            raise ValueError("%s: out must be a contiguous float64 [%d, %d]%s" % (name, rows, width, " on x's device" if on is not None else ""))
        return out

    def sdf_metrics(self, volume, pts, sdf, exclude_zero_gt=True, per_point=False, oob_fill=0.0):
        """(record f64[24], gt [n] or None, valid u8[n] or None) on the device: isdf_sdf_metrics, the ground-truth lookup and
        every sum of Trainer.eval_sdf / eval_object_sdf / eval_traj_cost (trainer.py:1831-1866,1993-2003,2026-2050) in one
        pass.  `volume`: isdf_amd.metrics.GtVolume; pts [n,3], sdf [n].  No host synchronisation; isdf_amd.metrics.sdf_metrics
        copies the record once and names its fields."""
        p, s = self._flat(pts, torch.float32, 3), self._flat(sdf, torch.float32)
        n = int(p.shape[0])
        if s.numel() != n:
            raise ValueError("sdf_metrics: %d points but %d sdf values" % (n, s.numel()))
        self._check_device("sdf_metrics", "the ground-truth volume", volume.values)
        ws = self._scratch("sdf_metrics", _ffi.SDF_METRICS_WS_BYTES)
        record = torch.empty(_ffi.METRICS_RECORD, dtype=torch.float64, device=self.device)
        gt = torch.empty(n, dtype=torch.float32, device=self.device) if per_point else None
        valid = torch.empty(n, dtype=torch.uint8, device=self.device) if per_point else None
        _ffi.check(self.lib.isdf_sdf_metrics(C.byref(volume.to_c()), _ffi.ptr(p), _ffi.ptr(s), n, int(bool(exclude_zero_gt)),
                                             float(oob_fill), _ffi.ptr(record), _ffi.ptr(gt), _ffi.ptr(valid),
                                             _ffi.ptr(ws), int(ws.numel()), _stream(self.device)), "isdf_sdf_metrics")
        return record, gt, valid

    def region_metrics(self, pts, sdf, volume=None, gt=None, sdf_grad=None, flags=None, delta=0.01, out=None):
        """records f64 [2, 27] on the device (vis, vox): isdf_region_metrics, the arithmetic of eval_pts.fixed_pts_eval after the
        network (eval_pts.py:96-299) in one pass, all in double.  pts [n,3], sdf [n]; ground truth from `volume`
        (isdf_amd.metrics.GtVolume) or from `gt` (float64 [n], the full-volume leg); flags u8 [n] (_ffi.FLAG_*; None: every point
        in both sdf sets); sdf_grad [n,3]: the gradient sets named by flag bits 4 / 8 are evaluated.  out: a [2, 27] float64 view
        to write into (several legs, one copy).  No host synchronisation."""
        dev = self.device
        p, s = self._flat(pts, torch.float32, 3), self._flat(sdf, torch.float32)
        n = int(p.shape[0])
        if s.numel() != n:
            raise ValueError("region_metrics: %d points but %d sdf values" % (n, s.numel()))
        if (volume is None) == (gt is None):
            raise ValueError("region_metrics: exactly one of volume and gt")
        a = _ffi.RegionArgs()
        keep = [p, s]
        if volume is not None:
            self._check_device("region_metrics", "the ground-truth volume", volume.values)
            vc = volume.to_c()
            keep.append(vc)
            a.vol = C.pointer(vc)
            for k in range(3):
                a.spacing[k], a.origin[k] = volume.spacing[k], volume.origin[k]
        else:
            g = self._flat(gt, torch.float64)
            if g.numel() != n:
                raise ValueError("region_metrics: %d points but %d ground-truth values" % (n, g.numel()))
            keep.append(g)
            a.gt_in = g.data_ptr() if n else 8        # n = 0: an empty tensor has no address; nothing is read
        for name, t, dt, width in (("sdf_grad", sdf_grad, torch.float32, 3), ("flags", flags, torch.uint8, 1)):
            if t is not None:
                t = self._flat(t, dt)
                if t.numel() != n * width:
                    raise ValueError("region_metrics: %s has %d elements for %d points" % (name, t.numel(), n))
                keep.append(t)
                setattr(a, name, t.data_ptr() if n else 8)
        a.pts, a.sdf, a.n = p.data_ptr(), s.data_ptr(), n
        a.grad_sets, a.delta = int(sdf_grad is not None), float(delta)
        ws = self._scratch("region_metrics", _ffi.REGION_METRICS_WS_BYTES)
        out = self._record_out("region_metrics", out, 2, _ffi.REGION_RECORD)
        _ffi.check(self.lib.isdf_region_metrics(C.byref(a), _ffi.ptr(out), _ffi.ptr(ws), int(ws.numel()), _stream(dev)),
                   "isdf_region_metrics")
        return out

    def nn_distance(self, query, target, want_index=False):
        """(dist [n] f32, index [n] i32 or None, dist_sum f64[1]) on the device: isdf_nn_distance, the exact distance from every
        query point to its nearest target point (the KD-tree queries of metrics.accuracy / completion, metrics.py:48-59) by
        brute force; the lowest target index on ties.  No host synchronisation."""
        q, t = self._flat(query, torch.float32, 3), self._flat(target, torch.float32, 3)
        n, m = int(q.shape[0]), int(t.shape[0])
        if n > 0 and m < 1:
            raise ValueError("nn_distance: empty target set")
        ws = self._scratch("nn_distance", _ffi.nn_ws_bytes(n))
        dist = torch.empty(n, dtype=torch.float32, device=self.device)
        index = torch.empty(n, dtype=torch.int32, device=self.device) if want_index else None
        total = torch.empty(1, dtype=torch.float64, device=self.device)
        _ffi.check(self.lib.isdf_nn_distance(_ffi.ptr(q), n, _ffi.ptr(t), m, _ffi.ptr(dist), _ffi.ptr(index), _ffi.ptr(total),
                                             _ffi.ptr(ws), int(ws.numel()), _stream(self.device)), "isdf_nn_distance")
        return dist, index, total

    def visible_points(self, pts, T_CW, depth, cam, trunc=0.2, want_mask=False):
        """(count i32 [n], mask u8 [F,n] or None, n_seen i64 [1]) on the device: isdf_visible_points, the predicate of
        geometry.frustum.is_visible_torch (frustum.py:87-133, use_projection=True) for every pair of the F posed depth frames and the
        n points in one pass -- count[i] frames see point i, n_seen points are seen by at least one.  pts [n,3]; T_CW [F,4,4]
        CAMERA-FROM-WORLD (isdf_amd.metrics.visible_points inverts T_WC); depth [F,H,W]; cam: anything with fx, fy, cx, cy.
        No host synchronisation, and nothing of size F * n unless `want_mask`."""
        if depth.dim() != 3:
            raise ValueError("visible_points: depth must be [F, H, W] (got %s)" % (tuple(depth.shape),))
        F, H, W = (int(v) for v in depth.shape)
        p, T, d = self._flat(pts, torch.float32, 3), self._flat(T_CW, torch.float32, 16), self._flat(depth, torch.float32)
        n = int(p.shape[0])
        if int(T.shape[0]) != F:
            raise ValueError("visible_points: %d poses for %d depth frames" % (T.shape[0], F))
        count = torch.empty(n, dtype=torch.int32, device=self.device)
        mask = torch.empty(F, n, dtype=torch.uint8, device=self.device) if want_mask else None
        n_seen = torch.empty(1, dtype=torch.int64, device=self.device)
        _ffi.check(self.lib.isdf_visible_points(_addr(p), n, _addr(T), _addr(d), F, H, W, float(cam.fx), float(cam.fy), float(cam.cx),
                                                float(cam.cy), float(trunc), _addr(count), _addr(mask), _ffi.ptr(n_seen),
                                                _stream(self.device)), "isdf_visible_points")
        return count, mask, n_seen

    # ---- the voxel baseline: TSDF fusion and the distance transform -----------------------
    def tsdf_integrate(self, tsdf, weight, depth, T_CW, cam, origin, spacing, trunc, max_weight=float("inf"), min_depth=0.0,
                       max_depth=float("inf")):
        """isdf_tsdf_integrate: the F posed depth frames fused, in index order, into the running pair `tsdf`, `weight` (contiguous
        float32 [nx,ny,nz] on this device, updated IN PLACE; zero before the first call), voxel (i, j, k) at origin + (i, j, k) *
        spacing.  depth [F,H,W]; T_CW [F,4,4] CAMERA-FROM-WORLD (isdf_amd.fusion.integrate inverts T_WC); cam: anything with fx,
        fy, cx, cy.  Per voxel a fixed fp32 sequence (include/isdf_hip.h): F frames in one call equal the same frames in any
        sequence of calls bit for bit.  Returns (tsdf, weight).  No host synchronisation."""
        if depth.dim() != 3:
            raise ValueError("tsdf_integrate: depth must be [F, H, W] (got %s)" % (tuple(depth.shape),))
        for name, t in (("tsdf", tsdf), ("weight", weight)):
            if t.dim() != 3 or t.dtype != torch.float32 or not t.is_contiguous() or t.device.type != self.device.type:
                raise ValueError("tsdf_integrate: %s must be a contiguous float32 [nx, ny, nz] tensor on %s" % (name, self.device))
        if tsdf.shape != weight.shape:
            raise ValueError("tsdf_integrate: tsdf is %s, weight %s" % (tuple(tsdf.shape), tuple(weight.shape)))
        F, H, W = (int(v) for v in depth.shape)
        T, d = self._flat(T_CW, torch.float32, 16), self._flat(depth, torch.float32)
        if int(T.shape[0]) != F:
            raise ValueError("tsdf_integrate: %d poses for %d depth frames" % (T.shape[0], F))
        a = _ffi.TsdfArgs()
        a.nx, a.ny, a.nz = (int(v) for v in tsdf.shape)
        a.F, a.H, a.W = F, H, W
        a.origin[:] = [float(v) for v in np.asarray(origin, np.float64).reshape(3)]
        a.spacing[:] = [float(v) for v in np.asarray(spacing, np.float64).reshape(3)]
        a.fx, a.fy, a.cx, a.cy = float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)
        a.trunc, a.max_weight, a.min_depth, a.max_depth = float(trunc), float(max_weight), float(min_depth), float(max_depth)
        a.depth, a.T_CW, a.tsdf, a.weight = _addr(d), _addr(T), _addr(tsdf), _addr(weight)
        _ffi.check(self.lib.isdf_tsdf_integrate(C.byref(a), _stream(self.device)), "isdf_tsdf_integrate")
        return tsdf, weight

    def _edt_workspace(self, dims):
        need = int(self.lib.isdf_edt_ws_bytes(*dims))
        _ffi.check(min(need, 0), "isdf_edt_ws_bytes%s" % (dims,))
        return self._scratch("edt", need)

    def _edt_feature(self, name, feature):
        if feature.dim() != 3 or min(feature.shape) < 1:
            raise ValueError("%s: a [nx, ny, nz] grid with every side >= 1 is needed (got %s)" % (name, tuple(feature.shape)))
        f = feature.detach()
        f = (f != 0) if f.dtype != torch.uint8 else f
        return f.to(device=self.device, dtype=torch.uint8).contiguous(), tuple(int(v) for v in feature.shape)

    def distance_transform(self, feature, invert=False):
        """dist2 int32 [nx,ny,nz] on the device: isdf_distance_transform, the exact squared Euclidean distance (voxel units) from
        every voxel to the nearest voxel q with (feature[q] != 0) != invert; _ffi.EDT_NONE (2^30) where there is none.
        sqrt(dist2) in float64 is scipy.ndimage.distance_transform_edt of the complement bit for bit.  Sides up to 1024.  The
        workspace is kept across calls.  No host synchronisation."""
        f, dims = self._edt_feature("distance_transform", feature)
        ws = self._edt_workspace(dims)
        out = torch.empty(dims, dtype=torch.int32, device=self.device)
        _ffi.check(self.lib.isdf_distance_transform(_ffi.ptr(f), dims[0], dims[1], dims[2], int(bool(invert)), _ffi.ptr(out),
                                                    _ffi.ptr(ws), int(ws.numel()), _stream(self.device)), "isdf_distance_transform")
        return out

    def occupancy_sdf(self, occ, voxel):
        """sdf float32 [nx,ny,nz] on the device: isdf_occupancy_sdf, the reference's sdf_from_occupancy (sdf_util.py:371-385) --
        (distance to the nearest occupied voxel - distance to the nearest free one) * voxel, positive in free space, from two
        exact distance transforms and float64 square roots.  +inf everywhere without an occupied voxel, -inf without a free one.
        The workspace is kept across calls.  No host synchronisation."""
        f, dims = self._edt_feature("occupancy_sdf", occ)
        ws = self._edt_workspace(dims)
        out = torch.empty(dims, dtype=torch.float32, device=self.device)
        _ffi.check(self.lib.isdf_occupancy_sdf(_ffi.ptr(f), dims[0], dims[1], dims[2], float(voxel), _ffi.ptr(out), _ffi.ptr(ws),
                                               int(ws.numel()), _stream(self.device)), "isdf_occupancy_sdf")
        return out

    # ---- routing through the map: geodesic field and path ---------------------------------
    def _route_volume(self, name, what, t, dtype):
        """(t, dims): `t` checked to be a contiguous `dtype` [nx, ny, nz] volume on this device, every side >= 1"""
        if not torch.is_tensor(t) or t.dim() != 3 or min(t.shape) < 1 or t.dtype != dtype or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous %s [nx, ny, nz] tensor with every side >= 1" % (name, what, dtype))
        self._check_device(name, what, t)
        dims = tuple(int(v) for v in t.shape)
        if dims[0] * dims[1] * dims[2] > _ffi.ROUTE_MAX_VOXELS:
            raise ValueError("%s: at most 2^27 voxels (got %s)" % (name, dims))
        return t, dims

    def _route_voxels(self, name, what, v):
        """voxel coordinates as a contiguous int32 [n, 3] tensor on this device"""
        v = torch.as_tensor(v)
        if v.dtype.is_floating_point or v.dtype == torch.bool or v.numel() % 3 != 0:
            raise ValueError("%s: %s must be integer voxel coordinates [n, 3]" % (name, what))
        return v.detach().reshape(-1, 3).to(device=self.device, dtype=torch.int32).contiguous()

    def route_init(self, free, goals, out=None):
        """dist int32 [nx,ny,nz] on the device: isdf_route_init -- _ffi.ROUTE_NONE (2^30) everywhere, 0 at every goal (integer voxel
        coordinates [n,3], n = 0 allowed) that is inside the grid and free.  free: contiguous uint8 [nx,ny,nz] on this device,
        non-zero = free.  out: a dist volume to overwrite.  No host synchronisation."""
        f, dims = self._route_volume("route_init", "free", free, torch.uint8)
        g = self._route_voxels("route_init", "goals", goals)
        if out is None:
            out = torch.empty(dims, dtype=torch.int32, device=self.device)
        elif self._route_volume("route_init", "out", out, torch.int32)[1] != dims:
            raise ValueError("route_init: out is %s, free %s" % (tuple(out.shape), dims))
        _ffi.check(self.lib.isdf_route_init(_ffi.ptr(f), dims[0], dims[1], dims[2], _addr(g), int(g.shape[0]), _ffi.ptr(out),
                                            _stream(self.device)), "isdf_route_init")
        return out

    def route_relax(self, free, dist, rounds=1, changed=None):
        """changed int32 [rounds] on the device: isdf_route_relax -- `rounds` rounds (two tile launches each) of the 26-neighbour
        <3,4,5> chamfer relaxation on `dist` IN PLACE (int32 [nx,ny,nz] from route_init on the same `free`); changed[r] = 1 iff
        round r lowered any voxel.  Once a round changes nothing, dist is the exact shortest-path distance to the nearest goal.
        changed: an int32 tensor of at least `rounds` elements to reuse.  The workspace is kept across calls.  No host
        synchronisation: the caller decides when to look (isdf_amd.routing.distance_field does)."""
        f, dims = self._route_volume("route_relax", "free", free, torch.uint8)
        if self._route_volume("route_relax", "dist", dist, torch.int32)[1] != dims:
            raise ValueError("route_relax: dist is %s, free %s" % (tuple(dist.shape), dims))
        rounds = int(rounds)
        if rounds < 1:
            raise ValueError("route_relax: rounds >= 1 (got %d)" % rounds)
        if changed is None:
            changed = torch.empty(rounds, dtype=torch.int32, device=self.device)
        elif changed.dtype != torch.int32 or changed.numel() < rounds or not changed.is_contiguous():
            raise ValueError("route_relax: changed must be a contiguous int32 tensor of at least %d elements" % rounds)
        else:
            self._check_device("route_relax", "changed", changed)
        ws = self._scratch("route", int(self.lib.isdf_route_ws_bytes(*dims)))
        _ffi.check(self.lib.isdf_route_relax(_ffi.ptr(f), dims[0], dims[1], dims[2], _ffi.ptr(dist), _ffi.ptr(ws), int(ws.numel()),
                                             rounds, _ffi.ptr(changed), _stream(self.device)), "isdf_route_relax")
        return changed.reshape(-1)[:rounds]

    def route_trace(self, dist, starts, max_len):
        """(path int32 [B, max_len], len int32 [B]) on the device: isdf_route_trace -- from every start (integer voxel coordinates
        [B,3]) down `dist` to a goal, at every voxel to the first neighbour, in lexicographic (di, dj, dk) order, that explains
        its distance.  path holds linear voxel indices (i * ny + j) * nz + k, len the number of voxels with both ends; 0 for a
        start that is outside, blocked or unreachable, -1 where max_len is too small or the field is not converged.  Entries of
        path beyond len are not written.  No host synchronisation."""
        d, dims = self._route_volume("route_trace", "dist", dist, torch.int32)
        s = self._route_voxels("route_trace", "starts", starts)
        B, max_len = int(s.shape[0]), int(max_len)
        if max_len < 1:
            raise ValueError("route_trace: max_len >= 1 (got %d)" % max_len)
        path = torch.empty(B, max_len, dtype=torch.int32, device=self.device)
        length = torch.empty(B, dtype=torch.int32, device=self.device)
        if B:
            _ffi.check(self.lib.isdf_route_trace(_ffi.ptr(d), dims[0], dims[1], dims[2], _ffi.ptr(s), B, max_len, _ffi.ptr(path),
                                                 _ffi.ptr(length), _stream(self.device)), "isdf_route_trace")
        return path, length

    # ---- where to look next: frontiers, clusters, view gain -------------------------------
    def _frontier_ws(self, dims):
        return self._scratch("frontier", int(self.lib.isdf_frontier_ws_bytes(*dims)))

    def frontier_init(self, state, out=None):
        """label int32 [nx,ny,nz] on the device: isdf_frontier_init -- the voxel's own linear index (i * ny + j) * nz + k where it is
        a frontier voxel (FREE with at least one of its six face neighbours inside the grid UNKNOWN), _ffi.FRONTIER_NONE (2^30)
        elsewhere.  state: contiguous uint8 [nx,ny,nz] on this device (_ffi.VOXEL_*; >= 2 is occupied).  out: a label volume to
        overwrite.  No host synchronisation."""
        s, dims = self._route_volume("frontier_init", "state", state, torch.uint8)
        if out is None:
            out = torch.empty(dims, dtype=torch.int32, device=self.device)
        elif self._route_volume("frontier_init", "out", out, torch.int32)[1] != dims:
            raise ValueError("frontier_init: out is %s, state %s" % (tuple(out.shape), dims))
        _ffi.check(self.lib.isdf_frontier_init(_ffi.ptr(s), dims[0], dims[1], dims[2], _ffi.ptr(out), _stream(self.device)),
                   "isdf_frontier_init")
        return out

    def frontier_relax(self, label, rounds=1, changed=None):
        """changed int32 [rounds] on the device: isdf_frontier_relax -- `rounds` rounds (two tile launches each) of label[p] <-
        min over p and its 26 neighbours, IN PLACE, for voxels below FRONTIER_NONE; changed[r] = 1 iff round r lowered any label.
        Once a round changes nothing every frontier voxel holds the least linear index of its 26-connected component.  changed:
        an int32 tensor of at least `rounds` elements to reuse.  The workspace is kept across calls.  No host synchronisation:
        the caller decides when to look (isdf_amd.explore.frontiers does)."""
        l, dims = self._route_volume("frontier_relax", "label", label, torch.int32)
        rounds = int(rounds)
        if rounds < 1:
            raise ValueError("frontier_relax: rounds >= 1 (got %d)" % rounds)
        if changed is None:
            changed = torch.empty(rounds, dtype=torch.int32, device=self.device)
        elif changed.dtype != torch.int32 or changed.numel() < rounds or not changed.is_contiguous():
            raise ValueError("frontier_relax: changed must be a contiguous int32 tensor of at least %d elements" % rounds)
        else:
            self._check_device("frontier_relax", "changed", changed)
        ws = self._frontier_ws(dims)
        _ffi.check(self.lib.isdf_frontier_relax(_ffi.ptr(l), dims[0], dims[1], dims[2], _ffi.ptr(ws), int(ws.numel()), rounds,
                                                _ffi.ptr(changed), _stream(self.device)), "isdf_frontier_relax")
        return changed.reshape(-1)[:rounds]

    def frontier_clusters(self, label, max_clusters):
        """(counts int32 [3], records int64 [max_clusters, 12]) on the device: isdf_frontier_clusters -- counts = the number of
        roots (label[p] == p), of frontier voxels, and of orphans (frontier voxels whose label is not a root: 0 on converged
        labels); records, one row per root in ascending order of the root's index, = root, count, sum_i, sum_j, sum_k, min_i,
        min_j, min_k, max_i, max_j, max_k, 0 over the root's voxels.  With more roots than max_clusters the counts are written
        and the records are not (isdf_amd.explore.clusters then calls once more); rows past the number of roots are not written.
        The workspace is kept across calls.  No host synchronisation."""
        l, dims = self._route_volume("frontier_clusters", "label", label, torch.int32)
        max_clusters = int(max_clusters)
        if max_clusters < 0:
            raise ValueError("frontier_clusters: max_clusters >= 0 (got %d)" % max_clusters)
        counts = torch.empty(3, dtype=torch.int32, device=self.device)
        records = torch.empty(max_clusters, _ffi.FRONTIER_RECORD, dtype=torch.int64, device=self.device)
        ws = self._frontier_ws(dims)
        _ffi.check(self.lib.isdf_frontier_clusters(_ffi.ptr(l), dims[0], dims[1], dims[2], _ffi.ptr(ws), int(ws.numel()),
                                                   max_clusters, _ffi.ptr(counts), _addr(records), _stream(self.device)),
                   "isdf_frontier_clusters")
        return counts, records

    def view_gain(self, state, origin, spacing, T_WC, cam, H, W, t_min=0.0, t_max=float("inf"), distinct=True):
        """(unknown int32 [B,H,W], depth float32 [B,H,W], distinct int32 [B] or None) on the device: isdf_view_gain -- for the B
        camera-to-world poses T_WC [B,4,4] one ray per pixel walks the voxels of `state` (contiguous uint8 [nx,ny,nz]; voxel
        (i, j, k) centred at origin + (i, j, k) * spacing) from z-depth t_min to t_max or its first occupied voxel: unknown = the
        UNKNOWN voxels it passes, depth = the z-depth at which it enters the occupied one (0 without), distinct = the number of
        different unknown voxels the rays of a view pass.  A fixed fp32 sequence per ray (include/isdf_hip.h): equal to
        tests/explore_model.py bit for bit.  cam: anything with fx, fy, cx, cy.  The bitmap workspace of `distinct` (one bit per
        voxel and view) is kept across calls.  No host synchronisation."""
        s, dims = self._route_volume("view_gain", "state", state, torch.uint8)
        T = self._flat(torch.as_tensor(T_WC), torch.float32, 16)
        B, H, W = int(T.shape[0]), int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError("view_gain: H and W >= 1 (got %d, %d)" % (H, W))
        o = (C.c_float * 3)(*[float(v) for v in np.asarray(origin, np.float64).reshape(3)])
        sp = (C.c_float * 3)(*[float(v) for v in np.asarray(spacing, np.float64).reshape(3)])
        unknown = torch.empty(B, H, W, dtype=torch.int32, device=self.device)
        depth = torch.empty(B, H, W, dtype=torch.float32, device=self.device)
        count = torch.empty(B, dtype=torch.int32, device=self.device) if distinct else None
        ws = self._scratch("view_gain", int(self.lib.isdf_view_gain_ws_bytes(dims[0], dims[1], dims[2], B))) if distinct and B else None
        _ffi.check(self.lib.isdf_view_gain(_ffi.ptr(s), dims[0], dims[1], dims[2], o, sp, _addr(T), B, float(cam.fx), float(cam.fy),
                                           float(cam.cx), float(cam.cy), H, W, float(t_min), float(t_max), _addr(unknown),
                                           _addr(depth), _addr(count), _ffi.ptr(ws), int(ws.numel()) if ws is not None else 0,
                                           _stream(self.device)), "isdf_view_gain")
        return unknown, depth, count

    # ---- ground truth from a triangle mesh ------------------------------------------------
    def tri_pack(self, vertices, faces, transform=None):
        """(packed f32 [slots, 24], counts i32 [2], m) on the device: isdf_tri_pack, the mesh gathered once into the layout
        isdf_tri_distance reads (include/isdf_hip.h), slot f for face f, padded to the kernel's tile.  vertices [nv,3]; faces
        [m,3] (any integer type; values beyond int32 become -1, a bad index); transform: None or a [3,4] / [4,4] affine applied to
        the vertices first.  counts[0]: faces skipped for an index outside [0, nv) or a non-finite vertex; counts[1]: faces skipped
        for zero fp32 area.  No host synchronisation."""
        v = self._flat(torch.as_tensor(vertices), torch.float32, 3)
        f = torch.as_tensor(faces).detach().to(self.device)
        if f.is_floating_point() or f.dtype == torch.bool:
            raise ValueError("tri_pack: faces must be integers (got %s)" % f.dtype)
        f = f.reshape(-1, 3)
        if f.dtype != torch.int32:
            f = torch.where((f < 0) | (f > 0x7fffffff), torch.full_like(f, -1), f).to(torch.int32)
        f = f.contiguous()
        nv, m = int(v.shape[0]), int(f.shape[0])
        T = None
        if transform is not None:
            A = host_array(transform, np.float32)
            if A.shape not in ((3, 4), (4, 4)):
                raise ValueError("tri_pack: transform must be [3, 4] or [4, 4] (got %s)" % (A.shape,))
            T = (C.c_float * 12)(*[float(x) for x in A[:3].reshape(-1)])
        nbytes = _ffi.tri_packed_bytes(m)
        packed = torch.empty(nbytes // (4 * _ffi.TRI_SLOT_FLOATS), _ffi.TRI_SLOT_FLOATS, dtype=torch.float32, device=self.device)
        counts = torch.empty(2, dtype=torch.int32, device=self.device)
        _ffi.check(self.lib.isdf_tri_pack(_addr(v), nv, _addr(f), m, T, _addr(packed), nbytes, _ffi.ptr(counts),
                                          _stream(self.device)), "isdf_tri_pack")
        return packed, counts, m

    def tri_distance(self, packed, m, pts, want_index=False, want_closest=False, want_winding=False, want_dist=True):
        """(dist [n] f32, index [n] i32, closest [n,3] f32, winding [n] f32, record f64 [4]) on the device, None for what was
        not asked for: isdf_tri_distance, every point of `pts` [n,3] against the `m` faces of `packed` (tri_pack) -- the exact
        distance to the nearest triangle by a fixed fp32 sequence (the lowest face index on ties), the nearest point, and the
        generalised winding number of the mesh around the point.  record: sum of dist over the finite points, their number, the
        number of non-finite points, the largest dist.  The workspace is kept across calls.  No host synchronisation."""
        p = self._flat(torch.as_tensor(pts), torch.float32, 3)
        n, m = int(p.shape[0]), int(m)
        if packed.dtype != torch.float32 or not packed.is_contiguous() or packed.numel() * 4 < _ffi.tri_packed_bytes(m):
            raise ValueError("tri_distance: packed must be the contiguous float32 tensor tri_pack returned for %d faces" % m)
        need = int(self.lib.isdf_tri_ws_bytes(n, m))
        _ffi.check(min(need, 0), "isdf_tri_ws_bytes(%d, %d)" % (n, m))
        ws = self._scratch("tri_distance", need)
        dev = self.device
        dist = torch.empty(n, dtype=torch.float32, device=dev) if want_dist else None
        index = torch.empty(n, dtype=torch.int32, device=dev) if want_index else None
        closest = torch.empty(n, 3, dtype=torch.float32, device=dev) if want_closest else None
        winding = torch.empty(n, dtype=torch.float32, device=dev) if want_winding else None
        record = torch.empty(_ffi.TRI_RECORD, dtype=torch.float64, device=dev)
        _ffi.check(self.lib.isdf_tri_distance(_addr(p), n, _addr(packed) if m else None, m, _addr(dist), _addr(index),
                                              _addr(closest), _addr(winding), _ffi.ptr(record), _ffi.ptr(ws), int(ws.numel()),
                                              _stream(dev)), "isdf_tri_distance")
        return dist, index, closest, winding, record

    def tri_tiles_build(self, packed, m, order):
        """(tiles f64 [n_tiles, 16], order_clean i32 [n_order], counts i32 [2]) on the device: isdf_tri_tiles_build, the flat tile
        index of a packed mesh for tri_distance_tiles.  order: integers [n_order], slot indices into `packed` or -1, padded here with
        -1 to whole tiles; tile t lists entries 256 t .. 256 t + 255.  tiles: per tile the box, area vector, area-weighted centroid,
        radius, area, count and extent of its valid slots (include/isdf_hip.h); order_clean: the entries that name a valid slot, -1
        elsewhere; counts[0]: entries that are neither -1 nor a slot, counts[1]: valid slots listed.  No host synchronisation."""
        m = int(m)
        if packed.dtype != torch.float32 or not packed.is_contiguous() or packed.numel() * 4 < _ffi.tri_packed_bytes(m):
            raise ValueError("tri_tiles_build: packed must be the contiguous float32 tensor tri_pack returned for %d faces" % m)
        o = torch.as_tensor(order).detach().to(self.device)
        if o.is_floating_point() or o.dtype == torch.bool:
            raise ValueError("tri_tiles_build: order must be integers (got %s)" % o.dtype)
        o = o.reshape(-1)
        if o.dtype != torch.int32:                        # beyond int32: no slot either way; -2 is counted as a bad entry
            o = torch.where((o < -1) | (o > 0x7fffffff), torch.full_like(o, -2), o).to(torch.int32)
        pad = -int(o.numel()) % _ffi.TRI_TILE
        if pad:
            o = torch.cat([o, o.new_full((pad,), -1)])
        o = o.contiguous()
        n_order = int(o.numel())
        tiles = torch.empty(n_order // _ffi.TRI_TILE, _ffi.TRI_TILE_RECORD, dtype=torch.float64, device=self.device)
        clean = torch.empty(n_order, dtype=torch.int32, device=self.device)
        counts = torch.empty(2, dtype=torch.int32, device=self.device)
        _ffi.check(self.lib.isdf_tri_tiles_build(_addr(packed) if m else None, m, _addr(o), n_order, _addr(tiles), _addr(clean),
                                                 _ffi.ptr(counts), _stream(self.device)), "isdf_tri_tiles_build")
        return tiles, clean, counts

    def tri_distance_tiles(self, packed, m, tiles, order_clean, pts, qperm=None, beta=0.0, want_index=False, want_closest=False,
                           want_winding=False, want_dist=True, want_stats=False):
        """(dist, index, closest, winding, record, stats) as tri_distance returns them, stats i64 [4] behind (None unless asked
        for): isdf_tri_distance_tiles, the same distance, index, nearest point and record -- bit for bit -- from the tiles of the
        index (tri_tiles_build) that a conservative test against each block of 1024 queries leaves.  winding: tiles farther than
        beta radii from a block add their dipole term instead of their triangles (beta <= 0: none does).  qperm: int32 [n], the
        order in which the queries form blocks; None: a Morton order of the points, non-finite points last (morton_order).
        stats: tiles staged for the distance, tiles staged as near, blocks, qperm entries skipped.  No host synchronisation."""
        p = self._flat(torch.as_tensor(pts), torch.float32, 3)
        n, m, n_tiles = int(p.shape[0]), int(m), int(tiles.shape[0])
        if packed.dtype != torch.float32 or not packed.is_contiguous() or packed.numel() * 4 < _ffi.tri_packed_bytes(m):
            raise ValueError("tri_distance_tiles: packed must be the contiguous float32 tensor tri_pack returned for %d faces" % m)
        if (tiles.dtype != torch.float64 or not tiles.is_contiguous() or tuple(tiles.shape) != (n_tiles, _ffi.TRI_TILE_RECORD)
                or order_clean.dtype != torch.int32 or not order_clean.is_contiguous()
                or order_clean.numel() != n_tiles * _ffi.TRI_TILE):
            raise ValueError("tri_distance_tiles: tiles and order_clean must be the tensors tri_tiles_build returned")
        for what, t in (("packed", packed), ("tiles", tiles), ("order_clean", order_clean)):
            self._check_device("tri_distance_tiles", what, t)
        if qperm is None:
            qperm = morton_order(p)
        qp = self._flat(torch.as_tensor(qperm), torch.int32)
        if int(qp.numel()) != n:
            raise ValueError("tri_distance_tiles: qperm must have one entry per point (got %d for %d)" % (qp.numel(), n))
        need = int(self.lib.isdf_tri_tiles_ws_bytes(n))
        _ffi.check(min(need, 0), "isdf_tri_tiles_ws_bytes(%d)" % n)
        ws = self._scratch("tri_distance", need)
        dev = self.device
        dist = torch.empty(n, dtype=torch.float32, device=dev) if want_dist else None
        index = torch.empty(n, dtype=torch.int32, device=dev) if want_index else None
        closest = torch.empty(n, 3, dtype=torch.float32, device=dev) if want_closest else None
        winding = torch.empty(n, dtype=torch.float32, device=dev) if want_winding else None
        stats = torch.empty(4, dtype=torch.int64, device=dev) if want_stats else None
        record = torch.empty(_ffi.TRI_RECORD, dtype=torch.float64, device=dev)
        _ffi.check(self.lib.isdf_tri_distance_tiles(_addr(p), n, _addr(qp), _addr(packed) if m else None, m, _addr(tiles),
                                                    _addr(order_clean), n_tiles, float(beta), _addr(dist), _addr(index),
                                                    _addr(closest), _addr(winding), _ffi.ptr(record), _ffi.ptr(stats), _ffi.ptr(ws),
                                                    int(ws.numel()), _stream(dev)), "isdf_tri_distance_tiles")
        return dist, index, closest, winding, record, stats

    # ---- frame-to-map pose alignment ---------------------------------------------------
    def _pose_args(self, name, depth, T_WC, cam, frame_of_pose, stride, min_depth, max_depth):
        """(isdf_pose_args, what it points to, B, n_pix): depth [F,H,W] on the device; T_WC [B,4,4] or [B,12] and frame_of_pose [B]
        as HOST arrays (the call checks them entry by entry and hands them on as launch arguments)"""
        if depth.dim() != 3:
            raise ValueError("%s: depth must be [F, H, W] (got %s)" % (name, tuple(depth.shape)))
        F, H, W = (int(v) for v in depth.shape)
        d = self._flat(depth, torch.float32)
        T = host_array(T_WC)
        if T.shape[-2:] == (4, 4):
            T = T.reshape(-1, 4, 4)[:, :3, :]
        elif T.ndim == 0 or T.shape[-1] != 12:
            raise ValueError("%s: T_WC must be [B, 4, 4] or [B, 12] (got %s)" % (name, T.shape))
        T = np.ascontiguousarray(T.reshape(-1, 12), dtype=np.float32)
        B = int(T.shape[0])
        fop = None
        if frame_of_pose is not None:
            fop = np.ascontiguousarray(host_array(frame_of_pose).reshape(-1), dtype=np.int32)
            if fop.size != B:
                raise ValueError("%s: %d poses but %d frame indices" % (name, B, fop.size))
        stride = int(stride)
        a = _ffi.PoseArgs()
        a.B, a.F, a.H, a.W, a.stride = B, F, H, W, stride
        a.fx, a.fy, a.cx, a.cy = float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)
        a.min_depth, a.max_depth = float(min_depth), float(max_depth)
        a.depth = _addr(d)
        a.T_WC = T.ctypes.data if B else None
        a.frame_of_pose = None if fop is None else fop.ctypes.data
        n_pix = (-(-H // stride)) * (-(-W // stride)) if stride >= 1 else 0
        return a, (d, T, fop), B, n_pix

    def pose_points(self, depth, T_WC, cam, frame_of_pose=None, stride=4, min_depth=0.0, max_depth=float("inf")):
        """pts [B * n_pix, 3] f32 on the device: isdf_pose_points, the world point of every stride-th pixel (rows and columns from 0,
        n_pix = ceil(H / stride) * ceil(W / stride), row-major) of the B poses T_WC ([B,4,4] or [B,12], host or device; read on the
        host), pose b against depth[frame_of_pose[b]] (None: depth[b]).  The back-projection of pointcloud_from_depth_torch
        (transform.py:189-190) and the pose, every operation rounded to fp32; a pixel whose depth is not finite, 0, below min_depth or
        above max_depth gets the camera centre.  cam: anything with fx, fy, cx, cy.  No host synchronisation."""
        a, keep, B, n_pix = self._pose_args("pose_points", depth, T_WC, cam, frame_of_pose, stride, min_depth, max_depth)
        pts = torch.empty(B * n_pix, 3, dtype=torch.float32, device=self.device)
        _ffi.check(self.lib.isdf_pose_points(C.byref(a), _addr(pts), _stream(self.device)), "isdf_pose_points")
        return pts

    def pose_system(self, depth, T_WC, cam, pts, sdf, grad, frame_of_pose=None, stride=4, min_depth=0.0, max_depth=float("inf"),
                    huber=0.05, trunc=0.3, out=None, workspace=None):
        """records f64 [B, 32] on the device: isdf_pose_system, per pose the sums of one Gauss-Newton linearisation of the
        point-to-SDF residual r = sdf over the points of `pose_points` with the same arguments -- [0] used points (valid pixel and
        |r| <= trunc), [1] valid pixels, [2] sum w r^2, [3] the Huber cost, [4..9] sum w r J, [10..30] the upper triangle of
        sum w J J^T (row-major), [31] sum |r| -- with w the Huber weight and J = [grad, (x - t) x grad] (include/isdf_hip.h).  All in
        double, summed in a fixed order: the same inputs give the same bytes, whatever else shares the call.  pts [B*n_pix,3],
        sdf [B*n_pix], grad [B*n_pix,3]: device f32.  out: a contiguous float64 [B, 32] to write into; workspace: a uint8 device
        tensor of isdf_pose_ws_bytes(B) or more (None: the engine keeps one).  No host synchronisation."""
        a, keep, B, n_pix = self._pose_args("pose_system", depth, T_WC, cam, frame_of_pose, stride, min_depth, max_depth)
        p, s, g = self._flat(pts, torch.float32, 3), self._flat(sdf, torch.float32), self._flat(grad, torch.float32, 3)
        if not (int(p.shape[0]) == s.numel() == int(g.shape[0]) == B * n_pix):
            raise ValueError("pose_system: %d poses x %d pixels need %d points, sdf values and gradients (got %d, %d, %d)"
                             % (B, n_pix, B * n_pix, p.shape[0], s.numel(), g.shape[0]))
        need = int(self.lib.isdf_pose_ws_bytes(B))
        _ffi.check(min(need, 0), "isdf_pose_ws_bytes(%d)" % B)
        if workspace is None:
            workspace = self._scratch("pose_system", need)
        out = self._record_out("pose_system", out, B, _ffi.POSE_RECORD)
        _ffi.check(self.lib.isdf_pose_system(C.byref(a), _ffi.ptr(p), _ffi.ptr(s), _ffi.ptr(g), float(huber), float(trunc),
                                             _ffi.ptr(out), _ffi.ptr(workspace), int(workspace.numel()), _stream(self.device)),
                   "isdf_pose_system")
        return out

    # ---- planning against the map ------------------------------------------------------
    def _traj_args(self, name, x, offsets, radii):
        """(isdf_traj_args, what it points to, B, T, S): x [B,T,3] f32 on the device, used where it lies (the step writes it);
        offsets [S,3] and radii [S] (or a scalar) as HOST arrays, checked by the call and handed on as launch arguments"""
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[-1] != 3 or x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("%s: x must be a contiguous float32 tensor [B, T, 3]" % name)
        self._check_device(name, "x", x)
        off = np.ascontiguousarray(host_array(offsets, np.float32))
        if off.ndim != 2 or off.shape[1] != 3:
            raise ValueError("%s: offsets must be [S, 3] (got %s)" % (name, off.shape))
        S = int(off.shape[0])
        rad = host_array(radii, np.float32)
        rad = np.ascontiguousarray(np.broadcast_to(rad.reshape(-1), (S,)) if rad.size == 1 else rad.reshape(-1))
        if rad.size != S:
            raise ValueError("%s: %d offsets but %d radii" % (name, S, rad.size))
        B, T = int(x.shape[0]), int(x.shape[1])
        a = _ffi.TrajArgs()
        a.B, a.T, a.S = B, T, S
        a.x = _addr(x)
        a.offsets = off.ctypes.data if S else None
        a.radii = rad.ctypes.data if S else None
        return a, (off, rad), B, T, S

    def _descent_step(self, name, a, var, what, S, state, q, sdf, grad, params, out, q_out, want_grad):
        """what traj_step and arm_step share: the checks of state, of the field values (with q, the points) against B*T*S, of out
        and of q_out; the state and the six parameters into `a`.  var [B,T,K]: x or theta, `what` its name.  Returns (the
        flattened q (if given), sdf and grad, the records, grad_out f64 [B,T,K] or None)."""
        B, T, K = (int(v) for v in var.shape)
        if not torch.is_tensor(state) or state.dtype != torch.int32 or state.numel() != B or not state.is_contiguous() \
                or state.device != var.device:
            raise ValueError("%s: state must be a contiguous int32 tensor [%d] on %s's device" % (name, B, what))
        flat = ([] if q is None else [self._flat(q, torch.float32, 3)]) + [self._flat(sdf, torch.float32), self._flat(grad, torch.float32, 3)]
        n = B * T * S
        if any(int(v.shape[0]) != n for v in flat):
            raise ValueError("%s: %d x %d x %d needs %d %ssdf values and gradients (got %s)"
                             % (name, B, T, S, n, "" if q is None else "points, ", ", ".join(str(int(v.shape[0])) for v in flat)))
        out = self._record_out(name, out, B, _ffi.TRAJ_RECORD, on=var.device)
        if q_out is not None and (q_out.dtype != torch.float32 or q_out.numel() != n * 3 or not q_out.is_contiguous()
                                  or q_out.device != var.device):
            raise ValueError("%s: q_out must be a contiguous float32 tensor of %d x 3 values on %s's device" % (name, n, what))
        a.state = _addr(state)
        a.eps, a.w_obs, a.w_smooth, a.eta, a.max_step, a.tol = (float(v) for v in params)
        return flat, out, torch.empty(B, T, K, dtype=torch.float64, device=self.device) if want_grad else None

    def traj_points(self, x, offsets, radii=0.0):
        """q [B*T*S, 3] f32 on the device: isdf_traj_points, the query points x[b][t] + offsets[s] (one fp32 add per coordinate,
        layout [B][T][S]) of B trajectories of T waypoints whose body is S spheres.  x: contiguous float32 [B,T,3] on the device;
        offsets [S,3], radii [S] or a scalar: host or device, read on the host.  No host synchronisation."""
        a, keep, B, T, S = self._traj_args("traj_points", x, offsets, radii)
        q = torch.empty(B * T * S, 3, dtype=torch.float32, device=self.device)
        _ffi.check(self.lib.isdf_traj_points(C.byref(a), _addr(q), _stream(self.device)), "isdf_traj_points")
        return q

    def traj_step(self, x, state, offsets, radii, sdf, grad, eps=0.2, w_obs=8.0, w_smooth=1.0, eta=8.0, max_step=0.05, tol=1e-5,
                  out=None, q_out=None, want_grad=False):
        """records f64 [B, 16] on the device (and the cost gradient f64 [B,T,3] with want_grad): isdf_traj_step, one iteration of
        covariant gradient descent on B trajectories from the field values sdf [B*T*S] and gradients grad [B*T*S,3] (device f32)
        at `traj_points(x, offsets, radii)`.  x (contiguous float32 [B,T,3]) and state (contiguous int32 [B]: 0 moving,
        1 converged, 2 invalid) are MODIFIED IN PLACE: a moving trajectory takes the step -(1/eta) K^-1 grad, clamped to max_step
        per waypoint, unless a field value is not finite (-> 2) or the step is below tol (-> 1); the others are left bit for
        bit.  Record: [0] F_obs, [1] F_smooth, [2] least clearance, [3] samples in collision, [4] samples within eps, [5] |grad|^2,
        [6] longest waypoint step, [7] the clamp factor applied, [8] non-finite field values, [9] state, [10] path length
        (include/isdf_hip.h).  out: a contiguous float64 [B, 16] to write into; q_out: a contiguous float32 tensor of B*T*S*3
        values that receives the query points of the x the call leaves -- the next field call's input.  One launch, summed
        in a fixed order: the same inputs give the same bytes, whatever else shares the call.  No host synchronisation."""
        a, keep, B, T, S = self._traj_args("traj_step", x, offsets, radii)
        (s, g), out, gout = self._descent_step("traj_step", a, x, "x", S, state, None, sdf, grad,
                                               (eps, w_obs, w_smooth, eta, max_step, tol), out, q_out, want_grad)
        _ffi.check(self.lib.isdf_traj_step(C.byref(a), _addr(s), _addr(g), _ffi.ptr(out),
                                           _ffi.ptr(q_out), _ffi.ptr(gout), _stream(self.device)), "isdf_traj_step")
        return (out, gout) if want_grad else out

    # ---- planning for articulated robots -----------------------------------------------
    def _arm_args(self, name, theta, chain):
        """(isdf_arm_args, what it points to, B, T, J, S): theta [B,T,J] f32 on the device, used where it lies (the step writes
        it); chain: anything with the attributes of isdf_amd.kinematics.Chain (base [3,4], X [J,3,4], kinds [J], axes [J,3],
        links [S], centres [S,3], radii [S], lo / hi [J] or None), read as HOST arrays, checked by the call and handed on as launch
        arguments"""
        if not torch.is_tensor(theta) or theta.dim() != 3 or theta.dtype != torch.float32 or not theta.is_contiguous():
            raise ValueError("%s: theta must be a contiguous float32 tensor [B, T, J]" % name)
        self._check_device(name, "theta", theta)
        B, T, J = (int(v) for v in theta.shape)
        f, i = np.float32, np.int32
        keep = dict(base=np.ascontiguousarray(host_array(chain.base, f)).reshape(-1), X=np.ascontiguousarray(host_array(chain.X, f)).reshape(-1),
                    kinds=np.ascontiguousarray(host_array(chain.kinds, i)).reshape(-1), axes=np.ascontiguousarray(host_array(chain.axes, f)).reshape(-1),
                    links=np.ascontiguousarray(host_array(chain.links, i)).reshape(-1), centres=np.ascontiguousarray(host_array(chain.centres, f)).reshape(-1),
                    radii=np.ascontiguousarray(host_array(chain.radii, f)).reshape(-1))
        for k in ("lo", "hi"):
            v = getattr(chain, k, None)
            if v is not None:
                keep[k] = np.ascontiguousarray(host_array(v, f)).reshape(-1)
        S = int(keep["links"].size)
        want = dict(base=12, X=12 * J, kinds=J, axes=3 * J, links=S, centres=3 * S, radii=S, lo=J, hi=J)
        for k, v in keep.items():
            if v.size != want[k] or v.size == 0:
                raise ValueError("%s: the chain's %s has %d entries; theta's %d joints and %d spheres need %d" % (name, k, v.size, J, S, want[k]))
        a = _ffi.ArmArgs()
        a.B, a.T, a.J, a.S = B, T, J, S
        a.theta = _addr(theta)
        for k, v in keep.items():
            setattr(a, k, v.ctypes.data)
        return a, keep, B, T, J, S

    def arm_points(self, theta, chain):
        """q [B*T*S, 3] f32 on the device: isdf_arm_points, the world centres of the chain's S collision spheres at every
        configuration theta[b][t] (forward kinematics in double, rounded once to fp32; layout [B][T][S]).  theta: contiguous
        float32 [B,T,J] on the device; chain: isdf_amd.kinematics.Chain.  No host synchronisation."""
        a, keep, B, T, J, S = self._arm_args("arm_points", theta, chain)
        q = torch.empty(B * T * S, 3, dtype=torch.float32, device=self.device)
        _ffi.check(self.lib.isdf_arm_points(C.byref(a), _addr(q), _stream(self.device)), "isdf_arm_points")
        return q

    def arm_step(self, theta, state, chain, q, sdf, grad, eps=0.2, w_obs=8.0, w_smooth=1.0, eta=32.0, max_step=0.05, tol=1e-5,
                 out=None, q_out=None, want_grad=False):
        """records f64 [B, 16] on the device (and the cost gradient f64 [B,T,J] with want_grad): isdf_arm_step, one iteration of
        covariant gradient descent on B joint-space trajectories from the field values sdf [B*T*S] and gradients grad [B*T*S,3]
        (device f32) at the query points q [B*T*S,3] = `arm_points(theta, chain)`.  theta (contiguous float32 [B,T,J]) and state
        (contiguous int32 [B]: 0 moving, 1 converged, 2 invalid) are MODIFIED IN PLACE: a moving trajectory takes the step
        -(1/eta) K^-1 grad, projected onto the joint limits and scaled so that no joint moves further than max_step, unless a field
        value is not finite (-> 2) or the step is below tol (-> 1); the others are left bit for bit.  Record: [0] .. [9] as
        `traj_step`, [10] the joint-space path length, [11] the entries of the step a limit cut (include/isdf_hip.h).  out: a
        contiguous float64 [B, 16] to write into; q_out: a contiguous float32 tensor of B*T*S*3 values (it may be q) that
        receives the query points of the theta the call leaves -- the next field call's input.  One launch, summed in a fixed
        order: the same inputs give the same bytes, whatever else shares the call.  No host synchronisation."""
        a, keep, B, T, J, S = self._arm_args("arm_step", theta, chain)
        (p, s, g), out, gout = self._descent_step("arm_step", a, theta, "theta", S, state, q, sdf, grad,
                                                  (eps, w_obs, w_smooth, eta, max_step, tol), out, q_out, want_grad)
        _ffi.check(self.lib.isdf_arm_step(C.byref(a), _addr(p), _addr(s), _addr(g), _ffi.ptr(out), _ffi.ptr(q_out), _ffi.ptr(gout),
                                          _stream(self.device)), "isdf_arm_step")
        return (out, gout) if want_grad else out

    # ---- SDF slice images --------------------------------------------------------------
    def slice_images(self, pts, sdf, cmap=None, volume=None, chomp_eps=None, oob_fill=0.0):
        """(pred_rgb u8 [n,3], gt f32 [n], gt_rgb u8 [n,3], pred_cost f32 [n], gt_cost f32 [n]) on the device, None for what was
        not asked: isdf_slice_images, everything Trainer.compute_slices / obj_slices_vis / get_sdf_grid_pc do after the network
        (trainer.py:1593-1639,1796-1807,1453-1461) in one pass.  sdf [n] (or None: no predicted outputs), pts [n,3] (needed with
        `volume`); cmap: isdf_amd.slices.Colormap (or None: no colours); volume: isdf_amd.metrics.GtVolume (or None: no ground
        truth); chomp_eps: epsilon of the CHOMP cost fields (or None).  No host synchronisation."""
        s = None if sdf is None else self._flat(sdf, torch.float32)
        p = None if pts is None else self._flat(pts, torch.float32, 3)
        if s is None and p is None:
            raise ValueError("slice_images: neither sdf nor pts")
        n = int(s.numel() if s is not None else p.shape[0])
        if s is not None and p is not None and int(p.shape[0]) != n:
            raise ValueError("slice_images: %d points but %d sdf values" % (p.shape[0], n))
        if volume is not None:
            if p is None:
                raise ValueError("slice_images: the ground truth needs the points")
            self._check_device("slice_images", "the ground-truth volume", volume.values)
        cost = chomp_eps is not None

        def out(want, *shape, dtype=torch.float32):
            return torch.empty(*shape, dtype=dtype, device=self.device) if want else None
        pred_rgb = out(s is not None and cmap is not None, n, 3, dtype=torch.uint8)
        pred_cost = out(s is not None and cost, n)
        gt = out(volume is not None, n)
        gt_rgb = out(volume is not None and cmap is not None, n, 3, dtype=torch.uint8)
        gt_cost = out(volume is not None and cost, n)
        if all(t is None for t in (pred_rgb, pred_cost, gt)):
            raise ValueError("slice_images: nothing to compute (no colour map, ground-truth volume or chomp_eps)")
        if n == 0:            # empty tensors have no address to hand over; there is nothing to launch
            return pred_rgb, gt, gt_rgb, pred_cost, gt_cost
        cm = None if cmap is None else cmap.to_c(self.device)
        vol = None if volume is None else volume.to_c()
        _ffi.check(self.lib.isdf_slice_images(_ffi.ptr(p), _ffi.ptr(s), n, None if cm is None else C.byref(cm),
                                              None if vol is None else C.byref(vol), float(oob_fill),
                                              float(chomp_eps) if cost else 0.0, _ffi.ptr(pred_rgb), _ffi.ptr(gt), _ffi.ptr(gt_rgb),
                                              _ffi.ptr(pred_cost), _ffi.ptr(gt_cost), _stream(self.device)), "isdf_slice_images")
        return pred_rgb, gt, gt_rgb, pred_cost, gt_cost

    def plane_points(self, origin, du, dv, H, W):
        """[H, W, 3] on the device: isdf_plane_points, p[i][j] = (origin + i * du) + j * dv with every operation rounded to fp32
        (origin, du, dv: three numbers each, on the host)."""
        H, W = int(H), int(W)
        if H < 0 or W < 0:
            raise ValueError("plane_points: H and W must be >= 0 (got %d, %d)" % (H, W))
        vec = [(C.c_float * 3)(*[float(x) for x in host_array(v, np.float64).reshape(3)]) for v in (origin, du, dv)]
        pts = torch.empty(H, W, 3, dtype=torch.float32, device=self.device)
        _ffi.check(self.lib.isdf_plane_points(vec[0], vec[1], vec[2], H, W, _ffi.ptr(pts), _stream(self.device)),
                   "isdf_plane_points")
        return pts

    # ---- AdamW ----------------------------------------------------------------------
    def adamw(self, lr=ADAMW_LR, weight_decay=ADAMW_WEIGHT_DECAY, betas=ADAMW_BETAS, eps=ADAMW_EPS, grad_scale=1.0,
              use_device_count=True):
        """torch.optim.AdamW.step on the flat buffer (trainer.py:435-439,982); the
        summed gradient is divided by the (all-reduced) element count on device."""
        self.opt_step += 1
        cnt = self.reduce_buf[self.n_params + _ffi.LS_COUNT:] if use_device_count else None
        _ffi.check(self.lib.isdf_adamw(C.byref(self.cnet), _ffi.ptr(self.params), _ffi.ptr(self.exp_avg),
                                       _ffi.ptr(self.exp_avg_sq), _ffi.ptr(self.reduce_buf), _ffi.ptr(cnt),
                                       float(grad_scale), float(lr), float(betas[0]), float(betas[1]),
                                       float(eps), float(weight_decay), int(self.opt_step),
                                       _ffi.ptr(self.shadow), _stream(self.device)), "isdf_adamw")
