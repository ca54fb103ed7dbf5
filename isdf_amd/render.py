"""Rendered views on the device: `isdf_render_views` (include/isdf_hip.h), the depth / normal renders of the reference's
`Trainer.render_depth_vis`, `render_normals_vis` and `latest_frame_vis` (trainer.py:1055-1147,1225-1280) for all views of a
call in ONE pass: samples, forward, first crossing and, optionally, camera-frame normals at the rendered or a given depth.

    depth, normals = Renderer(engine)(T_WC, dirs_C, H, W, n_samples, depth_images=..., min_depth=..., depth_offset=0.8)

The range source is one of: `scalar_range=(min, max)` (coarse pass of latest_frame_vis), `depth_images` [B, h, w] with
`min_depth` / `depth_offset` (render_depth_vis: max = cv2.resize(depth, INTER_LINEAR) + 0.8) or `upsample` [B, h, w] with
`depth_offset` (fine pass of latest_frame_vis: d +- 0.1 around the align-corners upsample of the coarse depth); or
`depth` [B, R] given (render_normals_vis: normals only).  Uniforms: `draws` [B, R, S] (torch's, parity) or in-kernel Philox
keyed by (seed, counter)."""
import ctypes as C

import numpy as np
import torch

from . import _ffi
from .engine import _stream, to_host


class Renderer:
    """Caller-side state of `isdf_render_views` on one engine: the workspace, kept (and only grown) across calls."""

    def __init__(self, engine):
        self.engine = engine
        self.lib = engine.lib
        self._ws = None
        self.calls = 0           # native render calls so far

    def _workspace(self, B, H, W, S):
        nb = self.lib.isdf_render_ws_bytes(C.byref(self.engine.cnet), B, H, W, S)
        _ffi.check(min(nb, 0), "isdf_render_ws_bytes(%d, %d, %d, %d)" % (B, H, W, S))
        if self._ws is None or self._ws.numel() < nb:
            self._ws = torch.empty(int(nb), dtype=torch.uint8, device=self.engine.device)
        return self._ws

    def samples(self, B, H, W, S):
        """(z_vals [B, R, S], pc [B, R, S, 3]) of the last call that rendered (views into the workspace, overwritten by the next)"""
        n = B * H * W * S
        f = self._ws.view(torch.float32)
        pc_off = ((4 * n + 255) // 256) * 64
        return f[:n].view(B, H * W, S), f[pc_off:pc_off + 3 * n].view(B, H * W, S, 3)

    def __call__(self, T_WC, dirs_C, H, W, n_samples=0, scalar_range=None, depth_images=None, min_depth=0.0, upsample=None,
                 depth_offset=0.0, draws=None, seed=0, counter=0, depth=None, want_depth=True, want_normals=False):
        eng, dev = self.engine, self.engine.device
        f32 = lambda t: None if t is None else t.detach().to(device=dev, dtype=torch.float32).contiguous()
        T = f32(T_WC).reshape(-1, 4, 4)
        B, R = int(T.shape[0]), int(H) * int(W)
        d_C = f32(dirs_C).reshape(R, 3)
        a = _ffi.RenderArgs()
        a.n_views, a.H, a.W, a.n_samples = B, int(H), int(W), int(n_samples)
        a.T_WC, a.dirs_C = T.data_ptr(), d_C.data_ptr()
        keep = [T, d_C]
        if depth is not None:
            depth = f32(depth).reshape(B, R)
            keep.append(depth)
            a.depth_in, a.n_samples = depth.data_ptr(), 1
            want_depth, want_normals = False, True
        else:
            if scalar_range is not None:
                lo, hi = (float(v) for v in scalar_range)
                a.range_mode, a.min_depth, a.max_depth = _ffi.RANGE_SCALAR, lo, hi
                a.bin_length = (hi - lo) / int(n_samples)          # a Python double, rounded to fp32 like torch's scalar operand
            else:
                src = f32(depth_images if depth_images is not None else upsample)
                a.range_mode = _ffi.RANGE_DEPTH if depth_images is not None else _ffi.RANGE_UPSAMPLE
                a.src_H, a.src_W = int(src.shape[-2]), int(src.shape[-1])
                a.src_depth, a.min_depth, a.depth_offset = src.data_ptr(), float(min_depth), float(depth_offset)
                keep.append(src)
            if draws is not None:
                u = f32(draws).reshape(B, R, int(n_samples))
                keep.append(u)
                a.rng_mode, a.draw_u = 0, u.data_ptr()
            else:
                a.rng_mode, a.seed, a.counter = 1, int(seed), int(counter)
        out_d = torch.empty(B, R, dtype=torch.float32, device=dev) if want_depth else None
        out_n = torch.empty(B, R, 3, dtype=torch.float32, device=dev) if want_normals else None
        ws = self._workspace(B, a.H, a.W, a.n_samples)
        _ffi.check(self.lib.isdf_render_views(C.byref(eng.cnet), _ffi.ptr(eng.params), _ffi.ptr(eng.shadow), C.byref(a),
                                              _ffi.ptr(out_d), _ffi.ptr(out_n), _ffi.ptr(ws), ws.numel(), _stream(dev)),
                   "isdf_render_views")
        self.calls += 1
        return out_d, out_n


class RenderMethods:
    """The trainer-level half (trainer.py:1055-1147,1225-1280): a base class of hot_path.HotPath; `self` is the grafted Trainer."""

    def _render_rng(self, B, R, S):
        """uniforms of one render pass: rng "torch" draws torch.rand(R, S) per view on the trainer's device, in the reference's
        order (sample.py:123) -> dict(draws=[B, R, S]); "philox" advances the render counter (visualisation only: not part of
        hip_state_dict) and leaves the torch generator alone"""
        hip = self._hip
        if hip.rng == "torch":
            return dict(draws=torch.stack([torch.rand(R, S, device=self.device) for _ in range(B)]))
        hip.render_count += 1
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
            render_depth, normals = to_host(fine.reshape(Hu, Wu), normals.reshape(Hu, Wu, 3))
        render_depth_viz = ref.imgviz.depth2rgb(render_depth, min_value=self.min_depth, max_value=self.max_depth)
        normals_viz = (normals * 255).astype(np.uint8)
        render_vis = np.hstack((normals_viz, render_depth_viz))
        render_vis = ref.cv2.resize(render_vis, (int(render_vis.shape[1] * 2), int(render_vis.shape[0] * 2)))
        elapsed = ref.end_timing(start, end)
        print("Time for depth and normal render", elapsed)
        return rgbd_vis, render_vis, T_WC_np
