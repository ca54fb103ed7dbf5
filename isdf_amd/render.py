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

import torch

from . import _ffi


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
        from .engine import _stream
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
