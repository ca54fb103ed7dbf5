"""numpy restatement of the rendered views (`isdf_render_views`, include/isdf_hip.h): the depth-range sources, stratified
samples, first crossing and camera-frame normals of Trainer.render_depth_vis / render_normals_vis / latest_frame_vis
(trainer.py:1055-1147,1225-1280; sample.py:77-178; render.py:12-57).  fp32 operation by operation, no contraction, so the
samples agree with the kernel to the last bit or two.  tests/test_render_cpu.py pins it to the reference's own functions.

`cv_resize_linear` states OpenCV's documented INTER_LINEAR mapping (src = (dst + 0.5) * scale - 0.5, clamped at the borders,
no antialiasing) as the kernel does; cv2 itself is not available to the tests, so agreement with real cv2 is unverified."""
import numpy as np

f32 = np.float32


def _cv_taps(n_dst, n_src):
    scale = 1.0 / (float(n_dst) / float(n_src))
    x = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(f32)
    s = np.floor(x).astype(np.int64)
    f = (x - s.astype(f32)).astype(f32)
    f[s < 0] = 0
    s[s < 0] = 0
    hi = s >= n_src - 1
    f[hi] = 0
    s[hi] = n_src - 1
    return s, np.minimum(s + 1, n_src - 1), f


def _ac_taps(n_dst, n_src):
    scale = f32(n_src - 1) / f32(n_dst - 1) if n_dst > 1 else f32(0)
    x = (f32(scale) * np.arange(n_dst, dtype=f32)).astype(f32)
    s = np.minimum(np.floor(x).astype(np.int64), n_src - 1)
    f = np.clip((x - s.astype(f32)).astype(f32), 0, 1).astype(f32)
    return s, np.where(s < n_src - 1, s + 1, s), f


def _bilerp(img, ys, xs):
    y0, y1, fy = ys
    x0, x1, fx = xs
    img = np.asarray(img, f32)
    ax, ay = (f32(1) - fx).astype(f32), (f32(1) - fy).astype(f32)
    r0 = (img[y0][:, x0] * ax + img[y0][:, x1] * fx).astype(f32)
    r1 = (img[y1][:, x0] * ax + img[y1][:, x1] * fx).astype(f32)
    return (r0 * ay[:, None] + r1 * fy[:, None]).astype(f32)


def cv_resize_linear(img, W, H):
    """cv2.resize(img, (W, H)) with the default INTER_LINEAR, for a 2-D float32 image"""
    h, w = img.shape
    return _bilerp(img, _cv_taps(H, h), _cv_taps(W, w))


def upsample_align_corners(img, H, W):
    """F.interpolate(img[None, None], size=[H, W], mode='bilinear', align_corners=True)[0, 0]"""
    h, w = img.shape
    return _bilerp(img, _ac_taps(H, h), _ac_taps(W, w))


def _linspace01(S):
    k = np.arange(S, dtype=np.int64)
    stp = f32(1) / f32(S)
    lo = (stp * k.astype(f32)).astype(f32)
    hi = (f32(1) - (stp * (S - k).astype(f32)).astype(f32)).astype(f32)
    return np.where(k < (S + 1) // 2, lo, hi).astype(f32)


def z_scalar(min_depth, max_depth, U):
    """stratified_sample with scalar [min, max] (sample.py:106-114): torch.linspace(min, max, S + 1), bin_length a double"""
    S = U.shape[-1]
    lo, hi = f32(min_depth), f32(max_depth)
    step = f32((hi - lo) / f32(S))
    k = np.arange(S, dtype=np.int64)
    lim = np.where(k < (S + 1) // 2, (lo + (step * k.astype(f32)).astype(f32)).astype(f32),
                   (hi - (step * (S - k).astype(f32)).astype(f32)).astype(f32)).astype(f32)
    blen = f32((float(max_depth) - float(min_depth)) / S)
    return (lim[None, :] + (U.astype(f32) * blen).astype(f32)).astype(f32)


def z_ranged(lo, hi, U):
    """stratified_sample with per-ray max (and min) tensors (sample.py:94-105)"""
    S = U.shape[-1]
    lo = np.broadcast_to(np.asarray(lo, f32), hi.shape).astype(f32)
    rng = (hi.astype(f32) - lo).astype(f32)
    lim = ((_linspace01(S)[None, :] * rng[:, None]).astype(f32) + lo[:, None]).astype(f32)
    blen = (rng / f32(S)).astype(f32)
    return (lim + (U.astype(f32) * blen[:, None]).astype(f32)).astype(f32)


def origin_dirs_W(T, dirs_C):
    """transform.origin_dirs_W for one pose: (R * d).sum(-1) left to right"""
    T = np.asarray(T, f32)
    d = np.asarray(dirs_C, f32).reshape(-1, 3)
    R = T[:3, :3]
    dW = ((R[None, :, 0] * d[:, 0:1]).astype(f32) + (R[None, :, 1] * d[:, 1:2]).astype(f32)).astype(f32)
    dW = (dW + (R[None, :, 2] * d[:, 2:3]).astype(f32)).astype(f32)
    return T[:3, 3].copy(), dW


def points(T, dirs_C, z):
    """pc = origins + dirs_W * z (sample.py:176); z [R, S] -> [R, S, 3], or [R] -> [R, 3]"""
    o, dW = origin_dirs_W(T, dirs_C)
    if z.ndim == 1:
        return (o[None, :] + (dW * z[:, None]).astype(f32)).astype(f32)
    return (o[None, None, :] + (dW[:, None, :] * z[:, :, None]).astype(f32)).astype(f32)


def first_crossing(z, sdf):
    """index of the crossing sample the library renders: the first negative sample in z order (stable), sample 0 of that order
    without one (render.py:19-31 on z-sorted samples, as isdf_render_depth does it)"""
    order = np.argsort(z, axis=1, kind="stable")
    zs, ss = np.take_along_axis(z, order, 1), np.take_along_axis(sdf, order, 1)
    neg = ss < 0
    k = np.where(neg.any(1), neg.argmax(1), 0)
    return order[np.arange(len(z)), k], k == z.shape[1] - 1


def render_depth(z, sdf):
    """render.sdf_render_depth on z-ordered samples: depth = z + sdf at the crossing, 0 if it is the last sample"""
    c, last = first_crossing(z, sdf)
    r = np.arange(len(z))
    d = (z[r, c] + sdf[r, c]).astype(f32)
    d[last] = 0
    return d


def normals_C(T, grad):
    """render.render_normals' tail (render.py:51-55): R_CW = inverse(R_WC) (general, float64 rounded to fp32),
    n_C = R_CW (-g / (|g| + 1e-4))"""
    g = np.asarray(grad, f32)
    Rinv = np.linalg.inv(np.asarray(T, np.float64)[:3, :3]).astype(f32)
    den = (np.sqrt((g * g).sum(-1, dtype=f32)).astype(f32) + f32(1e-4)).astype(f32)
    nW = (-g / den[:, None]).astype(f32)
    return (nW @ Rinv.T.astype(np.float64)).astype(f32)
