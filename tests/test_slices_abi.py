"""C ABI of the slice entry points: the built library exports isdf_slice_images / isdf_plane_points, the host vectors of the
latter are bound as float pointers, bad arguments are refused before anything is launched, and the ABI version is still 8 (no GPU
needed).  Their types, isdf_colormap's layout and the size macro are held to the header by tests/test_abi.py."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from isdf_amd import _ffi, build
    build.build(verbose=False)
    return _ffi.lib()


def test_header_declares_library_exports_and_ffi_binds_with_matching_types(lib):
    from isdf_amd import _ffi
    P, i32, f32, vp = C.POINTER, C.c_int32, C.c_float, C.c_void_p
    for fn in ("isdf_slice_images", "isdf_plane_points"):
        assert fn in _ffi.SYMBOLS and hasattr(lib, fn)
    assert len(lib.isdf_slice_images.argtypes) == 13
    # the three host vectors of isdf_plane_points are bound as float pointers (ctypes arrays of three floats are passed)
    assert list(lib.isdf_plane_points.argtypes) == [P(f32)] * 3 + [i32, i32, vp, vp]
    assert (_ffi.COLORMAP_MAX_COLORS + 3) * 4 == 65536     # the table fills 64 KiB of LDS


def test_abi_version_is_still_8(lib):
    from isdf_amd import _ffi
    assert lib.isdf_abi_version() == 8 == _ffi.ABI_VERSION


def test_argument_checks_refuse_before_any_launch(lib):
    from isdf_amd import _ffi
    cm = _ffi.ColormapArgs()
    cm.lut, cm.n_colors, cm.vmin, cm.range = 16, 401, -2.0, 4.0
    v = _ffi.GtVolumeArgs()
    v.values, v.nx, v.ny, v.nz = 16, 4, 4, 4
    for k in range(3):
        v.spacing[k], v.origin[k] = 0.1, 0.0

    def call(pts=16, sdf=16, n=8, cmap=cm, vol=v, eps=2.0, pred_rgb=16, gt=16, gt_rgb=16, pred_cost=16, gt_cost=16):
        return lib.isdf_slice_images(pts, sdf, n, None if cmap is None else C.byref(cmap), None if vol is None else C.byref(vol),
                                     0.0, eps, pred_rgb, gt, gt_rgb, pred_cost, gt_cost, None)
    none = dict(pred_rgb=None, gt=None, gt_rgb=None, pred_cost=None, gt_cost=None)
    assert call(n=-1) == -1 and call(**none) == -1                              # a negative count; nothing to write
    assert call(sdf=None) == -1 and call(pts=None) == -1                      # an output without its input
    assert call(vol=None) == -1 and call(cmap=None) == -1
    assert call(eps=0.0) == -1 and call(eps=-1.0) == -1 and call(eps=float("nan")) == -1
    only_pred = dict(none, pred_rgb=16)
    assert call(sdf=None, **only_pred) == -1 and call(cmap=None, **only_pred) == -1
    assert call(vol=None, **dict(none, gt=16)) == -1 and call(pts=None, vol=v, **dict(none, gt=16)) == -1
    assert call(eps=0.0, **dict(none, pred_cost=16)) == -1
    for field, value in (("n_colors", 0), ("n_colors", _ffi.COLORMAP_MAX_COLORS + 1), ("range", 0.0), ("range", -1.0),
                         ("range", float("inf")), ("range", float("nan")), ("vmin", float("nan")), ("lut", None)):
        bad = _ffi.ColormapArgs.from_buffer_copy(cm)
        setattr(bad, field, value)
        assert call(cmap=bad) == -1, (field, value)
    for field, value in (("nx", 1), ("values", None)):
        bad = _ffi.GtVolumeArgs.from_buffer_copy(v)
        setattr(bad, field, value)
        assert call(vol=bad) == -1, (field, value)
    bad = _ffi.GtVolumeArgs.from_buffer_copy(v)
    bad.spacing[2] = 0.0
    assert call(vol=bad) == -1
    assert call(n=0) == 0                                                       # nothing to do, nothing launched
    assert call(n=0, **none) == -1                                              # ... but still a call that asks for nothing

    F3 = C.c_float * 3
    o, du, dv = F3(0, 0, 0), F3(1, 0, 0), F3(0, 1, 0)
    pp = lib.isdf_plane_points
    assert pp(None, du, dv, 4, 4, 16, None) == -1 and pp(o, None, dv, 4, 4, 16, None) == -1 and pp(o, du, None, 4, 4, 16, None) == -1
    assert pp(o, du, dv, -1, 4, 16, None) == -1 and pp(o, du, dv, 4, -1, 16, None) == -1 and pp(o, du, dv, 4, 4, None, None) == -1
    assert pp(o, du, dv, 1 << 16, 1 << 15, 16, None) == -1                      # H * W beyond 2^31 - 1
    assert pp(o, du, dv, 0, 4, None, None) == 0 and pp(o, du, dv, 4, 0, None, None) == 0
