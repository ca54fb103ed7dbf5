"""CPU-side checks of the voxel-baseline entry points (include/isdf_hip.h): exported, the ABI version unchanged, and every
invalid argument refused before anything is launched."""
import ctypes as C

import pytest

from isdf_amd import _ffi, build

FUSION = ["isdf_tsdf_integrate", "isdf_edt_ws_bytes", "isdf_distance_transform", "isdf_occupancy_sdf"]
EINVAL, EWORKSPACE = -1, -3
ADDR = 0x1000          # a placeholder device address: a refused call dereferences none of them
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _ffi.lib()


def test_symbols_exported_and_version_kept(lib):
    for fn in FUSION:
        assert fn in _ffi.SYMBOLS and hasattr(lib, fn), fn
    assert lib.isdf_abi_version() == _ffi.ABI_VERSION == 8
    assert b"workspace" in lib.isdf_error_string(EWORKSPACE)
    assert (_ffi.EDT_NONE, _ffi.EDT_MAX_SIDE) == (1 << 30, 1024)


def _args(origin=None, spacing=None, **kw):
    """valid arguments for 3 frames of 48 x 64 into a 5 x 6 x 7 volume (device addresses are placeholders)"""
    a = _ffi.TsdfArgs()
    a.nx, a.ny, a.nz, a.F, a.H, a.W = 5, 6, 7, 3, 48, 64
    a.origin[:] = [0.0, 0.0, 0.0] if origin is None else origin
    a.spacing[:] = [0.1, 0.1, 0.1] if spacing is None else spacing
    a.fx, a.fy, a.cx, a.cy = 60.0, 60.0, 31.5, 23.5
    a.trunc, a.max_weight, a.min_depth, a.max_depth = 0.3, INF, 0.0, INF
    a.depth = a.T_CW = a.tsdf = a.weight = ADDR
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _integrate(lib, a):
    return lib.isdf_tsdf_integrate(None if a is None else C.byref(a), None)


@pytest.mark.parametrize("bad", [dict(nx=0), dict(ny=0), dict(nz=-1), dict(nx=2048, ny=1024, nz=1024), dict(nx=65536, ny=65536, nz=1),
                                 dict(F=-1), dict(H=0), dict(W=0), dict(H=65536, W=32768),
                                 dict(depth=None), dict(T_CW=None), dict(tsdf=None), dict(weight=None),
                                 dict(fx=NAN), dict(fy=INF), dict(cx=-INF), dict(cy=NAN),
                                 dict(trunc=0.0), dict(trunc=-0.3), dict(trunc=NAN), dict(trunc=INF),
                                 dict(max_weight=0.5), dict(max_weight=NAN), dict(max_weight=-INF),
                                 dict(min_depth=NAN), dict(min_depth=-0.1)])
def test_invalid_integrate_arguments_are_einval(lib, bad):
    assert _integrate(lib, _args(**bad)) == EINVAL


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("value", [0.0, -0.1, NAN, INF])
def test_a_bad_spacing_is_einval(lib, axis, value):
    s = [0.1, 0.1, 0.1]
    s[axis] = value
    assert _integrate(lib, _args(spacing=s)) == EINVAL


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("value", [NAN, INF, -INF])
def test_a_non_finite_origin_is_einval(lib, axis, value):
    o = [0.0, 0.0, 0.0]
    o[axis] = value
    assert _integrate(lib, _args(origin=o)) == EINVAL


def test_null_args_and_the_empty_call(lib):
    assert _integrate(lib, None) == EINVAL
    # F = 0 is a no-op that reads nothing: no frame pointer is needed, nothing is launched on the placeholder volumes
    assert _integrate(lib, _args(F=0, depth=None, T_CW=None)) == 0
    assert _integrate(lib, _args(F=0, max_weight=1.0, max_depth=0.0)) == 0
    assert _integrate(lib, _args(F=0, tsdf=None)) == EINVAL


def test_edt_ws_bytes(lib):
    up = lambda x: (x + 255) // 256 * 256
    for dims in ((1, 1, 1), (12, 9, 7), (1, 1, 70), (1024, 2, 2), (1024, 1024, 1024)):
        assert lib.isdf_edt_ws_bytes(*dims) == 2 * up(4 * dims[0] * dims[1] * dims[2]), dims
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (1025, 2, 2), (2, 1025, 2), (2, 2, 1025)):
        assert lib.isdf_edt_ws_bytes(*dims) == EINVAL, dims


def _edt(lib, feature=ADDR, dims=(12, 9, 7), out=ADDR, ws=ADDR, ws_bytes=None):
    ws_bytes = lib.isdf_edt_ws_bytes(12, 9, 7) if ws_bytes is None else ws_bytes
    return lib.isdf_distance_transform(feature, dims[0], dims[1], dims[2], 0, out, ws, ws_bytes, None)


def _occ(lib, occ=ADDR, dims=(12, 9, 7), voxel=0.05, out=ADDR, ws=ADDR, ws_bytes=None):
    ws_bytes = lib.isdf_edt_ws_bytes(12, 9, 7) if ws_bytes is None else ws_bytes
    return lib.isdf_occupancy_sdf(occ, dims[0], dims[1], dims[2], voxel, out, ws, ws_bytes, None)


@pytest.mark.parametrize("call", [_edt, _occ])
def test_transform_refusals(lib, call):
    big = 1 << 40
    for dims in ((0, 9, 7), (12, -1, 7), (12, 9, 0), (1025, 2, 2), (2, 1025, 2), (2, 2, 1025)):
        assert call(lib, dims=dims, ws_bytes=big) == EINVAL, dims
    assert call(lib, None) == EINVAL and call(lib, out=None) == EINVAL
    assert call(lib, ws=None) == EWORKSPACE
    assert call(lib, ws_bytes=lib.isdf_edt_ws_bytes(12, 9, 7) - 1) == EWORKSPACE and call(lib, ws_bytes=0) == EWORKSPACE


@pytest.mark.parametrize("voxel", [0.0, -0.05, NAN, INF])
def test_a_bad_voxel_size_is_einval(lib, voxel):
    assert _occ(lib, voxel=voxel) == EINVAL
