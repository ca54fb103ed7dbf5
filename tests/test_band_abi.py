"""CPU-side checks of the narrow-band entry points (include/isdf_hip.h): exported, the ABI version unchanged, the workspace size
as documented, and every invalid argument refused before anything is launched."""
import ctypes as C
import math

import pytest

from isdf_amd import _ffi, build

BAND = ["isdf_band_ws_bytes", "isdf_band_begin", "isdf_band_select", "isdf_band_emit", "isdf_band_update", "isdf_band_leaks",
        "isdf_grid_points"]
EINVAL, EWORKSPACE = -1, -3


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _ffi.lib()


def test_symbols_exported_and_version_kept(lib):
    for fn in BAND:
        assert fn in _ffi.SYMBOLS and hasattr(lib, fn), fn
    assert lib.isdf_abi_version() == _ffi.ABI_VERSION == 8


def _ws_formula(D0, D1, D2, coarse):
    """the comment above isdf_band_ws_bytes, written out"""
    up = lambda x: (x + 255) // 256 * 256
    total, s = 0, 2
    while s <= coarse:
        total += up(math.ceil((D0 - 1) / s) * math.ceil((D1 - 1) / s) * math.ceil((D2 - 1) / s))
        s *= 2
    nb = math.ceil(D0 * D1 * D2 / 256)
    return total + up(8 * nb) + up(16 * nb) + 256


@pytest.mark.parametrize("dims", [(2, 2, 2), (5, 3, 9), (37, 64, 50), (129, 129, 129), (1024, 1024, 1024)])
@pytest.mark.parametrize("coarse", [2, 8, 32])
def test_ws_bytes_matches_its_documented_formula(lib, dims, coarse):
    assert lib.isdf_band_ws_bytes(*dims, coarse) == _ws_formula(*dims, coarse)


def test_ws_bytes_refuses_bad_dims_and_strides(lib):
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 1), (2048, 1024, 1024)):
        assert lib.isdf_band_ws_bytes(*dims, 8) == EINVAL
    for coarse in (0, 1, 3, 6, 12, -8):
        assert lib.isdf_band_ws_bytes(8, 8, 8, coarse) == EINVAL


def _args(**kw):
    a = _ffi.BandArgs()
    a.D0, a.D1, a.D2, a.coarse, a.level, a.slack = 8, 8, 8, 8, 0.0, 1.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _calls(lib, a, stride=8, vol=0x1000, counts=0x1000, ws=0x1000, wsn=1 << 30, out=0x1000, n=4):
    """every entry point that takes isdf_band_args, with placeholder addresses: a refused call dereferences none of them"""
    p = None if a is None else C.byref(a)
    return [lib.isdf_band_begin(p, vol, None),
            lib.isdf_band_select(p, stride, vol, counts, ws, wsn, None),
            lib.isdf_band_emit(p, stride, vol, out, out, n, ws, wsn, None),
            lib.isdf_band_update(p, stride, vol, out, out, n, counts, ws, wsn, None),
            lib.isdf_band_leaks(p, vol, counts, ws, wsn, None)]


@pytest.mark.parametrize("bad", [dict(D0=0), dict(D1=-3), dict(D2=1), dict(D0=2048, D1=1024, D2=1024), dict(coarse=0), dict(coarse=1),
                                 dict(coarse=6), dict(coarse=-8), dict(slack=-0.5), dict(slack=float("inf")), dict(slack=float("nan")),
                                 dict(level=float("nan"))])
def test_invalid_args_are_einval_everywhere(lib, bad):
    assert _calls(lib, _args(**bad)) == [EINVAL] * 5


def test_null_pointers_and_bad_strides_are_einval(lib):
    assert _calls(lib, None) == [EINVAL] * 5
    assert _calls(lib, _args(), vol=None) == [EINVAL] * 5
    rc = _calls(lib, _args(), counts=None)
    assert rc[1] == rc[3] == rc[4] == EINVAL                          # select, update (stride > 1) and leaks report through counts
    rc = _calls(lib, _args(), out=None)
    assert rc[2] == rc[3] == EINVAL                                   # emit's lists, update's index and values
    for stride in (0, 3, 16, -2):
        rc = _calls(lib, _args(), stride=stride)
        assert rc[1:4] == [EINVAL] * 3, stride
    assert lib.isdf_band_emit(C.byref(_args()), 8, 0x1000, 0x1000, 0x1000, -1, 0x1000, 1 << 30, None) == EINVAL
    bad_affine = _args(has_transform=1)
    bad_affine.index_to_world[5] = float("nan")
    assert _calls(lib, bad_affine) == [EINVAL] * 5
    A = (C.c_float * 12)(*([1.0] * 12))
    assert lib.isdf_grid_points(0, 4, 4, A, 0x1000, None) == EINVAL
    assert lib.isdf_grid_points(4, 4, 4, None, 0x1000, None) == EINVAL
    assert lib.isdf_grid_points(4, 4, 4, A, None, None) == EINVAL


def test_missing_or_small_workspace_is_eworkspace(lib):
    need = lib.isdf_band_ws_bytes(8, 8, 8, 8)
    for ws, wsn in ((None, need), (0x1000, need - 1)):
        rc = _calls(lib, _args(), ws=ws, wsn=wsn)
        assert rc[1:] == [EWORKSPACE] * 4, (ws, wsn)
    assert lib.isdf_band_emit(C.byref(_args()), 8, 0x1000, None, None, 0, None, 0, None) == 0        # an empty list is a no-op
