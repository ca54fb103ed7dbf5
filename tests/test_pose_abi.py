"""CPU-side checks of the pose-alignment entry points (include/isdf_hip.h): exported, the ABI version unchanged, the workspace size
as documented, and every invalid argument refused before anything is launched."""
import ctypes as C

import numpy as np
import pytest

from isdf_amd import _ffi, build

POSE = ["isdf_pose_ws_bytes", "isdf_pose_points", "isdf_pose_system"]
EINVAL, EWORKSPACE = -1, -3
ADDR = 0x1000          # a placeholder device address: a refused call dereferences none of them


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _ffi.lib()


def test_symbols_exported_and_version_kept(lib):
    for fn in POSE:
        assert fn in _ffi.SYMBOLS and hasattr(lib, fn), fn
    assert lib.isdf_abi_version() == _ffi.ABI_VERSION == 8


@pytest.mark.parametrize("B", [1, 3, 20, 65536])
def test_ws_bytes_matches_its_documented_formula(lib, B):
    assert lib.isdf_pose_ws_bytes(B) == B * _ffi.POSE_MAX_BLOCKS * _ffi.POSE_RECORD * 8 == B * 64 * 32 * 8


def test_ws_bytes_refuses_bad_counts(lib):
    for B in (0, -1, 65537):
        assert lib.isdf_pose_ws_bytes(B) == EINVAL


def _args(T=None, fop=None, **kw):
    """valid arguments for B = 2 poses on F = 3 frames of 48 x 64 (host arrays real, device addresses placeholders)"""
    a = _ffi.PoseArgs()
    a.B, a.F, a.H, a.W, a.stride = 2, 3, 48, 64, 4
    a.fx, a.fy, a.cx, a.cy, a.min_depth, a.max_depth = 60.0, 60.0, 31.5, 23.5, 0.0, float("inf")
    a.depth = ADDR
    T = np.tile(np.eye(4, dtype=np.float32)[:3].reshape(1, 12), (2, 1)) if T is None else T
    a.T_WC = T.ctypes.data
    if fop is not None:
        a.frame_of_pose = fop.ctypes.data
    for k, v in kw.items():
        setattr(a, k, v)
    a._keep = (T, fop)
    return a


def _calls(lib, a, pts=ADDR, sdf=ADDR, grad=ADDR, huber=0.05, trunc=0.3, rec=ADDR, ws=ADDR, wsn=1 << 30, out=ADDR):
    p = None if a is None else C.byref(a)
    return [lib.isdf_pose_points(p, out, None), lib.isdf_pose_system(p, pts, sdf, grad, huber, trunc, rec, ws, wsn, None)]


INF, NAN = float("inf"), float("nan")


@pytest.mark.parametrize("bad", [dict(B=0), dict(B=-2), dict(B=65537), dict(F=0), dict(H=0), dict(W=-1), dict(H=65536, W=65536),
                                 dict(stride=0), dict(stride=-4), dict(fx=0.0), dict(fy=0.0), dict(fx=NAN), dict(fy=INF), dict(cx=NAN),
                                 dict(cy=-INF), dict(min_depth=1.0, max_depth=0.5), dict(min_depth=NAN), dict(max_depth=NAN),
                                 dict(depth=None), dict(T_WC=None), dict(B=3, F=2)])
def test_invalid_args_are_einval_in_both_calls(lib, bad):
    assert _calls(lib, _args(**bad)) == [EINVAL] * 2


def test_null_pointers_are_einval(lib):
    assert _calls(lib, None) == [EINVAL] * 2
    assert _calls(lib, _args(), out=None)[0] == EINVAL
    for name in ("pts", "sdf", "grad", "rec"):
        assert _calls(lib, _args(), **{name: None})[1] == EINVAL, name


@pytest.mark.parametrize("entry", [0, 7, 23])
@pytest.mark.parametrize("value", [NAN, INF, -INF])
def test_a_non_finite_pose_entry_is_einval(lib, entry, value):
    T = np.tile(np.eye(4, dtype=np.float32)[:3].reshape(1, 12), (2, 1))
    T.reshape(-1)[entry] = value
    assert _calls(lib, _args(T=T)) == [EINVAL] * 2


def test_frame_indices_outside_the_batch_are_einval(lib):
    for fop in ([0, 3], [-1, 0], [2, 1 << 20]):
        assert _calls(lib, _args(fop=np.asarray(fop, np.int32))) == [EINVAL] * 2, fop
    # in range: the system call gets as far as its workspace check (nothing is launched by either line)
    assert lib.isdf_pose_system(C.byref(_args(fop=np.asarray([2, 2], np.int32))), ADDR, ADDR, ADDR, 0.05, 0.3, ADDR, None, 0, None) \
        == EWORKSPACE


@pytest.mark.parametrize("kw", [dict(huber=0.0), dict(huber=-0.05), dict(huber=NAN), dict(huber=INF), dict(trunc=0.0), dict(trunc=-1.0),
                                dict(trunc=NAN), dict(trunc=INF)])
def test_bad_huber_or_trunc_is_einval(lib, kw):
    assert _calls(lib, _args(), **kw)[1] == EINVAL


def test_missing_or_small_workspace_is_eworkspace(lib):
    need = lib.isdf_pose_ws_bytes(2)
    for ws, wsn in ((None, need), (ADDR, need - 1), (ADDR, 0)):
        assert _calls(lib, _args(), ws=ws, wsn=wsn)[1] == EWORKSPACE, (ws, wsn)
