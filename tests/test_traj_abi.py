"""CPU-side checks of the planning entry points (include/isdf_hip.h): exported, the ABI version unchanged, and every invalid
argument refused before anything is launched."""
import ctypes as C

import numpy as np
import pytest

from isdf_amd import _ffi, build

TRAJ = ["isdf_traj_points", "isdf_traj_step"]
EINVAL = -1
ADDR = 0x1000          # a placeholder device address: a refused call dereferences none of them
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _ffi.lib()


def test_symbols_exported_and_version_kept(lib):
    for fn in TRAJ:
        assert fn in _ffi.SYMBOLS and hasattr(lib, fn), fn
    assert lib.isdf_abi_version() == _ffi.ABI_VERSION == 8
    assert (_ffi.TRAJ_RECORD, _ffi.TRAJ_MAX_WAYPOINTS, _ffi.TRAJ_MAX_SPHERES, _ffi.TRAJ_MAX_TRAJ) == (16, 1024, 32, 65536)


def _args(off=None, rad=None, **kw):
    """valid arguments for B = 2 trajectories of T = 8 waypoints and S = 2 spheres (host arrays real, device addresses placeholders)"""
    a = _ffi.TrajArgs()
    a.B, a.T, a.S = 2, 8, 2
    a.eps, a.w_obs, a.w_smooth, a.eta, a.max_step, a.tol = 0.2, 8.0, 1.0, 8.0, 0.05, 1e-5
    a.x, a.state = ADDR, ADDR
    off = np.zeros((32, 3), np.float32) if off is None else off
    rad = np.full(32, 0.1, np.float32) if rad is None else rad
    a.offsets, a.radii = off.ctypes.data, rad.ctypes.data
    for k, v in kw.items():
        setattr(a, k, v)
    a._keep = (off, rad)
    return a


def _points(lib, a, q=ADDR):
    return lib.isdf_traj_points(None if a is None else C.byref(a), q, None)


def _step(lib, a, sdf=ADDR, grad=ADDR, rec=ADDR):
    return lib.isdf_traj_step(None if a is None else C.byref(a), sdf, grad, rec, None, None, None)


def _calls(lib, a):
    """both calls on arguments that are NOT valid (a valid call would launch on the placeholder addresses)"""
    return [_points(lib, a), _step(lib, a)]


@pytest.mark.parametrize("bad", [dict(B=0), dict(B=-1), dict(B=65537), dict(T=2), dict(T=0), dict(T=-3), dict(T=1025), dict(S=0), dict(S=-1),
                                 dict(S=33), dict(B=65536, T=1024, S=32), dict(x=None), dict(offsets=None),
                                 dict(radii=None)])
def test_invalid_sizes_and_null_pointers_are_einval_in_both_calls(lib, bad):
    assert _calls(lib, _args(**bad)) == [EINVAL] * 2


def test_null_pointers_are_einval(lib):
    assert _calls(lib, None) == [EINVAL] * 2
    assert _points(lib, _args(), q=None) == EINVAL
    assert _step(lib, _args(state=None)) == EINVAL
    for name in ("sdf", "grad", "rec"):
        assert _step(lib, _args(), **{name: None}) == EINVAL, name


@pytest.mark.parametrize("entry", [0, 4, 5])
@pytest.mark.parametrize("value", [NAN, INF, -INF])
def test_a_non_finite_offset_is_einval(lib, entry, value):
    off = np.zeros((32, 3), np.float32)
    off.reshape(-1)[entry] = value
    assert _calls(lib, _args(off=off)) == [EINVAL] * 2


@pytest.mark.parametrize("sphere", [0, 1])
@pytest.mark.parametrize("value", [NAN, INF, -INF, -0.1])
def test_a_negative_or_non_finite_radius_is_einval(lib, sphere, value):
    rad = np.full(32, 0.1, np.float32)
    rad[sphere] = value
    assert _calls(lib, _args(rad=rad)) == [EINVAL] * 2


@pytest.mark.parametrize("kw", [dict(eps=0.0), dict(eps=-0.2), dict(eps=NAN), dict(eps=INF), dict(eta=0.0), dict(eta=-8.0), dict(eta=NAN),
                                dict(eta=INF), dict(max_step=0.0), dict(max_step=-0.05), dict(max_step=NAN), dict(max_step=-INF),
                                dict(w_obs=-1.0), dict(w_obs=NAN), dict(w_obs=INF), dict(w_smooth=-1.0), dict(w_smooth=NAN),
                                dict(w_smooth=INF), dict(tol=-1e-5), dict(tol=NAN), dict(tol=INF)])
def test_bad_parameters_are_einval_in_the_step(lib, kw):
    assert _step(lib, _args(**kw)) == EINVAL
