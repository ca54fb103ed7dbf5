"""CPU-side checks of the joint-space planning entry points (include/isdf_hip.h): exported, the ABI version unchanged, the constants
the header's, and every invalid argument refused before anything is launched."""
import ctypes as C

import numpy as np
import pytest

from isdf_amd import _ffi, build

ARM = ["isdf_arm_points", "isdf_arm_step"]
EINVAL = -1
ADDR = 0x1000          # a placeholder device address: a refused call dereferences none of them
INF, NAN = float("inf"), float("nan")
HOST = ("base", "X", "kinds", "axes", "links", "centres", "radii", "lo", "hi")


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _ffi.lib()


def test_symbols_exported_version_kept_and_constants_as_in_the_header(lib):
    for fn in ARM:
        assert fn in _ffi.SYMBOLS and hasattr(lib, fn), fn
    assert lib.isdf_abi_version() == _ffi.ABI_VERSION == 8
    assert (_ffi.ARM_MAX_JOINTS, _ffi.ARM_MAX_SPHERES, _ffi.ARM_MAX_TRAJ, _ffi.TRAJ_RECORD) == (8, 64, 131072, 16)
    assert _ffi.ARM_MAX_WAYPOINTS == 384 >= 256
    # the LDS the header derives the waypoint limit from: 2 J doubles per waypoint inside 48 KB
    assert 2 * _ffi.ARM_MAX_JOINTS * _ffi.ARM_MAX_WAYPOINTS * 8 == 48 * 1024


def _host(**edit):
    """the host arrays of a valid chain of J = 3 joints and S = 2 spheres, sized for the largest chain; edit: name -> (flat
    index, value) or name -> array"""
    eye = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)
    h = dict(base=eye.copy(), X=np.tile(eye, (8, 1, 1)), kinds=np.array([0, 1, 0, 0, 0, 0, 0, 0], np.int32),
             axes=np.tile(np.array([0.0, 0.0, 1.0], np.float32), (8, 1)), links=np.zeros(64, np.int32),
             centres=np.zeros((64, 3), np.float32), radii=np.full(64, 0.1, np.float32), lo=np.full(8, -1.0, np.float32),
             hi=np.full(8, 1.0, np.float32))
    h["links"][1] = 3
    for k, v in edit.items():
        if isinstance(v, tuple):
            h[k].reshape(-1)[v[0]] = v[1]
        else:
            h[k] = v
    return h


def _args(host=None, null=(), **kw):
    """valid arguments for B = 2 trajectories of T = 8 configurations (host arrays real, device addresses placeholders)"""
    a = _ffi.ArmArgs()
    a.B, a.T, a.J, a.S = 2, 8, 3, 2
    a.eps, a.w_obs, a.w_smooth, a.eta, a.max_step, a.tol = 0.2, 8.0, 1.0, 32.0, 0.05, 1e-5
    a.theta, a.state = ADDR, ADDR
    host = _host() if host is None else host
    for k in HOST:
        setattr(a, k, None if k in null else host[k].ctypes.data)
    for k, v in kw.items():
        setattr(a, k, v)
    a._keep = host
    return a


def _points(lib, a, q=ADDR):
    return lib.isdf_arm_points(None if a is None else C.byref(a), q, None)


def _step(lib, a, q=ADDR, sdf=ADDR, grad=ADDR, rec=ADDR):
    return lib.isdf_arm_step(None if a is None else C.byref(a), q, sdf, grad, rec, None, None, None)


def _calls(lib, a):
    """both calls on arguments that are NOT valid (a valid call would launch on the placeholder addresses)"""
    return [_points(lib, a), _step(lib, a)]


@pytest.mark.parametrize("bad", [dict(B=0), dict(B=-1), dict(B=131073), dict(T=2), dict(T=0), dict(T=-3), dict(T=385), dict(J=0), dict(J=-1),
                                 dict(J=9), dict(S=0), dict(S=-1), dict(S=65), dict(B=131072, T=384, S=64), dict(theta=None)])
def test_invalid_sizes_are_einval_in_both_calls(lib, bad):
    assert _calls(lib, _args(**bad)) == [EINVAL] * 2


@pytest.mark.parametrize("name", HOST[:7])
def test_a_null_chain_array_is_einval(lib, name):
    assert _calls(lib, _args(null=(name,))) == [EINVAL] * 2


def test_null_pointers_are_einval(lib):
    assert _calls(lib, None) == [EINVAL] * 2
    assert _points(lib, _args(), q=None) == EINVAL
    assert _step(lib, _args(state=None)) == EINVAL
    for name in ("q", "sdf", "grad", "rec"):
        assert _step(lib, _args(), **{name: None}) == EINVAL, name


@pytest.mark.parametrize("edit", [dict(kinds=(0, 2)), dict(kinds=(2, -1)), dict(links=(0, -1)), dict(links=(1, 4)), dict(links=(0, 9))])
def test_a_kind_outside_0_1_or_a_link_outside_0_J_is_einval(lib, edit):
    assert _calls(lib, _args(_host(**edit))) == [EINVAL] * 2


@pytest.mark.parametrize("axis", [(0.0, 0.0, 1.00002), (0.0, 0.0, 0.99998), (0.0, 0.0, 0.0), (1.0, 1.0, 0.0), (NAN, 0.0, 1.0), (INF, 0.0, 0.0)])
@pytest.mark.parametrize("joint", [0, 2])
def test_an_axis_that_is_not_a_unit_vector_is_einval(lib, joint, axis):
    """|u|^2 in float32 further than 1e-5 from 1 (1.00002^2 = 1.00004, 0.99998^2 = 0.99996)"""
    axes = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (8, 1))
    axes[joint] = axis
    assert _calls(lib, _args(_host(axes=axes))) == [EINVAL] * 2


@pytest.mark.parametrize("name,entry", [("base", 0), ("base", 11), ("X", 3), ("X", 35), ("centres", 0), ("centres", 5)])
@pytest.mark.parametrize("value", [NAN, INF, -INF])
def test_a_non_finite_transform_or_centre_is_einval(lib, name, entry, value):
    assert _calls(lib, _args(_host(**{name: (entry, value)}))) == [EINVAL] * 2


@pytest.mark.parametrize("sphere", [0, 1])
@pytest.mark.parametrize("value", [NAN, INF, -INF, -0.1])
def test_a_negative_or_non_finite_radius_is_einval(lib, sphere, value):
    assert _calls(lib, _args(_host(radii=(sphere, value)))) == [EINVAL] * 2


@pytest.mark.parametrize("edit", [dict(lo=(1, 2.0)), dict(hi=(2, -2.0)), dict(lo=(0, NAN)), dict(hi=(0, NAN)), dict(lo=(2, INF)),
                                  dict(hi=(1, -INF))])
def test_a_limit_pair_out_of_order_or_nan_is_einval(lib, edit):
    """lo = +inf above hi = 1 and hi = -inf below lo = -1 are out of order too"""
    assert _calls(lib, _args(_host(**edit))) == [EINVAL] * 2
    # one array alone is checked against the other side's infinity
    assert _calls(lib, _args(_host(lo=(0, NAN)), null=("hi",))) == [EINVAL] * 2
    assert _calls(lib, _args(_host(hi=(0, NAN)), null=("lo",))) == [EINVAL] * 2


@pytest.mark.parametrize("kw", [dict(eps=0.0), dict(eps=-0.2), dict(eps=NAN), dict(eps=INF), dict(eta=0.0), dict(eta=-8.0), dict(eta=NAN),
                                dict(eta=INF), dict(max_step=0.0), dict(max_step=-0.05), dict(max_step=NAN), dict(max_step=-INF),
                                dict(w_obs=-1.0), dict(w_obs=NAN), dict(w_obs=INF), dict(w_smooth=-1.0), dict(w_smooth=NAN),
                                dict(w_smooth=INF), dict(tol=-1e-5), dict(tol=NAN), dict(tol=INF)])
def test_bad_parameters_are_einval_in_the_step(lib, kw):
    assert _step(lib, _args(**kw)) == EINVAL
