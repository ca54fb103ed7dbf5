"""CPU-side checks of the exploration entry points (include/isdf_hip.h): exported, the ABI version unchanged, the constants and the
two size queries as documented, and every invalid argument refused before anything is launched (host code only)."""
import ctypes as C

import pytest

from isdf_amd import _ffi, build

EXPLORE = ["isdf_frontier_init", "isdf_frontier_ws_bytes", "isdf_frontier_relax", "isdf_frontier_clusters", "isdf_view_gain_ws_bytes",
           "isdf_view_gain"]
EINVAL, EWORKSPACE = -1, -3
ADDR = 0x1000          # a placeholder device address: a refused call dereferences none of them
MAXV = 1 << 27
BAD_DIMS = [(0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (4, -3, 4), (4, 4, -2), (1, 1, MAXV + 1), (MAXV + 1, 1, 1), (1024, 1024, 129),
            (513, 512, 512), (65536, 65536, 65536), (1 << 30, 1 << 30, 4), (2147483647, 2147483647, 2147483647)]
NAN, INF = float("nan"), float("inf")
up = lambda x: (x + 255) // 256 * 256


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _ffi.lib()


def test_symbols_exported_version_kept_and_constants_as_in_the_header(lib):
    for fn in EXPLORE:
        assert fn in _ffi.SYMBOLS and hasattr(lib, fn), fn
    assert _ffi.SYMBOLS[-len(EXPLORE):] == EXPLORE                       # in the header's order, after routing
    assert lib.isdf_abi_version() == _ffi.ABI_VERSION == 8
    assert (_ffi.VOXEL_UNKNOWN, _ffi.VOXEL_FREE, _ffi.VOXEL_OCCUPIED) == (0, 1, 2)
    assert _ffi.FRONTIER_NONE == 1 << 30 > _ffi.ROUTE_MAX_VOXELS and _ffi.FRONTIER_RECORD == 12      # no voxel index reaches NONE


def test_the_two_size_queries(lib):
    for dims in ((1, 1, 1), (1, 1, 40), (9, 10, 11), (33, 2, 3), (17, 17, 17), (256, 256, 256), (512, 512, 512), (1, 1, MAXV), (MAXV, 1, 1)):
        n = dims[0] * dims[1] * dims[2]
        assert lib.isdf_frontier_ws_bytes(*dims) == up(4 * n) + up(4 * ((n + 255) // 256)), dims
        for B in (0, 1, 5, 64):
            assert lib.isdf_view_gain_ws_bytes(*dims, B) == up(4 * B * ((n + 31) // 32)), (dims, B)
    assert lib.isdf_view_gain_ws_bytes(33, 2, 3, 5) == 256 and lib.isdf_view_gain_ws_bytes(256, 256, 256, 256) == 512 << 20
    for dims in BAD_DIMS:
        assert lib.isdf_frontier_ws_bytes(*dims) == EINVAL and lib.isdf_view_gain_ws_bytes(*dims, 1) == EINVAL, dims
    assert lib.isdf_view_gain_ws_bytes(9, 10, 11, -1) == EINVAL


def test_frontier_init_refusals(lib):
    call = lambda state=ADDR, dims=(9, 10, 11), label=ADDR: lib.isdf_frontier_init(state, *dims, label, None)
    for bad in [dict(state=None), dict(label=None)] + [dict(dims=d) for d in BAD_DIMS]:
        assert call(**bad) == EINVAL, bad


def _relax(lib, label=ADDR, dims=(9, 10, 11), ws=ADDR, ws_bytes=None, rounds=2, changed=ADDR):
    ws_bytes = lib.isdf_frontier_ws_bytes(9, 10, 11) if ws_bytes is None else ws_bytes
    return lib.isdf_frontier_relax(label, *dims, ws, ws_bytes, rounds, changed, None)


def test_frontier_relax_refusals(lib):
    for bad in [dict(label=None), dict(changed=None), dict(rounds=0), dict(rounds=-1), dict(rounds=0, ws=None)] \
            + [dict(dims=d, ws_bytes=1 << 62) for d in BAD_DIMS]:
        assert _relax(lib, **bad) == EINVAL, bad
    need = lib.isdf_frontier_ws_bytes(9, 10, 11)
    assert need == 4096 + 256
    for bad in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws_bytes=-1), dict(dims=(9, 10, 12))):
        assert _relax(lib, **bad) == EWORKSPACE, bad


def _clusters(lib, label=ADDR, dims=(9, 10, 11), ws=ADDR, ws_bytes=None, max_clusters=4, counts=ADDR, records=ADDR):
    ws_bytes = lib.isdf_frontier_ws_bytes(9, 10, 11) if ws_bytes is None else ws_bytes
    return lib.isdf_frontier_clusters(label, *dims, ws, ws_bytes, max_clusters, counts, records, None)


def test_frontier_clusters_refusals(lib):
    for bad in [dict(label=None), dict(counts=None), dict(records=None), dict(max_clusters=-1), dict(max_clusters=-1, records=None)] \
            + [dict(dims=d, ws_bytes=1 << 62) for d in BAD_DIMS]:
        assert _clusters(lib, **bad) == EINVAL, bad
    need = lib.isdf_frontier_ws_bytes(9, 10, 11)
    for bad in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(max_clusters=0, records=None, ws=None),
                dict(dims=(9, 10, 12))):
        assert _clusters(lib, **bad) == EWORKSPACE, bad


def _gain(lib, state=ADDR, dims=(9, 10, 11), origin=(0.3, -0.2, -0.4), spacing=(0.1, 0.07, 0.13), T=ADDR, B=3, fx=4.0, fy=4.0, cx=2.0,
          cy=3.0, H=7, W=5, t_min=0.0, t_max=INF, unknown=ADDR, depth=ADDR, distinct=ADDR, ws=ADDR, ws_bytes=None):
    ws_bytes = lib.isdf_view_gain_ws_bytes(9, 10, 11, 3) if ws_bytes is None else ws_bytes
    o = None if origin is None else (C.c_float * 3)(*origin)
    s = None if spacing is None else (C.c_float * 3)(*spacing)
    return lib.isdf_view_gain(state, *dims, o, s, T, B, fx, fy, cx, cy, H, W, t_min, t_max, unknown, depth, distinct, ws, ws_bytes, None)


def test_view_gain_refusals(lib):
    bad_args = [dict(state=None), dict(origin=None), dict(spacing=None), dict(T=None), dict(unknown=None), dict(depth=None),
                dict(B=-1), dict(H=0), dict(W=0), dict(H=-3), dict(W=-1), dict(H=65536, W=32768), dict(B=1 << 20, H=1 << 10, W=1 << 10),
                dict(spacing=(0.1, 0.0, 0.13)), dict(spacing=(-0.1, 0.07, 0.13)), dict(spacing=(0.1, 0.07, NAN)),
                dict(spacing=(INF, 0.07, 0.13)), dict(origin=(NAN, 0.0, 0.0)), dict(origin=(0.0, -INF, 0.0)),
                dict(fx=0.0), dict(fy=0.0), dict(fx=-0.0), dict(fx=NAN), dict(fy=INF), dict(cx=NAN), dict(cy=-INF),
                dict(t_min=-0.1), dict(t_min=NAN), dict(t_min=INF), dict(t_max=0.0), dict(t_min=1.0, t_max=1.0), dict(t_min=2.0, t_max=1.0),
                dict(t_max=NAN), dict(t_max=-INF)]
    for bad in bad_args + [dict(dims=d, ws_bytes=1 << 62) for d in BAD_DIMS]:
        assert _gain(lib, **bad) == EINVAL, bad
    need = lib.isdf_view_gain_ws_bytes(9, 10, 11, 3)
    assert need == 512
    for bad in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws_bytes=-1), dict(B=5)):
        assert _gain(lib, **bad) == EWORKSPACE, bad
    # B = 0 is a no-op that needs neither poses, outputs nor a workspace; it launches nothing
    assert _gain(lib, B=0, T=None, unknown=None, depth=None, distinct=None, ws=None, ws_bytes=0) == 0
    assert _gain(lib, B=0, ws=None, ws_bytes=0) == 0
