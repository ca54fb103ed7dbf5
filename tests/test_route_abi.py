"""CPU-side checks of the routing entry points (include/isdf_hip.h): exported, the ABI version unchanged, the constants and the
size query as documented, and every invalid argument refused before anything is launched (host code only)."""
import pytest

from isdf_amd import _ffi, build

ROUTE = ["isdf_route_init", "isdf_route_ws_bytes", "isdf_route_relax", "isdf_route_trace"]
EINVAL, EWORKSPACE = -1, -3
ADDR = 0x1000          # a placeholder device address: a refused call dereferences none of them
MAXV = 1 << 27
BAD_DIMS = [(0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (4, -3, 4), (4, 4, -2), (1, 1, MAXV + 1), (MAXV + 1, 1, 1), (1024, 1024, 129),
            (513, 512, 512), (65536, 65536, 65536), (1 << 30, 1 << 30, 4), (2147483647, 2147483647, 2147483647)]


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _ffi.lib()


def test_symbols_exported_version_kept_and_constants_as_in_the_header(lib):
    for fn in ROUTE:
        assert fn in _ffi.SYMBOLS and hasattr(lib, fn), fn
    assert lib.isdf_abi_version() == _ffi.ABI_VERSION == 8
    assert _ffi.ROUTE_NONE == 1 << 30 and _ffi.ROUTE_MAX_VOXELS == MAXV and _ffi.ROUTE_TILE >= 2
    assert 5 * _ffi.ROUTE_MAX_VOXELS < _ffi.ROUTE_NONE and _ffi.ROUTE_NONE + 5 < 1 << 31      # nothing saturates, nothing wraps


def test_ws_bytes(lib):
    for dims in ((1, 1, 1), (1, 1, 40), (9, 10, 11), (17, 17, 17), (60, 30, 50), (256, 256, 256), (512, 512, 512), (1, 1, MAXV),
                 (MAXV, 1, 1), (1024, 1024, 128)):
        n = dims[0] * dims[1] * dims[2]
        assert lib.isdf_route_ws_bytes(*dims) == (4 * n + 255) // 256 * 256, dims
    for dims in BAD_DIMS:
        assert lib.isdf_route_ws_bytes(*dims) == EINVAL, dims


def _init(lib, free=ADDR, dims=(9, 10, 11), goals=ADDR, n_goals=3, dist=ADDR):
    return lib.isdf_route_init(free, dims[0], dims[1], dims[2], goals, n_goals, dist, None)


def test_init_refusals(lib):
    for bad in [dict(free=None), dict(dist=None), dict(goals=None), dict(goals=None, n_goals=1), dict(n_goals=-1),
                dict(n_goals=-1, goals=None)] + [dict(dims=d) for d in BAD_DIMS]:
        assert _init(lib, **bad) == EINVAL, bad


def _relax(lib, free=ADDR, dims=(9, 10, 11), dist=ADDR, ws=ADDR, ws_bytes=None, rounds=2, changed=ADDR):
    ws_bytes = lib.isdf_route_ws_bytes(9, 10, 11) if ws_bytes is None else ws_bytes
    return lib.isdf_route_relax(free, dims[0], dims[1], dims[2], dist, ws, ws_bytes, rounds, changed, None)


def test_relax_refusals(lib):
    for bad in [dict(free=None), dict(dist=None), dict(changed=None), dict(rounds=0), dict(rounds=-1), dict(rounds=0, ws=None)] \
            + [dict(dims=d, ws_bytes=1 << 62) for d in BAD_DIMS]:
        assert _relax(lib, **bad) == EINVAL, bad
    need = lib.isdf_route_ws_bytes(9, 10, 11)
    assert need == 4096
    for bad in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws_bytes=-1),
                dict(dims=(9, 10, 12))):               # one more plane no longer fits what the smaller grid needs
        assert _relax(lib, **bad) == EWORKSPACE, bad


def _trace(lib, dist=ADDR, dims=(9, 10, 11), starts=ADDR, B=2, max_len=16, path=ADDR, length=ADDR):
    return lib.isdf_route_trace(dist, dims[0], dims[1], dims[2], starts, B, max_len, path, length, None)


def test_trace_refusals(lib):
    for bad in [dict(dist=None), dict(starts=None), dict(path=None), dict(length=None), dict(B=-1), dict(max_len=0),
                dict(max_len=-5)] + [dict(dims=d) for d in BAD_DIMS]:
        assert _trace(lib, **bad) == EINVAL, bad
