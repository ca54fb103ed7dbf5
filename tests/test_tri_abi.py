"""CPU-side checks of the triangle-mesh entry points (include/isdf_hip.h): exported, the ABI version unchanged, the size queries
as their formulas, and every invalid argument refused before anything is launched."""
import ctypes as C

import pytest

from isdf_amd import _ffi, build

TRI = ["isdf_tri_pack", "isdf_tri_ws_bytes", "isdf_tri_distance"]
EINVAL, EWORKSPACE = -1, -3
ADDR = 0x1000          # a placeholder device address: a refused call dereferences none of them
BIG = 1 << 30
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _ffi.lib()


def test_symbols_exported_and_version_kept(lib):
    for fn in TRI:
        assert fn in _ffi.SYMBOLS and hasattr(lib, fn), fn
    assert lib.isdf_abi_version() == _ffi.ABI_VERSION == 8


def _splits(n, m):
    """the header's C(n, m)"""
    ceil = lambda a, b: -(-a // b)
    t = ceil(m, _ffi.TRI_TILE)
    if t == 0:
        return 1
    c = min(max(ceil(1024, ceil(n, 1024)) if n else 1, 1), t, 65535)
    return ceil(t, ceil(t, c))


def test_ws_bytes_and_packed_bytes(lib):
    for n, m in ((0, 0), (1, 1), (1, 255), (8, 100000), (1023, 256), (1024, 257), (1025, 515), (4000, 996), (1 << 20, 100000),
                 (5, BIG), (BIG, 7), (BIG, BIG)):
        assert lib.isdf_tri_ws_bytes(n, m) == 8 * n * (1 + _splits(n, m)) + 32 * ((n + 255) // 256) + 256, (n, m)
    assert _splits(8, 100000) == 391 and _splits(1 << 20, 100000) == 1 and _splits(4000, 996) == 4
    for n, m in ((-1, 4), (4, -1), (BIG + 1, 4), (4, BIG + 1)):
        assert lib.isdf_tri_ws_bytes(n, m) == EINVAL, (n, m)
    assert [_ffi.tri_packed_bytes(m) for m in (0, 1, 256, 257)] == [0, 24576, 24576, 49152]


def _pack(lib, vertices=ADDR, nv=10, faces=ADDR, m=12, transform=None, packed=ADDR, packed_bytes=None, counts=ADDR):
    T = None if transform is None else (C.c_float * 12)(*transform)
    packed_bytes = _ffi.tri_packed_bytes(12) if packed_bytes is None else packed_bytes
    return lib.isdf_tri_pack(vertices, nv, faces, m, T, packed, packed_bytes, counts, None)


def test_pack_refusals(lib):
    for bad in (dict(vertices=None), dict(faces=None), dict(packed=None), dict(counts=None), dict(nv=-1), dict(m=-1),
                dict(nv=BIG + 1), dict(m=BIG + 1, packed_bytes=1 << 62)):
        assert _pack(lib, **bad) == EINVAL, bad
    eye = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    for k in range(12):
        for v in (NAN, INF, -INF):
            T = list(eye)
            T[k] = v
            assert _pack(lib, transform=T) == EINVAL, (k, v)
    assert _pack(lib, packed_bytes=_ffi.tri_packed_bytes(12) - 1) == EWORKSPACE and _pack(lib, packed_bytes=0) == EWORKSPACE
    assert _pack(lib, m=257, packed_bytes=_ffi.tri_packed_bytes(256)) == EWORKSPACE
    assert _pack(lib, packed_bytes=-1) == EWORKSPACE


def _dist(lib, pts=ADDR, n=100, packed=ADDR, m=12, record=ADDR, ws=ADDR, ws_bytes=None):
    ws_bytes = lib.isdf_tri_ws_bytes(100, 12) if ws_bytes is None else ws_bytes
    return lib.isdf_tri_distance(pts, n, packed, m, ADDR, ADDR, ADDR, ADDR, record, ws, ws_bytes, None)


def test_distance_refusals(lib):
    for bad in (dict(pts=None), dict(packed=None), dict(record=None), dict(n=-1), dict(m=-1), dict(n=BIG + 1, ws_bytes=1 << 62),
                dict(m=BIG + 1, ws_bytes=1 << 62)):
        assert _dist(lib, **bad) == EINVAL, bad
    assert _dist(lib, ws=None) == EWORKSPACE
    assert _dist(lib, ws_bytes=lib.isdf_tri_ws_bytes(100, 12) - 1) == EWORKSPACE and _dist(lib, ws_bytes=0) == EWORKSPACE
    # the workspace grows with the number of chunks: what fits one tile does not fit three
    assert _dist(lib, m=600, ws_bytes=lib.isdf_tri_ws_bytes(100, 12)) == EWORKSPACE
    # record is required even when nothing else is asked for and there is nothing to do
    assert lib.isdf_tri_distance(None, 0, None, 0, None, None, None, None, None, ADDR, 1 << 20, None) == EINVAL
