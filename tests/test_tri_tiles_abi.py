"""CPU-side checks of the tile-index entry points (include/isdf_hip.h: isdf_tri_tiles_build, isdf_tri_tiles_ws_bytes,
isdf_tri_distance_tiles): exported and bound with the header's argument lists, the ABI version unchanged, the size query as its
formula, and every invalid argument refused before anything is launched."""
import pytest

from isdf_amd import _ffi, build
from tests import abi_util as au

TILES = {"isdf_tri_tiles_build": 8, "isdf_tri_tiles_ws_bytes": 1, "isdf_tri_distance_tiles": 18}
EINVAL, EWORKSPACE = -1, -3
ADDR = 0x1000          # a placeholder device address: a refused call dereferences none of them
BIG = 1 << 30
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _ffi.lib()


def test_symbols_argument_counts_and_version(lib):
    declared = au.prototypes()
    names = list(declared)
    # in header order, directly behind the brute-force call
    assert names[names.index("isdf_tri_distance") + 1:][:3] == list(TILES)
    for fn, n_args in TILES.items():
        assert fn in _ffi.SYMBOLS and hasattr(lib, fn), fn
        assert len(declared[fn][1]) == n_args == len(_ffi.PROTOTYPES[fn][1]), fn
    assert lib.isdf_abi_version() == _ffi.ABI_VERSION == 8
    assert _ffi.TRI_TILE_RECORD == 16 and "ISDF_TRI_TILE_EPS" in au.constant_names()


def test_ws_bytes(lib):
    for n in (0, 1, 255, 256, 257, 1023, 1024, 1025, 4096, 1 << 20, BIG):
        assert lib.isdf_tri_tiles_ws_bytes(n) == 16 * n + 32 * ((n + 255) // 256) + 256, n
    assert lib.isdf_tri_tiles_ws_bytes(-1) == EINVAL and lib.isdf_tri_tiles_ws_bytes(BIG + 1) == EINVAL
    # one winding partial whatever the mesh: never more than the brute-force workspace
    assert lib.isdf_tri_tiles_ws_bytes(100) == lib.isdf_tri_ws_bytes(100, 12) < lib.isdf_tri_ws_bytes(100, 600)


def _build(lib, packed=ADDR, m=12, order=ADDR, n_order=256, tiles=ADDR, clean=ADDR, counts=ADDR):
    return lib.isdf_tri_tiles_build(packed, m, order, n_order, tiles, clean, counts, None)


def test_build_refusals(lib):
    for bad in (dict(packed=None), dict(order=None), dict(tiles=None), dict(clean=None), dict(counts=None), dict(m=-1),
                dict(m=BIG + 1), dict(n_order=-256), dict(n_order=255), dict(n_order=257), dict(n_order=1 << 31),
                dict(n_order=0, counts=None)):
        assert _build(lib, **bad) == EINVAL, bad


def _dist(lib, pts=ADDR, n=100, qperm=ADDR, packed=ADDR, m=12, tiles=ADDR, clean=ADDR, n_tiles=1, beta=3.0, record=ADDR, ws=ADDR,
          ws_bytes=None):
    ws_bytes = lib.isdf_tri_tiles_ws_bytes(100) if ws_bytes is None else ws_bytes
    return lib.isdf_tri_distance_tiles(pts, n, qperm, packed, m, tiles, clean, n_tiles, beta, None, None, None, None, record, None,
                                       ws, ws_bytes, None)


def test_distance_refusals(lib):
    for bad in (dict(pts=None), dict(qperm=None), dict(packed=None), dict(tiles=None), dict(clean=None), dict(record=None),
                dict(n=-1), dict(m=-1), dict(n_tiles=-1), dict(n_tiles=(1 << 23) + 1), dict(beta=NAN),
                dict(n=BIG + 1, ws_bytes=1 << 62), dict(m=BIG + 1)):
        assert _dist(lib, **bad) == EINVAL, bad
    # a short or missing workspace, with every optional output (dist, index, closest, winding, stats) NULL
    assert _dist(lib, ws=None) == EWORKSPACE
    assert _dist(lib, ws_bytes=lib.isdf_tri_tiles_ws_bytes(100) - 1) == EWORKSPACE and _dist(lib, ws_bytes=0) == EWORKSPACE
    assert _dist(lib, n=101) == EWORKSPACE and _dist(lib, ws_bytes=-1) == EWORKSPACE
    # record is required even when there is nothing to do
    assert lib.isdf_tri_distance_tiles(None, 0, None, None, 0, None, None, 0, 0.0, None, None, None, None, None, None, ADDR, 1 << 20,
                                       None) == EINVAL
