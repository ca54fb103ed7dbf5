"""C ABI of the evaluation entry points: isdf_sdf_metrics / isdf_nn_distance keep their parameter counts, and bad arguments are
refused before anything is launched (no GPU needed).  What the header says of their types, of isdf_gt_volume's layout and of the
size macros is held to isdf_amd/_ffi.py by tests/test_abi.py."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from isdf_amd import _ffi, build
    build.build(verbose=False)
    return _ffi.lib()


def test_header_declares_library_exports_and_ffi_binds_with_matching_types(lib):
    from isdf_amd import _ffi
    for fn in ("isdf_sdf_metrics", "isdf_nn_distance"):
        assert fn in _ffi.SYMBOLS and hasattr(lib, fn)
    assert len(lib.isdf_sdf_metrics.argtypes) == 12 and len(lib.isdf_nn_distance.argtypes) == 10


def test_argument_checks_refuse_before_any_launch(lib):
    from isdf_amd import _ffi
    v = _ffi.GtVolumeArgs()
    v.values, v.nx, v.ny, v.nz = 16, 4, 4, 4
    for k in range(3):
        v.spacing[k], v.origin[k] = 0.1, 0.0
    ws = _ffi.SDF_METRICS_WS_BYTES

    def call(vol=v, pts=16, sdf=16, n=8, record=16, wsp=16, nb=ws):
        return lib.isdf_sdf_metrics(C.byref(vol) if vol is not None else None, pts, sdf, n, 1, 0.0, record, None, None, wsp, nb, None)
    assert call(vol=None) == -1 and call(record=None) == -1 and call(pts=None) == -1 and call(sdf=None) == -1 and call(n=-1) == -1
    assert call(nb=ws - 1) == -3 and call(wsp=None) == -3
    bad = _ffi.GtVolumeArgs.from_buffer_copy(v)
    bad.nx = 1
    assert call(vol=bad) == -1                                        # a side of one grid point has no cell
    bad = _ffi.GtVolumeArgs.from_buffer_copy(v)
    bad.spacing[1] = 0.0
    assert call(vol=bad) == -1
    bad.spacing[1] = -0.1
    assert call(vol=bad) == -1                                        # descending axes are not scipy's grid either
    bad = _ffi.GtVolumeArgs.from_buffer_copy(v)
    bad.nx, bad.ny, bad.nz = 2048, 2048, 2048
    assert call(vol=bad) == -1
    bad = _ffi.GtVolumeArgs.from_buffer_copy(v)
    bad.values = None
    assert call(vol=bad) == -1

    def nn(q=16, n=8, t=16, m=8, total=16, wsp=16, nb=1 << 20):
        return lib.isdf_nn_distance(q, n, t, m, None, None, total, wsp, nb, None)
    assert nn(total=None) == -1 and nn(q=None) == -1 and nn(t=None) == -1 and nn(n=-1) == -1
    assert nn(m=0) == -1                                              # no target: there is no nearest one
    assert nn(m=1 << 32) == -1                                        # the index half of a key is 32 bits
    assert nn(nb=_ffi.nn_ws_bytes(8) - 1) == -3 and nn(wsp=None) == -3
