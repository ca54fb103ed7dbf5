"""C ABI of isdf_region_metrics: the built library exports it, isdf_amd/_ffi.py binds it, and every bad argument is refused before
anything is launched (no GPU needed).  Its types, the layout of isdf_region_args (which carries doubles) and the size macros are
held to the header by tests/test_abi.py."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from isdf_amd import _ffi, build
    build.build(verbose=False)
    return _ffi.lib()


def test_header_declares_library_exports_and_ffi_binds(lib):
    from isdf_amd import _ffi
    assert "isdf_region_metrics" in _ffi.SYMBOLS and hasattr(lib, "isdf_region_metrics")
    assert len(lib.isdf_region_metrics.argtypes) == 5
    assert _ffi.REGION_RECORD == _ffi.METRICS_RECORD + 3
    assert _ffi.RegionArgs.delta.offset + 8 == C.sizeof(_ffi.RegionArgs)    # the last field: no tail padding
    assert lib.isdf_abi_version() == _ffi.ABI_VERSION == 8                  # an added entry point: the ABI number stays


def test_argument_checks_refuse_before_any_launch(lib):
    """the pointers are small non-null integers: a call that got as far as a launch would not return ISDF_EINVAL"""
    from isdf_amd import _ffi
    v = _ffi.GtVolumeArgs()
    v.values, v.nx, v.ny, v.nz = 16, 4, 4, 4
    for k in range(3):
        v.spacing[k], v.origin[k] = 0.1, 0.0
    ws = _ffi.REGION_METRICS_WS_BYTES

    def args(vol=True, gt_in=None, sdf_grad=None, grad_sets=0, delta=0.01, n=8, pts=16, sdf=16, spacing=0.1):
        a = _ffi.RegionArgs()
        a.pts, a.sdf, a.sdf_grad, a.flags, a.gt_in, a.n = pts, sdf, sdf_grad, 16, gt_in, n
        if vol:
            a.vol = C.pointer(v)
        a.grad_sets, a.delta = grad_sets, delta
        for k in range(3):
            a.spacing[k], a.origin[k] = spacing, 0.0
        return a

    def call(a, records=16, wsp=16, nb=ws):
        return lib.isdf_region_metrics(C.byref(a) if a is not None else None, records, wsp, nb, None)
    EINVAL, EWORKSPACE = -1, -3
    assert call(None) == EINVAL and call(args(), records=None) == EINVAL
    assert call(args(vol=False)) == EINVAL                                   # no ground-truth source
    assert call(args(vol=True, gt_in=16)) == EINVAL                          # ... or both
    assert call(args(grad_sets=1)) == EINVAL                                 # gradient flags without sdf_grad
    assert call(args(vol=False, gt_in=16, sdf_grad=16, grad_sets=1)) == EINVAL   # gradient sets together with gt_in
    assert call(args(delta=0.0)) == EINVAL and call(args(delta=-0.01)) == EINVAL and call(args(delta=float("nan"))) == EINVAL
    assert call(args(n=-1)) == EINVAL and call(args(pts=None)) == EINVAL and call(args(sdf=None)) == EINVAL
    assert call(args(spacing=0.0)) == EINVAL and call(args(spacing=float("inf"))) == EINVAL
    v.nx = 1
    assert call(args()) == EINVAL                                            # a side of one grid point has no cell
    v.nx = 4
    # good arguments get as far as the workspace check (which comes last), and no further
    assert call(args(), nb=ws - 1) == EWORKSPACE and call(args(), wsp=None) == EWORKSPACE
    assert call(args(sdf_grad=16, grad_sets=1), nb=0) == EWORKSPACE and call(args(vol=False, gt_in=16), nb=0) == EWORKSPACE
