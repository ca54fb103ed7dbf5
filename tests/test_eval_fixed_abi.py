"""C ABI of isdf_region_metrics: the header declares it, the built library exports it, isdf_amd/_ffi.py binds it, the layout of
isdf_region_args (which carries doubles) and the size macros match what the host C compiler makes of the header, and every bad
argument is refused before anything is launched (no GPU needed)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["pts", "sdf", "sdf_grad", "flags", "vol", "gt_in", "n", "grad_sets", "reserved", "spacing", "origin", "delta"]


@pytest.fixture(scope="module")
def lib():
    from isdf_amd import _ffi, build
    build.build(verbose=False)
    return _ffi.lib()


def test_header_declares_library_exports_and_ffi_binds(lib):
    from isdf_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "isdf_hip.h")).read()
    assert "int isdf_region_metrics(const isdf_region_args* args, double* records, void* workspace, int64_t workspace_bytes, void* stream);" in hdr
    assert "isdf_region_metrics" in _ffi.SYMBOLS and hasattr(lib, "isdf_region_metrics")
    assert list(lib.isdf_region_metrics.argtypes) == [C.POINTER(_ffi.RegionArgs), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    assert lib.isdf_region_metrics.restype is C.c_int
    assert lib.isdf_abi_version() == _ffi.ABI_VERSION == 8                  # an added entry point: the ABI number stays


def test_region_args_layout_and_size_macros_match_the_header(tmp_path, lib):
    from isdf_amd import _ffi
    c = tmp_path / "ra.c"
    body = "".join('  printf("%%zu\\n", offsetof(isdf_region_args, %s));\n' % f for f in FIELDS)
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "isdf_hip.h"\nint main(void) {\n'
                 '  printf("%zu\\n", sizeof(isdf_region_args));\n' + body +
                 '  printf("%d %d\\n", ISDF_REGION_RECORD, (int)ISDF_REGION_METRICS_WS_BYTES);\n  return 0;\n}\n')
    exe = tmp_path / "ra"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert C.sizeof(_ffi.RegionArgs) == out[0]
    assert [getattr(_ffi.RegionArgs, f).offset for f in FIELDS] == out[1:1 + len(FIELDS)]
    assert _ffi.RegionArgs.delta.offset == out[len(FIELDS)] and _ffi.RegionArgs.delta.offset + 8 == out[0]   # the last field
    assert [f for f, _ in _ffi.RegionArgs._fields_] == FIELDS
    assert out[-2:] == [_ffi.REGION_RECORD, _ffi.REGION_METRICS_WS_BYTES]
    assert _ffi.REGION_RECORD == _ffi.METRICS_RECORD + 3


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
