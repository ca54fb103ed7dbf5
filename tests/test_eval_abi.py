"""C ABI of the evaluation entry points: the header declares isdf_sdf_metrics / isdf_nn_distance, the built library exports
them, isdf_amd/_ffi.py binds them with matching argument types, isdf_gt_volume's layout and the size macros match what the host
C compiler makes of the header, and bad arguments are refused before anything is launched (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["values", "nx", "ny", "nz", "reserved", "spacing", "origin"]
C_TYPES = {"const isdf_gt_volume*": "P(GtVolumeArgs)", "const float*": "vp", "float*": "vp", "double*": "vp", "uint8_t*": "vp",
           "int32_t*": "vp", "void*": "vp", "int64_t": "i64", "int32_t": "i32", "float": "f32"}


@pytest.fixture(scope="module")
def lib():
    from isdf_amd import _ffi, build
    build.build(verbose=False)
    return _ffi.lib()


def _declared(name):
    hdr = open(os.path.join(ROOT, "include", "isdf_hip.h")).read()
    m = re.search(r"\bint %s\(([^;]*?)\);" % name, hdr, re.S)
    assert m, name + " is not declared in include/isdf_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    return [a.rsplit(" ", 1)[0] for a in args]            # the types, parameter names dropped


def test_header_declares_library_exports_and_ffi_binds_with_matching_types(lib):
    from isdf_amd import _ffi
    P, i32, i64, f32, vp = C.POINTER, C.c_int32, C.c_int64, C.c_float, C.c_void_p
    names = {"P(GtVolumeArgs)": P(_ffi.GtVolumeArgs), "vp": vp, "i64": i64, "i32": i32, "f32": f32}
    for fn in ("isdf_sdf_metrics", "isdf_nn_distance"):
        assert fn in _ffi.SYMBOLS and hasattr(lib, fn)
        want = [names[C_TYPES[t]] for t in _declared(fn)]
        assert list(getattr(lib, fn).argtypes) == want, fn
        assert getattr(lib, fn).restype is C.c_int
    assert len(_declared("isdf_sdf_metrics")) == 12 and len(_declared("isdf_nn_distance")) == 10


def test_gt_volume_layout_and_size_macros_match_the_header(tmp_path, lib):
    from isdf_amd import _ffi
    c = tmp_path / "gv.c"
    body = "".join('  printf("%%zu\\n", offsetof(isdf_gt_volume, %s));\n' % f for f in FIELDS)
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "isdf_hip.h"\nint main(void) {\n'
                 '  printf("%zu\\n", sizeof(isdf_gt_volume));\n' + body +
                 '  printf("%d %d %lld %lld %lld\\n", ISDF_METRICS_RECORD, (int)ISDF_SDF_METRICS_WS_BYTES,\n'
                 '         (long long)ISDF_NN_WS_BYTES(0), (long long)ISDF_NN_WS_BYTES(257), (long long)ISDF_NN_WS_BYTES(200000));\n'
                 '  return 0;\n}\n')
    exe = tmp_path / "gv"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split()
    assert C.sizeof(_ffi.GtVolumeArgs) == int(out[0])
    assert [getattr(_ffi.GtVolumeArgs, f).offset for f in FIELDS] == [int(x) for x in out[1:1 + len(FIELDS)]]
    assert [f for f, _ in _ffi.GtVolumeArgs._fields_] == FIELDS
    assert [int(x) for x in out[-5:]] == [_ffi.METRICS_RECORD, _ffi.SDF_METRICS_WS_BYTES, _ffi.nn_ws_bytes(0), _ffi.nn_ws_bytes(257),
                                          _ffi.nn_ws_bytes(200000)]


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
