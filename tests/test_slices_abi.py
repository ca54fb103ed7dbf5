"""C ABI of the slice entry points: the header declares isdf_slice_images / isdf_plane_points, the built library exports them,
isdf_amd/_ffi.py binds them with matching argument types, isdf_colormap's layout and the size macro match what the host C compiler
makes of the header, bad arguments are refused before anything is launched, and the ABI version is still 8 (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["lut", "n_colors", "vmin", "range"]
C_TYPES = {"const isdf_colormap*": "P(ColormapArgs)", "const isdf_gt_volume*": "P(GtVolumeArgs)", "const float*": "vp",
           "float*": "vp", "uint8_t*": "vp", "void*": "vp", "int64_t": "i64", "int32_t": "i32", "float": "f32"}


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
    names = {"P(ColormapArgs)": P(_ffi.ColormapArgs), "P(GtVolumeArgs)": P(_ffi.GtVolumeArgs), "vp": vp, "i64": i64, "i32": i32,
             "f32": f32}
    fn = "isdf_slice_images"
    assert fn in _ffi.SYMBOLS and hasattr(lib, fn)
    assert list(lib.isdf_slice_images.argtypes) == [names[C_TYPES[t]] for t in _declared(fn)] and len(_declared(fn)) == 13
    # the three host vectors of isdf_plane_points are bound as float pointers (ctypes arrays of three floats are passed)
    fn = "isdf_plane_points"
    assert fn in _ffi.SYMBOLS and hasattr(lib, fn)
    assert _declared(fn) == ["const float*"] * 3 + ["int32_t", "int32_t", "float*", "void*"]
    assert list(lib.isdf_plane_points.argtypes) == [P(f32)] * 3 + [i32, i32, vp, vp]
    assert lib.isdf_slice_images.restype is C.c_int and lib.isdf_plane_points.restype is C.c_int


def test_abi_version_is_still_8(lib):
    from isdf_amd import _ffi
    assert lib.isdf_abi_version() == 8 == _ffi.ABI_VERSION


def test_colormap_layout_and_size_macro_match_the_header(tmp_path, lib):
    from isdf_amd import _ffi
    c = tmp_path / "cm.c"
    body = "".join('  printf("%%zu\\n", offsetof(isdf_colormap, %s));\n' % f for f in FIELDS)
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "isdf_hip.h"\nint main(void) {\n'
                 '  printf("%zu\\n", sizeof(isdf_colormap));\n' + body +
                 '  printf("%d\\n", (int)ISDF_COLORMAP_MAX_COLORS);\n  return 0;\n}\n')
    exe = tmp_path / "cm"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split()
    assert C.sizeof(_ffi.ColormapArgs) == int(out[0])
    assert [getattr(_ffi.ColormapArgs, f).offset for f in FIELDS] == [int(x) for x in out[1:1 + len(FIELDS)]]
    assert [f for f, _ in _ffi.ColormapArgs._fields_] == FIELDS
    assert int(out[-1]) == _ffi.COLORMAP_MAX_COLORS and (_ffi.COLORMAP_MAX_COLORS + 3) * 4 == 65536     # the table fills 64 KiB of LDS


def test_argument_checks_refuse_before_any_launch(lib):
    from isdf_amd import _ffi
    cm = _ffi.ColormapArgs()
    cm.lut, cm.n_colors, cm.vmin, cm.range = 16, 401, -2.0, 4.0
    v = _ffi.GtVolumeArgs()
    v.values, v.nx, v.ny, v.nz = 16, 4, 4, 4
    for k in range(3):
        v.spacing[k], v.origin[k] = 0.1, 0.0

    def call(pts=16, sdf=16, n=8, cmap=cm, vol=v, eps=2.0, pred_rgb=16, gt=16, gt_rgb=16, pred_cost=16, gt_cost=16):
        return lib.isdf_slice_images(pts, sdf, n, None if cmap is None else C.byref(cmap), None if vol is None else C.byref(vol),
                                     0.0, eps, pred_rgb, gt, gt_rgb, pred_cost, gt_cost, None)
    none = dict(pred_rgb=None, gt=None, gt_rgb=None, pred_cost=None, gt_cost=None)
    assert call(n=-1) == -1 and call(**none) == -1                              # a negative count; nothing to write
    assert call(sdf=None) == -1 and call(pts=None) == -1                      # an output without its input
    assert call(vol=None) == -1 and call(cmap=None) == -1
    assert call(eps=0.0) == -1 and call(eps=-1.0) == -1 and call(eps=float("nan")) == -1
    only_pred = dict(none, pred_rgb=16)
    assert call(sdf=None, **only_pred) == -1 and call(cmap=None, **only_pred) == -1
    assert call(vol=None, **dict(none, gt=16)) == -1 and call(pts=None, vol=v, **dict(none, gt=16)) == -1
    assert call(eps=0.0, **dict(none, pred_cost=16)) == -1
    for field, value in (("n_colors", 0), ("n_colors", _ffi.COLORMAP_MAX_COLORS + 1), ("range", 0.0), ("range", -1.0),
                         ("range", float("inf")), ("range", float("nan")), ("vmin", float("nan")), ("lut", None)):
        bad = _ffi.ColormapArgs.from_buffer_copy(cm)
        setattr(bad, field, value)
        assert call(cmap=bad) == -1, (field, value)
    for field, value in (("nx", 1), ("values", None)):
        bad = _ffi.GtVolumeArgs.from_buffer_copy(v)
        setattr(bad, field, value)
        assert call(vol=bad) == -1, (field, value)
    bad = _ffi.GtVolumeArgs.from_buffer_copy(v)
    bad.spacing[2] = 0.0
    assert call(vol=bad) == -1
    assert call(n=0) == 0                                                       # nothing to do, nothing launched
    assert call(n=0, **none) == -1                                              # ... but still a call that asks for nothing

    F3 = C.c_float * 3
    o, du, dv = F3(0, 0, 0), F3(1, 0, 0), F3(0, 1, 0)
    pp = lib.isdf_plane_points
    assert pp(None, du, dv, 4, 4, 16, None) == -1 and pp(o, None, dv, 4, 4, 16, None) == -1 and pp(o, du, None, 4, 4, 16, None) == -1
    assert pp(o, du, dv, -1, 4, 16, None) == -1 and pp(o, du, dv, 4, -1, 16, None) == -1 and pp(o, du, dv, 4, 4, None, None) == -1
    assert pp(o, du, dv, 1 << 16, 1 << 15, 16, None) == -1                      # H * W beyond 2^31 - 1
    assert pp(o, du, dv, 0, 4, None, None) == 0 and pp(o, du, dv, 4, 0, None, None) == 0
