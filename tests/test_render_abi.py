"""C ABI of the rendered views: isdf_render_args' layout against the header (compiled with the host C compiler), the workspace
size, and argument checks that refuse before anything is launched (no GPU needed)."""
import ctypes as C
import os
import subprocess

import pytest

FIELDS = ["n_views", "H", "W", "n_samples", "T_WC", "dirs_C", "range_mode", "min_depth", "max_depth", "bin_length",
          "depth_offset", "src_H", "src_W", "rng_mode", "src_depth", "draw_u", "seed", "counter", "depth_in"]


@pytest.fixture(scope="module")
def lib():
    from isdf_amd import _ffi, build
    build.build(verbose=False)
    return _ffi.lib()


def test_render_args_layout_matches_the_header(tmp_path, lib):
    from isdf_amd import _ffi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    c = tmp_path / "ra.c"
    body = "".join('  printf("%%zu\\n", offsetof(isdf_render_args, %s));\n' % f for f in FIELDS)
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "isdf_hip.h"\nint main(void) {\n'
                 '  printf("%zu\\n", sizeof(isdf_render_args));\n' + body +
                 '  printf("%d %d %d\\n", ISDF_RANGE_SCALAR, ISDF_RANGE_DEPTH, ISDF_RANGE_UPSAMPLE);\n  return 0;\n}\n')
    exe = tmp_path / "ra"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(c), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split()
    assert C.sizeof(_ffi.RenderArgs) == int(out[0])
    assert [getattr(_ffi.RenderArgs, f).offset for f in FIELDS] == [int(x) for x in out[1:1 + len(FIELDS)]]
    assert [int(x) for x in out[-3:]] == [_ffi.RANGE_SCALAR, _ffi.RANGE_DEPTH, _ffi.RANGE_UPSAMPLE]
    assert [f for f, _ in _ffi.RenderArgs._fields_] == FIELDS


def test_workspace_bytes_and_argument_checks(lib):
    from isdf_amd import _ffi
    from isdf_amd.engine import NetConfig
    net = NetConfig().to_c()
    n1 = lib.isdf_render_ws_bytes(C.byref(net), 1, 42, 75, 19)
    n3 = lib.isdf_render_ws_bytes(C.byref(net), 3, 42, 75, 19)
    assert n3 > n1 >= 42 * 75 * 19 * 20                               # z, pc, sdf per sample point at least
    assert lib.isdf_render_ws_bytes(C.byref(net), 0, 42, 75, 19) > 0   # zero views: a valid (no-op) size
    assert lib.isdf_render_ws_bytes(C.byref(net), -1, 42, 75, 19) == -1
    assert lib.isdf_render_ws_bytes(C.byref(net), 1, 0, 75, 19) == -1
    assert lib.isdf_render_ws_bytes(C.byref(net), 1, 42, 75, 0) == -1
    assert lib.isdf_render_ws_bytes(None, 1, 42, 75, 19) == -1
    a = _ffi.RenderArgs()
    a.n_views, a.H, a.W, a.n_samples, a.T_WC, a.dirs_C = 2, 4, 4, 3, 16, 16
    a.range_mode, a.rng_mode, a.draw_u = _ffi.RANGE_SCALAR, 0, 16
    call = lambda a, d, n, ws, nb: lib.isdf_render_views(C.byref(net), 16, 16, C.byref(a) if a is not None else None, d, n, ws, nb,
                                                         None)
    assert call(None, 16, None, 16, 1 << 30) == -1                    # no arguments
    assert call(a, None, None, 16, 1 << 30) == -1                     # neither output
    a.range_mode = 7
    assert call(a, 16, None, 16, 1 << 30) == -1                       # unknown range source
    a.range_mode = _ffi.RANGE_DEPTH
    assert call(a, 16, None, 16, 1 << 30) == -1                       # depth source without images
    a.range_mode, a.draw_u = _ffi.RANGE_SCALAR, None
    assert call(a, 16, None, 16, 1 << 30) == -1                       # injected draws missing
    a.rng_mode = 1
    assert call(a, 16, None, 16, 8) == -3                             # workspace too small
    a.depth_in = 16
    assert call(a, 16, None, 16, 1 << 30) == -1                       # a given depth renders normals only
    a.n_views = 0
    assert call(a, 16, None, None, 0) == 0                            # zero views: nothing is checked further, nothing runs
