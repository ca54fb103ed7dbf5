"""C ABI of the rendered views: the workspace size, and argument checks that refuse before anything is launched (no GPU needed)."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from isdf_amd import _ffi, build
    build.build(verbose=False)
    return _ffi.lib()


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
