"""C ABI of isdf_visible_points: the built library exports it, isdf_amd/_ffi.py binds its 16 parameters, the ABI number is
unchanged, and every bad argument is refused before anything is launched.  Its types are held to the header by tests/test_abi.py."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from isdf_amd import _ffi, build
    build.build(verbose=False)
    return _ffi.lib()


def test_header_declares_library_exports_and_ffi_binds_with_matching_types(lib):
    from isdf_amd import _ffi
    assert "isdf_visible_points" in _ffi.SYMBOLS and hasattr(lib, "isdf_visible_points")
    assert len(lib.isdf_visible_points.argtypes) == 16
    assert lib.isdf_abi_version() == _ffi.ABI_VERSION == 8                  # an added entry point: the ABI number stays


def test_argument_checks_refuse_before_any_launch(lib):
    """the pointers are small non-null integers: a call that got as far as a memset or a launch would not return ISDF_EINVAL"""
    def call(pts=16, n=8, T=16, depth=16, F=2, H=48, W=64, fx=60.0, fy=60.0, cx=31.5, cy=23.5, trunc=0.2, count=16, mask=None,
             n_seen=None):
        return lib.isdf_visible_points(pts, n, T, depth, F, H, W, fx, fy, cx, cy, trunc, count, mask, n_seen, None)
    assert call(pts=None) == EINVAL and call(T=None) == EINVAL and call(depth=None) == EINVAL and call(count=None) == EINVAL
    assert call(H=0) == EINVAL and call(W=0) == EINVAL and call(H=-3) == EINVAL and call(W=-1) == EINVAL
    assert call(n=-1) == EINVAL and call(F=-1) == EINVAL
    assert call(n=1 << 38, F=1 << 26, mask=16) == EINVAL                    # F * n = 2^64: the mask's index leaves int64
    assert call(n=(1 << 38) + 1) == EINVAL
    assert call(H=1 << 16, W=1 << 15) == EINVAL                              # a frame of 2^31 pixels
    for name in ("fx", "fy", "cx", "cy", "trunc"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(**{name: bad}) == EINVAL, (name, bad)
    # nothing to do and nothing to write: accepted without a pointer being touched
    assert call(pts=None, n=0, T=None, depth=None, F=0, count=None) == 0
    assert call(pts=None, n=0, T=None, depth=None, F=5, count=None) == 0
