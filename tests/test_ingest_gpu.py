"""`isdf_estimate_normals` against the float64 model of tests/ingest_model.py on EVERY pixel, and `isdf_render_depth` bit for bit
against `oracle.isdf_oracle.keyframe_ratio` on every ray.  Needs a real MI355X: `pytest -m gpu`.

Normals: images smaller than the 32 x 16 block, exactly one block, one pixel more and one less, several ragged blocks; noisy, clean,
NaN-pixel and zero-patch depth; a centred and a skewed camera; the roof image (first minimum wins) and the reference's own fixture.
The acceptance rule, its bounds and the conditions that keep it sharp are derived in ingest_model and checked on any host by
tests/test_ingest_cpu.py; nothing here is tuned to what the kernel returns.

Keyframe render: R around the 128-ray block, S from 1 to 64, shuffled samples with duplicate z values, rays without a crossing, a
crossing at the last sorted sample, -0.0 and NaN sdf values, zero depth samples; the device-side n_valid path with n_valid below
max_rays; two launches give the same bytes.

Measured on an MI355X (each test prints its figures): 0 failing pixels on all 80 inputs, the roof and the reference fixture; worst
error / bound 0.048 (the bounds are worst-case, the errors typical); multi-candidate share 0 .. 0.83 % (0.65 % on the fixture); view
depth array-equal and the count equal on all 20 (R, S) pairs and the 6 n_valid cases.  Before ingest.hip was built without
floating-point contraction this module failed on 17x33/centred/noise_0.002, pixel (16, 17): both neighbours of the best pair are
zero-depth pixels (the same point), the reference's cross product is exactly 0 and its normal NaN, and the fused cross product left
a product's rounding error that normalised to a finite unit vector.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import golden_util as gu
from tests import ingest_model as im

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from isdf_amd.engine import Engine, NetConfig
    return Engine(NetConfig(), "cuda")


def _normals(eng, d, cam):
    from isdf_amd.engine import SampleConfig
    sc = SampleConfig(H=cam["H"], W=cam["W"], fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"])
    return eng.estimate_normals(torch.as_tensor(np.ascontiguousarray(d)).cuda(), sc).cpu().numpy()


def _report(name, j):
    fin = j["ratio"][np.isfinite(j["ratio"])]
    print("%-32s failing %d  worst error/bound %.3f  multi-candidate %.2f %%" % (name, j["fail"].sum(), fin.max() if fin.size else 0.0, 100 * j["multi"].mean()))


@pytest.mark.parametrize("H,W", im.SHAPES)
def test_normals_every_pixel_within_the_model_bound(eng, H, W):
    for name, _, d, cam in im.all_inputs([(H, W)]):
        n = _normals(eng, d, cam)
        assert n.shape == (H, W, 3) and n.dtype == np.float32
        j = im.judge(im.model(d, cam["fx"], cam["fy"], cam["cx"], cam["cy"]), n)
        _report(name, j)
        assert not j["fail"].any(), (name, np.argwhere(j["fail"])[:8].tolist(), j["ratio"][j["fail"]][:8].tolist())


def test_normals_roof_first_minimum_wins(eng):
    d, cam = im.roof()
    n = _normals(eng, d, cam)
    print("ridge column, rows 2..6:", n[2:7, 4].tolist())
    fail = im.judge_roof(n)
    assert not fail.any(), np.argwhere(fail).tolist()
    assert np.abs(n[2:7, 4].astype(np.float64) - im.ROOF_NORMAL).max() <= 4 * 2.0 ** -23          # pair 0's normal, not its mirror image


def test_normals_reference_fixture_every_pixel(eng):
    g = gu.load("ingest_small")
    cam = gu.cam_of(g)
    j = im.judge(im.model(g["depth"], cam["fx"], cam["fy"], cam["cx"], cam["cy"]), _normals(eng, g["depth"], cam))
    _report("ingest_small", j)
    assert not j["fail"].any(), np.argwhere(j["fail"])[:8].tolist()


def test_normals_two_launches_give_the_same_bytes(eng):
    d, cam = im.depth_input(37, 100, "nan_pixels", "skewed")
    a, b = _normals(eng, d, cam), _normals(eng, d, cam)
    assert a.tobytes() == b.tobytes()


# ---- isdf_render_depth ------------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("S", im.RENDER_S)
@pytest.mark.parametrize("R", im.RENDER_R)
def test_render_depth_bit_for_bit_and_count_as_an_integer(eng, R, S):
    z, sdf, ds = im.render_case(R, S)
    view_ref, count_ref = im.render_reference(z, sdf, ds)
    zd, sd, dd = _dev(z), _dev(sdf), _dev(ds)
    view, below = eng.render_depth(zd, sd, dd, im.KF_DIST_TH)
    v = view.cpu().numpy()
    differ = int((~((v == view_ref) | (np.isnan(v) & np.isnan(view_ref)))).sum())
    print("R=%d S=%d: below %d (reference %d), view depth differs on %d rays" % (R, S, int(below.item()), count_ref, differ))
    assert np.array_equal(v, view_ref, equal_nan=True)
    assert np.array_equal(np.signbit(v), np.signbit(view_ref))
    assert int(below.item()) == count_ref
    view2, below2 = eng.render_depth(zd, sd, dd, im.KF_DIST_TH)                       # determinism: the same bytes
    assert view2.cpu().numpy().tobytes() == v.tobytes() and int(below2.item()) == count_ref
    view3, below3 = eng.render_depth(zd, sd)                                          # no depth sample: the view alone, count untouched
    assert view3.cpu().numpy().tobytes() == v.tobytes() and int(below3.item()) == 0


@pytest.mark.parametrize("R,S,nv", [(129, 27, 128), (129, 27, 1), (1000, 64, 257), (1000, 2, 0), (128, 1, 127), (127, 27, 127)])
def test_render_depth_device_n_valid_below_max_rays(eng, R, S, nv):
    """the C entry point with a device n_valid < max_rays: rows at or beyond n_valid keep their NaN prefill, the count (prefilled
    with a non-zero value) covers the first n_valid rays only"""
    from isdf_amd import _ffi
    from isdf_amd.engine import _stream
    z, sdf, ds = im.render_case(R, S)
    zd, sd, dd = _dev(z), _dev(sdf), _dev(ds)
    n_valid = torch.tensor([nv], dtype=torch.int32, device="cuda")
    view = torch.full((R,), float("nan"), dtype=torch.float32, device="cuda")
    below = torch.full((1,), 12345, dtype=torch.int32, device="cuda")
    rc = _ffi.lib().isdf_render_depth(_ffi.ptr(n_valid), 0, R, S, _ffi.ptr(zd), _ffi.ptr(sd), _ffi.ptr(dd), C.c_float(im.KF_DIST_TH),
                                      _ffi.ptr(view), _ffi.ptr(below), _stream(eng.device))
    assert rc == 0
    torch.cuda.synchronize()
    v = view.cpu().numpy()
    assert np.isnan(v[nv:]).all()
    if nv:
        view_ref, count_ref = im.render_reference(z[:nv], sdf[:nv], ds[:nv])
        assert np.array_equal(v[:nv], view_ref, equal_nan=True)
    else:
        count_ref = 0
    assert int(below.item()) == count_ref
