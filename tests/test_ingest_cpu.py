"""The float64 ingest model (tests/ingest_model.py) and the conditions on its inputs, on any host.

  * the float32 oracle and the REAL reference's normals (tests/golden/ingest_small.npz) pass the acceptance rule on every pixel of
    every input tests/test_ingest_gpu.py uses -- that, and the derivation in ingest_model's docstring, is what justifies the bounds;
  * every noisy input keeps the rule sharp: at most 2 % of its pixels have more than one admissible neighbour pair and at least
    99 % of its single-candidate finite pixels are held to t <= 1e-3;
  * six defects (argmin keeps the last minimum, pair (k, k+1), zero padding, stride 1, a seam at column 32, cx ignored) each fail
    the rule on at least one input;
  * the roof image pins `first minimum wins`;
  * every keyframe-render input keeps |d - ds| / ds at least 4 ulp away from the threshold, so the below-threshold count is exact.

Measured over the 80 inputs (8 shapes x 2 cameras x 5 depth variants): float32 oracle 0 failing pixels, worst error / bound 0.053
(the bounds are worst-case, the errors typical); reference fixture 0 failing pixels, worst 0.040, multi-candidate share 0.65 %;
multi-candidate share of the noisy inputs 0 .. 0.70 % (37x100 skewed with NaN pixels); every single-candidate finite pixel has
t <= 1e-3, the largest t is 2.3e-4.  Failing pixels per mutant over the 80 inputs (+ on the roof): last_minimum 0 (+ 5: an exact tie
admits every tied pair, so only the roof's pinned answer catches it), pair_k_k1 80 109, zero_padding 666, stride_1 81 830 (+ 81),
seam_column_32 968, cx_ignored 99 697 (+ 64).
"""
import numpy as np
import pytest

import oracle.isdf_oracle as orc
from tests import golden_util as gu
from tests import ingest_model as im


@pytest.fixture(scope="module")
def inputs():
    """every GPU input with its model, computed once"""
    out = []
    for name, variant, d, cam in im.all_inputs():
        out.append((name, variant, d, cam, im.model(d, cam["fx"], cam["fy"], cam["cx"], cam["cy"])))
    return out


def _args(cam):
    return cam["fx"], cam["fy"], cam["cx"], cam["cy"]


def test_transcription_is_the_oracle_bit_for_bit(inputs):
    for name, _, d, cam, _ in inputs:
        ref = orc.estimate_pointcloud_normals(orc.pointcloud_from_depth(d, *_args(cam)))
        assert np.array_equal(im.f32_normals(d, *_args(cam)), ref, equal_nan=True), name


def test_float32_oracle_passes_on_every_pixel_of_every_input(inputs):
    worst = 0.0
    for name, _, d, cam, m in inputs:
        j = im.judge(m, im.f32_normals(d, *_args(cam)))
        print("%-32s failing %d  worst error/bound %.3f  multi-candidate %.2f %%" % (name, j["fail"].sum(), j["ratio"].max(), 100 * j["multi"].mean()))
        assert not j["fail"].any(), (name, np.argwhere(j["fail"])[:5], j["ratio"].max())
        worst = max(worst, j["ratio"].max())
    print("float32 oracle: 0 failing pixels, worst error/bound %.3f" % worst)


def test_reference_fixture_passes_on_every_pixel():
    g = gu.load("ingest_small")
    cam = gu.cam_of(g)
    m = im.model(g["depth"], *_args(cam))
    for who, n in (("reference", g["normals"]), ("oracle", im.f32_normals(g["depth"], *_args(cam)))):
        j = im.judge(m, n)
        print("ingest_small %-9s failing %d  worst error/bound %.3f  multi-candidate %.2f %%" % (who, j["fail"].sum(), j["ratio"].max(), 100 * j["multi"].mean()))
        assert not j["fail"].any(), (who, np.argwhere(j["fail"])[:5])


def test_noisy_inputs_keep_the_rule_sharp(inputs):
    for name, variant, _, _, m in inputs:
        if variant not in im.NOISY:
            continue
        multi, sharp, tmax = im.conditions(m)
        print("%-32s multi-candidate %.2f %%  single-candidate t <= 1e-3: %.2f %%  max t %.2e" % (name, 100 * multi, 100 * sharp, tmax))
        assert multi <= 0.02, (name, multi)
        assert sharp >= 0.99, (name, sharp)


@pytest.mark.parametrize("mutant", im.MUTANTS)
def test_each_defect_fails_the_rule(inputs, mutant):
    failing = 0
    for name, _, d, cam, m in inputs:
        failing += int(im.judge(m, im.f32_normals(d, *_args(cam), mutant=mutant))["fail"].sum())
    d, cam = im.roof()
    roof = int(im.judge_roof(im.f32_normals(d, *_args(cam), mutant=mutant)).sum())
    print("mutant %-15s: %d failing pixels over the 80 inputs, %d on the roof" % (mutant, failing, roof))
    assert failing + roof > 0


def test_roof_pins_first_minimum_wins():
    d, cam = im.roof()
    n, scores = im.f32_normals(d, *_args(cam), want_scores=True)
    assert np.array_equal(n, orc.estimate_pointcloud_normals(orc.pointcloud_from_depth(d, *_args(cam))), equal_nan=True)
    rows = slice(2, 7)
    ridge = scores[:, rows, 4]                                         # [8, rows]
    for k in (2, 4, 6):
        assert np.array_equal(ridge[k].view(np.uint32), ridge[0].view(np.uint32))          # the four even pairs tie bit for bit
    assert (ridge[[1, 3, 5, 7]] > ridge[0]).all()
    want = im.ROOF_NORMAL.astype(np.float32)
    np.testing.assert_allclose(want, [-0.3714, 0.0, 0.9285], atol=5e-5)
    assert np.abs(n[rows, 4] - want).max() <= 2.0 ** -23                 # pair 0's normal, not the mirror image
    mirror = im.f32_normals(d, *_args(cam), mutant="last_minimum")[rows, 4]
    assert np.abs(mirror - want * np.float32([-1, 1, 1])).max() <= 2.0 ** -23
    # the model sees the tie (several candidates on the ridge) and still rejects nothing the oracle computes
    m = im.model(d, *_args(cam))
    j = im.judge(m, n)
    assert not j["fail"].any() and j["multi"][rows, 4].all()
    assert not im.judge_roof(n).any() and im.judge_roof(im.f32_normals(d, *_args(cam), mutant="last_minimum"))[rows, 4].all()


@pytest.mark.parametrize("S", im.RENDER_S)
@pytest.mark.parametrize("R", im.RENDER_R)
def test_render_inputs_stay_clear_of_the_threshold(R, S):
    z, sdf, ds = im.render_case(R, S)
    view, count = im.render_reference(z, sdf, ds)
    margin = im.render_margin(view, ds)
    print("R=%d S=%d: below %d of %d, nearest ratio %.1f ulp from the threshold" % (R, S, count, R, margin))
    assert margin >= 4.0
    assert view.dtype == np.float32 and 0 <= count <= R
    if R >= 128 and S >= 27:           # the cases do what they are there for
        k = np.arange(R) % 8
        assert (view[k == 3] == 0).all() and np.isnan(view[(np.arange(R) % 16) == 5]).all() and 0 < count < R
