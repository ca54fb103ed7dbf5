"""Point visibility against posed depth frames, host side (no GPU): the float32 model of tests/visible_model.py against the
reference's recorded masks (fixture visible_small, tests/golden/make_visible_golden.py), isdf_amd.metrics.visible_points on a
model-backed engine stand-in, and Trainer.eval_object_sdf on the REAL reference Trainer grafted with such an engine -- one
visible_points call instead of frustum.is_visible_torch, the same list, the same generator state."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import visible_model as vm
from tests.test_eval_cpu import EvalFakeEngine, _close, _eval_trainer, needs_ref, ref_mods  # noqa: F401  (ref_mods: a fixture)


@pytest.fixture(scope="module")
def g():
    return vm.load_golden()


class VisibleFakeEngine(EvalFakeEngine):
    """EvalFakeEngine + visible_points, answered by the float32 model (same return contract as engine.Engine)"""

    def visible_points(self, pts, T_CW, depth, cam, trunc=0.2, want_mask=False):
        m = vm.visible32(pts.detach().numpy().reshape(-1, 3), T_CW.detach().numpy(), depth.detach().numpy(), cam.fx, cam.fy,
                         cam.cx, cam.cy, trunc)
        self.calls.append("visible_points")
        self.visible_args = dict(T_CW=T_CW.detach().numpy().copy(), n=m.shape[1], F=m.shape[0], trunc=trunc, want_mask=want_mask)
        count = torch.from_numpy(m.sum(0).astype(np.int32))
        return (count, torch.from_numpy(m.astype(np.uint8)) if want_mask else None,
                torch.tensor([int((m.sum(0) > 0).sum())], dtype=torch.int64))


def test_float32_model_equals_the_reference_outside_the_border(g):
    assert len(g["cases"]) == 6
    for c in g["cases"]:
        F = c["F"]
        m = vm.visible32(c["pts"], g["T_CW"][:F], g["depth"][:F], vm.CAM["fx"], vm.CAM["fy"], vm.CAM["cx"], vm.CAM["cy"], c["trunc"])
        assert m.shape == c["mask"].shape == c["border"].shape == (F, c["n"])
        assert c["border"].mean() < 0.01 and 0.01 < c["mask"].mean() < 0.60
        assert np.array_equal(m[~c["border"]], c["mask"][~c["border"]]), (F, c["n"], c["trunc"])


def test_metrics_visible_points_on_a_model_backed_engine(g):
    from isdf_amd import metrics
    from isdf_amd.engine import NetConfig
    eng = VisibleFakeEngine(NetConfig(hidden=64, blocks=1))
    cam = vm.Cam(**vm.CAM)
    for c in g["cases"]:
        F = c["F"]
        for want_mask in (True, False):
            eng.calls.clear()
            count, mask, n_seen = metrics.visible_points(eng, torch.from_numpy(c["pts"]), torch.from_numpy(g["T_WC"][:F]),
                                                         torch.from_numpy(g["depth"][:F]), cam, trunc=c["trunc"], want_mask=want_mask)
            assert eng.calls == ["visible_points"]                                  # the poses inverted, then ONE call
            a = eng.visible_args
            assert (a["F"], a["n"], a["trunc"], a["want_mask"]) == (F, c["n"], c["trunc"], want_mask)
            np.testing.assert_allclose(a["T_CW"], g["T_CW"][:F], rtol=0, atol=1e-5)
            assert count.dtype == torch.int32 and tuple(count.shape) == (c["n"],) and n_seen.dtype == torch.int64
            assert int(n_seen.item()) == int((count > 0).sum())
            if want_mask:
                assert mask.dtype == torch.uint8 and tuple(mask.shape) == (F, c["n"])
                assert np.array_equal(count.numpy(), mask.numpy().sum(0))
                keep = ~c["border"]
                assert np.array_equal(mask.numpy().astype(bool)[keep], c["mask"][keep])
            else:
                assert mask is None
    # no frame: zero counts
    count, mask, n_seen = metrics.visible_points(eng, torch.zeros(5, 3), torch.zeros(0, 4, 4), torch.zeros(0, 48, 64), cam, want_mask=True)
    assert count.tolist() == [0] * 5 and tuple(mask.shape) == (0, 5) and int(n_seen.item()) == 0


@needs_ref
def test_bound_eval_object_sdf_asks_the_engine_once_and_equals_the_reference(ref_mods, tmp_path, monkeypatch):
    mg, mods = ref_mods
    from isdf.geometry import frustum
    from isdf_amd.hot_path import graft
    entered = []
    inner = frustum.is_visible_torch

    def counting(*a, **k):
        entered.append(1)
        return inner(*a, **k)
    monkeypatch.setattr(frustum, "is_visible_torch", counting)

    def run(tr):
        torch.manual_seed(11); np.random.seed(11)
        with contextlib.redirect_stdout(io.StringIO()):
            return tr.eval_object_sdf(samples=500), torch.rand(1).item()

    ref = _eval_trainer(mg, mods, tmp_path, False)
    want, want_after = run(ref)
    assert len(entered) == 1 and len(want) == 2 and np.isfinite(want[0]) and np.isnan(want[1])

    hip = _eval_trainer(mg, mods, tmp_path, False)
    with contextlib.redirect_stdout(io.StringIO()):
        graft(hip, rng="torch", engine_factory=VisibleFakeEngine)
    hip.engine.calls.clear()
    del entered[:]
    got, got_after = run(hip)
    _close(got, want, "eval_object_sdf")
    assert got_after == want_after                                # the torch generator advanced exactly as in the reference
    assert hip.engine.calls.count("visible_points") == 1 and not entered
    a = hip.engine.visible_args
    assert (a["n"], a["trunc"], a["want_mask"]) == (100 * 2, 0.05, False) and a["F"] == 30

    # an engine without the method: the reference's own function answers, as before
    old = _eval_trainer(mg, mods, tmp_path, True)
    assert getattr(old.engine, "visible_points", None) is None
    got, got_after = run(old)
    _close(got, want, "eval_object_sdf without visible_points")
    assert got_after == want_after and len(entered) == 1
