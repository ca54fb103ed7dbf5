"""The shape of the binding layer (`isdf_amd.hot_path`) after its split by feature: which methods `HotPath` binds, that every
`super()` call inside a mix-in still reaches the trainer's own method, what `trainer._hip` (a `HipState`) carries and with
which defaults, what of it a checkpoint restores, and the module's import surface.  Host logic only: the engine is
`tests.fake_engine.FakeEngine`."""
import contextlib
import dataclasses
import io
import sys

import numpy as np
import pytest
import torch

from bench_support.driver_loop import run_train_loop
from bench_support.standin_trainer import HipTrainer, StandinTrainer
from tests import golden_util as gu
from tests.accuracy_experiment import config
from tests.fake_engine import FakeEngine

BOUND = {"sample_points", "sdf_eval_and_loss", "step", "is_keyframe", "get_data", "get_sdf_grid", "mesh_rec", "render_depth_vis",
         "render_normals_vis", "latest_frame_vis", "drop_eval_cache", "eval_sdf", "eval_sdf_visible", "eval_object_sdf",
         "eval_traj_cost", "eval_mesh", "eval_fixed", "compute_slices", "obj_slices_vis", "get_sdf_grid_pc",
         "check_keyframe_latest", "add_frame", "hip_state_dict", "load_hip_state_dict"}


def _cfg():
    cfg = config(dict(H=48, W=64, fx=60.0, fy=60.0, cx=31.5, cy=23.5))
    cfg["model"].update(hidden_feature_size=64, hidden_layers_block=1)
    cfg["sample"].update(n_rays=4, n_rays_is_kf=8)
    return cfg


def _trainer(**kw):
    return HipTrainer("cpu", _cfg(), inv_bounds_transform=gu.bounds_transform(), engine_factory=FakeEngine, **kw)


def test_hotpath_binds_exactly_the_documented_methods():
    from isdf_amd.hot_path import HotPath
    from isdf_amd.mesh import MeshMethods
    from isdf_amd.metrics import EvalMethods
    from isdf_amd.render import RenderMethods
    from isdf_amd.slices import SliceMethods
    assert HotPath.__bases__ == (MeshMethods, RenderMethods, EvalMethods, SliceMethods)
    public = {n for c in HotPath.__mro__ if c is not object for n in vars(c) if not n.startswith("_")}
    assert public == BOUND | {"engine"}, public ^ (BOUND | {"engine"})
    assert isinstance(HotPath.engine, property)
    for n in BOUND:
        assert callable(getattr(HotPath, n)), n


class _Toy(StandinTrainer):
    """a trainer base whose own versions of the methods the mix-ins defer to answer with sentinels"""

    def get_data(self, idxs):
        return ("base get_data", idxs)

    def latest_frame_vis(self, do_render=True):
        return ("base latest_frame_vis", do_render)

    def eval_fixed(self):
        return "base eval_fixed"

    def check_keyframe_latest(self):
        return "base check_keyframe_latest"

    def add_frame(self, frame_data):
        return ("base add_frame", frame_data)


def test_super_calls_in_the_mixins_reach_the_trainer_base():
    from isdf_amd.hot_path import HotPath, graft
    tr = graft(_Toy("cpu", _cfg(), inv_bounds_transform=gu.bounds_transform(), engine_factory=FakeEngine),
               engine_factory=FakeEngine)
    assert type(tr).__name__ == "Hip_Toy" and type(tr).__mro__[:2] == (type(tr), HotPath) and isinstance(tr, _Toy)
    for n in ("get_data", "latest_frame_vis", "eval_fixed", "check_keyframe_latest", "add_frame"):
        assert getattr(type(tr), n) is getattr(HotPath, n), n
    tr.do_normal = False
    assert tr.get_data([3]) == ("base get_data", [3])
    assert tr.latest_frame_vis(do_render=False) == ("base latest_frame_vis", False)
    assert tr.dataset_format not in ("replicaCAD", "ScanNet")
    assert tr.eval_fixed() == "base eval_fixed"
    assert tr._hip.dist_group is None
    assert tr.check_keyframe_latest() == "base check_keyframe_latest"
    frame = object()
    assert tr.add_frame(frame) == ("base add_frame", frame)


def test_hip_state_is_declared_once_with_its_defaults():
    from isdf_amd.hot_path import HipState
    tr = _trainer(seed=5)
    hip = tr._hip
    assert type(hip) is HipState and not hasattr(hip, "__dict__")
    with pytest.raises(AttributeError):
        hip.draw_cuont = 1                                  # a misspelt name is an error, not a new attribute
    with pytest.raises(AttributeError):
        hip.anything_else = None
    expected = dict(
        # configuration given to graft()
        device=torch.device("cpu"), rng="philox", dist_group=None, fix_normal_window=False, fuse_optimiser=True,
        overlap_allreduce=False, virtual_step_ms=None, inline_window=True, ref_module=sys.modules[StandinTrainer.__module__],
        geometry_transform=None,
        # counters saved by hip_state_dict()
        seed=5, draw_count=0, noise_count=0, step_count=0, prev_step_ms=0.0, window_rng_state=None,
        # caches that are never saved
        idx_cache=None, timing_events=None, prof_events=None, pinned_key=None, pinned_ok=False, ingest_launches=0,
        render_count=0, gt_volume=None, eval_cache=None, slice_cmaps={},
        # data-parallel state
        rank=0, world=1, clock_slots=0, rccl=None, collective=None, split_event=None, comm_stream=None)
    names = [f.name for f in dataclasses.fields(HipState)]
    assert set(names) == set(expected) | {"loss_host"} and len(names) == len(set(names))
    for k, v in expected.items():
        got = getattr(hip, k)
        assert got == v and type(got) is type(v), (k, got, v)
    assert hip.loss_host.shape == (8,) and hip.loss_host.dtype == torch.float32 and not hip.loss_host.any()
    # every default but the ones graft() computes is the dataclass's own
    computed = {"device", "seed", "ref_module", "slice_cmaps", "loss_host"}
    for f in dataclasses.fields(HipState):
        if f.name not in computed:
            assert f.default == expected[f.name], f.name


def test_checkpoint_round_trip_restores_the_saved_counters():
    depth, _, T = gu.synth_frames(np.random.RandomState(5), 4, 48, 64, 60.0, 60.0, 31.5, 23.5)
    np.random.seed(3); torch.manual_seed(3)
    tr = _trainer(seed=7, virtual_step_ms=12.0)
    with contextlib.redirect_stdout(io.StringIO()):
        n, _, _ = run_train_loop(tr, lambda i: tr.make_frame(i, depth[i], T[i]), depth.shape[0], 3, first_frame_iters=60)
    assert n == 3
    tr._hip.prev_step_ms = 1.25                             # (only data parallelism moves it: give it a value to carry)
    sd = tr.hip_state_dict()
    assert tr._hip.step_count == 3 and tr._hip.draw_count == 3 and tr._hip.noise_count == 3
    tr2 = _trainer(seed=1, virtual_step_ms=12.0)
    tr2._hip.idx_cache = ("stale",)
    tr2.load_hip_state_dict(sd)
    for k in ("draw_count", "noise_count", "seed", "step_count", "prev_step_ms"):
        assert getattr(tr2._hip, k) == getattr(tr._hip, k), k
    assert (tr2._hip.seed, tr2._hip.prev_step_ms) == (7, 1.25)
    assert tr2._hip.idx_cache is None
    assert tr2.tot_step_time == tr.tot_step_time and len(tr2.frames) == len(tr.frames) == 1
    # nothing but the documented counters of the state object is in the checkpoint
    assert set(sd["rng"]) == {"draw_count", "noise_count", "seed", "window", "numpy", "torch", "torch_cuda"}
    assert {"step_count", "prev_step_ms"} <= set(sd["clock"])


def test_import_surface_of_hot_path():
    import isdf_amd.hot_path as hp
    for n in ("FlatAdamW", "HotPath", "StepLosses", "graft", "can_graft", "unsupported_reason", "ENGINE_FACTORY", "FRAME_FIELDS",
              "UNSUPPORTED_HINT", "HipState"):
        assert hasattr(hp, n), n
    from isdf_amd.hot_path import (FlatAdamW, HotPath, StepLosses, graft, can_graft, unsupported_reason,      # noqa: F401
                                   ENGINE_FACTORY, FRAME_FIELDS, UNSUPPORTED_HINT)
    assert FRAME_FIELDS[-1] == "count" and len(FRAME_FIELDS) == 12
