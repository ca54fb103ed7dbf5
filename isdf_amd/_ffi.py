"""ctypes binding of include/isdf_hip.h (the C-ABI drop-in boundary).

Loads the in-tree `libisdf_hip.so` built by `isdf_amd/build.py`.  There is NO
fallback: if the library is missing or a call fails, an exception is raised --
the product path never routes around the HIP kernels.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# ISDF_HIP_LIB: development override (A/B variants and the instrumented build of tools/build_variants.py)
LIB_PATH = os.environ.get("ISDF_HIP_LIB") or os.path.join(HERE, "libisdf_hip.so")

ABI_VERSION = 8

MC_MAX_TRIS = 5      # ISDF_MC_MAX_TRIS

LS_SDF, LS_GRAD, LS_EIK, LS_TOTAL, LS_COUNT = 0, 1, 2, 3, 4


class NetCfg(C.Structure):
    _fields_ = [("hidden", C.c_int32), ("blocks", C.c_int32), ("n_freqs", C.c_int32),
                ("has_transform", C.c_int32), ("scale_input", C.c_float),
                ("scale_output", C.c_float), ("bounds_T", C.c_float * 12),
                ("fwd_operand", C.c_int32), ("bwd_operand", C.c_int32), ("spill_operand", C.c_int32)]


class SampleArgs(C.Structure):
    _fields_ = [("depth_batch", C.c_void_p), ("normal_batch", C.c_void_p),
                ("T_WC_batch", C.c_void_p), ("frame_idx", C.c_void_p), ("normal_idx", C.c_void_p),
                ("n_frames", C.c_int32), ("n_rays", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("n_strat", C.c_int32), ("n_surf", C.c_int32), ("min_depth", C.c_float),
                ("dist_behind_surf", C.c_float), ("rng_mode", C.c_int32),
                ("draw_h", C.c_void_p), ("draw_w", C.c_void_p), ("draw_u", C.c_void_p),
                ("draw_n", C.c_void_p), ("seed", C.c_uint64), ("offset", C.c_uint64),
                ("n_inline", C.c_int32), ("frame_idx_inline", C.c_int32 * 8), ("normal_idx_inline", C.c_int32 * 8),
                ("reserved_inline", C.c_int32)]


class SampleOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in
                ["n_valid", "indices_b", "indices_h", "indices_w", "depth_sample", "dirs_C_sample",
                 "norm_sample", "T_WC_sample", "dirs_W_sample", "z_vals", "pc"]]


class LossCfg(C.Structure):
    _fields_ = [("bounds_method", C.c_int32), ("loss_type", C.c_int32),
                ("trunc_weight", C.c_float), ("trunc_distance", C.c_float),
                ("eik_weight", C.c_float), ("eik_apply_dist", C.c_float),
                ("grad_weight", C.c_float), ("orien_loss", C.c_int32)]


class StepArgs(C.Structure):
    _fields_ = [("n_valid", C.c_void_p), ("max_rays", C.c_int32), ("S", C.c_int32),
                ("n_frames", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("pc", C.c_void_p), ("z_vals", C.c_void_p), ("depth_sample", C.c_void_p),
                ("dirs_C_sample", C.c_void_p), ("dirs_W_sample", C.c_void_p),
                ("norm_sample", C.c_void_p), ("indices_b", C.c_void_p), ("indices_h", C.c_void_p),
                ("indices_w", C.c_void_p), ("noise", C.c_void_p), ("noise_std", C.c_float),
                ("reserved0", C.c_uint32), ("noise_seed", C.c_uint64), ("noise_offset", C.c_uint64),
                ("pc_bounds", C.c_void_p),
                ("pc_grad_vec", C.c_void_p), ("extra_floats", C.c_int32), ("extra_slot", C.c_int32),
                ("extra_value", C.c_float), ("reserved1", C.c_int32)]


class StepOut(C.Structure):
    _fields_ = [("reduce_buf", C.c_void_p), ("sdf", C.c_void_p), ("sdf_grad", C.c_void_p),
                ("tot_loss_mat", C.c_void_p), ("prof_events", C.POINTER(C.c_void_p)), ("host_mailbox", C.c_void_p),
                ("split_event", C.c_void_p)]


class OptimArgs(C.Structure):
    _fields_ = [("params", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("shadow", C.c_void_p),
                ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("weight_decay", C.c_float), ("grad_scale", C.c_float), ("step", C.c_int32), ("reserved", C.c_int32),
                ("loss_approx", C.c_void_p), ("frame_avg", C.c_void_p), ("frame_avg_index", C.c_void_p),
                ("frame_avg_inline_n", C.c_int32), ("frame_avg_index_inline", C.c_int32 * 8), ("reserved_inline", C.c_int32)]
MAX_INLINE_FRAMES = 8


class McArgs(C.Structure):
    _fields_ = [("volume", C.c_void_p), ("D0", C.c_int32), ("D1", C.c_int32), ("D2", C.c_int32), ("level", C.c_float),
                ("has_transform", C.c_int32), ("index_to_world", C.c_float * 12)]


class BandArgs(C.Structure):
    """isdf_band_args"""
    _fields_ = [("D0", C.c_int32), ("D1", C.c_int32), ("D2", C.c_int32), ("coarse", C.c_int32), ("level", C.c_float),
                ("slack", C.c_float), ("has_transform", C.c_int32), ("reserved", C.c_int32), ("index_to_world", C.c_float * 12),
                ("points", C.c_void_p)]


class PoseArgs(C.Structure):
    """isdf_pose_args (T_WC and frame_of_pose are HOST arrays)"""
    _fields_ = [("B", C.c_int32), ("F", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("stride", C.c_int32),
                ("reserved", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("min_depth", C.c_float), ("max_depth", C.c_float), ("depth", C.c_void_p), ("T_WC", C.c_void_p),
                ("frame_of_pose", C.c_void_p)]


class TrajArgs(C.Structure):
    """isdf_traj_args (offsets and radii are HOST arrays)"""
    _fields_ = [("B", C.c_int32), ("T", C.c_int32), ("S", C.c_int32), ("reserved", C.c_int32), ("eps", C.c_float),
                ("w_obs", C.c_float), ("w_smooth", C.c_float), ("eta", C.c_float), ("max_step", C.c_float), ("tol", C.c_float),
                ("x", C.c_void_p), ("state", C.c_void_p), ("offsets", C.c_void_p), ("radii", C.c_void_p)]


class ArmArgs(C.Structure):
    """isdf_arm_args (everything from base on is a HOST array)"""
    _fields_ = [("B", C.c_int32), ("T", C.c_int32), ("J", C.c_int32), ("S", C.c_int32), ("eps", C.c_float),
                ("w_obs", C.c_float), ("w_smooth", C.c_float), ("eta", C.c_float), ("max_step", C.c_float), ("tol", C.c_float),
                ("theta", C.c_void_p), ("state", C.c_void_p), ("base", C.c_void_p), ("X", C.c_void_p), ("kinds", C.c_void_p),
                ("axes", C.c_void_p), ("links", C.c_void_p), ("centres", C.c_void_p), ("radii", C.c_void_p), ("lo", C.c_void_p),
                ("hi", C.c_void_p)]


class TsdfArgs(C.Structure):
    """isdf_tsdf_args"""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("F", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("origin", C.c_float * 3), ("spacing", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("trunc", C.c_float), ("max_weight", C.c_float), ("min_depth", C.c_float),
                ("max_depth", C.c_float), ("depth", C.c_void_p), ("T_CW", C.c_void_p), ("tsdf", C.c_void_p), ("weight", C.c_void_p)]


RANGE_SCALAR, RANGE_DEPTH, RANGE_UPSAMPLE = 0, 1, 2


class RenderArgs(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("n_samples", C.c_int32),
                ("T_WC", C.c_void_p), ("dirs_C", C.c_void_p), ("range_mode", C.c_int32), ("min_depth", C.c_float),
                ("max_depth", C.c_float), ("bin_length", C.c_float), ("depth_offset", C.c_float), ("src_H", C.c_int32),
                ("src_W", C.c_int32), ("rng_mode", C.c_int32), ("src_depth", C.c_void_p), ("draw_u", C.c_void_p),
                ("seed", C.c_uint64), ("counter", C.c_uint64), ("depth_in", C.c_void_p)]

class GtVolumeArgs(C.Structure):
    _fields_ = [("values", C.c_void_p), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("reserved", C.c_int32),
                ("spacing", C.c_float * 3), ("origin", C.c_float * 3)]


class RegionArgs(C.Structure):
    """isdf_region_args"""
    _fields_ = [("pts", C.c_void_p), ("sdf", C.c_void_p), ("sdf_grad", C.c_void_p), ("flags", C.c_void_p),
                ("vol", C.POINTER(GtVolumeArgs)), ("gt_in", C.c_void_p), ("n", C.c_int64), ("grad_sets", C.c_int32),
                ("reserved", C.c_int32), ("spacing", C.c_double * 3), ("origin", C.c_double * 3), ("delta", C.c_double)]


class ColormapArgs(C.Structure):
    _fields_ = [("lut", C.c_void_p), ("n_colors", C.c_int32), ("vmin", C.c_float), ("range", C.c_float)]


COLORMAP_MAX_COLORS = 16381                           # ISDF_COLORMAP_MAX_COLORS
METRICS_RECORD = 24                                   # ISDF_METRICS_RECORD (doubles)
SDF_METRICS_WS_BYTES = 1024 * METRICS_RECORD * 8      # ISDF_SDF_METRICS_WS_BYTES
REGION_RECORD = 27                                    # ISDF_REGION_RECORD (doubles per set; a call writes two)
REGION_METRICS_WS_BYTES = 1024 * 2 * REGION_RECORD * 8    # ISDF_REGION_METRICS_WS_BYTES
POSE_RECORD = 32                                      # ISDF_POSE_RECORD (doubles per pose)
POSE_MAX_BLOCKS = 64                                  # ISDF_POSE_MAX_BLOCKS
TRAJ_RECORD = 16                                      # ISDF_TRAJ_RECORD (doubles per trajectory)
TRAJ_MAX_WAYPOINTS, TRAJ_MAX_SPHERES, TRAJ_MAX_TRAJ = 1024, 32, 65536    # ISDF_TRAJ_MAX_*
ARM_MAX_JOINTS, ARM_MAX_SPHERES, ARM_MAX_WAYPOINTS, ARM_MAX_TRAJ = 8, 64, 384, 131072    # ISDF_ARM_MAX_*
EDT_NONE, EDT_MAX_SIDE = 1 << 30, 1024              # ISDF_EDT_NONE, ISDF_EDT_MAX_SIDE
TRI_TILE, TRI_SLOT_FLOATS, TRI_RECORD = 256, 24, 4   # ISDF_TRI_TILE, ISDF_TRI_SLOT_FLOATS, ISDF_TRI_RECORD (doubles)
TRI_TILE_RECORD = 16                                  # ISDF_TRI_TILE_RECORD (doubles per tile)
ROUTE_NONE, ROUTE_MAX_VOXELS, ROUTE_TILE = 1 << 30, 1 << 27, 8    # ISDF_ROUTE_NONE, ISDF_ROUTE_MAX_VOXELS, ISDF_ROUTE_TILE
VOXEL_UNKNOWN, VOXEL_FREE, VOXEL_OCCUPIED = 0, 1, 2          # ISDF_VOXEL_*: the states of a u8 state volume (>= 2 is occupied)
FRONTIER_NONE, FRONTIER_RECORD = 1 << 30, 12                  # ISDF_FRONTIER_NONE, ISDF_FRONTIER_RECORD (int64 per cluster)
FLAG_VIS_SDF, FLAG_VOX_SDF, FLAG_VIS_GRAD, FLAG_VOX_GRAD = 1, 2, 4, 8    # isdf_region_args.flags


def nn_ws_bytes(n):
    """ISDF_NN_WS_BYTES(n)"""
    return 8 * int(n) + 8 * ((int(n) + 255) // 256) + 256


def tri_packed_bytes(m):
    """ISDF_TRI_PACKED_BYTES(m)"""
    return (int(m) + TRI_TILE - 1) // TRI_TILE * TRI_TILE * TRI_SLOT_FLOATS * 4


P, i32, i64, f32, vp = C.POINTER, C.c_int32, C.c_int64, C.c_float, C.c_void_p

# the C struct names of include/isdf_hip.h -> their mirrors above
STRUCTS = {"isdf_net_cfg": NetCfg, "isdf_sample_args": SampleArgs, "isdf_sample_out": SampleOut, "isdf_loss_cfg": LossCfg,
           "isdf_step_args": StepArgs, "isdf_step_out": StepOut, "isdf_optim_args": OptimArgs, "isdf_mc_args": McArgs,
           "isdf_render_args": RenderArgs, "isdf_gt_volume": GtVolumeArgs, "isdf_region_args": RegionArgs,
           "isdf_colormap": ColormapArgs, "isdf_band_args": BandArgs, "isdf_pose_args": PoseArgs, "isdf_traj_args": TrajArgs,
           "isdf_arm_args": ArmArgs, "isdf_tsdf_args": TsdfArgs}

# every function include/isdf_hip.h declares, in header order: name -> (restype, argtypes).  This is the one place a function is
# declared on the Python side; tests/test_abi.py holds every line (and STRUCTS, and the constants above) to the header.
PROTOTYPES = {
    "isdf_abi_version": (C.c_int, []),
    "isdf_error_string": (C.c_char_p, [C.c_int]),
    "isdf_check_net": (C.c_int, [P(NetCfg)]),
    "isdf_param_count": (i64, [P(NetCfg)]),
    "isdf_shadow_bytes": (i64, [P(NetCfg)]),
    "isdf_workspace_bytes": (i64, [P(NetCfg), i64, i32]),
    "isdf_reduce_floats": (i64, [P(NetCfg), i32]),
    "isdf_reduce_split_floats": (i64, [P(NetCfg)]),
    "isdf_pack_weights": (C.c_int, [P(NetCfg), vp, vp, vp]),
    "isdf_sample_scan_bytes": (i64, [i64]),
    "isdf_sample_rays": (C.c_int, [P(SampleArgs), P(SampleOut), vp, i64, vp]),
    "isdf_sdf_eval": (C.c_int, [P(NetCfg), vp, vp, vp, i64, vp, vp, vp, vp, i64, vp]),
    "isdf_train_step": (C.c_int, [P(NetCfg), P(LossCfg), vp, vp, P(StepArgs), P(StepOut), vp, i64, vp]),
    "isdf_train_step_adamw": (C.c_int, [P(NetCfg), P(LossCfg), P(StepArgs), P(StepOut), P(OptimArgs), vp, i64, vp]),
    "isdf_train_step_finish": (C.c_int, [P(NetCfg), P(OptimArgs), vp, i32, i32, vp, vp]),
    "isdf_allreduce_sum_f32": (C.c_int, [vp, vp, vp, i64, vp]),
    "isdf_bounds_pc": (C.c_int, [vp, i32, i32, vp, vp, vp, vp, i64, vp, vp, vp]),
    "isdf_frame_avg": (C.c_int, [vp, i64, i32, vp, vp, vp, vp]),
    "isdf_estimate_normals": (C.c_int, [vp, i32, i32, f32, f32, f32, f32, vp, vp]),
    "isdf_render_depth": (C.c_int, [vp, i64, i64, i32, vp, vp, vp, f32, vp, vp, vp]),
    "isdf_adamw": (C.c_int, [P(NetCfg), vp, vp, vp, vp, vp, f32, f32, f32, f32, f32, f32, i32, vp, vp]),
    "isdf_mesh_ws_bytes": (i64, [i32, i32, i32]),
    "isdf_marching_cubes": (C.c_int, [P(McArgs), vp, vp, vp, i64, vp, i64, vp, i64, vp]),
    "isdf_mc_tables": (C.c_int, [vp, vp]),
    "isdf_render_ws_bytes": (i64, [P(NetCfg), i32, i32, i32, i32]),
    "isdf_render_views": (C.c_int, [P(NetCfg), vp, vp, P(RenderArgs), vp, vp, vp, i64, vp]),
    "isdf_sdf_metrics": (C.c_int, [P(GtVolumeArgs), vp, vp, i64, i32, f32, vp, vp, vp, vp, i64, vp]),
    "isdf_region_metrics": (C.c_int, [P(RegionArgs), vp, vp, i64, vp]),
    "isdf_nn_distance": (C.c_int, [vp, i64, vp, i64, vp, vp, vp, vp, i64, vp]),
    "isdf_slice_images": (C.c_int, [vp, vp, i64, P(ColormapArgs), P(GtVolumeArgs), f32, f32, vp, vp, vp, vp, vp, vp]),
    "isdf_plane_points": (C.c_int, [P(f32), P(f32), P(f32), i32, i32, vp, vp]),
    "isdf_visible_points": (C.c_int, [vp, i64, vp, vp, i32, i32, i32, f32, f32, f32, f32, f32, vp, vp, vp, vp]),
    "isdf_band_ws_bytes": (i64, [i32, i32, i32, i32]),
    "isdf_band_begin": (C.c_int, [P(BandArgs), vp, vp]),
    "isdf_band_select": (C.c_int, [P(BandArgs), i32, vp, vp, vp, i64, vp]),
    "isdf_band_emit": (C.c_int, [P(BandArgs), i32, vp, vp, vp, i64, vp, i64, vp]),
    "isdf_band_update": (C.c_int, [P(BandArgs), i32, vp, vp, vp, i64, vp, vp, i64, vp]),
    "isdf_band_leaks": (C.c_int, [P(BandArgs), vp, vp, vp, i64, vp]),
    "isdf_grid_points": (C.c_int, [i32, i32, i32, P(f32), vp, vp]),
    "isdf_pose_ws_bytes": (i64, [i32]),
    "isdf_pose_points": (C.c_int, [P(PoseArgs), vp, vp]),
    "isdf_pose_system": (C.c_int, [P(PoseArgs), vp, vp, vp, f32, f32, vp, vp, i64, vp]),
    "isdf_traj_points": (C.c_int, [P(TrajArgs), vp, vp]),
    "isdf_traj_step": (C.c_int, [P(TrajArgs), vp, vp, vp, vp, vp, vp]),
    "isdf_arm_points": (C.c_int, [P(ArmArgs), vp, vp]),
    "isdf_arm_step": (C.c_int, [P(ArmArgs), vp, vp, vp, vp, vp, vp, vp]),
    "isdf_tsdf_integrate": (C.c_int, [P(TsdfArgs), vp]),
    "isdf_edt_ws_bytes": (i64, [i32, i32, i32]),
    "isdf_distance_transform": (C.c_int, [vp, i32, i32, i32, i32, vp, vp, i64, vp]),
    "isdf_occupancy_sdf": (C.c_int, [vp, i32, i32, i32, C.c_double, vp, vp, i64, vp]),
    "isdf_tri_pack": (C.c_int, [vp, i64, vp, i64, P(f32), vp, i64, vp, vp]),
    "isdf_tri_ws_bytes": (i64, [i64, i64]),
    "isdf_tri_distance": (C.c_int, [vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, i64, vp]),
    "isdf_tri_tiles_build": (C.c_int, [vp, i64, vp, i64, vp, vp, vp, vp]),
    "isdf_tri_tiles_ws_bytes": (i64, [i64]),
    "isdf_tri_distance_tiles": (C.c_int, [vp, i64, vp, vp, i64, vp, vp, i64, C.c_double, vp, vp, vp, vp, vp, vp, vp, i64, vp]),
    "isdf_route_init": (C.c_int, [vp, i32, i32, i32, vp, i32, vp, vp]),
    "isdf_route_ws_bytes": (i64, [i32, i32, i32]),
    "isdf_route_relax": (C.c_int, [vp, i32, i32, i32, vp, vp, i64, i32, vp, vp]),
    "isdf_route_trace": (C.c_int, [vp, i32, i32, i32, vp, i32, i32, vp, vp, vp]),
    "isdf_frontier_init": (C.c_int, [vp, i32, i32, i32, vp, vp]),
    "isdf_frontier_ws_bytes": (i64, [i32, i32, i32]),
    "isdf_frontier_relax": (C.c_int, [vp, i32, i32, i32, vp, i64, i32, vp, vp]),
    "isdf_frontier_clusters": (C.c_int, [vp, i32, i32, i32, vp, i64, i32, vp, vp, vp]),
    "isdf_view_gain_ws_bytes": (i64, [i32, i32, i32, i32]),
    "isdf_view_gain": (C.c_int, [vp, i32, i32, i32, P(f32), P(f32), vp, i32, f32, f32, f32, f32, i32, i32, f32, f32, vp, vp, vp, vp,
                                 i64, vp]),
}
SYMBOLS = list(PROTOTYPES)


class IsdfError(RuntimeError):
    pass


_lib = None


def lib():
    """The loaded library (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IsdfError("%s not found: run `python -m isdf_amd.build` (or __graft_entry__.build())"
                        % LIB_PATH)
    # torch first: its bundled HIP runtime then answers the library's libamdhip64.so.7 as well.  Loaded the other way round, the
    # process holds two HIP runtimes (torch asks for the unversioned name), and the library's own finds no device next to torch's.
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    if L.isdf_abi_version() != ABI_VERSION:
        raise IsdfError("libisdf_hip.so ABI %d != binding ABI %d" % (L.isdf_abi_version(), ABI_VERSION))
    _lib = L
    return L


def check(rc, what):
    if rc != 0:
        raise IsdfError("%s failed: %s (%d)" % (what, lib().isdf_error_string(int(rc)).decode(), rc))


def ptr(t):
    """device/host pointer of a torch tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())
