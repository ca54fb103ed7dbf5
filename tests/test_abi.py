"""CPU-side checks of the C-ABI library.  The first three tests hold the whole Python side of the boundary (isdf_amd/_ffi.py:
PROTOTYPES, STRUCTS and the constants) to include/isdf_hip.h, table-driven through tests/abi_util.py; the rest check that the
library loads and that its size queries (pure host code) are right.  No kernel is launched here."""
import ctypes as C

import numpy as np

import pytest

from isdf_amd import _ffi, build
from tests import abi_util as au


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _ffi.lib()


def test_every_prototype_is_bound_as_the_header_declares_it(lib):
    """all functions of the header: declared, exported, and bound in _ffi.PROTOTYPES with the restype and every argtype the
    header's C types require (abi_util.bindings)"""
    declared = au.prototypes()
    assert list(declared) == _ffi.SYMBOLS and len(declared) >= 55
    for name, (ret, params) in declared.items():
        fn = getattr(lib, name)
        assert fn.restype in au.bindings(ret, _ffi.STRUCTS), (name, ret, fn.restype)
        assert len(fn.argtypes) == len(params), name
        for k, (c_type, bound) in enumerate(zip(params, fn.argtypes)):
            assert bound in au.bindings(c_type, _ffi.STRUCTS), (name, k, c_type, bound)


def test_ctypes_structs_match_the_header_layout(tmp_path):
    """every struct that crosses the boundary: the mirror in _ffi.STRUCTS names the header's fields in the header's order, and its
    size and every field offset are what gcc makes of include/isdf_hip.h (a silent mismatch would hand the kernels shifted
    pointers)"""
    assert au.struct_fields("isdf_tsdf_args")[:8] == ["nx", "ny", "nz", "F", "H", "W", "origin", "spacing"]     # the parser itself:
    assert au.struct_fields("isdf_gt_volume") == ["values", "nx", "ny", "nz", "reserved", "spacing", "origin"]  # commas and arrays
    assert au.struct_fields("isdf_step_out")[4:6] == ["prof_events", "host_mailbox"]                            # void**
    assert sorted(au.struct_names()) == sorted(_ffi.STRUCTS) and len(_ffi.STRUCTS) >= 16
    sizes, offsets, _ = au.probe(tmp_path, structs=_ffi.STRUCTS)
    for name, ct in _ffi.STRUCTS.items():
        fields = [f for f, _ in ct._fields_]
        assert fields == au.struct_fields(name), name
        assert C.sizeof(ct) == sizes[name], name
        assert {f: getattr(ct, f).offset for f in fields} == offsets[name], name


# upper-case integers of _ffi that the header does not define: the bits of isdf_region_args.flags, which it documents in prose
NOT_IN_HEADER = {"FLAG_VIS_SDF", "FLAG_VOX_SDF", "FLAG_VIS_GRAD", "FLAG_VOX_GRAD"}
MIRRORED = {"ABI_VERSION", "MC_MAX_TRIS", "LS_SDF", "LS_GRAD", "LS_EIK", "LS_TOTAL", "LS_COUNT", "MAX_INLINE_FRAMES", "RANGE_SCALAR",
            "RANGE_DEPTH", "RANGE_UPSAMPLE", "COLORMAP_MAX_COLORS", "METRICS_RECORD", "SDF_METRICS_WS_BYTES", "REGION_RECORD",
            "REGION_METRICS_WS_BYTES", "POSE_RECORD", "POSE_MAX_BLOCKS", "TRAJ_RECORD", "TRAJ_MAX_WAYPOINTS", "TRAJ_MAX_SPHERES",
            "TRAJ_MAX_TRAJ", "EDT_NONE", "EDT_MAX_SIDE", "TRI_TILE", "TRI_SLOT_FLOATS", "TRI_RECORD", "ROUTE_NONE", "ROUTE_MAX_VOXELS",
            "ROUTE_TILE"}


def test_constants_and_size_macros_equal_the_header_s(tmp_path):
    """every upper-case integer X of _ffi equals ISDF_X (a macro or an enumerator) as gcc evaluates it, or is on NOT_IN_HEADER;
    the set that is compared never shrinks; the two size functions equal the header's function-like macros"""
    header = set(au.constant_names())
    mine = {k: v for k, v in vars(_ffi).items() if k.isupper() and type(v) is int}
    matched = {k for k in mine if "ISDF_" + k in header}
    assert set(mine) - matched == NOT_IN_HEADER
    assert matched >= MIRRORED
    sizes = (0, 1, 256, 257, 200000)
    macros = ["ISDF_NN_WS_BYTES(%d)" % n for n in sizes] + ["ISDF_TRI_PACKED_BYTES(%d)" % n for n in sizes]
    _, _, values = au.probe(tmp_path, constants=["ISDF_" + k for k in sorted(matched)], macros=macros)
    assert {k: mine[k] for k in matched} == {k: values["ISDF_" + k] for k in matched}
    for n in sizes:
        assert _ffi.nn_ws_bytes(n) == values["ISDF_NN_WS_BYTES(%d)" % n], n
        assert _ffi.tri_packed_bytes(n) == values["ISDF_TRI_PACKED_BYTES(%d)" % n], n


def test_abi_version_and_errors(lib):
    assert lib.isdf_abi_version() == _ffi.ABI_VERSION
    assert lib.isdf_error_string(0) == b"ok"
    assert b"invalid" in lib.isdf_error_string(-1)


def test_size_queries_default_net(lib):
    from isdf_amd.engine import NetConfig
    c = NetConfig().to_c()
    assert lib.isdf_param_count(C.byref(c)) == 460033          # probe of the reference net
    assert lib.isdf_reduce_floats(C.byref(c), 5) == 460033 + 8 + 2 * 5 * 64
    sh = lib.isdf_shadow_bytes(C.byref(c))
    fwd = 256 * 256 + 4 * 256 * 256 + 256 * 512
    bwd = 5 * 256 * 256 + 256 * 512
    assert sh == 2 * (3 * fwd + 2 * bwd)      # default "fp16x2": + one forward set of fp16 weight residuals
    for op, sets in (("fp16", 2), ("bf16", 2)):
        assert lib.isdf_shadow_bytes(C.byref(NetConfig(fwd_operand=op).to_c())) == 2 * (sets * fwd + 2 * bwd)
    full = NetConfig(fwd_operand="fp16x2_full").to_c()       # exact-forward instrument: same residual set, used by every layer
    assert lib.isdf_shadow_bytes(C.byref(full)) == sh and lib.isdf_check_net(C.byref(full)) == 0
    for wide in (NetConfig(fwd_operand="fp16x2_full", n_freqs=9, blocks=3), NetConfig(fwd_operand="fp16x2_full", hidden=512, n_freqs=10)):
        assert lib.isdf_check_net(C.byref(wide.to_c())) == -2     # ISDF_EUNSUPPORTED: four operand regions do not fit those tiles
    # any hidden_feature_size up to 512 runs zero-padded on the 256 / 512 tiles; the parameter vector keeps the reference's shapes
    for hidden, blocks, nf in ((64, 1, 6), (64, 3, 11), (128, 2, 6), (300, 2, 6)):
        nc = NetConfig(hidden=hidden, blocks=blocks, n_freqs=nf)
        assert lib.isdf_check_net(C.byref(nc.to_c())) == 0
        assert lib.isdf_param_count(C.byref(nc.to_c())) == sum(int(np.prod(sh)) for _, sh in nc.param_shapes())
    assert lib.isdf_check_net(C.byref(NetConfig(hidden=513).to_c())) == -2
    bad = NetConfig().to_c()
    bad.fwd_operand = 4
    assert lib.isdf_shadow_bytes(C.byref(bad)) == -1
    assert lib.isdf_workspace_bytes(C.byref(c), 27000, 1) > lib.isdf_workspace_bytes(C.byref(c), 27000, 0) > 0


def test_invalid_arguments_are_reported_not_crashed(lib):
    assert lib.isdf_param_count(None) == -1
    from isdf_amd.engine import NetConfig
    bad = NetConfig(blocks=0).to_c()
    assert lib.isdf_param_count(C.byref(bad)) == -1
    assert lib.isdf_sample_rays(None, None, None, 0, None) == -1
    assert lib.isdf_adamw(C.byref(NetConfig().to_c()), None, None, None, None, None, 1.0, 1e-3, 0.9, 0.999,
                          1e-8, 0.0, 1, None, None) == -1


def test_param_layout_matches_reference_state_dict_order():
    from isdf_amd.engine import NetConfig
    import oracle.isdf_oracle as orc
    import numpy as np
    net = NetConfig()
    ref = orc.init_params(256, 2, 6, np.random.RandomState(0))
    assert [k for k, _ in net.param_shapes()] == list(ref.keys())
    assert all(tuple(ref[k].shape) == tuple(s) for k, s in net.param_shapes())


def test_engine_refuses_cpu():
    from isdf_amd.engine import Engine, NetConfig
    with pytest.raises(_ffi.IsdfError):
        Engine(NetConfig(), "cpu")


def test_allreduce_entry_point_checks_its_arguments_and_reports_a_refusing_collective():
    """isdf_allreduce_sum_f32 (the data-parallel step's collective on the step's own stream): no collective library is linked, the
    caller passes RCCL's ncclAllReduce -- here a stand-in that refuses, which never touches the buffer, so this runs without a GPU."""
    import ctypes as C
    lib = _ffi.lib()
    buf = (C.c_float * 16)()
    assert lib.isdf_allreduce_sum_f32(None, 1, C.addressof(buf), 16, None) == -1          # ISDF_EINVAL: no function
    assert lib.isdf_allreduce_sum_f32(1, None, C.addressof(buf), 16, None) == -1          # ... no communicator
    assert lib.isdf_allreduce_sum_f32(1, 1, None, 16, None) == -1
    assert lib.isdf_allreduce_sum_f32(1, 1, C.addressof(buf), 0, None) == -1
    seen = []

    def refuse(send, recv, count, dtype, op, comm, stream):
        seen.append((send, recv, count, dtype, op, comm))
        return 5
    fn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p)(refuse)
    rc = lib.isdf_allreduce_sum_f32(C.cast(fn, C.c_void_p).value, 0x1234, C.addressof(buf), 16, None)
    assert rc == -5 and b"ncclResult_t 5" in lib.isdf_error_string(rc)                   # ISDF_ECOLLECTIVE
    # in place, fp32 (ncclFloat32 = 7), sum (ncclSum = 0), the caller's communicator
    assert seen == [(C.addressof(buf), C.addressof(buf), 16, 7, 0, 0x1234)]


def test_rccl_direct_is_off_for_non_rccl_groups():
    from isdf_amd import dp
    assert dp.rccl_direct(None, "cpu") is None
