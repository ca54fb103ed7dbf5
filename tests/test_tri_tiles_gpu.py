"""The tile index and the culled distance on the device: isdf_tri_tiles_build / isdf_tri_distance_tiles through Engine and
isdf_amd.mesh_sdf.  The oracle for distance, index, nearest point and record is the device's own brute-force call on the same inputs
(tests/test_tri_gpu.py pins that call to the float32 model): every output must have its bits.  The tile records, the staging counts
and the far-field winding number are held to tests/tri_tiles_model.py."""
import itertools

import numpy as np
import pytest
import torch

from isdf_amd import _ffi, mesh_sdf, synthetic as syn
from isdf_amd.engine import morton_order
from tests import tri_model as tm, tri_tiles_model as ttm
from tests.test_tri_gpu import HAND, ONE, WIND_GAP, _soup
from tests.test_tri_tiles_cpu import bricks

pytestmark = pytest.mark.gpu

TILE = _ffi.TRI_TILE
BLOCK = 1024
PAD = [-1] * (TILE - 1)


@pytest.fixture(scope="module")
def eng():
    from isdf_amd.engine import Engine, NetConfig
    return Engine(NetConfig(hidden=64, blocks=1), "cuda")


@pytest.fixture(scope="module")
def pts():
    return np.random.RandomState(0).uniform(syn.ROOM_LO - 0.5, syn.ROOM_HI + 0.5, (4096, 3)).astype(np.float32)


@pytest.fixture(scope="module")
def room4(eng, pts):
    """room_mesh(4) in the default order against the seeded points: the index, one brute-force call and one call through the tiles
    with every output, shared and left unchanged"""
    v, f = syn.room_mesh(4)
    mesh = mesh_sdf.PackedMesh(eng, v, f)
    tiles, clean = mesh.tiles()
    qperm = morton_order(torch.from_numpy(pts).cuda())
    brute = eng.tri_distance(mesh.packed, mesh.n_faces, pts, want_index=True, want_closest=True, want_winding=True)
    out = eng.tri_distance_tiles(mesh.packed, mesh.n_faces, tiles, clean, pts, qperm, beta=3.0, want_index=True, want_closest=True,
                                 want_winding=True, want_stats=True)
    return dict(v=v, f=f, mesh=mesh, tiles=tiles, clean=clean, qperm=qperm, brute=brute, out=out)


def _int(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def assert_same_outputs(got, want, what="", which=(0, 1, 2, 4)):
    """dist, index, closest and record: the same bits (NaN included)"""
    for k in which:
        assert torch.equal(_int(got[k]), _int(want[k])), "%s: output %d differs at %d places" % (
            what, k, int((_int(got[k]) != _int(want[k])).sum()))


def solid64_device(rows, P):
    """tri_tiles_model.solid64 in torch float64 on the device (the reference, not the code under test)"""
    r = torch.from_numpy(np.asarray(rows, np.float64)).cuda()
    q = torch.from_numpy(np.asarray(P, np.float64)).cuda()[:, None, :]
    a, b, c = r[None, :, 0:3] - q, r[None, :, 12:15] - q, r[None, :, 16:19] - q
    la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
    det = (a * torch.linalg.cross(b, c)).sum(-1)
    den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
    return (2.0 * torch.atan2(det, den)).sum(1).cpu().numpy()


def winding64_device(packed, p, chunk=512):
    """tri_model.winding64 over the valid slots of `packed`, in torch float64 on the device"""
    rows = packed[packed[:, 15] != 0]
    return np.concatenate([solid64_device(rows, p[i:i + chunk]) for i in range(0, len(p), chunk)]) / (4.0 * np.pi)


def check_equal(eng, v, f, p, order=None, qperms=(None,), transform=None):
    """brute force against the tiles on the same pack, for every qperm given; returns the brute-force outputs"""
    packed, _, m = eng.tri_pack(v, f, transform)
    if order is None:
        order = mesh_sdf.tile_order(packed, m)
    tiles, clean, counts = eng.tri_tiles_build(packed, m, order)
    brute = eng.tri_distance(packed, m, p, want_index=True, want_closest=True)
    assert counts.tolist() == [0, int((packed[:, 15] != 0).sum())]
    for qperm in qperms:
        got = eng.tri_distance_tiles(packed, m, tiles, clean, p, qperm, want_index=True, want_closest=True)
        assert_same_outputs(got, brute, "m %d n %d" % (m, len(p)))
    return brute


def test_room_mesh_bit_equal_to_brute_force(eng, room4, pts):
    assert_same_outputs(room4["out"], room4["brute"], "morton qperm")
    assert len(np.unique(room4["brute"][1].cpu().numpy())) > 100      # most points are nearest to a wall
    m = room4["mesh"]
    rng = np.random.RandomState(1)
    for qperm in (np.arange(len(pts)), rng.permutation(len(pts))):
        got = eng.tri_distance_tiles(m.packed, m.n_faces, room4["tiles"], room4["clean"], pts, qperm, want_index=True,
                                     want_closest=True)
        assert_same_outputs(got, room4["brute"], "qperm")
    # a reversed and a random order of the faces: other tiles, the same bits
    for order in (room4["clean"].flip(0), rng.permutation(m.n_faces)):
        tiles, clean, counts = eng.tri_tiles_build(m.packed, m.n_faces, order)
        assert counts.tolist() == [0, m.n_faces]
        got = eng.tri_distance_tiles(m.packed, m.n_faces, tiles, clean, pts, room4["qperm"], want_index=True, want_closest=True)
        assert_same_outputs(got, room4["brute"], "order")


def test_one_triangle_every_region_and_border(eng):
    p = np.concatenate([np.array([h[0] for h in HAND], np.float32), np.random.RandomState(3).uniform(-3, 7, (200, 3)).astype(np.float32)])
    brute = check_equal(eng, ONE[0], ONE[1], p, qperms=(None, np.arange(len(p))))
    assert np.array_equal(brute[2].cpu().numpy()[:len(HAND)], np.array([h[1] for h in HAND], np.float32))
    check_equal(eng, ONE[0], ONE[1], p, order=[-1, -1, 0], transform=np.array([[0, -2, 0, 1], [0.5, 0, 0, -3], [0, 0, 1.5, 0.25]], np.float32))


@pytest.mark.parametrize("faces_order", [(0, 1), (1, 0)])
@pytest.mark.parametrize("tile_order", [(0, 1), (1, 0)])
def test_the_lower_index_wins_a_tie_across_tiles(eng, faces_order, tile_order):
    """the shared edge and vertices of tests/test_tri_gpu.py, the two tying faces in tiles of their own, visited in either order"""
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [4, 4, 0]], np.float32)
    faces = np.array([[0, 1, 2], [1, 3, 2]], np.int32)[list(faces_order)]
    p = np.array([[2, 2, 1], [3, 1, -2], [1, 3, 0.5], [5, -1, 0], [-1, 5, 1], [4, 0, 3], [2, 2, 0], [3.5, 3.5, 1]], np.float32)
    order = [tile_order[0]] + PAD + [tile_order[1]] + PAD
    brute = check_equal(eng, v, faces, p, order=order, qperms=(None, np.arange(8), np.arange(8)[::-1].copy()))
    assert brute[1].cpu().numpy().tolist() == [0] * 7 + [faces_order.index(1)]


def test_queries_on_axis_aligned_faces_keep_their_exact_zeros(eng, room4):
    """1 024 points on each of two walls of the room: one block each whose U is 0 after the seed, so that only tiles
    whose box touches the block's are staged -- and every distance is exactly 0 as brute force has it"""
    g = np.stack(np.meshgrid(np.arange(32), np.arange(32), indexing="ij"), -1).reshape(-1, 2).astype(np.float32) * np.float32(0.03125)
    lo = syn.ROOM_LO.astype(np.float32)
    back = np.concatenate([lo[0] + 1 + g[:, :1], lo[1] + np.float32(0.5) + g[:, 1:], np.full((BLOCK, 1), lo[2], np.float32)], 1)
    wall = np.concatenate([np.full((BLOCK, 1), lo[0], np.float32), lo[1] + np.float32(0.5) + g[:, :1], lo[2] + 1 + g[:, 1:]], 1)
    p = np.concatenate([back, wall])
    m = room4["mesh"]
    brute = eng.tri_distance(m.packed, m.n_faces, p, want_index=True, want_closest=True)
    got = eng.tri_distance_tiles(m.packed, m.n_faces, room4["tiles"], room4["clean"], p, np.arange(len(p)), want_index=True,
                                 want_closest=True, want_stats=True)
    assert_same_outputs(got, brute, "on faces")
    assert (brute[0] == 0).all()
    model = ttm.run(m.packed.cpu().numpy(), room4["tiles"].cpu().numpy(), room4["clean"].cpu().numpy(), p)
    print("on faces: staged %s of %d" % (model["stats"], 2 * 61))
    assert got[5].tolist() == model["stats"] and model["stats"][0] <= 2 * 61 // 4


@pytest.mark.parametrize("m", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_sizes_around_the_tile(eng, m):
    v, f, p = _soup(m, BLOCK + 1, m)
    check_equal(eng, v, f, p, qperms=(None, np.arange(len(p))))


@pytest.mark.parametrize("n", [1, BLOCK - 1, BLOCK, BLOCK + 1])
def test_sizes_around_the_block(eng, n):
    v, f, p = _soup(2 * TILE + 3, n, 1000 + n)
    rng = np.random.RandomState(n)
    check_equal(eng, v, f, p, qperms=(None, rng.permutation(n)))
    check_equal(eng, v, f, p, order=rng.permutation(2 * TILE + 3))
    check_equal(eng, v, f, p, order=np.arange(2 * TILE + 3)[::-1].copy())


def test_skipped_faces_an_all_invalid_mesh_and_non_finite_points(eng):
    v, f = syn.room_mesh(1)
    v_bad = np.concatenate([v, [[np.nan, 1.0, 1.0], [0, 0, 0], [1, 1, 1], [3, 3, 3]]])
    nv = len(v)
    faces = np.concatenate([f[:50], [[0, 0, 0], [nv, 1, 2], [nv + 1, nv + 2, nv + 3]], f[50:], [[2, 2, 9]]]).astype(np.int32)
    p = np.random.RandomState(2).uniform(syn.ROOM_LO - 0.5, syn.ROOM_HI + 0.5, (1500, 3)).astype(np.float32)
    p[[0, 255, 256, 700, 1499], [0, 1, 2, 0, 1]] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    packed, counts, m = eng.tri_pack(v_bad, faces)
    assert counts.tolist() == [1, 3]
    tiles, clean, tcounts = eng.tri_tiles_build(packed, m, mesh_sdf.tile_order(packed, m))
    assert tcounts.tolist() == [0, m - 4]
    # a skipped slot that an order lists all the same is cleaned, not counted as bad, and never wins
    tiles2, clean2, tcounts2 = eng.tri_tiles_build(packed, m, np.arange(m))
    assert tcounts2.tolist() == [0, m - 4] and (clean2[[50, 51, 52, m - 1]] == -1).all()
    brute = eng.tri_distance(packed, m, p, want_index=True, want_closest=True, want_winding=True)
    for t, c in ((tiles, clean), (tiles2, clean2)):
        got = eng.tri_distance_tiles(packed, m, t, c, p, beta=0.0, want_index=True, want_closest=True, want_winding=True)
        assert_same_outputs(got, brute, "skipped faces")
        w, wb = got[3].cpu().numpy(), brute[3].cpu().numpy()
        assert np.array_equal(np.isnan(w), np.isnan(wb)) and np.isnan(w).sum() == 5
        assert np.nanmax(np.abs(w - wb)) <= 4 * WIND_GAP
    assert brute[4].cpu().numpy()[1:3].tolist() == [1495.0, 5.0]
    # no valid face at all, and no face at all: +inf, -1, NaN and a winding number of 0 (NaN for the non-finite points)
    vv = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [np.nan, 0, 0]], np.float32)
    q = np.array([[0.5, 0.5, 0.5], [np.nan, 0, 0], [1, 2, 3], [0, np.inf, 0], [0, 0, -np.inf]], np.float32)
    for faces in (np.array([[0, 1, 2], [0, 0, 1], [0, 1, 3], [0, 1, 7]], np.int32), np.zeros((0, 3), np.int32)):
        packed, _, m = eng.tri_pack(vv, faces)
        tiles, clean, tcounts = eng.tri_tiles_build(packed, m, mesh_sdf.tile_order(packed, m))
        assert tcounts.tolist() == [0, 0] and (tiles[:, 14] == 0).all()
        brute = eng.tri_distance(packed, m, q, want_index=True, want_closest=True, want_winding=True)
        got = eng.tri_distance_tiles(packed, m, tiles, clean, q, beta=3.0, want_index=True, want_closest=True, want_winding=True)
        assert_same_outputs(got, brute, "no valid face", which=(0, 1, 2, 3, 4))
        assert got[4].cpu().numpy().tolist() == [np.inf, 2.0, 3.0, np.inf]
    # no point at all: the record of nothing
    assert eng.tri_distance_tiles(packed, m, tiles, clean, np.zeros((0, 3), np.float32))[4].cpu().numpy().tolist() == [0.0] * 4


def test_tile_records_against_the_model(eng, room4):
    packed = room4["mesh"].packed.cpu().numpy()
    order = mesh_sdf.tile_order(room4["mesh"].packed, room4["mesh"].n_faces)
    tiles, clean, counts = ttm.build64(packed, order.cpu().numpy())
    got = room4["tiles"].cpu().numpy()
    assert np.array_equal(room4["clean"].cpu().numpy(), clean) and counts == [0, room4["mesh"].n_faces]
    assert np.array_equal(got[:, 0:6], tiles[:, 0:6])                               # the boxes: exact float values, bit for bit
    assert np.array_equal(got[:, 14:16], tiles[:, 14:16])
    full = tiles[:, 14] > 0
    assert full.sum() == 61 and (got[~full, 6:14] == 0).all()
    # double sums of 256 terms: N against the tile's area (it may cancel), c against the mesh's extent, r and the area themselves
    scale = np.concatenate([np.repeat(tiles[full, 13:14], 3, 1), np.full((full.sum(), 3), 6.0), tiles[full, 12:14]], 1)
    rel = np.abs(got[full, 6:14] - tiles[full, 6:14]) / scale
    print("largest relative difference of the dipole fields %.2e" % rel.max())
    assert rel.max() <= 1e-12


def test_bad_order_and_qperm_entries_are_counted_and_nothing_goes_through_them(eng, room4, pts):
    m = room4["mesh"]
    slots = int(m.packed.shape[0])
    order = mesh_sdf.tile_order(m.packed, m.n_faces).clone()
    lost = order[[3, 300, 301]].tolist()
    order[[3, 300, 301]] = torch.tensor([slots, -7, 0x7fffffff], dtype=torch.int32, device=order.device)
    tiles, clean, counts = eng.tri_tiles_build(m.packed, m.n_faces, order)
    assert counts.tolist() == [3, m.n_faces - 3] and (clean[[3, 300, 301]] == -1).all()
    with pytest.raises(ValueError, match="3 entries outside"):
        m.tiles(order=order)
    twice = mesh_sdf.tile_order(m.packed, m.n_faces).clone()
    twice[300] = twice[301]
    with pytest.raises(ValueError, match="1 slots listed twice"):
        m.tiles(order=twice)
    # the three faces are gone from the index: the result is brute force on the mesh without them
    keep = np.setdiff1d(np.arange(m.n_faces), lost)
    p = pts[:2048]
    ref = eng.tri_distance(*eng.tri_pack(room4["v"], room4["f"][keep])[::2], p, want_index=True, want_closest=True)
    got = eng.tri_distance_tiles(m.packed, m.n_faces, tiles, clean, p, want_index=True, want_closest=True)
    assert_same_outputs(got, ref, "without three faces", which=(0, 2, 4))
    assert np.array_equal(got[1].cpu().numpy(), keep[ref[1].cpu().numpy()])
    # qperm: entries outside [0, n) are skipped and counted; the queries they should have named keep +inf, -1, NaN, 0
    qperm = morton_order(torch.from_numpy(p).cuda())
    hit = qperm[[5, 1030, 2047]].long()
    qperm[[5, 1030, 2047]] = torch.tensor([-1, 2048, -(1 << 31)], dtype=torch.int32, device=qperm.device)
    full = eng.tri_distance_tiles(m.packed, m.n_faces, room4["tiles"], room4["clean"], p, beta=3.0, want_index=True, want_closest=True,
                                  want_winding=True)
    got = eng.tri_distance_tiles(m.packed, m.n_faces, room4["tiles"], room4["clean"], p, qperm, beta=3.0, want_index=True,
                                 want_closest=True, want_winding=True, want_stats=True)
    assert got[5].tolist()[2:] == [2, 3]
    assert (got[0][hit] == np.inf).all() and (got[1][hit] == -1).all() and got[2][hit].isnan().all() and (got[3][hit] == 0).all()
    rest = torch.ones(2048, dtype=torch.bool, device=hit.device)
    rest[hit] = False
    for k in range(3):
        assert torch.equal(_int(got[k])[rest], _int(full[k])[rest])


def test_stats_equal_the_model_on_bricks_and_scattered_points(eng, room4, pts):
    """what keeps a visit-everything kernel from passing: the number of tiles staged, block by block, is the model's"""
    m = room4["mesh"]
    packed, tiles, clean = m.packed.cpu().numpy(), room4["tiles"].cpu().numpy(), room4["clean"].cpu().numpy()
    b = bricks(40, 7)
    got = eng.tri_distance_tiles(m.packed, m.n_faces, room4["tiles"], room4["clean"], b, np.arange(len(b)), want_stats=True)
    model = ttm.run(packed, tiles, clean, b)
    print("bricks: staged %s, model %s, of %d" % (got[5].tolist(), model["stats"], 40 * 61))
    assert got[5].tolist() == model["stats"] and model["stats"][0] <= 40 * 61 // 4
    assert np.array_equal(got[0].cpu().numpy().view(np.uint32), model["dist"].view(np.uint32))
    model = ttm.run(packed, tiles, clean, pts, room4["qperm"].cpu().numpy())
    print("scattered points: staged %s, model %s, of %d" % (room4["out"][5].tolist(), model["stats"], 4 * 61))
    assert room4["out"][5].tolist()[0] == model["stats"][0] and room4["out"][5].tolist()[2:] == [4, 0]


def test_winding_number_against_the_model_and_sign(eng, room4, pts):
    """The device within 4 * WIND_GAP = 1.2e-5 of the float64 model of the approximation at beta = 3 (the same kind of arithmetic as
    the brute-force sum, the same bar), and of the exact float64 winding number at beta = 0; the sign of mesh_sdf(accel="tiles") is
    brute force's at every point; two runs give the same bits."""
    m = room4["mesh"]
    packed, tiles, clean = m.packed.cpu().numpy(), room4["tiles"].cpu().numpy(), room4["clean"].cpu().numpy()
    model = ttm.run(packed, tiles, clean, pts, room4["qperm"].cpu().numpy(), beta=3.0, winding=True, solid=solid64_device)
    w = room4["out"][3].cpu().numpy()
    gap = np.abs(w - model["winding"]).max()
    exact = winding64_device(packed, pts)
    print("beta 3: device - model %.3e, model - exact %.3e, near tiles %s of %d" % (gap, np.abs(model["winding"] - exact).max(),
                                                                                   model["stats"][1], 4 * 61))
    assert room4["out"][5].tolist() == model["stats"]
    assert gap <= 4 * WIND_GAP
    w0 = eng.tri_distance_tiles(m.packed, m.n_faces, room4["tiles"], room4["clean"], pts, room4["qperm"], beta=0.0, want_winding=True,
                                want_stats=True)
    gap0 = np.abs(w0[3].cpu().numpy() - exact).max()
    print("beta 0: device - exact %.3e" % gap0)
    assert gap0 <= 4 * WIND_GAP and w0[5].tolist()[1] == 4 * 61
    sdf_b, w_b = mesh_sdf.mesh_sdf(eng, m, pts, free_winding=-1)
    sdf_t, w_t = mesh_sdf.mesh_sdf(eng, m, pts, free_winding=-1, accel="tiles")
    assert np.minimum(np.abs(w_b.cpu().numpy() + 1), np.abs(w_b.cpu().numpy())).max() < 0.01
    assert torch.equal(sdf_t > 0, sdf_b > 0) and torch.equal(_int(sdf_t.abs()), _int(sdf_b.abs()))
    assert torch.equal(_int(w_t), _int(room4["out"][3]))                              # the default beta and qperm: the same bits
    again = eng.tri_distance_tiles(m.packed, m.n_faces, room4["tiles"], room4["clean"], pts, room4["qperm"], beta=3.0, want_index=True,
                                   want_closest=True, want_winding=True, want_stats=True)
    for a, b in zip(again, room4["out"]):
        assert torch.equal(_int(a), _int(b))


def test_every_combination_of_optional_outputs(eng, room4, pts):
    m, p = room4["mesh"], pts[:1300]
    full = eng.tri_distance_tiles(m.packed, m.n_faces, room4["tiles"], room4["clean"], p, beta=3.0, want_index=True, want_closest=True,
                                  want_winding=True, want_stats=True)
    for want in itertools.product([False, True], repeat=5):
        out = eng.tri_distance_tiles(m.packed, m.n_faces, room4["tiles"], room4["clean"], p, beta=3.0, want_dist=want[0],
                                     want_index=want[1], want_closest=want[2], want_winding=want[3], want_stats=want[4])
        for k, j in enumerate((0, 1, 2, 3, 5)):
            assert (out[j] is not None) == want[k]
            # without the winding number no tile is staged as near
            if want[k] and (j != 5 or want[3]):
                assert torch.equal(_int(out[j]), _int(full[j])), (want, j)
        assert torch.equal(_int(out[4]), _int(full[4]))


def test_mesh_volume_through_the_tiles(eng):
    """the 25 x 13 x 21 grid of tests/test_tri_gpu.py: without spheres every bit of brute force's volume, the exact zeros on the
    surface nodes included; with spheres at k = 3 the magnitude bit for bit and the sign at every node"""
    dims, h = (25, 13, 21), 0.25
    for v, f in (syn.room_mesh(spheres=False), syn.room_mesh(3)):
        mesh = mesh_sdf.PackedMesh(eng, v.astype(np.float32).astype(np.float64), f)
        ref = mesh_sdf.mesh_volume(eng, mesh, h, syn.ROOM_LO, dims, free_winding=-1, chunk=2000)
        got = mesh_sdf.mesh_volume(eng, mesh, h, syn.ROOM_LO, dims, free_winding=-1, chunk=2000, accel="tiles")
        assert torch.equal(_int(got.values.abs()), _int(ref.values.abs()))
        assert torch.equal(got.values > 0, ref.values > 0)
        if len(f) == 36:
            assert torch.equal(_int(got.values), _int(ref.values)) and int((ref.values == 0).sum()) > 1000
    assert got.spacing == ref.spacing and tuple(got.values.shape) == dims


def test_mesh_accuracy_completion_through_the_tiles(eng):
    v, f = syn.room_mesh(3)
    gt = mesh_sdf.PackedMesh(eng, v, f)
    rec = mesh_sdf.PackedMesh(eng, v[:, [0, 1, 2]] + np.array([0.01, -0.02, 0.015]), f)
    ref = mesh_sdf.mesh_accuracy_completion(eng, gt, rec, 20000, torch.Generator("cuda").manual_seed(7))
    got = mesh_sdf.mesh_accuracy_completion(eng, gt, rec, 20000, torch.Generator("cuda").manual_seed(7), accel="tiles")
    assert got == ref and 0 < ref[0] < 0.03 and 0 < ref[1] < 0.03
    with pytest.raises(ValueError, match="accel"):
        mesh_sdf.surface_distance(eng, gt, v[:4], accel="bvh")
