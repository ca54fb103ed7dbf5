"""Ground truth from a triangle mesh on the device: isdf_tri_pack / isdf_tri_distance through Engine and isdf_amd.mesh_sdf.
References: tests/tri_model.py -- distance, index and closest point must equal its float32 sequence bit for bit, the record its
ordered sums -- its float64 winding number, and the closed-form room of isdf_amd.synthetic."""
import itertools

import numpy as np
import pytest
import torch

from isdf_amd import _ffi, mesh_sdf, metrics, synthetic as syn
from tests import tri_model as tm

pytestmark = pytest.mark.gpu

TILE = _ffi.TRI_TILE
BLOCK = 1024                 # query points per block (TRI_Q * 256)
GAP32 = 4.75e-7              # float32 vs float64 model of the distance (tests/test_tri_cpu.py), asserted fourfold
WIND_GAP = 2.96e-6           # measured: max |device winding number - float64 model| on the seeded 4 000 points, room mesh k = 2


@pytest.fixture(scope="module")
def eng():
    from isdf_amd.engine import Engine, NetConfig
    return Engine(NetConfig(hidden=64, blocks=1), "cuda")


@pytest.fixture(scope="module")
def pts():
    return np.random.RandomState(0).uniform(syn.ROOM_LO - 0.5, syn.ROOM_HI + 0.5, (4000, 3)).astype(np.float32)


@pytest.fixture(scope="module")
def room2(eng, pts):
    """the room mesh at k = 2 against the seeded points: one device call with every output, one model, shared and left unchanged"""
    v, f = syn.room_mesh(2)
    packed, counts, m = eng.tri_pack(v, f)
    out = eng.tri_distance(packed, m, pts, want_index=True, want_closest=True, want_winding=True)
    model_packed, model_counts = tm.pack32(v, f)
    return dict(v=v, f=f, packed=packed, counts=counts, m=m, out=out, model_packed=model_packed, model_counts=model_counts,
                model=tm.distance32(model_packed, pts))


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_floats(got, want, what):
    """bit for bit; NaN matches NaN"""
    g, w = (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x, np.float32) for x in (got, want))
    assert g.shape == w.shape, what
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), what
    bad = (_bits(g) != _bits(w)) & ~nan
    assert not bad.any(), "%s: %d of %d differ, first at %s" % (what, bad.sum(), bad.size, np.argwhere(bad)[0])


def check_against_model(eng, v, f, p, transform=None):
    packed, counts, m = eng.tri_pack(v, f, transform)
    dist, index, closest, _, record = eng.tri_distance(packed, m, p, want_index=True, want_closest=True)
    mp, mc = tm.pack32(v, f, transform)
    assert_same_floats(packed, mp, "packed")
    assert counts.tolist() == mc
    md, mi, mcl = tm.distance32(mp, p)
    assert_same_floats(dist, md, "dist")
    assert np.array_equal(index.cpu().numpy(), mi)
    assert_same_floats(closest, mcl, "closest")
    assert np.array_equal(record.cpu().numpy(), tm.record(md))
    return md, mi, mcl


ONE = (np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
# (point, nearest point of the triangle): the seven regions, then their borders and the triangle itself
HAND = [((1, 1, 1), (1, 1, 0)), ((-1, -1, 0.5), (0, 0, 0)), ((6, -1, 0), (4, 0, 0)), ((-1, 6, 0), (0, 4, 0)),
        ((2, -1, 1), (2, 0, 0)), ((-1, 2, 1), (0, 2, 0)), ((3, 3, 1), (2, 2, 0)),
        ((0, -1, 0), (0, 0, 0)), ((4, -1, 0), (4, 0, 0)), ((-1, 0, 0), (0, 0, 0)), ((-1, 4, 2), (0, 4, 0)), ((5, 1, 0), (4, 0, 0)),
        ((1, 5, 0), (0, 4, 0)), ((2, 0, 0), (2, 0, 0)), ((0, 0, 0), (0, 0, 0)), ((4, 0, 0), (4, 0, 0)), ((0, 4, 0), (0, 4, 0)),
        ((2, 2, 0), (2, 2, 0)), ((0, 1, 0), (0, 1, 0)), ((1, 1, 0), (1, 1, 0)), ((1, 2, -3), (1, 2, 0)), ((0, 0, 2), (0, 0, 0)),
        ((2, 2, 5), (2, 2, 0))]


def test_one_triangle_every_region_and_border(eng):
    p = np.array([h[0] for h in HAND], np.float32)
    rng = np.random.RandomState(3)
    p = np.concatenate([p, rng.uniform(-3, 7, (200, 3)).astype(np.float32)])
    md, mi, mcl = check_against_model(eng, ONE[0], ONE[1], p)
    want = np.array([h[1] for h in HAND], np.float32)
    assert np.array_equal(mcl[:len(HAND)], want)                     # dyadic coordinates: the sequence is exact here
    assert np.array_equal(md[:len(HAND)], np.linalg.norm(p[:len(HAND)] - want, axis=1).astype(np.float32))
    assert (mi == 0).all()
    # the same triangle through an affine: the pack's own chain
    T = np.array([[0, -2, 0, 1], [0.5, 0, 0, -3], [0, 0, 1.5, 0.25]], np.float32)
    check_against_model(eng, ONE[0], ONE[1], p, T)


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_the_lower_index_wins_a_shared_edge_and_vertex(eng, order):
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [4, 4, 0]], np.float32)
    faces = np.array([[0, 1, 2], [1, 3, 2]], np.int32)[list(order)]
    # above the shared edge, at its ends, and beyond both shared vertices: the nearest point belongs to both faces
    p = np.array([[2, 2, 1], [3, 1, -2], [1, 3, 0.5], [5, -1, 0], [-1, 5, 1], [4, 0, 3], [2, 2, 0]], np.float32)
    md, mi, mcl = check_against_model(eng, v, faces, p)
    assert (mi == 0).all()
    assert np.array_equal(mcl, np.array([[2, 2, 0], [3, 1, 0], [1, 3, 0], [4, 0, 0], [0, 4, 0], [4, 0, 0], [2, 2, 0]], np.float32))
    # ... and a point nearer to the second face goes to it
    assert check_against_model(eng, v, faces, np.array([[3.5, 3.5, 1]], np.float32))[1][0] == order.index(1)


def test_room_mesh_bit_equal_to_the_float32_model(room2):
    dist, index, closest, _, record = room2["out"]
    assert_same_floats(room2["packed"], room2["model_packed"], "packed")
    assert room2["counts"].tolist() == room2["model_counts"] == [0, 0]
    md, mi, mcl = room2["model"]
    assert_same_floats(dist, md, "dist")
    assert np.array_equal(index.cpu().numpy(), mi)
    assert_same_floats(closest, mcl, "closest")
    assert len(np.unique(mi)) > 100


def _soup(m, n, seed):
    rng = np.random.RandomState(seed)
    v = rng.uniform(-1, 1, (3 * m, 3)).astype(np.float32)
    return v, np.arange(3 * m, dtype=np.int32).reshape(m, 3), rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)


@pytest.mark.parametrize("m", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_sizes_around_the_tile(eng, m):
    check_against_model(eng, *_soup(m, BLOCK + 1, m))


@pytest.mark.parametrize("n", [1, 255, BLOCK - 1, BLOCK, BLOCK + 1])
def test_sizes_around_the_block(eng, n):
    check_against_model(eng, *_soup(2 * TILE + 3, n, 1000 + n))


def test_few_points_and_many_triangles_force_several_chunks(eng):
    v, f = syn.room_mesh(3)
    p = np.random.RandomState(5).uniform(syn.ROOM_LO, syn.ROOM_HI, (5, 3)).astype(np.float32)
    tiles = -(-len(f) // TILE)
    assert tiles == 16 and eng.lib.isdf_tri_ws_bytes(5, len(f)) == 8 * 5 * (1 + tiles) + 32 + 256      # one chunk per tile
    check_against_model(eng, v, f, p)
    packed, _, m = eng.tri_pack(v, f)
    w = eng.tri_distance(packed, m, p, want_winding=True)[3].cpu().numpy()
    assert np.abs(w - tm.winding64(v.astype(np.float32), f, p)).max() <= 4 * WIND_GAP


def test_winding_number_against_the_float64_model(eng, room2, pts):
    """Measured: max |device - float64 model| = WIND_GAP on the seeded 4 000 points, none excluded (some lie within a millimetre
    of the surface); asserted with a fourfold margin."""
    w = room2["out"][3].cpu().numpy()
    w64 = tm.winding64(room2["v"].astype(np.float32), room2["f"], pts)
    gap = np.abs(w - w64).max()
    print("winding gap %.3e" % gap)
    assert gap <= 4 * WIND_GAP
    assert np.minimum(np.abs(w + 1), np.abs(w)).max() < 0.01
    mesh = mesh_sdf.PackedMesh(eng, room2["v"], room2["f"])
    assert (mesh.n_faces, mesh.n_invalid, mesh.n_degenerate, mesh.n_valid) == (996, 0, 0, 996)
    sdf, w2 = mesh_sdf.mesh_sdf(eng, mesh, pts, free_winding=-1)
    gt = syn.gt_sdf(pts.astype(np.float64))
    sel = np.abs(gt) > 1e-3
    assert np.array_equal(sdf.cpu().numpy()[sel] > 0, gt[sel] > 0)
    assert_same_floats(sdf.abs(), room2["model"][0], "|sdf|")
    # two runs give identical bits
    assert np.array_equal(_bits(w2), _bits(w))
    again = eng.tri_distance(room2["packed"], room2["m"], pts, want_index=True, want_closest=True, want_winding=True)
    for a, b in zip(again, room2["out"]):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_skipped_triangles_contribute_nothing(eng):
    v, f = syn.room_mesh(0)
    nv = len(v)
    # two vertices that are not finite, then three distinct collinear ones
    v_bad = np.concatenate([v, [[np.nan, 1.0, 1.0], [1.0, np.inf, 2.0]], [[0, 0, 0], [1, 1, 1], [3, 3, 3]]])
    # (position in the clean face list, face): repeated vertices and the collinear face (zero area); indices outside [0, nv + 5);
    # faces through a non-finite vertex
    extra = [(0, [0, 0, 0]), (0, [3, 5, 5]), (96, [2, 2, 9]), (50, [nv + 2, nv + 3, nv + 4]),
             (7, [nv + 5, 1, 2]), (7, [0, -1, 2]), (96, [1, 2, 1 << 20]),
             (40, [nv, 1, 2]), (40, [4, nv + 1, 6])]
    faces, kept = [], []
    for i in range(len(f) + 1):
        faces += [e[1] for e in extra if e[0] == i]
        if i < len(f):
            kept.append(len(faces))
            faces.append(f[i].tolist())
    faces, kept = np.array(faces, np.int64), np.array(kept)
    p = np.random.RandomState(2).uniform(syn.ROOM_LO - 0.5, syn.ROOM_HI + 0.5, (700, 3)).astype(np.float32)
    clean_packed, clean_counts, m0 = eng.tri_pack(v, f)
    clean = eng.tri_distance(clean_packed, m0, p, want_index=True, want_closest=True, want_winding=True)
    packed, counts, m = eng.tri_pack(v_bad, faces)
    assert m == len(f) + 9 and clean_counts.tolist() == [0, 0]
    assert counts.tolist() == [5, 4] == tm.pack32(v_bad, faces)[1]
    got = eng.tri_distance(packed, m, p, want_index=True, want_closest=True, want_winding=True)
    assert np.array_equal(got[1].cpu().numpy(), kept[clean[1].cpu().numpy()])
    for k in (0, 2, 3):
        assert_same_floats(got[k], clean[k], "output %d" % k)
    assert np.array_equal(got[4].cpu().numpy(), clean[4].cpu().numpy())
    with pytest.raises(ValueError, match="3 of 105 faces"):
        mesh_sdf.PackedMesh(eng, v_bad, faces)
    ok = mesh_sdf.PackedMesh(eng, v_bad, faces[(faces >= 0).all(1) & (faces < len(v_bad)).all(1)])
    assert (ok.n_invalid, ok.n_degenerate, ok.n_valid) == (2, 4, 96)


def test_a_mesh_without_a_valid_face_and_non_finite_points(eng):
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [np.nan, 0, 0]], np.float32)
    p = np.array([[0.5, 0.5, 0.5], [np.nan, 0, 0], [1, 2, 3], [0, np.inf, 0], [0, 0, -np.inf]], np.float32)
    for faces in (np.array([[0, 1, 2], [0, 0, 1], [0, 1, 3], [0, 1, 7]], np.int32), np.zeros((0, 3), np.int32)):
        packed, counts, m = eng.tri_pack(v, faces)
        assert counts.tolist() == ([2, 2] if len(faces) else [0, 0])
        dist, index, closest, winding, record = eng.tri_distance(packed, m, p, want_index=True, want_closest=True, want_winding=True)
        fin = np.array([True, False, True, False, False])
        d, w = dist.cpu().numpy(), winding.cpu().numpy()
        assert (d[fin] == np.inf).all() and np.isnan(d[~fin]).all()
        assert (w[fin] == 0).all() and np.isnan(w[~fin]).all()
        assert (index.cpu().numpy() == -1).all() and np.isnan(closest.cpu().numpy()).all()
        assert record.cpu().numpy().tolist() == [np.inf, 2.0, 3.0, np.inf]
    # non-finite points among finite ones: counted, and excluded from the sum and the maximum
    vr, fr = syn.room_mesh(0)
    q = np.random.RandomState(4).uniform(syn.ROOM_LO, syn.ROOM_HI, (1500, 3)).astype(np.float32)
    q[[0, 255, 256, 700, 1499], [0, 1, 2, 0, 1]] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    md = check_against_model(eng, vr, fr, q)[0]
    assert np.isnan(md).sum() == 5
    packed, _, m = eng.tri_pack(vr, fr)
    out = eng.tri_distance(packed, m, q, want_winding=True)
    assert np.array_equal(np.isnan(out[3].cpu().numpy()), np.isnan(md))
    assert out[4].cpu().numpy()[1:3].tolist() == [1495.0, 5.0] and np.array_equal(out[4].cpu().numpy(), tm.record(md))
    # no point at all: the record of nothing
    assert eng.tri_distance(packed, m, np.zeros((0, 3), np.float32))[4].cpu().numpy().tolist() == [0.0, 0.0, 0.0, 0.0]


def test_every_combination_of_optional_outputs(eng, room2, pts):
    p = pts[:1300]
    full = [t[:1300] for t in room2["out"][:4]]
    for want in itertools.product([False, True], repeat=4):
        out = eng.tri_distance(room2["packed"], room2["m"], p, want_dist=want[0], want_index=want[1], want_closest=want[2],
                               want_winding=want[3])
        for k in range(4):
            assert (out[k] is not None) == want[k]
            if want[k]:
                assert torch.equal(out[k].view(torch.int32), full[k].view(torch.int32)), (want, k)
        assert np.array_equal(out[4].cpu().numpy(), tm.record(room2["model"][0][:1300]))


def test_the_record_equals_the_ordered_sums_of_the_model(room2):
    rec = room2["out"][4].cpu().numpy()
    assert np.array_equal(rec, tm.record(room2["model"][0]))
    assert rec[1] == 4000 and rec[2] == 0 and rec[3] == room2["model"][0].max()


def _trilinear64(values, spacing, origin, p):
    g = (p - origin) / spacing
    i = np.clip(np.floor(g).astype(np.int64), 0, np.array(values.shape) - 2)
    t = g - i
    out = np.zeros(len(p))
    for dx, dy, dz in itertools.product((0, 1), repeat=3):
        wgt = np.where(dx, t[:, 0], 1 - t[:, 0]) * np.where(dy, t[:, 1], 1 - t[:, 1]) * np.where(dz, t[:, 2], 1 - t[:, 2])
        out += wgt * values[i[:, 0] + dx, i[:, 1] + dy, i[:, 2] + dz]
    return out


def _gt_without_spheres(p, boxes):
    d = np.minimum(p - syn.ROOM_LO, syn.ROOM_HI - p).min(-1)
    for lo, hi in boxes:
        q = np.maximum(lo - p, p - hi)
        d = np.minimum(d, np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0))
    return d


def test_mesh_volume_nodes_and_metrics(eng):
    """Node values: the float32 model bit for bit, exactly 0 on the surface, within 4 * GAP32 of the closed form.  Then the check of
    the mesh volume as ground truth: sdf_metrics of the closed form against it reports an av_l1 no larger than the closed form's own
    trilinear error on the grid (float64, computed here).  Like is compared with like: the surface is the one the device holds (the
    mesh's vertices are float32, so the closed form takes the float32-rounded box corners: 2.2 and 0.6 are no float32 numbers), and
    the evaluation points are float32 numbers, the closed form evaluated AT them.  Measured: av_l1 6.505594464e-3 m against
    6.505594584e-3 m (the closed form's float32 nodes through the same device lookup: 6.505594457e-3 m)."""
    v, f = syn.room_mesh(spheres=False)
    v = v.astype(np.float32).astype(np.float64)
    boxes = [(lo.astype(np.float32).astype(np.float64), hi.astype(np.float32).astype(np.float64)) for lo, hi in syn.BOXES]
    mesh = mesh_sdf.PackedMesh(eng, v, f)
    dims, h = (25, 13, 21), 0.25
    vol = mesh_sdf.mesh_volume(eng, mesh, h, syn.ROOM_LO, dims, free_winding=-1, chunk=2000)      # four chunks, the last partial
    assert tuple(vol.values.shape) == dims and vol.spacing == (h, h, h)
    idx = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3)
    nodes = syn.ROOM_LO.astype(np.float32) + idx.astype(np.float32) * np.float32(h)
    md = tm.distance32(tm.pack32(v, f)[0], nodes)[0]
    got = vol.values.reshape(-1).cpu().numpy()
    assert_same_floats(np.abs(got), md, "|node values|")
    # the sign wherever it means something: a node of this grid lies ON the surface (the walls, the floor boxes' faces at 4.0 and
    # 3.0), where the distance is exactly 0 and the winding number a half or a quarter, or at least 0.05 m off it
    w64 = tm.winding64(v, f, nodes.astype(np.float64))
    off = md > 0
    assert md[off].min() > 0.049
    assert np.array_equal(got[off] > 0, np.abs(w64[off] + 1) < 0.5)
    assert (~off).sum() > 1000 and (got[off] > 0).sum() > 1000 and (got[off] < 0).sum() > 10
    one = mesh_sdf.mesh_volume(eng, mesh, h, syn.ROOM_LO, dims, free_winding=-1)
    assert torch.equal(one.values.view(torch.int32), vol.values.view(torch.int32))            # chunking changes nothing
    # the nodes against the closed form itself: the float32 sequence's own error, as tests/test_tri_cpu.py bounds it
    closed = _gt_without_spheres(syn.ROOM_LO + idx * h, boxes)
    assert np.abs(got.astype(np.float64) - closed).max() <= 4 * GAP32
    # sdf_metrics of the closed form against the volume: no larger than the closed form's own trilinear error on this grid
    p32 = np.random.RandomState(1).uniform(syn.ROOM_LO, syn.ROOM_HI, (4000, 3)).astype(np.float32)
    p = p32.astype(np.float64)
    gt = _gt_without_spheres(p, boxes)
    bound = np.abs(_trilinear64(closed.reshape(dims), h, syn.ROOM_LO, p) - gt).mean()
    pd, gd = torch.from_numpy(p32).cuda(), torch.from_numpy(gt.astype(np.float32)).cuda()
    m = metrics.sdf_metrics(eng, vol, pd, gd, exclude_zero_gt=False)
    same_path = metrics.sdf_metrics(eng, metrics.GtVolume(closed.reshape(dims).astype(np.float32), (h, h, h), syn.ROOM_LO, "cuda"), pd, gd,
                                    exclude_zero_gt=False)
    print("av_l1 %.12e  trilinear error of the closed form %.12e (float64), %.12e (its float32 nodes through the device's lookup)"
          % (m.av_l1, bound, same_path.av_l1))
    assert m.n_valid == 4000
    assert m.av_l1 <= bound


def _sample_bound(c):
    """how far a float32 barycentric sample may lie off its triangle (tests/test_tri_cpu.py) plus the float32 distance sequence's own
    error (fourfold GAP32)"""
    return np.sqrt(3.0) * 8 * 2.0 ** -24 * c + 4 * GAP32


def test_mesh_accuracy_completion(eng):
    v, f = syn.room_mesh(3)
    gt_mesh = mesh_sdf.PackedMesh(eng, v, f)
    n = 20000
    bound = _sample_bound(6.0)
    acc, comp = mesh_sdf.mesh_accuracy_completion(eng, gt_mesh, gt_mesh, n, torch.Generator("cuda").manual_seed(0))
    print("self comparison: acc %.3e comp %.3e (bound %.3e)" % (acc, comp, bound))
    assert 0 <= acc <= bound and 0 <= comp <= bound
    # the marching-cubes mesh of the analytic volume against the analytic mesh
    dims, h, lo = (62, 32, 52), 0.1, np.array([-0.05, -0.05, -0.05])
    idx = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1)
    grid = torch.from_numpy(syn.gt_sdf(lo + idx * h).astype(np.float32)).cuda()
    A = np.concatenate([np.eye(3) * h, lo[:, None]], 1).astype(np.float32)
    rv, rf, _ = eng.marching_cubes(grid, 0.0, A)
    rec_mesh = mesh_sdf.PackedMesh(eng, rv, rf)
    assert rec_mesh.n_valid > 10000 and rec_mesh.n_invalid == 0
    acc, comp = mesh_sdf.mesh_accuracy_completion(eng, gt_mesh, rec_mesh, n, torch.Generator("cuda").manual_seed(7))
    g = torch.Generator("cuda").manual_seed(7)                      # the same samples: ground truth first, then reconstruction
    gt_pts = mesh_sdf.sample_surface(gt_mesh.vertices, gt_mesh.faces, n, g)[0]
    rec_pts = mesh_sdf.sample_surface(rec_mesh.vertices, rec_mesh.faces, n, g)[0]
    acc_pp, comp_pp = metrics.accuracy_completion(eng, gt_pts, rec_pts)
    print("acc %.5f (sample to sample %.5f)  comp %.5f (sample to sample %.5f)" % (acc, acc_pp, comp, comp_pp))
    assert 0 < acc <= acc_pp + bound and 0 < comp <= comp_pp + bound
    assert acc < 0.05 and comp < 0.05                              # a 0.1 m grid: within half a cell of the surface on average
