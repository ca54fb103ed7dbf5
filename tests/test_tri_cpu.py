"""The triangle-mesh ground truth without a device: synthetic.room_mesh, the float64 models of distance and winding number against
the closed-form room, the float32 model (what the kernel computes bit for bit) against the float64 one, and sample_surface."""
import numpy as np
import pytest
import torch

from isdf_amd import mesh_sdf, synthetic as syn
from tests import tri_model as tm


@pytest.fixture(scope="module")
def pts():
    return np.random.RandomState(0).uniform(syn.ROOM_LO - 0.5, syn.ROOM_HI + 0.5, (4000, 3))


def _inside(p):
    return ((p > syn.ROOM_LO) & (p < syn.ROOM_HI)).all(1)


def _gt_without_spheres(p):
    d = np.minimum(p - syn.ROOM_LO, syn.ROOM_HI - p).min(-1)
    for lo, hi in syn.BOXES:
        q = np.maximum(lo - p, p - hi)
        d = np.minimum(d, np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0))
    return d


@pytest.mark.parametrize("k", [0, 2, 3])
def test_room_mesh_is_watertight_and_consistently_oriented(k):
    v, f = syn.room_mesh(k)
    assert v.dtype == np.float64 and f.dtype == np.int32 and f.shape == (36 + 3 * 20 * 4 ** k, 3)
    assert f.min() == 0 and f.max() == len(v) - 1
    edges = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    uniq, counts = np.unique(edges, axis=0, return_counts=True)
    assert counts.max() == 1                                          # every directed edge occurs once
    have = set(map(tuple, uniq))
    assert all((b, a) in have for a, b in have)                       # ... and its reverse occurs once
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    volume = (a * np.cross(b, c)).sum() / 6.0
    boxes = sum(np.prod(hi - lo) for lo, hi in syn.BOXES)
    balls = sum(4.0 / 3.0 * np.pi * r ** 3 for _, r in syn.SPHERES)
    room = np.prod(syn.ROOM_HI - syn.ROOM_LO)
    # the room inward (negative), the solids outward; an inscribed icosphere is smaller than its ball, by 40 % at k = 0 and by
    # O(4^-k) after
    assert -room + boxes + 0.6 * balls <= volume < -room + boxes + balls
    if k == 3:
        assert abs(volume - (-room + boxes + balls)) < 0.01 * balls
    v0, f0 = syn.room_mesh(k, spheres=False)
    assert np.array_equal(f0, f[:36]) and np.array_equal(v0, v[:24])


def test_float64_model_against_the_closed_form(pts, k=2):
    """winding number and sign at every one of the seeded points; the signed distance differs from the closed form by the
    icospheres' tessellation sag, measured 8.8 mm at k = 2 (and 2.2 mm at k = 3, which takes four times as long and is not run
    here); printed, not asserted: it is a property of the mesh, not of the model"""
    v, f = syn.room_mesh(k)
    w = tm.winding64(v, f, pts)
    assert np.minimum(np.abs(w + 1.0), np.abs(w)).max() < 0.01         # no point is left out
    gt = syn.gt_sdf(pts)
    free = np.abs(w + 1.0) < 0.5
    sel = np.abs(gt) > 1e-3
    assert np.array_equal(free[sel], gt[sel] > 0)
    d = tm.distance64(tm.pack64(v, f), pts)[0]
    sd = np.where(free, d, -d)
    print("k = %d: sag %.3e" % (k, np.abs(sd - gt)[_inside(pts)].max()))


def test_float64_model_is_the_closed_form_without_the_spheres(pts):
    v, f = syn.room_mesh(spheres=False)
    assert len(f) == 36
    w = tm.winding64(v, f, pts)
    assert np.minimum(np.abs(w + 1.0), np.abs(w)).max() < 0.01
    d = tm.distance64(tm.pack64(v, f), pts)[0]
    sd = np.where(np.abs(w + 1.0) < 0.5, d, -d)
    ins = _inside(pts)
    # double rounding only: coordinates up to 6.5, a handful of operations
    assert np.abs(sd - _gt_without_spheres(pts))[ins].max() <= 16 * np.finfo(np.float64).eps * 6.5


GAP32 = 4.75e-7      # measured: max |float32 model - float64 model| of the distance, k = 2 and k = 3, the seeded 4 000 points


@pytest.mark.parametrize("k", [2, 3])
def test_float32_model_against_the_float64_model(pts, k):
    """Both models on the float32-rounded mesh and points.  Measured gap of the distance: 4.75e-7 m at k = 2 and at k = 3
    (coordinates up to 6.5 m: four ulp); asserted with a fourfold margin for other seeds.  The winner's index differs at about
    100 of the 4 000 points -- shared edges and vertices, where the distances tie up to rounding -- so index and closest point are
    not compared here."""
    v, f = syn.room_mesh(k)
    p32 = pts.astype(np.float32)
    packed, counts = tm.pack32(v, f)
    assert counts == [0, 0]
    d32 = tm.distance32(packed, p32)[0]
    d64 = tm.distance64(tm.pack64(v.astype(np.float32), f), p32)[0]
    gap = np.abs(d32.astype(np.float64) - d64).max()
    print("k = %d: float32 vs float64 distance gap %.3e" % (k, gap))
    assert gap <= 4 * GAP32


def test_float32_model_pack_rules():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [2, 0, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 1, 4], [0, 1, 1], [0, 1, 5], [-1, 1, 2], [0, 3, 2], [2, 1, 0]])
    packed, counts = tm.pack32(v, f)
    assert counts == [3, 2] and packed.shape == (256, 24)
    assert packed[:, 15].tolist() == [1, 0, 0, 0, 0, 0, 1] + [0] * 249
    assert not packed[1:6].any()
    d, i, c = tm.distance32(packed, np.array([[0.25, 0.25, 1.0], [np.inf, 0, 0]], np.float32))
    assert d[0] == 1.0 and i[0] == 0 and c[0].tolist() == [0.25, 0.25, 0.0]        # the lower index of the two coincident faces
    assert np.isnan(d[1]) and i[1] == -1 and np.isnan(c[1]).all()
    d, i, c = tm.distance32(packed[1:6], np.zeros((1, 3), np.float32))
    assert d[0] == np.inf and i[0] == -1


def test_sample_surface_points_lie_on_their_triangles():
    v64, f = syn.room_mesh(2)
    v = torch.from_numpy(v64.astype(np.float32))
    g = torch.Generator().manual_seed(0)
    p, face = mesh_sdf.sample_surface(v, torch.from_numpy(f), 20000, g)
    assert p.dtype == torch.float32 and p.shape == (20000, 3) and face.shape == (20000,) and face.dtype == torch.int64
    slots = tm.pack64(v.numpy(), f)[face.numpy()]
    ap = p.numpy().astype(np.float64) - slots[:, 0:3]
    t = [slots[:, k] for k in range(12)]
    vv, ww, _ = tm._weights(np.float64, 1.0, ap[:, 0], ap[:, 1], ap[:, 2], t)
    d = ap - (slots[:, 4:7] * vv[:, None] + slots[:, 8:11] * ww[:, None])
    # p = w0 a + w1 b + w2 c in float32: three products and two sums per coordinate (each within 2^-24 relative, 4 * 2^-24 * C
    # in all, C the largest coordinate), and weights that sum to 1 within 3 * 2^-24 (one more C each); per coordinate 8 * 2^-24 C
    bound = np.sqrt(3.0) * 8 * 2.0 ** -24 * np.abs(v64).max()
    assert np.linalg.norm(d, axis=1).max() <= bound
    assert float(vv.min()) >= 0 and float(ww.min()) >= 0 and float((vv + ww).max()) <= 1 + 1e-6


def test_sample_surface_counts_follow_the_area():
    v, f = syn.room_mesh(spheres=False)
    n = 20000
    _, face = mesh_sdf.sample_surface(torch.from_numpy(v), torch.from_numpy(f), n, torch.Generator().manual_seed(0))
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    prob = area / area.sum()
    counts = np.bincount(face.numpy(), minlength=len(f))
    assert counts.sum() == n
    assert (np.abs(counts - n * prob) <= 3.0 * np.sqrt(n * prob * (1.0 - prob))).all()
    # a face without area is never drawn, and a mesh without any is refused
    f2 = np.concatenate([f, [[0, 0, 1]]]).astype(np.int32)
    _, face = mesh_sdf.sample_surface(torch.from_numpy(v), torch.from_numpy(f2), 5000, torch.Generator().manual_seed(1))
    assert int(face.max()) < len(f)
    with pytest.raises(ValueError):
        mesh_sdf.sample_surface(torch.from_numpy(v), torch.tensor([[0, 0, 1]]), 4)
