"""The tile index and the culling rule of isdf_tri_distance_tiles on the host (tests/tri_tiles_model.py): the rule leaves the brute
force model's winner at every point, the far-field winding number stays within its measured error of the exact one, and the
default order keeps the share of staged tiles under a cap.  No GPU."""
import numpy as np
import pytest
import torch

from isdf_amd import mesh_sdf, synthetic as syn
from tests import tri_model as tm, tri_tiles_model as ttm

# largest |approximated - exact| winding number over the eight seeded bricks of room_mesh(3), float64, measured here (the sign test
# is at 0.5); the 1 000 scattered points form ONE block that spans the room, for which no tile is far: 6.7e-16 at every beta
WIND_ERR = {2: 4.087e-3, 3: 8.687e-4, 4: 5.553e-4}


def bricks(count, seed, h=0.02, dims=(16, 8, 8)):
    """float32 [count * 1024, 3]: `count` bricks of 16 x 8 x 8 nodes at spacing h, placed uniformly inside the room; one brick is one
    block of queries"""
    rng = np.random.RandomState(seed)
    idx = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3)
    size = (np.array(dims) - 1) * h
    return np.concatenate([(rng.uniform(syn.ROOM_LO, syn.ROOM_HI - size) + idx * h).astype(np.float32) for _ in range(count)])


def index_of(k, order=None):
    """the model's pack and tile index of room_mesh(k) in the default order (or `order`)"""
    v, f = syn.room_mesh(k)
    packed, _ = tm.pack32(v, f)
    if order is None:
        order = mesh_sdf.tile_order(torch.from_numpy(packed), len(f)).numpy()
    tiles, clean, counts = ttm.build64(packed, order)
    return dict(v=v, f=f, packed=packed, order=order, tiles=tiles, clean=clean, counts=counts)


@pytest.fixture(scope="module")
def room3():
    return index_of(3)


@pytest.fixture(scope="module")
def pts():
    return np.random.RandomState(0).uniform(syn.ROOM_LO - 0.5, syn.ROOM_HI + 0.5, (1000, 3)).astype(np.float32)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_default_order_and_build(room3):
    o, m = room3["order"], len(room3["f"])
    assert len(o) == (-(-m // 256) + 1) * 256 and sorted(o[o >= 0].tolist()) == list(range(m))
    # the 36 room-spanning faces of the three boxes have tile 0 to themselves
    assert sorted(o[:256][o[:256] >= 0].tolist()) == list(range(36)) and (o[36:256] == -1).all()
    assert room3["counts"] == [0, m]
    tiles = room3["tiles"]
    assert tiles[:, 14].sum() == m and tiles[0, 14] == 36 and tiles[0, 15] == 36 and tiles[-1, 14] == 0
    # the area vectors of a closed mesh cancel; the areas are those of the mesh
    v, f = room3["v"].astype(np.float32).astype(np.float64), room3["f"]
    n = 0.5 * np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert np.abs(tiles[:, 6:9].sum(0)).max() < 1e-12 and abs(tiles[:, 13].sum() - np.linalg.norm(n, axis=1).sum()) < 1e-10
    for t in np.nonzero(tiles[:, 14])[0]:
        e = room3["clean"][t * 256:(t + 1) * 256]
        tri = v[f[e[e >= 0]]].reshape(-1, 3)
        assert np.array_equal(tiles[t, 0:3], tri.min(0)) and np.array_equal(tiles[t, 3:6], tri.max(0))
        assert abs(np.linalg.norm(tri - tiles[t, 9:12], axis=1).max() - tiles[t, 12]) < 1e-12
    # bad entries are counted and cleaned; a skipped slot is cleaned without being counted as bad
    packed = room3["packed"].copy()
    packed[5] = 0
    _, clean, counts = ttm.build64(packed, [5, 7, -1, len(packed), -2, 1 << 20, 7])
    assert counts == [3, 2] and clean[:8].tolist() == [-1, 7, -1, -1, -1, -1, 7, -1] and len(clean) == 256


@pytest.mark.parametrize("which", ["default", "random"])
def test_the_rule_leaves_the_brute_force_winner(room3, pts, which):
    """scattered points, then points ON the mesh: vertices of the icospheres (five or six faces tie at dist2 = 0 exactly), edge
    midpoints and face centroids as float32 rounds them.  In the random order the tying faces lie in different tiles."""
    r = room3 if which == "default" else index_of(3, np.random.RandomState(3).permutation(len(room3["f"])))
    v32, f = r["v"].astype(np.float32), r["f"]
    rng = np.random.RandomState(4)
    vert = v32[rng.choice(np.arange(24, len(v32)), 150, replace=False)]
    tri = v32[f[rng.choice(len(f), 150, replace=False)]]
    on = np.concatenate([vert, (tri[:, 0] + tri[:, 1]) * np.float32(0.5), (tri[:, 0] + tri[:, 1] + tri[:, 2]) / np.float32(3)])
    p = np.concatenate([pts, on]).astype(np.float32)
    qperm = np.random.RandomState(5).permutation(len(p))           # two blocks, each a mixture
    md, mi, _ = tm.distance32(r["packed"], p)
    out = ttm.run(r["packed"], r["tiles"], r["clean"], p, qperm)
    assert _same_bits(out["dist"], md) and np.array_equal(out["index"], mi)
    assert (md[1000:1150] == 0).all()
    if which == "random":
        tile_of = np.empty(len(f), np.int64)
        tile_of[r["clean"][r["clean"] >= 0]] = np.nonzero(r["clean"] >= 0)[0] // 256
        split = 0
        for x in vert:
            tying = np.nonzero((v32[f] == x).all(2).any(1))[0]
            assert len(tying) >= 5
            split += len(set(tile_of[tying])) > 1
        assert split >= 140                                        # five or six faces over 16 tiles: nearly always apart
    # compact blocks: here tiles ARE left out, and the winner stays
    b = bricks(8, 7)
    md, mi, _ = tm.distance32(r["packed"], b)
    out = ttm.run(r["packed"], r["tiles"], r["clean"], b)
    assert _same_bits(out["dist"], md) and np.array_equal(out["index"], mi)
    assert out["stats"][2:] == [8, 0] and out["stats"][0] < 8 * 16
    if which == "default":
        assert out["stats"][0] == 24


def test_far_field_winding_number_against_the_exact_one(room3, pts):
    """Measured (float64 model): the scattered points form one block spanning the room, so every tile is near and the sum is the
    exact one (6.7e-16); on eight bricks WIND_ERR per beta.  Asserted fourfold."""
    v32, f = room3["v"].astype(np.float32), room3["f"]
    w64 = tm.winding64(v32, f, pts)
    b = bricks(8, 7)
    w64b = tm.winding64(v32, f, b)
    for beta in (2, 3, 4):
        out = ttm.run(room3["packed"], room3["tiles"], room3["clean"], pts, beta=beta, winding=True)
        assert out["stats"][:2] == [16, 16]
        assert np.abs(out["winding"] - w64).max() < 1e-13
        out = ttm.run(room3["packed"], room3["tiles"], room3["clean"], b, beta=beta, winding=True)
        err = np.abs(out["winding"] - w64b).max()
        print("beta %d: largest winding error %.3e, near tiles %d of %d" % (beta, err, out["stats"][1], 8 * 16))
        assert err <= 4 * WIND_ERR[beta]
        assert out["stats"][1] < 8 * 16
    out = ttm.run(room3["packed"], room3["tiles"], room3["clean"], b, beta=0.0, winding=True)
    assert out["stats"][1] == 8 * 16 and np.abs(out["winding"] - w64b).max() < 1e-13


def test_default_order_stages_at_most_a_quarter_on_bricks():
    """room_mesh(4): 61 non-empty tiles; forty seeded bricks of 16 x 8 x 8 nodes at 2 cm.  Measured: 301 of 2 440."""
    r = index_of(4)
    nonempty = int((r["tiles"][:, 14] > 0).sum())
    assert nonempty == 61
    out = ttm.run(r["packed"], r["tiles"], r["clean"], bricks(40, 7))
    print("staged %d of %d" % (out["stats"][0], 40 * nonempty))
    assert out["stats"][2] == 40 and 40 <= out["stats"][0] <= 40 * nonempty // 4
