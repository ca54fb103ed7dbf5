"""Host models of the routing entry points (include/isdf_hip.h: isdf_route_init / isdf_route_relax / isdf_route_trace): Dijkstra
with a binary heap on the same graph -- voxels 26-connected, integer chamfer weights 3 / 4 / 5 for face / edge / corner moves, a
move iff both voxels are inside the grid and free -- and the trace with the header's neighbour order.  All integers: the device's
converged field and its paths must equal these exactly.  Also the grids the CPU and GPU tests share."""
import heapq

import numpy as np

NONE = 1 << 30
# (di, dj, dk) lexicographic over -1..1 without (0, 0, 0), and each move's weight
NEIGHBOURS = [(di, dj, dk) for di in (-1, 0, 1) for dj in (-1, 0, 1) for dk in (-1, 0, 1) if (di, dj, dk) != (0, 0, 0)]
WEIGHTS = [2 + (di != 0) + (dj != 0) + (dk != 0) for di, dj, dk in NEIGHBOURS]


def dijkstra(free, goals):
    """int32 [nx,ny,nz]: the cost of the cheapest path from every voxel to any goal (goals outside the grid or on a blocked voxel
    are ignored); NONE where blocked or unreachable"""
    free = np.asarray(free) != 0
    nx, ny, nz = free.shape
    dist = np.full(free.shape, NONE, np.int64)
    heap = []
    for g in np.asarray(goals, np.int64).reshape(-1, 3):
        i, j, k = (int(v) for v in g)
        if 0 <= i < nx and 0 <= j < ny and 0 <= k < nz and free[i, j, k] and dist[i, j, k] != 0:
            dist[i, j, k] = 0
            heap.append((0, i, j, k))
    heapq.heapify(heap)
    while heap:
        d, i, j, k = heapq.heappop(heap)
        if d > dist[i, j, k]:
            continue
        for (di, dj, dk), w in zip(NEIGHBOURS, WEIGHTS):
            a, b, c = i + di, j + dj, k + dk
            if 0 <= a < nx and 0 <= b < ny and 0 <= c < nz and free[a, b, c] and d + w < dist[a, b, c]:
                dist[a, b, c] = d + w
                heapq.heappush(heap, (d + w, a, b, c))
    return dist.astype(np.int32)


def trace(dist, start, max_len=None):
    """(path, len): the linear voxel indices from `start` down `dist`, at every voxel to the FIRST neighbour in NEIGHBOURS order
    with dist[q] + w == dist[p], until dist == 0.  len = 0: start outside / blocked / unreachable; len = -1: max_len too small or
    no neighbour matches (path then holds the voxels found so far)"""
    dist = np.asarray(dist)
    nx, ny, nz = dist.shape
    i, j, k = (int(v) for v in start)
    if not (0 <= i < nx and 0 <= j < ny and 0 <= k < nz) or dist[i, j, k] >= NONE:
        return [], 0
    path = []
    while True:
        if max_len is not None and len(path) == max_len:
            return path, -1
        path.append((i * ny + j) * nz + k)
        d = int(dist[i, j, k])
        if d == 0:
            return path, len(path)
        for (di, dj, dk), w in zip(NEIGHBOURS, WEIGHTS):
            a, b, c = i + di, j + dj, k + dk
            if 0 <= a < nx and 0 <= b < ny and 0 <= c < nz and int(dist[a, b, c]) + w == d:
                i, j, k = a, b, c
                break
        else:
            return path, -1


def closed_form(shape, goal):
    """the empty grid: 3 a + b + c for the sorted offsets a >= b >= c (c corner moves, b - c edge moves, a - b face moves)"""
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1)
    off = np.sort(np.abs(idx - np.asarray(goal)), -1)
    return (3 * off[..., 2] + off[..., 1] + off[..., 0]).astype(np.int32)


# ---- the grids of the tests -------------------------------------------------------------------------------------------------
def diagonal_corridor(tile, edge_only=False):
    """(free, goals): n = 2 tile + 1; the only free voxels are (i, i, i) -- every move a corner move, two of them across tile
    corners -- or, edge_only, (i, i, 0): every move an edge move, two across tile edges.  Goal at the origin."""
    n = 2 * tile + 1
    free = np.zeros((n, n, n), np.uint8)
    r = np.arange(n)
    free[r, r, 0 if edge_only else r] = 1
    return free, np.array([[0, 0, 0]])


RANDOM_SHAPE, RANDOM_SEED, RANDOM_DENSITY = (20, 17, 23), 2, 0.35


def random_obstacles():
    """(free, goals): 20 x 17 x 23 with about 35 % of the voxels FREE, from a fixed seed -- the density at which a 26-connected
    grid still hangs together but leaves a few free voxels walled in (at 35 % obstacles there are none: a voxel with all its
    neighbours blocked has probability 0.35^26).  Three goals: two on free voxels, the third on a blocked one."""
    rng = np.random.RandomState(RANDOM_SEED)
    free = (rng.uniform(size=RANDOM_SHAPE) < RANDOM_DENSITY).astype(np.uint8)
    open_ = np.argwhere(free != 0)
    goals = open_[rng.choice(len(open_), 2, replace=False)]
    blocked = np.argwhere(free == 0)
    return free, np.concatenate([goals, blocked[rng.choice(len(blocked), 1)]])


def serpentine(shape=(24, 8, 24)):
    """(free, goals): a corridor one voxel wide.  Every even i-plane is a slab whose even j-lines run the whole length in k and are
    joined at alternating ends (walls one voxel thick: no move crosses one); consecutive slabs are joined by one door voxel, at
    the end of the last line or the start of the first in turn.  From the last slab to the goal at the origin the path runs the
    length of every line of every slab: many times the grid's diameter, and far more tiles than a round crosses."""
    nx, ny, nz = shape
    free = np.zeros(shape, np.uint8)
    free[0::2, 0::2, :] = 1
    for j in range(1, ny - 1, 2):                  # the joint between lines j - 1 and j + 1
        free[0::2, j, nz - 1 if j % 4 == 1 else 0] = 1
    last = ny - 2 if ny % 2 == 0 else ny - 1       # the last even line; it ends at k = 0 when the slab has an even number of lines
    assert ((last // 2) + 1) % 2 == 0
    free[1::4, last, 0] = 1
    free[3::4, 0, 0] = 1
    return free, np.array([[0, 0, 0]])
