"""Host models of the exploration entry points (include/isdf_hip.h: isdf_frontier_init / isdf_frontier_relax /
isdf_frontier_clusters / isdf_view_gain) -- TEST INFRASTRUCTURE -- written from the header's statements: the frontier rule,
components by a plain union-find with least-index labels, the cluster records, and the voxel walk of a ray in np.float32, one
rounded operation per line.  Integers and one stated fp32 sequence: the device must equal these bit for bit.  `walk_ray` is the
readable per-ray form (the distinct count a Python set per view); `view_gain` is the same sequence over all rays at once, for the
sizes a Python loop cannot do; tests/test_explore_cpu.py holds the two equal.  Also the grids the CPU and GPU tests share and a
stand-in for the Engine backed by these models."""
import numpy as np
import torch

from tests import route_model as rm

UNKNOWN, FREE, OCCUPIED = 0, 1, 2
NONE = 1 << 30
RECORD = 12
FACES = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
f32 = np.float32


# ---- frontiers, labels, records ---------------------------------------------------------------------------------------------
def frontier_mask(state):
    """bool [nx,ny,nz]: FREE with at least one of the six face neighbours inside the grid UNKNOWN"""
    s = np.asarray(state)
    unk = np.pad(s == UNKNOWN, 1, constant_values=False)      # the outside of the grid is not unknown
    near = np.zeros(s.shape, bool)
    nx, ny, nz = s.shape
    for di, dj, dk in FACES:
        near |= unk[1 + di:1 + di + nx, 1 + dj:1 + dj + ny, 1 + dk:1 + dk + nz]
    return (s == FREE) & near


def init_labels(state):
    m = frontier_mask(state)
    return np.where(m, np.arange(m.size, dtype=np.int64).reshape(m.shape), NONE).astype(np.int32)


def labels(state):
    """int32 [nx,ny,nz]: per frontier voxel the least linear index of its 26-connected component of frontier voxels, NONE elsewhere"""
    m = frontier_mask(state)
    nx, ny, nz = m.shape
    parent = {int(p): int(p) for p in np.flatnonzero(m)}

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for p in list(parent):
        i, j, k = p // (ny * nz), (p // nz) % ny, p % nz
        for di, dj, dk in rm.NEIGHBOURS[13:]:                   # each pair once
            a, b, c = i + di, j + dj, k + dk
            if 0 <= a < nx and 0 <= b < ny and 0 <= c < nz and m[a, b, c]:
                ra, rb = find(p), find((a * ny + b) * nz + c)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)           # the least index is the root
    out = np.full(m.size, NONE, np.int32)
    for p in parent:
        out[p] = find(p)
    return out.reshape(m.shape)


def cluster_records(label, max_clusters=None):
    """(counts int32 [3], records int64 [m,12] or None): roots, frontier voxels, orphans; one row per root in ascending order --
    root, count, sums, minima, maxima of (i, j, k), 0 -- over the frontier voxels whose label is that root.  None in place of the
    records when there are more roots than max_clusters."""
    l = np.asarray(label).astype(np.int64)
    nx, ny, nz = l.shape
    flat = l.reshape(-1)
    n = flat.size
    p = np.arange(n)
    frontier = (flat >= 0) & (flat < NONE)
    is_root = frontier & (flat == p)
    q = np.where(frontier & (flat < n), flat, 0)
    joined = frontier & (flat < n) & (flat[q] == q)
    roots = np.flatnonzero(is_root)
    counts = np.array([len(roots), frontier.sum(), (frontier & ~joined).sum()], np.int32)
    if max_clusters is not None and len(roots) > max_clusters:
        return counts, None
    rec = np.zeros((len(roots), RECORD), np.int64)
    ijk = np.stack([p // (ny * nz), (p // nz) % ny, p % nz], -1)
    for row, r in enumerate(roots):
        v = ijk[joined & (flat == r)]
        rec[row] = [r, len(v), *v.sum(0), *v.min(0), *v.max(0), 0]
    return counts, rec


# ---- the walk of one ray, as the header states it ---------------------------------------------------------------------------
def ray_setup(T, r, c, cam, origin, spacing):
    """(g0 [3], dg [3]) float32 of pixel (r, c) under the camera-to-world pose T"""
    T = np.asarray(T, f32).reshape(4, 4)
    o, s = np.asarray(origin, f32), np.broadcast_to(np.asarray(spacing, f32).reshape(-1), (3,))
    with np.errstate(all="ignore"):
        x = (f32(c) - f32(cam["cx"])) / f32(cam["fx"])
        y = (f32(r) - f32(cam["cy"])) / f32(cam["fy"])
        g0, dg = np.zeros(3, f32), np.zeros(3, f32)
        for a in range(3):
            dW = (T[a, 0] * x + T[a, 1] * y) + T[a, 2]
            g0[a] = (T[a, 3] - o[a]) / s[a]
            dg[a] = dW / s[a]
    return g0, dg


def walk_cells(g0, dg, dims, t_min=0.0, t_max=np.inf):
    """[(cell (i, j, k), t_in float32)] in the order the walk visits them, the states ignored: clip, start and steps of the header"""
    g0, dg = np.asarray(g0, f32), np.asarray(dg, f32)
    assert g0.dtype == f32 and dg.dtype == f32
    if not (np.isfinite(g0).all() and np.isfinite(dg).all()):
        return []
    half = f32(0.5)
    t0, t1 = f32(t_min), f32(t_max)
    with np.errstate(all="ignore"):
        for a in range(3):
            hi = f32(dims[a]) - half
            if dg[a] == 0:
                if g0[a] < -half or g0[a] >= hi:
                    return []
                continue
            ta, tb = (-half - g0[a]) / dg[a], (hi - g0[a]) / dg[a]
            t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
        if not t0 < t1:
            return []
        cell, step, inv, tmax = [0] * 3, [0] * 3, [f32(0)] * 3, [f32(np.inf)] * 3

        def boundary(a):
            return f32(np.inf) if dg[a] == 0 else ((f32(cell[a]) + half * f32(step[a])) - g0[a]) * inv[a]

        for a in range(3):
            cell[a] = int(min(max(np.floor((g0[a] + t0 * dg[a]) + half), f32(0)), f32(dims[a] - 1)))
            step[a] = 1 if dg[a] > 0 else -1
            inv[a] = f32(1) / dg[a]
            tmax[a] = boundary(a)
        out, t_in = [], t0
        for _ in range(sum(dims)):
            out.append((tuple(cell), t_in))
            axis = 1 if tmax[1] < tmax[0] else 0
            axis = 2 if tmax[2] < tmax[axis] else axis
            t_in = tmax[axis]
            if not t_in < t1:
                break
            cell[axis] += step[axis]
            if not 0 <= cell[axis] < dims[axis]:
                break
            tmax[axis] = boundary(axis)
    return out


def walk_ray(state, g0, dg, t_min=0.0, t_max=np.inf):
    """(count, depth float32, [linear indices of the unknown voxels passed])"""
    s = np.asarray(state)
    passed = []
    for cell, t_in in walk_cells(g0, dg, s.shape, t_min, t_max):
        v = s[cell]
        if v == UNKNOWN:
            passed.append(int(np.ravel_multi_index(cell, s.shape)))
        elif v >= OCCUPIED:
            return len(passed), f32(t_in), passed
    return len(passed), f32(0), passed


def view_gain_by_rays(state, origin, spacing, T_WC, cam, H, W, t_min=0.0, t_max=np.inf):
    """(unknown int32 [B,H,W], depth float32 [B,H,W], distinct int32 [B]) ray by ray; distinct is the size of a Python set per view"""
    T_WC = np.asarray(T_WC, f32).reshape(-1, 4, 4)
    unknown = np.zeros((len(T_WC), H, W), np.int32)
    depth = np.zeros((len(T_WC), H, W), f32)
    distinct = np.zeros(len(T_WC), np.int32)
    for b, T in enumerate(T_WC):
        seen = set()
        for r in range(H):
            for c in range(W):
                unknown[b, r, c], depth[b, r, c], passed = walk_ray(state, *ray_setup(T, r, c, cam, origin, spacing), t_min, t_max)
                seen.update(passed)
        distinct[b] = len(seen)
    return unknown, depth, distinct


def view_gain(state, origin, spacing, T_WC, cam, H, W, t_min=0.0, t_max=np.inf):
    """`view_gain_by_rays` with every ray advanced at once: the same float32 operations in the same order, element by element"""
    s = np.ascontiguousarray(state)
    nx, ny, nz = dims = s.shape
    flat = s.reshape(-1)
    T = np.asarray(T_WC, f32).reshape(-1, 4, 4)
    B = len(T)
    o, sp = np.asarray(origin, f32), np.broadcast_to(np.asarray(spacing, f32).reshape(-1), (3,))
    half = f32(0.5)
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        x = ((cc.astype(f32) - f32(cam["cx"])) / f32(cam["fx"]))[None]
        y = ((rr.astype(f32) - f32(cam["cy"])) / f32(cam["fy"]))[None]
        g0, dg = [], []
        for a in range(3):
            dW = (T[:, a, 0, None, None] * x + T[:, a, 1, None, None] * y) + T[:, a, 2, None, None]
            g0.append(np.broadcast_to(((T[:, a, 3] - o[a]) / sp[a])[:, None, None], dW.shape).reshape(-1))
            dg.append((dW / sp[a]).reshape(-1))
        assert all(v.dtype == f32 for v in g0 + dg)
        N = B * H * W
        view = np.repeat(np.arange(B), H * W)
        hit = np.ones(N, bool)
        for v in g0 + dg:
            hit &= np.isfinite(v)
        t0, t1 = np.full(N, t_min, f32), np.full(N, t_max, f32)
        for a in range(3):
            hi = f32(dims[a]) - half
            zero = dg[a] == 0
            hit &= ~(zero & ((g0[a] < -half) | (g0[a] >= hi)))
            ta, tb = (-half - g0[a]) / dg[a], (hi - g0[a]) / dg[a]
            t0 = np.where(zero | ~hit, t0, np.maximum(t0, np.minimum(ta, tb)))
            t1 = np.where(zero | ~hit, t1, np.minimum(t1, np.maximum(ta, tb)))
        hit &= t0 < t1
        cell, step, inv, tmax = [], [], [], []

        def boundary(a, c):
            return np.where(dg[a] == 0, f32(np.inf), ((c.astype(f32) + half * step[a].astype(f32)) - g0[a]) * inv[a])

        for a in range(3):
            c = np.minimum(np.maximum(np.floor((g0[a] + t0 * dg[a]) + half), f32(0)), f32(dims[a] - 1))
            cell.append(np.where(hit, c, 0).astype(np.int64))
            step.append(np.where(dg[a] > 0, 1, -1).astype(np.int64))
            inv.append(f32(1) / dg[a])
            tmax.append(boundary(a, cell[a]))
        assert all(v.dtype == f32 for v in inv + tmax)
        count, depth = np.zeros(N, np.int32), np.zeros(N, f32)
        bits = np.zeros((B, flat.size), bool)
        active, t_in = hit.copy(), t0.copy()
        for _ in range(nx + ny + nz):
            if not active.any():
                break
            p = np.where(active, (cell[0] * ny + cell[1]) * nz + cell[2], 0)
            v = flat[p]
            unk = active & (v == UNKNOWN)
            count += unk
            bits[view[unk], p[unk]] = True
            occ = active & (v >= OCCUPIED)
            depth = np.where(occ, t_in, depth)
            active &= ~occ
            ay = tmax[1] < tmax[0]
            mxy = np.where(ay, tmax[1], tmax[0])
            az = tmax[2] < mxy
            t_in = np.where(active, np.where(az, tmax[2], mxy), t_in)
            active &= t_in < t1
            for a, sel in ((2, active & az), (1, active & ~az & ay), (0, active & ~az & ~ay)):
                cell[a] = np.where(sel, cell[a] + step[a], cell[a])
                left = sel & ((cell[a] < 0) | (cell[a] >= dims[a]))
                active &= ~left
                cell[a] = np.where(left, 0, cell[a])
                tmax[a] = np.where(sel & ~left, boundary(a, cell[a]), tmax[a])
    return count.reshape(B, H, W), depth.reshape(B, H, W), bits.sum(1).astype(np.int32)


# ---- the grids of the tests -------------------------------------------------------------------------------------------------
def chain_state(dims, voxels):
    """OCCUPIED everywhere but FREE at `voxels`, each given one UNKNOWN face neighbour (the first, in FACES order, that is inside the
    grid and not one of `voxels`): the frontier is exactly `voxels`"""
    s = np.full(dims, OCCUPIED, np.uint8)
    vox = {tuple(int(x) for x in v) for v in voxels}
    for v in vox:
        s[v] = FREE
    for v in sorted(vox):
        for d in FACES:
            q = tuple(a + b for a, b in zip(v, d))
            if all(0 <= a < n for a, n in zip(q, dims)) and q not in vox:
                s[q] = UNKNOWN
                break
        else:
            raise AssertionError("no face neighbour left for %s" % (v,))
    assert {tuple(v) for v in np.argwhere(frontier_mask(s))} == vox
    return s


def random_state(dims=(9, 10, 11), seed=5):
    """a third of each state, from a fixed seed"""
    return np.random.RandomState(seed).randint(0, 3, dims).astype(np.uint8)


def serpentine_state():
    """route_model.serpentine's corridor FREE, everything else UNKNOWN: every corridor voxel is a frontier voxel, and the frontier
    is ONE component whose least index has to travel the whole corridor"""
    free, _ = rm.serpentine()
    return np.where(free != 0, FREE, UNKNOWN).astype(np.uint8)


def label_grids(tile=8):
    """name -> state, the grids of the label and cluster tests"""
    n = 2 * tile + 1
    r = np.arange(n)
    one = lambda v: np.full((1, 1, 1), v, np.uint8)
    thin = np.full((1, 1, 40), FREE, np.uint8)
    thin[0, 0, [0, 7, 8, 20, 39]] = UNKNOWN
    thin[0, 0, 30] = OCCUPIED
    face = np.full((5, 6, 7), OCCUPIED, np.uint8)
    face[0, 2, 3] = FREE                                         # on the grid face: its only non-occupied neighbour is outside
    c = tile - 1
    return {
        "one_unknown": one(UNKNOWN), "one_free": one(FREE), "one_occupied": one(OCCUPIED),
        "thin": thin,
        "random": random_state(),
        "corner_chain": chain_state((n, n, n), np.stack([r, r, r], -1)),
        "edge_chain": chain_state((n, n, n), np.stack([r, r, 0 * r], -1)),
        "corner_touch": chain_state((n, n, n), [(c, c, c), (c + 1, c + 1, c + 1)]),
        "corner_apart": chain_state((n, n, n), [(c, c, c), (c + 2, c + 2, c + 2)]),
        "serpentine": serpentine_state(),
        "no_frontier": np.full((9, 10, 11), FREE, np.uint8),
        "face_voxel": face,
    }


# ---- the views of the tests -------------------------------------------------------------------------------------------------
VIEW_DIMS, VIEW_SPACING, VIEW_ORIGIN = (9, 10, 11), (0.1, 0.07, 0.13), (0.3, -0.2, -0.4)
VIEW_CAM = dict(fx=4.0, fy=4.0, cx=2.0, cy=3.0)      # integer cx, cy: the centre ray of an axis-aligned camera has two zero components
VIEW_H, VIEW_W = 7, 5                                # 35 rays: no multiple of the block or of a pixel tile


def exact_coordinate(a, frac, origin=VIEW_ORIGIN, spacing=VIEW_SPACING, bases=(4, 5, 6, 3, 7, 2, 1, 8)):
    """float32 world coordinate e on axis a whose index coordinate (e - origin) / spacing, computed in float32, is EXACTLY
    base + frac for the first base of `bases` that has such a float (not every value has one)"""
    o, s = f32(origin[a]), f32(spacing[a])
    for base in bases:
        want = f32(base + frac)
        e = f32(np.float64(o) + np.float64(want) * np.float64(s))
        lo = hi = e
        for _ in range(16):
            for cand in (lo, hi):
                if (cand - o) / s == want:
                    return cand
            lo, hi = np.nextafter(lo, f32(-np.inf)), np.nextafter(hi, f32(np.inf))
    raise AssertionError("no float32 on axis %d sits at a fraction %s of a voxel" % (a, frac))


def axis_pose(axis, sign, eye):
    """camera-to-world pose looking along sign * e_axis: z = sign e_a, x = e_(a+1), y = z cross x -- every entry 0 or +-1"""
    T = np.eye(4, dtype=f32)
    z, x = np.zeros(3), np.zeros(3)
    z[axis], x[(axis + 1) % 3] = sign, 1.0
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T


def view_poses():
    """(names, T_WC float32 [B,4,4]) over the VIEW grid: inside, outside looking in, looking away, the twelve axis-aligned cameras
    (eye on voxel boundary planes / on voxel centres), a NaN pose and an inf pose"""
    from isdf_amd import explore
    centre = np.asarray(VIEW_ORIGIN) + 0.5 * (np.asarray(VIEW_DIMS) - 1) * np.asarray(VIEW_SPACING)
    names = ["inside", "outside_in", "away"]
    poses = [explore.look_at(centre + [0.03, 0.01, -0.02], centre + [1.0, 0.6, 0.8]).astype(f32),
             explore.look_at(centre + [-1.1, -0.7, 0.4], centre + [0.05, 0.0, 0.1]).astype(f32),
             explore.look_at(centre + [-1.1, -0.7, 0.4], centre + [-3.0, -2.0, 0.5]).astype(f32)]
    for axis in range(3):
        for sign in (1, -1):
            for kind, off in (("boundary", 0.5), ("centre", 0.0)):
                eye = np.array([exact_coordinate(a, off) for a in range(3)], f32)
                eye[axis] = f32(VIEW_ORIGIN[axis] + (-3.0 if sign > 0 else VIEW_DIMS[axis] + 2.0) * VIEW_SPACING[axis])
                names.append("%s%s_%s" % ("+" if sign > 0 else "-", "ijk"[axis], kind))
                poses.append(axis_pose(axis, sign, eye))
    bad = poses[1].copy()
    bad[1, 2] = np.nan
    names.append("nan")
    poses.append(bad)
    bad = poses[1].copy()
    bad[0, 3] = np.inf
    names.append("inf")
    poses.append(bad)
    return names, np.stack(poses).astype(f32)


# ---- the partitioned room of the routing tests, seen from one side ------------------------------------------------------------
WALL_LO, WALL_HI = (2.85, 0.0, 1.2), (3.15, 3.0, 5.0)      # tests/test_route_gpu.py: the door is z < 1.2
ROOM_VOXEL, ROOM_DIMS = 0.1, (60, 30, 50)
ROOM_ORIGIN = (ROOM_VOXEL / 2,) * 3
ROOM_CAM = dict(H=30, W=40, fx=20.0, fy=20.0, cx=19.5, cy=14.5)
ROOM_ROBOT = (1.5, 1.5, 3.0)
ROOM_UP = (0.0, -1.0, 0.0)                                 # the room's y points down


def room_depth(T_WC, cam=ROOM_CAM):
    """float32 [H,W]: synthetic.render_depth of the analytic room with the partition wall in it (no noise, no invalid pixels)"""
    from isdf_amd import synthetic
    T = np.asarray(T_WC, np.float64).reshape(4, 4)
    d = synthetic.dirs_C(cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"]) @ T[:3, :3].T
    o = T[:3, 3]
    t = synthetic.raycast(o, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (np.asarray(WALL_LO) - o) / d, (np.asarray(WALL_HI) - o) / d
        tn, tf = np.nanmax(np.minimum(t1, t2), -1), np.nanmin(np.maximum(t1, t2), -1)
    t = np.where((tn <= tf) & (tn > 1e-6), np.minimum(t, tn), t).astype(f32)
    t[t > 12.0] = 0.0
    return t


def room_first_views():
    """float32 [3,4,4]: three poses at the robot's place that see the near side of the wall only"""
    from isdf_amd import synthetic
    eye = np.asarray(ROOM_ROBOT)
    return np.stack([synthetic.look_at(eye, np.asarray(t)) for t in ((0.3, 1.8, 4.5), (1.5, 1.2, 5.0), (0.2, 1.6, 2.0))])


ROOM_NBV = dict(min_size=20, n_per_cluster=16, radius=0.6, up=ROOM_UP, t_max=5.0)      # next_best_view's options in the room


def room_volume(engine, device):
    """(vol, cam): a fusion.TsdfVolume of the room at 0.1 m voxels with `room_first_views` fused into it by `engine`"""
    import types
    from isdf_amd import fusion
    cam = types.SimpleNamespace(**ROOM_CAM)
    vol = fusion.TsdfVolume(ROOM_DIMS, ROOM_VOXEL, ROOM_ORIGIN, 0.3, device)
    T = room_first_views()
    depth = torch.from_numpy(np.stack([room_depth(t) for t in T])).to(device)
    fusion.integrate(engine, vol, depth, torch.from_numpy(T).to(device), cam)
    return vol, cam


def room_look(engine, vol, cam, T_WC):
    """integrate the depth frame the analytic room shows from T_WC; returns the number of UNKNOWN voxels before and after"""
    from isdf_amd import explore, fusion
    before = int((explore.volume_states(vol) == UNKNOWN).sum())
    depth = torch.from_numpy(room_depth(T_WC)[None]).to(vol.device)
    fusion.integrate(engine, vol, depth, torch.from_numpy(np.asarray(T_WC, f32))[None].to(vol.device), cam)
    return before, int((explore.volume_states(vol) == UNKNOWN).sum())


# ---- a stand-in for the Engine ----------------------------------------------------------------------------------------------
class StubEngine:
    """the tensor-level calls of isdf_amd.engine.Engine that isdf_amd.explore (and, for next_best_view, isdf_amd.routing) uses,
    computed by the models on the host (CPU tensors in and out).  A relax call reaches the fixed point in its first round."""

    def __init__(self):
        self.device = torch.device("cpu")
        self.calls = []
        self._goals = None

    def frontier_init(self, state, out=None):
        self._state = state.numpy().copy()
        return torch.from_numpy(init_labels(self._state))

    def frontier_relax(self, label, rounds=1, changed=None):
        fixed = torch.from_numpy(labels(self._state))
        flags = torch.zeros(rounds, dtype=torch.int32)
        flags[0] = int(not torch.equal(fixed, label))
        label.copy_(fixed)
        return flags

    def frontier_clusters(self, label, max_clusters):
        counts, rec = cluster_records(label.numpy(), max_clusters)
        records = torch.zeros(max_clusters, RECORD, dtype=torch.int64)
        if rec is not None:
            records[:len(rec)] = torch.from_numpy(rec)
        self.calls.append(("clusters", int(max_clusters)))
        return torch.from_numpy(counts), records

    def view_gain(self, state, origin, spacing, T_WC, cam, H, W, t_min=0.0, t_max=np.inf, distinct=True):
        c = dict(fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy)
        T = torch.as_tensor(T_WC).to(torch.float32).reshape(-1, 4, 4).numpy()
        u, d, n = view_gain(state.numpy(), origin, spacing, T, c, H, W, t_min, t_max)
        self.calls.append(("view_gain", len(T), bool(distinct)))
        return torch.from_numpy(u), torch.from_numpy(d), torch.from_numpy(n) if distinct else None

    def tsdf_integrate(self, *args, **kw):
        from tests import fusion_model
        return fusion_model.StubEngine.tsdf_integrate(self, *args, **kw)

    def route_init(self, free, goals, out=None):
        self._goals = np.asarray(goals, np.int64).reshape(-1, 3)
        return torch.full(tuple(free.shape), rm.NONE, dtype=torch.int32)

    def route_relax(self, free, dist, rounds=1, changed=None):
        fixed = torch.from_numpy(rm.dijkstra(free.numpy(), self._goals))
        flags = torch.zeros(rounds, dtype=torch.int32)
        flags[0] = int(not torch.equal(fixed, dist))
        dist.copy_(fixed)
        return flags

    def route_trace(self, dist, starts, max_len):
        s = np.asarray(starts).reshape(-1, 3)
        path = torch.zeros(len(s), max_len, dtype=torch.int32)
        length = torch.zeros(len(s), dtype=torch.int32)
        for b, start in enumerate(s):
            p, n = rm.trace(dist.numpy(), start, max_len)
            path[b, :len(p)] = torch.as_tensor(p, dtype=torch.int32)
            length[b] = n
        return path, length
