"""Numpy models of the tile index and the culled distance (include/isdf_hip.h: isdf_tri_tiles_build, isdf_tri_distance_tiles) -- TEST
INFRASTRUCTURE.

    build64     the tile records in float64, the sums in the record kernels' order (tests/reduce_model.py); order_clean and counts
    run         THE RULE of the header restated per block of 1024 qperm entries on tests/tri_model.py's float32 per-pair sequence:
                which tiles are staged (stats), the (dist2, index) minimum over the staged tiles only, and the winding number with
                the far tiles' dipole terms, near tiles summed in float64
"""
import numpy as np

from tests import tri_model as tm
from tests.reduce_model import block_sum

F = np.float32
TILE, REC, BLOCK = 256, 16, 1024
EPS = 2.0 ** -16
NONE = 0xffffffff


def pad_order(order):
    o = np.asarray(order, np.int64).reshape(-1)
    return np.concatenate([o, np.full(-len(o) % TILE, -1, np.int64)])


def build64(packed, order):
    """(tiles float64 [T, 16], order_clean int32 [T * 256], counts [2]) as isdf_tri_tiles_build writes them"""
    packed = np.asarray(packed, F)
    slots = len(packed)
    o = pad_order(order)
    T = len(o) // TILE
    tiles, clean, counts = np.zeros((T, REC)), np.full(len(o), -1, np.int32), [0, 0]
    for t in range(T):
        e = o[t * TILE:(t + 1) * TILE]
        listed = (e >= 0) & (e < slots)
        s = packed[np.where(listed, e, 0)] if slots else np.zeros((TILE, tm.SLOT), F)
        valid = listed & (s[:, 15] != 0)
        counts[0] += int((~listed & (e != -1)).sum())
        counts[1] += int(valid.sum())
        clean[t * TILE:(t + 1) * TILE] = np.where(valid, e, -1)
        f32 = np.stack([s[:, 0:3], s[:, 12:15], s[:, 16:19]], 1)                       # [256, vertex, xyz]
        p = np.where(valid[:, None, None], f32.astype(np.float64), 0.0)
        ab, ac = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        n = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2],
                      ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], 1)
        area = 0.5 * np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        acc = np.concatenate([0.5 * n, area[:, None] * (((p[:, 0] + p[:, 1]) + p[:, 2]) / 3.0), area[:, None]], 1)
        res = block_sum(acc)
        rec = tiles[t]
        rec[0:3], rec[3:6] = np.inf, -np.inf
        if valid.any():
            c = res[3:6] / res[6]
            d = p[valid] - c
            rec[0:3], rec[3:6] = f32[valid].min((0, 1)), f32[valid].max((0, 1))
            rec[9:12] = c
            rec[12] = np.sqrt(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).max())
            rec[15] = np.nonzero(valid)[0].max() + 1
        rec[6:9], rec[13], rec[14] = res[0:3], res[6], valid.sum()
    return tiles, clean, counts


def pair_d2(rows, P):
    """float32 [len(P), len(rows)]: dist2 of every pair by the header's sequence (tests/tri_model.py); +inf for NaN and skipped slots"""
    rows, P = np.asarray(rows, F), np.asarray(P, F)
    t = [rows[None, :, k] for k in range(12)]
    nh = [rows[None, :, 20 + k] for k in range(3)]
    with np.errstate(all="ignore"):
        ap = [P[:, k, None] - t[k] for k in range(3)]
        v, w, face = tm._weights(F, F(1), ap[0], ap[1], ap[2], t)
        d = [ap[k] - (t[4 + k] * v + t[8 + k] * w) for k in range(3)]
        dn = (nh[0] * ap[0] + nh[1] * ap[1]) + nh[2] * ap[2]
        d2 = np.where(face, dn * dn, (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return np.where((rows[None, :, 15] != 0) & ~np.isnan(d2), d2, F(np.inf))


def solid64(rows, P):
    """float64 [len(P)]: the sum of the solid angles of the triangles `rows` seen from every point"""
    r = np.asarray(rows, np.float64)
    q = np.asarray(P, np.float64)[:, None, :]
    a, b, c = r[None, :, 0:3] - q, r[None, :, 12:15] - q, r[None, :, 16:19] - q
    la, lb, lc = np.linalg.norm(a, axis=-1), np.linalg.norm(b, axis=-1), np.linalg.norm(c, axis=-1)
    det = (a * np.cross(b, c)).sum(-1)
    den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
    return (2.0 * np.arctan2(det, den)).sum(1)


def _norm3(x):
    return np.sqrt((x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2])


def run(packed, tiles, order_clean, pts, qperm=None, beta=0.0, winding=False, solid=solid64):
    """dict(dist f32 [n], index i32 [n], winding f64 [n] or None, stats [4]): isdf_tri_distance_tiles for FINITE results -- a point
    that is not finite or that qperm does not list keeps dist +inf, index -1, winding 0 here.  solid: what sums a near tile's solid
    angles in float64 (solid64, or the same arithmetic elsewhere)"""
    packed, pts = np.asarray(packed, F), np.asarray(pts, F).reshape(-1, 3)
    tiles, clean = np.asarray(tiles, np.float64), np.asarray(order_clean, np.int64)
    n, T = len(pts), len(tiles)
    qperm = np.arange(n) if qperm is None else np.asarray(qperm, np.int64)
    best, index, wn, stats = np.full(n, np.inf, F), np.full(n, -1, np.int32), np.zeros(n), [0, 0, 0, 0]
    tl, th, N, c, r, nonempty = tiles[:, 0:3], tiles[:, 3:6], tiles[:, 6:9], tiles[:, 9:12], tiles[:, 12], tiles[:, 14] > 0
    for g in range(-(-n // BLOCK)):
        ent = qperm[g * BLOCK:(g + 1) * BLOCK]
        ok = (ent >= 0) & (ent < n)
        stats[2] += 1
        stats[3] += int((~ok).sum())
        q = ent[ok]
        q = q[np.isfinite(pts[q]).all(1)]
        if not len(q) or not nonempty.any():
            continue
        P = pts[q]
        P64 = P.astype(np.float64)
        bl, bh = P64.min(0), P64.max(0)
        with np.errstate(invalid="ignore"):
            mind = _norm3(np.maximum(0.0, np.maximum(tl - bh, bl - th)))
            maxd = _norm3(np.maximum(np.abs(th - bl), np.abs(bh - tl)))
        seed = int(np.argmin(np.where(nonempty, maxd, np.inf)))                          # the first minimum: the lowest tile
        U = F(np.inf)
        b, bi, ws = np.full(len(q), np.inf, F), np.full(len(q), NONE, np.int64), np.zeros(len(q))
        for t in [seed] + [t for t in range(T) if t != seed]:
            if not nonempty[t]:
                continue
            do_dist = t == seed or mind[t] - EPS * maxd[t] <= np.sqrt(np.float64(U))
            near = False
            if winding:
                dc = _norm3(np.maximum(0.0, np.maximum(c[t] - bh, bl - c[t])))
                near = not beta > 0 or not dc >= beta * r[t]
                if not near:
                    d = c[t] - P64
                    r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                    ws = ws + ((N[t, 0] * d[:, 0] + N[t, 1] * d[:, 1]) + N[t, 2] * d[:, 2]) / (r2 * np.sqrt(r2))
            if not do_dist and not near:
                continue
            stats[0] += int(do_dist)
            stats[1] += int(near)
            e = clean[t * TILE:(t + 1) * TILE]
            e = e[(e >= 0) & (e < len(packed))]
            rows = packed[e]
            if do_dist:
                d2 = pair_d2(rows, P)
                dmin = d2.min(1)
                cand = np.where(d2 == dmin[:, None], e[None, :], NONE).min(1)            # the lowest index of a tie within the tile
                better = (dmin < b) | ((dmin == b) & (cand < bi))
                b, bi = np.where(better, dmin, b), np.where(better, cand, bi)
                U = b.max()
            if near:
                ws = ws + solid(rows[rows[:, 15] != 0], P)
        found = b < np.inf
        best[q], index[q] = b, np.where(found, bi, -1)
        wn[q] = ws / (4.0 * np.pi)
    return dict(dist=np.sqrt(best), index=index, winding=wn if winding else None, stats=stats)
