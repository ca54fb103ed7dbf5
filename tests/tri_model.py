"""Numpy models of the triangle-mesh kernels (include/isdf_hip.h: isdf_tri_pack, isdf_tri_distance) -- TEST INFRASTRUCTURE.

    pack32 / distance32   float32, the header's pack rules and per-pair sequence restated operation for operation (every numpy
                          float32 operation is rounded once, as the kernel's are: the file is built without contraction)
    distance64 / winding64   float64 models of the distance (the same regions, plain double arithmetic) and of the generalised
                          winding number
    record                the ordered sums of the record (the kernels' one summation order, tests/reduce_model.py)
"""
import numpy as np

from tests.reduce_model import ordered_sum

F = np.float32
TILE, SLOT = 256, 24


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def pack32(vertices, faces, transform=None):
    """(packed float32 [slots, 24], counts [2]) as isdf_tri_pack writes them"""
    v = np.asarray(vertices, F).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    nv, m = len(v), len(f)
    slots = (m + TILE - 1) // TILE * TILE
    out = np.zeros((slots, SLOT), F)
    counts = [0, 0]
    if transform is not None:
        T = np.asarray(transform, F)[:3]
    with np.errstate(all="ignore"):
        for s in range(m):
            if not all(0 <= i < nv for i in f[s]):
                counts[0] += 1
                continue
            p = v[f[s]]
            if transform is not None:
                p = np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], -1)
            if not np.isfinite(p).all():
                counts[0] += 1
                continue
            a, b, c = p
            ab, ac = b - a, c - a
            n = (ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0])
            nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
            if not nn > 0:
                counts[1] += 1
                continue
            ln = np.sqrt(nn)
            out[s] = [a[0], a[1], a[2], _dot(*ab, *ab), ab[0], ab[1], ab[2], _dot(*ab, *ac), ac[0], ac[1], ac[2], _dot(*ac, *ac),
                      b[0], b[1], b[2], 1.0, c[0], c[1], c[2], 0.0, n[0] / ln, n[1] / ln, n[2] / ln, 0.0]
    return out, counts


def _weights(dt, one, apx, apy, apz, t):
    """(v, w, face) by the header's sequence in dtype `dt`; t: the twelve leading floats of the slots, broadcast against the points"""
    d1 = _dot(t[4], t[5], t[6], apx, apy, apz)
    d2 = _dot(t[8], t[9], t[10], apx, apy, apz)
    d3, d4, d5, d6 = d1 - t[3], d2 - t[7], d1 - t[7], d2 - t[11]
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    zero, unit = np.zeros_like(d1), np.ones_like(d1)
    den, nv, nw = (va + vb) + vc, vb, vc
    face = np.ones(d1.shape, bool)
    for cond, (cd, cv, cw) in (((va < 0) & (e43 >= 0) & (e56 >= 0), (e43 + e56, e56, e43)),
                               ((vb < 0) & (d2 >= 0) & (d6 <= 0), (d2 - d6, zero, d2)),
                               ((d6 >= 0) & (d5 <= d6), (unit, zero, unit)),
                               ((vc < 0) & (d1 >= 0) & (d3 <= 0), (d1 - d3, d1, zero)),
                               ((d3 >= 0) & (d4 <= d3), (unit, unit, zero)),
                               ((d1 <= 0) & (d2 <= 0), (unit, zero, zero))):
        den, nv, nw, face = np.where(cond, cd, den), np.where(cond, cv, nv), np.where(cond, cw, nw), face & ~cond
    r = one / den
    return nv * r, nw * r, face


def _distance(dt, packed, pts, block=512):
    packed = np.asarray(packed, dt)
    p = np.asarray(pts, dt).reshape(-1, 3)
    n = len(p)
    valid = packed[:, 15] != 0
    t = [packed[None, :, k] for k in range(12)]
    nh = [packed[None, :, 20 + k] for k in range(3)]
    dist, index, closest = np.empty(n, dt), np.empty(n, np.int32), np.empty((n, 3), dt)
    with np.errstate(all="ignore"):
        for i in range(0, n, block):
            q = p[i:i + block]
            ap = [q[:, k, None] - t[k] for k in range(3)]
            v, w, face = _weights(dt, dt(1), ap[0], ap[1], ap[2], t)
            d = [ap[k] - (t[4 + k] * v + t[8 + k] * w) for k in range(3)]
            dn = (nh[0] * ap[0] + nh[1] * ap[1]) + nh[2] * ap[2]
            d2 = np.where(face, dn * dn, (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            d2 = np.where(valid[None, :] & ~np.isnan(d2), d2, dt(np.inf))
            if d2.shape[1] == 0:
                d2 = np.full((len(q), 1), np.inf, dt)
            win = d2.argmin(1)                              # the first minimum: the lowest index of a tie
            rows = np.arange(len(q))
            best = d2[rows, win]
            none = ~(best < np.inf)
            dist[i:i + block] = np.where(none, dt(np.inf), np.sqrt(best))
            index[i:i + block] = np.where(none, -1, win)
            win = np.where(none, 0, win)
            for k in range(3):
                if packed.shape[0]:
                    c = packed[win, k] + (packed[win, 4 + k] * v[rows, win] + packed[win, 8 + k] * w[rows, win])
                else:
                    c = np.full(len(q), np.nan, dt)
                closest[i:i + block, k] = np.where(none, dt(np.nan), c)
    bad = ~np.isfinite(p).all(1)
    dist[bad], index[bad], closest[bad] = np.nan, -1, np.nan
    return dist, index, closest


def distance32(packed, pts):
    """(dist f32 [n], index i32 [n], closest f32 [n,3]) bit for bit as isdf_tri_distance writes them"""
    return _distance(F, packed, pts)


def distance64(packed, pts):
    """the same regions in plain float64 arithmetic on a float64 `packed` (pack64)"""
    return _distance(np.float64, packed, pts)


def pack64(vertices, faces):
    """float64 slots of a mesh with valid faces only (exact inputs: no pack rule is modelled)"""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    ab, ac = b - a, c - a
    out = np.zeros((len(f), SLOT))
    out[:, 0:3], out[:, 4:7], out[:, 8:11], out[:, 12:15], out[:, 16:19] = a, ab, ac, b, c
    out[:, 3], out[:, 7], out[:, 11], out[:, 15] = (ab * ab).sum(1), (ab * ac).sum(1), (ac * ac).sum(1), 1.0
    n = np.cross(ab, ac)
    out[:, 20:23] = n / np.linalg.norm(n, axis=1, keepdims=True)
    return out


def winding64(vertices, faces, pts, block=512):
    """generalised winding number in float64: sum over the faces of 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|)
    / 4 pi, with a, b, c the vertices minus the point"""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    out = np.empty(len(p))
    for i in range(0, len(p), block):
        q = p[i:i + block, None, :]
        a, b, c = v[f[:, 0]][None] - q, v[f[:, 1]][None] - q, v[f[:, 2]][None] - q
        la, lb, lc = np.linalg.norm(a, axis=-1), np.linalg.norm(b, axis=-1), np.linalg.norm(c, axis=-1)
        det = (a * np.cross(b, c)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        out[i:i + block] = (2.0 * np.arctan2(det, den)).sum(1) / (4.0 * np.pi)
    return out


def record(dist):
    """the four doubles of the record for the per-point distances `dist` (NaN = a non-finite query point)"""
    d = np.asarray(dist, np.float64)
    fin = ~np.isnan(d)
    with np.errstate(invalid="ignore"):
        return np.array([ordered_sum(np.where(fin, d, 0.0)), float(fin.sum()), float((~fin).sum()),
                         d[fin].max() if fin.any() else 0.0])
