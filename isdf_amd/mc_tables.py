"""Marching-cubes tables of isdf_amd/csrc/mesh.hip, generated from first principles (no table is copied from anywhere).

    python -m isdf_amd.mc_tables            # rewrites isdf_amd/csrc/mc_tables.h
    python -m isdf_amd.mc_tables --check    # exit status 1 if the committed header is stale

Conventions (shared with the kernels, the C ABI's isdf_mc_tables and tests/mc_oracle.py):
  * corner c of the cell at grid point (i, j, k) is the point (i + (c & 1), j + (c >> 1 & 1), k + (c >> 2 & 1));
    the case index has bit c set iff corner c is INSIDE (value < level);
  * edge e = 4 * axis + m runs along `axis` (0: i, 1: j, 2: k) from EDGE_CORNERS[e][0] (the corner whose `axis` bit is 0, the
    m-th such corner in increasing order) to EDGE_CORNERS[e][1]; its vertex is owned by the grid point of that lower corner;
  * TRI_TABLE[case] lists the case's triangles as edge triples, -1 padded; the right-hand normal of (e0, e1, e2) points to the
    OUTSIDE (increasing value).

How a case is triangulated.  Each of the cube's six faces contributes boundary segments between its sign-changing edges: one
segment when two of its edges change sign, two when all four do (the ambiguous face: diagonal corners share a sign).  An
ambiguous face is always resolved by cutting off its two INSIDE corners -- a rule that reads nothing but that face's four corner
signs, so the two cells sharing a face always draw the same segments on it and the surface has no cracks (a table built by
complement symmetry breaks exactly this).  Every sign-changing edge then lies on two segments (one per face through it), so the
segments close into loops; each loop is oriented as the boundary of the inside region of the cube's surface and fanned into
triangles, with the fan's apex chosen so that no interior diagonal joins two edges of a common face (a diagonal the neighbour could
also draw would be shared by four triangles)."""
import itertools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "csrc", "mc_tables.h")


def _corner(c):
    return (c & 1, c >> 1 & 1, c >> 2 & 1)


def _edges():
    out = []
    for axis in range(3):
        lows = [c for c in range(8) if not c >> axis & 1]
        out += [(c, c | 1 << axis) for c in lows]
    return out


EDGE_CORNERS = _edges()


def _faces():
    """(axis, side, [corners in cyclic order], [edges in the same cyclic order: edge q joins corner q and q+1])"""
    out = []
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        for side in range(2):
            base = side << axis
            cyc = [base, base | 1 << u, base | 1 << u | 1 << v, base | 1 << v]
            eds = []
            for q in range(4):
                a, b = cyc[q], cyc[(q + 1) % 4]
                eds.append(next(e for e, (x, y) in enumerate(EDGE_CORNERS) if {x, y} == {a, b}))
            out.append((axis, side, cyc, eds))
    return out


FACES = _faces()
EDGE_FACES = [[f for f, (_, _, _, eds) in enumerate(FACES) if e in eds] for e in range(12)]


def _mid(e):
    a, b = EDGE_CORNERS[e]
    return tuple(0.5 * (x + y) for x, y in zip(_corner(a), _corner(b)))


def _sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _face_segments(case, face):
    """boundary segments (edge_from, edge_to) on one face, oriented with the inside corner on their left seen from outside"""
    axis, side, cyc, eds = face
    inside = [case >> c & 1 for c in cyc]
    changing = [q for q in range(4) if inside[q] != inside[(q + 1) % 4]]
    if not changing:
        return []
    if len(changing) == 2:
        pairs = [(changing[0], changing[1], next(cyc[q] for q in range(4) if inside[q]))]
    else:   # ambiguous face: cut off each inside corner (edges q-1 and q meet at corner q)
        pairs = [((q - 1) % 4, q, cyc[q]) for q in range(4) if inside[q]]
    normal = tuple((1.0 if side else -1.0) if a == axis else 0.0 for a in range(3))
    segs = []
    for qa, qb, cin in pairs:
        p, r = _mid(eds[qa]), _mid(eds[qb])
        s = _dot(normal, _cross(_sub(r, p), _sub(_corner(cin), p)))
        segs.append((eds[qa], eds[qb]) if s > 0 else (eds[qb], eds[qa]))
    return segs


def _shares_face(e1, e2):
    return bool(set(EDGE_FACES[e1]) & set(EDGE_FACES[e2]))


def _fan(loop):
    n = len(loop)
    for apex in range(n):
        rot = loop[apex:] + loop[:apex]
        if all(not _shares_face(rot[0], rot[i]) for i in range(2, n - 1)):
            return [(rot[0], rot[i], rot[i + 1]) for i in range(1, n - 1)]
    raise AssertionError("no fan without a shared-face diagonal: %r" % (loop,))


def triangulate(case):
    segs = [s for f in FACES for s in _face_segments(case, f)]
    nxt = {}
    for a, b in segs:
        assert a not in nxt, (case, a)
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values())
    tris, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        # the loop runs with the inside on its left seen from outside the cube; its fan's right-hand normal then points to the
        # inside corners -- reversed, it points to the outside (increasing value)
        for t in _fan(loop):
            tris.append((t[0], t[2], t[1]))
    return tris


TRIS = [triangulate(c) for c in range(256)]
MAX_TRIS = max(len(t) for t in TRIS)
TRI_WIDTH = 3 * MAX_TRIS


def tri_table():
    return [list(itertools.chain(*t)) + [-1] * (TRI_WIDTH - 3 * len(t)) for t in TRIS]


def header_text():
    rows = ",\n".join("  {" + ", ".join("%d" % v for v in row) + "}" for row in tri_table())
    cnt = ", ".join("%d" % len(t) for t in TRIS)
    ec = ", ".join("{%d, %d}" % p for p in EDGE_CORNERS)
    return ("// Generated by `python -m isdf_amd.mc_tables` -- do not edit (conventions and construction: isdf_amd/mc_tables.py).\n"
            "#pragma once\n#include <stdint.h>\n\nnamespace isdf {\nnamespace mc {\n\n"
            "constexpr int kMaxTris = %d;\n"
            "constexpr int kTriWidth = 3 * kMaxTris;\n\n"
            "// edge e: from corner [e][0] to corner [e][1]; axis e / 4\n"
            "constexpr int8_t kEdgeCorners[12][2] = {%s};\n\n"
            "constexpr uint8_t kTriCount[256] = {%s};\n\n"
            "constexpr int8_t kTriTable[256][kTriWidth] = {\n%s};\n\n"
            "}  // namespace mc\n}  // namespace isdf\n") % (MAX_TRIS, ec, cnt, rows)


if __name__ == "__main__":
    text = header_text()
    if "--check" in sys.argv:
        ok = os.path.exists(HEADER) and open(HEADER).read() == text
        print("mc_tables.h is %s" % ("up to date" if ok else "STALE"))
        sys.exit(0 if ok else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    print("wrote %s (max %d triangles per cell)" % (HEADER, MAX_TRIS))
