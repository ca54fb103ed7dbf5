"""A float32 numpy model of the narrow-band selection rule (include/isdf_hip.h, "narrow-band selection"; isdf_amd/csrc/band.hip),
and the analytic distance fields the band tests share.

`band(vol, A, level, slack, coarse)` takes the DENSE volume of the field and reads it only where the rule has evaluated it.  It
returns the kept cells per stride, the evaluated mask, the per-level counts and the leak count.  The kernel forms the cell
diagonal d with fused multiply-adds, the model without: `min_margin`, the smallest relative distance of any decided cell's
max|f - level| from slack * d, says whether that rounding could matter for the given input (the tests ask for > 1e-4)."""
import numpy as np


def cells(D, s):
    """cells of stride s along an axis of D lattice points, the last one clipped"""
    return (D - 1 + s - 1) // s


def strides(coarse):
    out, s = [], int(coarse)
    while s >= 2:
        out.append(s)
        s //= 2
    return out


def _corner_axes(dims, s):
    lo = [np.arange(cells(D, s)) * s for D in dims]
    hi = [np.minimum(l + s, D - 1) for l, D in zip(lo, dims)]
    return lo, hi


def sign_changing_cells(vol, level=0.0):
    """bool [D0-1, D1-1, D2-1]: unit cells marching cubes meshes (eight finite corners, not all on one side of level)"""
    D0, D1, D2 = vol.shape
    c = [vol[a:D0 - 1 + a, b:D1 - 1 + b, cc:D2 - 1 + cc] for a in (0, 1) for b in (0, 1) for cc in (0, 1)]
    fin = np.all([np.isfinite(x) for x in c], axis=0)
    inside = np.sum([x < level for x in c], axis=0)
    return fin & (inside != 0) & (inside != 8)


def band(vol, A=None, level=0.0, slack=1.5, coarse=8):
    vol = np.asarray(vol, np.float32)
    dims = vol.shape
    A3 = np.eye(3, dtype=np.float32) if A is None else np.asarray(A, np.float32).reshape(3, 4)[:, :3]
    level, slack = np.float32(level), np.float32(slack)
    ev = np.zeros(dims, bool)
    parent, levels, kept_by_stride = None, [], {}
    min_margin = np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        for s in strides(coarse):
            n = [cells(D, s) for D in dims]
            if parent is None:
                cand = np.ones(n, bool)
            else:
                cand = parent.repeat(2, 0).repeat(2, 1).repeat(2, 2)[:n[0], :n[1], :n[2]]
            lo, hi = _corner_axes(dims, s)
            need = np.zeros(dims, bool)
            corners = []
            for q in range(8):
                ix = np.ix_(*[(hi if q >> a & 1 else lo)[a] for a in range(3)])
                need[ix] |= cand
                corners.append(vol[ix])
            new = need & ~ev
            ev |= need
            f = np.stack(corners)
            bad = ~np.isfinite(f).all(0)
            inside = (f < level).sum(0)
            mixed = (inside != 0) & (inside != 8)
            m = np.fmax.reduce(np.abs(f - level), axis=0).astype(np.float32)
            e = np.stack(np.meshgrid(*[(h - l).astype(np.float32) for l, h in zip(lo, hi)], indexing="ij"))     # [3, n0, n1, n2]
            w = [A3[r, 0] * e[0] + A3[r, 1] * e[1] + A3[r, 2] * e[2] for r in range(3)]
            d = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]).astype(np.float32)
            thr = (slack * d).astype(np.float32)
            kept = cand & (bad | mixed | (m <= thr))
            decided = cand & ~bad & ~mixed & (thr > 0)
            if decided.any():
                min_margin = min(min_margin, float(np.min(np.abs(m[decided].astype(np.float64) - thr[decided]) / thr[decided])))
            levels.append(dict(stride=s, candidates=int(cand.sum()), kept=int(kept.sum()), evaluated=int(new.sum())))
            kept_by_stride[s] = kept
            parent = kept
        kept2 = kept_by_stride[2]
        n = kept2.shape
        need = np.zeros(dims, bool)
        for oi in range(-1, 4):
            for oj in range(-1, 4):
                for ok in range(-1, 4):
                    idx = [2 * np.arange(n[a]) + o for a, o in enumerate((oi, oj, ok))]
                    val = [(x >= 0) & (x <= D - 1) for x, D in zip(idx, dims)]
                    need[np.ix_(*[x[v] for x, v in zip(idx, val)])] |= kept2[np.ix_(*val)]
        new = need & ~ev
        ev |= need
        levels.append(dict(stride=1, evaluated=int(new.sum())))
        out = np.where(ev, vol, np.float32(np.nan)).astype(np.float32)
        D0, D1, D2 = dims
        all_ev = np.all([ev[a:D0 - 1 + a, b:D1 - 1 + b, c:D2 - 1 + c] for a in (0, 1) for b in (0, 1) for c in (0, 1)], axis=0)
        in_kept = kept2.repeat(2, 0).repeat(2, 1).repeat(2, 2)[:D0 - 1, :D1 - 1, :D2 - 1]
        sc = sign_changing_cells(vol, level)
        leaks = int((sc & all_ev & ~in_kept).sum())
    return dict(levels=levels, kept=kept_by_stride, evaluated_mask=ev, in_kept=in_kept, volume=out, leaks=leaks,
                evaluated=int(ev.sum()), dense=int(np.prod(dims)), min_margin=min_margin)


def lattice_points(dims, A):
    """float64 [D0, D1, D2, 3]: the affine at every lattice point"""
    A = np.asarray(A, np.float64).reshape(3, 4)
    G = np.stack(np.meshgrid(*[np.arange(D, dtype=np.float64) for D in dims], indexing="ij"), -1)
    return G @ A[:, :3].T + A[:, 3]


# ---- analytic distance fields with |grad f| = 1, written once for numpy and torch (xp = the module, p = [..., 3] points).
# Lengths are in units of R, the smallest half extent of the grid's world box, positions relative to its centre c.
def _norm(xp, v):
    return xp.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])


def _shift(p, c, off, R):
    return p - (c + R * off)


def _vec(xp, p, v):
    return np.asarray(v, dtype=p.dtype) if xp is np else xp.tensor(v, dtype=p.dtype, device=p.device)


def sphere(xp, p, c, R, r=0.6230, off=(0.031, -0.017, 0.023)):
    return _norm(xp, _shift(p, c, _vec(xp, p, off), R)) - r * R


def torus(xp, p, c, R, major=0.5470, minor=0.2130, off=(0.013, 0.029, -0.011)):
    q = _shift(p, c, _vec(xp, p, off), R)
    ring = xp.sqrt(q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) - major * R
    return xp.sqrt(ring * ring + q[..., 2] * q[..., 2]) - minor * R


def two_spheres(xp, p, c, R, r1=0.4130, r2=0.3370, o1=(-0.27, 0.05, 0.02), o2=(0.33, -0.04, 0.06)):
    a = _norm(xp, _shift(p, c, _vec(xp, p, o1), R)) - r1 * R
    b = _norm(xp, _shift(p, c, _vec(xp, p, o2), R)) - r2 * R
    return xp.minimum(a, b)


def slab(xp, p, c, R, half=0.1730, n=(0.48, 0.6, 0.64), off=(0.02, 0.01, -0.03)):
    """a tilted plane slab (|n| = 1): it runs through the whole box, so the band meets every border"""
    q = _shift(p, c, _vec(xp, p, off), R)
    return xp.abs(q[..., 0] * n[0] + q[..., 1] * n[1] + q[..., 2] * n[2]) - half * R


FIELDS = {"sphere": sphere, "torus": torus, "two_spheres": two_spheres, "slab": slab}


def box_of(dims, A):
    """(centre [3], R): the world box of the lattice and its smallest half extent along the affine's columns"""
    A = np.asarray(A, np.float64).reshape(3, 4)
    half = (np.asarray(dims, np.float64) - 1) / 2
    c = A[:, :3] @ half + A[:, 3]
    R = float(np.min(np.linalg.norm(A[:, :3], axis=0) * half))
    return c, R


def affine(kind, dims):
    """the tests' index -> world affines: "unit" (world = index) and "aniso" (unequal voxel sizes, rotated about z, shifted)"""
    if kind == "unit":
        return np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)
    c, s = np.cos(0.4), np.sin(0.4)
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    A = np.concatenate([Rz * np.array([0.031, 0.047, 0.038])[None, :], np.array([[0.4], [-1.2], [0.7]])], 1)
    return A.astype(np.float32)


# (field, dims, affine kind, field size): sizes searched so that every case's min_margin at slack 1.05 exceeds 2.5e-4; tests/test_band_cpu.py
# asserts > 1e-4 for each, which makes the exact count comparisons against the device meaningful
CASES = [("sphere", (64, 64, 64), "unit", dict(r=0.6233)), ("torus", (64, 64, 64), "unit", dict(minor=0.2133)),
         ("two_spheres", (64, 64, 64), "unit", dict(r1=0.4134)), ("slab", (64, 64, 64), "unit", dict(half=0.1731)),
         ("sphere", (37, 64, 50), "unit", dict(r=0.6237)), ("torus", (37, 64, 50), "unit", dict(minor=0.2131)),
         ("two_spheres", (37, 64, 50), "unit", dict(r1=0.4134, r2=0.3373)), ("slab", (37, 64, 50), "unit", dict(half=0.1730)),
         ("torus", (64, 64, 64), "aniso", dict(minor=0.2135))]
SLACK = 1.05


def case_id(case):
    return "%s-%s-%s" % (case[0], "x".join(str(d) for d in case[1]), case[2])


def dense_volume(name, dims, kind, kw):
    """(float32 volume, A) of a case: the field on the float32-rounded lattice points"""
    A = affine(kind, dims)
    c, R = box_of(dims, A)
    p = lattice_points(dims, A).astype(np.float32)
    return FIELDS[name](np, p, c.astype(np.float32), np.float32(R), **kw).astype(np.float32), A


def torch_field(name, dims, kind, kw):
    """(callable device points [n, 3] -> values [n], A): the same field in torch float32, for `field=`"""
    import torch
    A = affine(kind, dims)
    c, R = box_of(dims, A)

    def field(p):
        return FIELDS[name](torch, p, torch.tensor(c, dtype=p.dtype, device=p.device), float(np.float32(R)), **kw)
    return field, A
