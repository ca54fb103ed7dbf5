"""Float64 model of the per-frame ingest (`isdf_estimate_normals`, isdf_amd/csrc/ingest.hip) with a per-pixel bound on what
float32 arithmetic may do to it, the acceptance rule built on that bound, the inputs of tests/test_ingest_cpu.py and
tests/test_ingest_gpu.py, and the inputs of the keyframe-render (`isdf_render_depth`) checks.  numpy only.

The operation sequence of the kernel (u = 2^-24 is the unit round-off, "ulp" = 2^-23 relative):

  point      x = fl(fl(z * fl(j - cx)) * rcp(fx)), rcp = v_rcp_f32, 1 ulp = 2u: relative error <= u + u + 2u + u = 5u.  y likewise,
             z is the depth itself (exact).  The float32 oracle and the reference divide (u instead of 3u for the last two
             steps).  Per point and component         delta = 3 * 2^-23 * max(|x|, |y|)          (6u >= 5u)
  difference q = fl(p_neighbour - p_centre), per component:
                                                     dq = delta_n + delta_c + 2^-24 * max_i |q_i|
             so the computed vector is within sqrt(3) dq of the exact one (Euclidean).
  length     fl-sum of three squares (three products, two additions of non-negative terms: relative error <= 3u), v_sqrt_f32
             (halves it, adds 2u): <= 3.5u relative on the length OF THE COMPUTED difference; by the triangle inequality that
             length is within sqrt(3) dq of the exact one.
  score      s_k = fl(len_k + len_k2), one more u:
                                                     E_k = (1 + 2^-20) sqrt(3) (dq_k + dq_k2) + 4 * 2^-23 * s_k
             (4.5u s_k is what the sequence gives; 8u leaves room for a reference that sums the squares in another order).
  cross      c = a x b on the computed differences, each component fl(fl(a_i b_j) - fl(a_j b_i)).  |a_i b_j| + |a_j b_i| <=
             |a||b| (Cauchy-Schwarz), so the rounding is <= 2u |a||b| per component, sqrt(3) 2u |a||b| < 2 * 2^-23 |a||b| as a
             vector; the perturbed inputs add |da x b| + |a x db| + |da x db| <= sqrt(3)(dq_a |b| + dq_b |a|) + 3 dq_a dq_b:
                                                     e_k = sqrt(3)(dq_k |q_k2| + dq_k2 |q_k|) + 3 dq_k dq_k2 + 2 * 2^-23 |q_k||q_k2|
  normalise  | x/|x| - y/|y| | <= 2 |x - y| / max(|x|, |y|); then the norm (3.5u as above), v_rcp_f32 (2u) and the product (u):
             6.5u on a component of a unit vector:
                                                     t_k = 2 e_k / |q_k x q_k2| + 4 * 2^-23
             Where e_k >= |q_k x q_k2| the computed cross product may vanish, so a NaN is admissible for that pair as well.

Acceptance of a pixel: the candidate pairs are {k : s_k finite, s_k - E_k <= min_j (s_j + E_j)} -- the pairs float32 arithmetic may
rank first -- or pair 0 if no score is finite.  The kernel's normal must be within t_k (max-abs over the components) of n_k for
some candidate k; where n_k is NaN (no finite pair, or a zero cross product) the kernel's normal must be NaN.  Nothing is excluded.
"""
import numpy as np

import oracle.isdf_oracle as orc

U23 = 2.0 ** -23
LOOK = [(-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1)]      # times the stride; transform.py:226-236


def _shift(P, pad, k, stride, H, W):
    dy, dx = LOOK[k][0] * stride, LOOK[k][1] * stride
    return P[..., pad + dy:pad + dy + H, pad + dx:pad + dx + W]


def model(depth, fx, fy, cx, cy):
    """depth float32 [H,W]; intrinsics as the kernel gets them (rounded to float32).  Returns float64 arrays over [8,H,W]:
    s (score, inf where not finite), E, n ([8,H,W,3]), t, and nan_ok (a vanishing computed cross product is possible)."""
    z = np.asarray(depth, np.float32).astype(np.float64)
    H, W = z.shape
    fx, fy, cx, cy = (float(np.float32(v)) for v in (fx, fy, cx, cy))
    j = np.arange(W, dtype=np.float64)[None, :]
    i = np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        p = np.stack((z * (j - cx) / fx, z * (i - cy) / fy, z))                 # [3,H,W]
        delta = 3 * U23 * np.maximum(np.abs(p[0]), np.abs(p[1]))
        d = 2
        P = np.full((3, H + 2 * d, W + 2 * d), np.nan)
        P[:, d:-d, d:-d] = p
        D = np.full((1, H + 2 * d, W + 2 * d), np.nan)
        D[0, d:-d, d:-d] = delta
        q = np.stack([_shift(P, d, k, d, H, W) - p for k in range(8)])          # [8,3,H,W]
        dq = np.stack([_shift(D, d, k, d, H, W)[0] + delta for k in range(8)]) + 2.0 ** -24 * np.abs(q).max(1)
        L = np.sqrt((q * q).sum(1))                                             # [8,H,W]
        k2 = (np.arange(8) + 2) % 8
        s = L + L[k2]
        E = (1 + 2.0 ** -20) * np.sqrt(3.0) * (dq + dq[k2]) + 4 * U23 * s
        a, b = np.moveaxis(q, 1, -1), np.moveaxis(q[k2], 1, -1)                 # [8,H,W,3]
        c = np.cross(a, b)
        cn = np.sqrt((c * c).sum(-1))
        n = c / cn[..., None]
        e = np.sqrt(3.0) * (dq * L[k2] + dq[k2] * L) + 3 * dq * dq[k2] + 2 * U23 * L * L[k2]
        t = 2 * e / cn + 4 * U23
        nan_ok = ~(e < cn)                                                      # also where cn is 0 or NaN
    fin = np.isfinite(s)
    s = np.where(fin, s, np.inf)
    return dict(s=s, E=np.where(fin, E, 0.0), n=n, t=t, nan_ok=nan_ok, finite=fin)


def candidates(m):
    """[8,H,W] bool: the pairs float32 arithmetic may rank first (pair 0 where no score is finite)"""
    hi = np.where(m["finite"], m["s"] + m["E"], np.inf).min(0)
    cand = m["finite"] & (m["s"] - m["E"] <= hi)
    none = ~m["finite"].any(0)
    cand[0] |= none
    return cand


def judge(m, normals):
    """The acceptance rule on every pixel.  Returns dict(fail [H,W] bool, ratio [H,W] = error / bound of the best admissible
    candidate (0 where a NaN answers a NaN), multi [H,W] bool = more than one candidate)."""
    got = np.asarray(normals, np.float32).astype(np.float64)
    cand = candidates(m)
    got_nan = np.isnan(got).any(-1)                                             # [H,W]
    with np.errstate(invalid="ignore"):
        err = np.abs(got[None] - m["n"]).max(-1)                                # [8,H,W]; NaN where either is NaN
        ratio = err / m["t"]
    n_nan = np.isnan(m["n"]).any(-1)
    ok_fin = cand & ~n_nan & ~got_nan[None] & (ratio <= 1.0)
    ok_nan = cand & got_nan[None] & (n_nan | m["nan_ok"])
    ok = ok_fin | ok_nan
    best = np.where(ok_fin, ratio, np.where(ok_nan, 0.0, np.inf)).min(0)
    worst = np.where(cand & ~n_nan & ~got_nan[None], ratio, np.inf).min(0)      # for reporting a failing pixel's ratio
    fail = ~ok.any(0)
    return dict(fail=fail, ratio=np.where(fail, worst, best), multi=cand.sum(0) > 1, cand=cand)


def conditions(m):
    """(share of pixels with more than one candidate, share of the single-candidate finite pixels with t <= 1e-3, their largest
    t): conditions on an INPUT, from the model alone"""
    cand = candidates(m)
    multi = cand.sum(0) > 1
    single = ~multi & m["finite"].any(0)
    t1 = np.where(cand, m["t"], 0.0).sum(0)[single]                             # the one candidate's t
    t1 = t1[np.isfinite(t1)] if t1.size else t1
    return float(multi.mean()), (float((t1 <= 1e-3).mean()) if t1.size else 1.0), (float(t1.max()) if t1.size else 0.0)


# ---- the float32 oracle, transcribed with switches for the sensitivity mutants -------------------------------------------------
MUTANTS = ("last_minimum", "pair_k_k1", "zero_padding", "stride_1", "seam_column_32", "cx_ignored")


def f32_normals(depth, fx, fy, cx, cy, mutant=None, want_scores=False):
    """`oracle.isdf_oracle.estimate_pointcloud_normals` of `pointcloud_from_depth`, operation for operation (mutant None is
    bit-identical to it: tests/test_ingest_cpu.py), with one defect switched on per mutant."""
    assert mutant is None or mutant in MUTANTS
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    pts = orc.pointcloud_from_depth(depth, fx, fy, 0.0 if mutant == "cx_ignored" else cx, cy)
    d = 1 if mutant == "stride_1" else 2
    P = np.full((H + 2 * d, W + 2 * d, 3), 0.0 if mutant == "zero_padding" else np.nan, np.float32)
    P[d:-d, d:-d] = pts
    step = 1 if mutant == "pair_k_k1" else 2
    sh = lambda k: P[d + LOOK[k][0] * d:d + LOOK[k][0] * d + H, d + LOOK[k][1] * d:d + LOOK[k][1] * d + W]
    best, nrm, scores = None, None, []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(8):
            p2, p3 = sh(k), sh((k + step) % 8)
            diff = np.linalg.norm(p2 - pts, axis=-1) + np.linalg.norm(p3 - pts, axis=-1)
            diff = np.where(np.isnan(diff), np.float32(np.inf), diff)
            scores.append(diff)
            n = np.cross(p2 - pts, p3 - pts)
            if best is None:
                best, nrm = diff, n
            else:
                take = diff <= best if mutant == "last_minimum" else diff < best
                nrm = np.where(take[..., None], n, nrm)
                best = np.where(take, diff, best)
        out = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    if mutant == "seam_column_32" and W > 32:
        out[:, 32] = out[:, 31]
    return (out, np.stack(scores)) if want_scores else out


# ---- inputs ------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (2, 3), (5, 7), (15, 31), (16, 32), (17, 33), (37, 100), (60, 80)]     # block: 32 wide, 16 high, 2-pixel halo
VARIANTS = ("noise_0.01", "noise_0.002", "clean", "nan_pixels", "zero_patch")
NOISY = ("noise_0.01", "noise_0.002", "nan_pixels", "zero_patch")                         # the caps of `conditions` apply to these
CAMERAS = ("centred", "skewed")


def camera(H, W, which):
    if which == "centred":
        return dict(H=H, W=W, fx=0.9 * W, fy=0.9 * W, cx=(W - 1) / 2.0, cy=(H - 1) / 2.0)
    return dict(H=H, W=W, fx=0.8 * W + 3.3, fy=1.1 * W + 1.7, cx=0.3 * W, cy=0.7 * H)       # fx != fy, principal point well off centre


def depth_input(H, W, variant, which):
    """(depth float32 [H,W], cam) of one GPU input: `synthetic.render_depth` of the first room pose"""
    from isdf_amd import synthetic
    cam = camera(H, W, which)
    seed = 1000 * H + W + (0 if which == "centred" else 500000) + 17 * VARIANTS.index(variant)
    rng = np.random.RandomState(seed)
    T = synthetic.trajectory(1)[0]
    if variant == "noise_0.01":
        d = synthetic.render_depth(T, cam, rng, invalid_frac=0.05, noise_std=0.01)
    elif variant == "clean":
        d = synthetic.render_depth(T, cam, None, invalid_frac=0.0, noise_std=0.0)
    else:
        d = synthetic.render_depth(T, cam, rng, invalid_frac=0.02, noise_std=0.002)
    if variant == "nan_pixels":
        for _ in range(5):
            d[rng.randint(H), rng.randint(W)] = np.nan
    if variant == "zero_patch":
        i0, j0 = max((H - 3) // 2, 0), max((W - 3) // 3, 0)
        d[i0:i0 + 3, j0:j0 + 3] = 0.0
    return d, cam


def all_inputs(shapes=SHAPES):
    for H, W in shapes:
        for which in CAMERAS:
            for variant in VARIANTS:
                d, cam = depth_input(H, W, variant, which)
                yield "%dx%d/%s/%s" % (H, W, which, variant), variant, d, cam


def roof():
    """9 x 9, fx = fy = 4, cx = cy = 4, depth = 2 + |j - 4| / 4: every quantity is exactly representable.  On the ridge column the
    float32 scores of pairs 0, 2, 4 and 6 tie bit for bit; pairs 0 and 2 give (-0.3714, 0, 0.9285), pairs 4 and 6 its mirror image,
    and `first minimum wins` asks for pair 0's."""
    j = np.arange(9, dtype=np.float32)[None, :].repeat(9, 0)
    return (2 + 0.25 * np.abs(j - 4)).astype(np.float32), dict(H=9, W=9, fx=4.0, fy=4.0, cx=4.0, cy=4.0)


ROOF_NORMAL = np.array([-0.5, 0.0, 1.25]) / np.sqrt(0.25 + 1.5625)


def judge_roof(normals):
    """[9,9] bool, failing pixels of the roof image: the acceptance rule everywhere and, on rows 2..6 of the ridge column (where the
    four tied pairs are all inside the image and float32 arithmetic is exact up to the final normalisation), pair 0's normal to
    4 * 2^-23 -- the rule alone admits every tied pair, the reference's argmin admits the first"""
    d, cam = roof()
    fail = judge(model(d, cam["fx"], cam["fy"], cam["cx"], cam["cy"]), normals)["fail"].copy()
    with np.errstate(invalid="ignore"):
        fail[2:7, 4] |= ~(np.abs(np.asarray(normals, np.float64)[2:7, 4] - ROOF_NORMAL).max(-1) <= 4 * U23)
    return fail


# ---- isdf_render_depth inputs ----------------------------------------------------------------------------------------------
RENDER_R = [1, 127, 128, 129, 1000]          # the block is 128 rays
RENDER_S = [1, 2, 27, 64]
KF_DIST_TH = 0.1


def render_case(R, S):
    """(z_vals, sdf, depth_sample) float32 of R rays with S shuffled samples; ray r is of kind r % 8:
      0 plain            1 two samples share the smallest z that has a negative sdf, with different sdf values (stable order)
      2 no negative sdf  3 only the farthest sample is negative (first crossing = last sorted sample: depth 0)
      4 sdf = -0.0 at the nearest sample, nothing negative before it        5 NaN sdf entries (one of them at the nearest sample)
      6 depth_sample = 0                      7 every z of the ray equal"""
    rng = np.random.RandomState(100 * R + S)
    z = rng.uniform(0.1, 4.0, (R, S)).astype(np.float32)          # already in random order along the ray
    sdf = (0.4 * rng.standard_normal((R, S))).astype(np.float32)
    ds = rng.uniform(0.5, 3.5, R).astype(np.float32)
    for r in range(R):
        kind = r % 8
        if kind == 1 and S >= 2:
            a, b = rng.choice(S, 2, replace=False)
            z[r, b] = z[r, a]
            sdf[r] = np.where(z[r] < z[r, a], np.abs(sdf[r]) + np.float32(0.01), sdf[r])
            sdf[r, a], sdf[r, b] = -0.125, -0.375
        elif kind == 2:
            sdf[r] = np.abs(sdf[r]) + np.float32(0.01)
        elif kind == 3:
            sdf[r] = np.abs(sdf[r]) + np.float32(0.01)
            sdf[r, z[r].argmax()] = -0.25
        elif kind == 4:
            sdf[r, z[r].argmin()] = -0.0
        elif kind == 5:
            sdf[r, rng.randint(S)] = np.nan
            if r % 16 == 5:
                sdf[r] = np.abs(sdf[r]) + np.float32(0.01)
                sdf[r, z[r].argmin()] = np.nan
        elif kind == 6:
            ds[r] = 0.0
        elif kind == 7:
            z[r] = z[r, 0]
    # three rays in four get a depth sample within 25 % of what the ray renders to, so that both sides of the threshold are populated
    with np.errstate(invalid="ignore", divide="ignore"):
        view = orc.keyframe_ratio(z, sdf, np.ones(R, np.float32), 1.0)[1]
    near = (rng.uniform(size=R) < 0.75) & np.isfinite(view) & (view > 0) & (np.arange(R) % 8 != 6)
    ds = np.where(near, view * rng.uniform(0.75, 1.25, R), ds).astype(np.float32)
    return z, sdf, ds


def render_reference(z, sdf, ds, th=KF_DIST_TH):
    """(view_depth float32 [R], below count int) from `oracle.isdf_oracle.keyframe_ratio`"""
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio, view = orc.keyframe_ratio(z, sdf, ds, th)
    count = int(round(ratio * z.shape[0]))
    assert count / z.shape[0] == ratio
    return view, count


def render_margin(view, ds, th=KF_DIST_TH):
    """smallest distance, in float32 ulps of the threshold, between the float64 |d - ds| / ds and the threshold over the rays with
    a finite positive depth sample and a finite view depth (a NaN or an infinite ratio is on neither side's edge)"""
    v, d = view.astype(np.float64), ds.astype(np.float64)
    ok = np.isfinite(v) & np.isfinite(d) & (d > 0)
    if not ok.any():
        return np.inf
    ratio = np.abs(v[ok] - d[ok]) / d[ok]
    th32 = np.float32(th)
    return float(np.abs(ratio - float(th32)).min() / float(np.spacing(th32)))
