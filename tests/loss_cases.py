"""Hand-made batches for the loss stage (tests/test_loss_stage_{cpu,gpu}.py): every operand exact, every ray in ONE class of the
case table, no sampler.  numpy only.

How a point gets its class bit for bit (bounds_method "ray"):
  bnd = |dirs_C| (depth - z) with dirs_C in DIRS (norms 1, 2, 5, exact under any contraction) and depth, z on a 2^-6 grid, or
        depth = the fp32 neighbour of a threshold and z = 0 -- the difference and the product are fp32 values
  sd  = the step's `noise`, through a net whose head is zero (out_alpha = 0, scale_output = 1): sdf = noise, d sdf / dx = 0
Thresholds: trunc_distance = 0.25, eik_apply_dist = 0.125 (fp32 values).  LC_A's weights are dyadic (trunc 5.5, eikonal 0.25, normal
2^-6) and sd - bnd sits on a 2^-4 grid, so every term, every total and every partial sum of at most a few hundred points is an fp32
value: the kernel must give them EXACTLY, in whatever order it adds.  LC_B keeps the shipped weights of the terms.

Classes (gn = 0 everywhere: gl = 1, ek = eik_weight where bnd >= eik_apply_dist, tot = sl + grad_weight + ek; v = sd - bnd,
w = trunc_weight, e = exp(-5 sd)):
  class             region       construction                                  sl  L1 | L2            sbar  L1 | L2
  trunc_lt          truncation   0 < bnd <= 0.25, sd < bnd                     w |v| | w v^2          -w | 2 w v
  trunc_gt          truncation   0 < bnd <= 0.25, sd > bnd                     w |v| | w v^2          +w | 2 w v
  trunc_eq          truncation   sd == bnd                                     0                      0
  trunc_at_border   truncation   bnd == 0.25 (`>` is strict), sd != bnd        w |v| | w v^2          w sign v | 2 w v
  free_next_above   free space   bnd = nextafter(0.25, +inf), 0 <= sd <= 0.25  0                      0
  trunc_behind      truncation   bnd < 0 (z > depth), sd != bnd                w |v| | w v^2          w sign v | 2 w v
  free_gt           free space   bnd > 0.25, sd > bnd   (dv = 1)               v | v^2                1 | 2 v
  free_v0           free space   bnd > 0.25, 0 <= sd <= bnd (0 and bnd incl.)  0                      0
  free_exp          free space   bnd > 0.25, sd < 0                            e - 1 | (e - 1)^2      -5 e | -10 e (e - 1)
  free_zero         free space   bnd > 0.25, sd = -0.0 and +0.0                0                      0
(the head adds the noise to +0.0, so -0.0 reaches the loss stage as +0.0: dbg["sdf"] == noise holds numerically, and both give v = 0.)
"""
import numpy as np

DIRS = np.array([[0, 0, 1], [0, 0, 2], [3, 4, 0]], np.float32)
NORMS = (1, 2, 5)
TRUNC, EIK = 0.25, 0.125
LC_A = dict(trunc_weight=5.5, trunc_distance=TRUNC, eik_weight=0.25, eik_apply_dist=EIK, grad_weight=2.0 ** -6)
LC_B = dict(trunc_distance=TRUNC, eik_apply_dist=EIK)
CAM = dict(H=48, W=64, fx=60.0, fy=60.0, cx=31.5, cy=23.5)
N_FRAMES = 2
DEPTH0 = 2.0

CLASSES_A = ("trunc_lt", "trunc_gt", "trunc_eq", "trunc_at_border", "free_next_above", "trunc_behind", "free_gt", "free_v0",
             "free_exp", "free_zero")
LABELS = {"trunc_lt": {"trunc:sd<bnd"}, "trunc_gt": {"trunc:sd>bnd"}, "trunc_eq": {"trunc:sd=bnd"},
          "trunc_at_border": {"trunc:sd<bnd", "trunc:sd>bnd"}, "free_next_above": {"free:v=0"},
          "trunc_behind": {"trunc:sd<bnd", "trunc:sd>bnd"}, "free_gt": {"free:sd>bnd"}, "free_v0": {"free:v=0"},
          "free_exp": {"free:exp"}, "free_zero": {"free:v=0"},
          "eik_at_border": {"trunc:sd=bnd"}, "eik_below_border": {"trunc:sd=bnd"}}
EXACT = set(CLASSES_A) - {"free_exp"}          # classes whose every value is an fp32 value


def _ray(cls, S, rng):
    """-> (index into DIRS, depth, z [S], sd [S]) of one ray of class `cls`"""
    di = int(rng.integers(0, 3))
    nrm = NORMS[di]
    j = rng.integers(1, 9, S) / 16.0
    sgn = rng.choice([-1.0, 1.0], S)
    free_q = lambda: rng.integers(16 // nrm + 1, 128 // nrm + 1, S) / 64.0           # bnd in (0.25, 2]
    depth = DEPTH0
    if cls in ("trunc_lt", "trunc_gt", "trunc_eq"):
        q = rng.integers(1, 16 // nrm + 1, S) / 64.0
        sd = nrm * q + {"trunc_lt": -j, "trunc_gt": j, "trunc_eq": 0 * j}[cls]
    elif cls == "trunc_at_border":
        di = int(rng.integers(0, 2)); nrm = NORMS[di]
        q = np.full(S, TRUNC / nrm)
        sd = TRUNC + sgn * j
    elif cls == "free_next_above":
        di, nrm = 0, 1
        depth = float(np.nextafter(np.float32(TRUNC), np.float32(np.inf)))
        q = np.full(S, depth)
        sd = rng.integers(0, 5, S) / 16.0
    elif cls == "trunc_behind":
        q = -rng.integers(1, 65, S) / 64.0
        sd = nrm * q + sgn * j
    elif cls == "free_gt":
        q = free_q()
        sd = nrm * q + j
    elif cls == "free_v0":
        q = free_q()
        bnd = nrm * q
        sd = np.floor(bnd * 16 * rng.uniform(size=S)) / 16.0
        pick = rng.integers(0, 3, S)
        sd = np.where(pick == 0, 0.0, np.where(pick == 1, bnd, sd))
    elif cls == "free_exp":
        q = free_q()
        sd = -rng.integers(1, 17, S) / 16.0
    elif cls == "free_zero":
        q = free_q()
        sd = np.where(np.arange(S) % 2 == 0, -0.0, 0.0)
        if S == 1 and rng.integers(0, 2):
            sd = np.array([0.0])
    elif cls in ("eik_at_border", "eik_below_border"):
        if cls == "eik_at_border":
            di = int(rng.integers(0, 2)); nrm = NORMS[di]
            q = np.full(S, EIK / nrm)
        else:
            di, nrm = 0, 1
            depth = float(np.nextafter(np.float32(EIK), np.float32(0)))
            q = np.full(S, depth)
        sd = nrm * q                                       # v = 0: tot = grad_weight + ek, two fp32 values added once
    else:
        raise KeyError(cls)
    z = np.zeros(S) if depth != DEPTH0 else depth - q
    return di, depth, z, sd


def make_batch(classes, S, seed):
    """one ray per entry of `classes` -> the batch dict tests/gpu_step_util.smp takes, plus cls (per ray) and noise = the wanted sdf"""
    rng = np.random.default_rng(seed)
    R = len(classes)
    di, depth, z, sd = zip(*[_ray(c, S, rng) for c in classes])
    unit = lambda a: (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(np.float32)
    b = dict(pc=rng.uniform(-1, 1, (R, S, 3)).astype(np.float32), z_vals=np.array(z, np.float32), depth_sample=np.array(depth, np.float32),
             dirs_C_sample=DIRS[list(di)], dirs_W_sample=rng.standard_normal((R, 3)).astype(np.float32),
             norm_sample=unit(rng.standard_normal((R, 3))), indices_b=(np.arange(R) % N_FRAMES).astype(np.int64),
             indices_h=rng.integers(0, CAM["H"], R).astype(np.int64), indices_w=rng.integers(0, CAM["W"], R).astype(np.int64),
             noise=np.array(sd, np.float32), n_frames=N_FRAMES, cls=np.array(classes))
    assert np.array_equal(b["z_vals"].astype(np.float64), np.array(z)) and np.array_equal(b["noise"].astype(np.float64), np.array(sd))
    return b


def mixed_batch(R, S, seed):
    """every class of the table, interleaved ray by ray"""
    return make_batch([CLASSES_A[r % len(CLASSES_A)] for r in range(R)], S, seed)


# P = 1, TILE_PTS - 1, TILE_PTS, TILE_PTS + 1, 2 TILE_PTS + 1 (TILE_PTS = 64, checked against isdf_common.h by the CPU test)
SHAPES = ((1, 1), (21, 3), (64, 1), (65, 1), (43, 3))


def pc_nan_batch(seed):
    """bounds_method "pc": 6 rays x 3 samples on a 2^-3 grid; sample 1 of ray 0 sits exactly on ray 1's surface point and sample 2
    of ray 3 on ray 5's: distance 0, target 0 / 0 = NaN, the loss stage takes the normal there"""
    rng = np.random.default_rng(seed)
    b = make_batch(["trunc_eq"] * 6, 3, seed)
    pc = rng.integers(-8, 9, (6, 3, 3)) / 8.0
    pc[:, 0] = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1]]
    pc[0, 1], pc[3, 2] = pc[1, 0], pc[5, 0]
    b["pc"] = pc.astype(np.float32)
    b["z_vals"] = np.tile(np.array([1.0, 0.5, 1.5], np.float32), (6, 1))      # sample 2 is behind the surface
    b["depth_sample"] = np.ones(6, np.float32)
    b["noise"] = (rng.integers(-8, 9, (6, 3)) / 16.0).astype(np.float32)
    return b


def pad_dead(b, extra):
    """the batch in max_rays = R + extra ray slots: every float input of the dead slots is NaN (noise too), n_valid = R"""
    R = b["z_vals"].shape[0]
    out = dict(b, n_valid=R)
    for k, v in b.items():
        if isinstance(v, np.ndarray) and k != "cls":
            fill = np.nan if v.dtype.kind == "f" else 0
            out[k] = np.concatenate((v, np.full((extra,) + v.shape[1:], fill, v.dtype)))
    return out


def closed_form(cls, loss_type, bnd, sd, lc):
    """(sl, sbar, ek) per point as the table states them, float64, kernel scale; bnd, sd: float64 of the fp32 operands"""
    w, l1 = lc.trunc_weight, loss_type == "L1"
    v = sd - bnd
    zero = np.zeros_like(v)
    if cls.startswith("trunc") or cls.startswith("eik"):
        sl, sb = (w * np.abs(v), w * np.sign(v)) if l1 else (w * v * v, 2 * w * v)
    elif cls == "free_gt":
        sl, sb = (v, np.ones_like(v)) if l1 else (v * v, 2 * v)
    elif cls == "free_exp":
        e = np.exp(-5.0 * sd)
        sl, sb = (e - 1, -5 * e) if l1 else ((e - 1) ** 2, -10 * e * (e - 1))
    else:
        sl, sb = zero, zero
    ek = np.where(bnd >= lc.eik_apply_dist, lc.eik_weight, 0.0)
    return sl, sb, ek


# ---- the committed fixtures, in the same batch form ---------------------------------------------------------------------------------
CONFIGS = {"ray_L1": dict(bounds_method="ray", loss_type="L1"), "ray_L2": dict(bounds_method="ray", loss_type="L2"),
           "pc_L1": dict(bounds_method="pc", loss_type="L1"), "pc_L2": dict(bounds_method="pc", loss_type="L2"),
           "ray_L1_orien": dict(bounds_method="ray", loss_type="L1", orien_loss=True)}
FIXTURES = ("eval_full_ray", "trained_default")


def fixture_batch(name):
    """(fixture dict, batch dict) of eval_full_ray (random initialisation) or of the trained fixture's eval batch"""
    import oracle.isdf_oracle as orc
    from tests import golden_util as gu
    g = gu.load(name)
    if name.startswith("trained"):
        src = gu.trained_batch(g, "eval/")
        noise, F = src["noise"], int(g["n_frames"][0])
    else:
        src = {k: g[k] for k in ("pc", "z_vals", "depth_sample", "dirs_C_sample", "T_WC_sample", "norm_sample", "indices_b",
                                 "indices_h", "indices_w")}
        noise, F = g["draw_noise"] * np.float32(g["noise_std"][0]), int(g["indices_b"].max()) + 1
    R, S = src["z_vals"].shape
    T, dC = src["T_WC_sample"].astype(np.float32), src["dirs_C_sample"].astype(np.float32)
    b = dict(pc=src["pc"], z_vals=src["z_vals"], depth_sample=src["depth_sample"], dirs_C_sample=dC, T_WC_sample=T,
             dirs_W_sample=orc.origin_dirs_W(T, dC)[1].astype(np.float32), norm_sample=src["norm_sample"],
             indices_b=src["indices_b"].astype(np.int64), indices_h=src["indices_h"].astype(np.int64),
             indices_w=src["indices_w"].astype(np.int64), noise=noise.reshape(R, S).astype(np.float32), n_frames=F)
    return g, {k: (np.ascontiguousarray(v.astype(np.float32) if v.dtype.kind == "f" else v) if isinstance(v, np.ndarray) else v)
               for k, v in b.items()}


def loss_cfg(base, **over):
    """a copy of the LossCfg `base` with fields replaced"""
    import oracle.isdf_oracle as orc
    kw = {k: getattr(base, k) for k in ("bounds_method", "loss_type", "trunc_weight", "trunc_distance", "eik_weight",
                                        "eik_apply_dist", "grad_weight", "orien_loss")}
    kw.update(over)
    return orc.LossCfg(**kw)
