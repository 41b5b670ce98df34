"""Seeded PnPRansac inputs (test infrastructure), one per edge regime of csrc/pnp.hip and of the host control in
csrc/pnp_host.cpp: point counts on the strides of the inlier count (12 lanes, four points in flight: 12, 36, 48, 60),
of the mask / compaction passes (64-lane ballots, 256-thread passes, the 4096-entry inlier list) and of the wave of
five hypotheses; inliers placed across those waves and passes; RANSAC iteration counts and best iterations on every
hand-over between the first device chunk, the second device chunk and the host's doubling chunks, for the three
chunk schedules (K0, K1) = (8, 16), (4, 4), (64, 64); degenerate and non-finite input; every operator argument away
from its default.  case(name) returns (p3, p2, prm): prm holds the arguments of pnp_params (and of the oracle).
expected(oracle, p3, p2, prm) is the oracle's answer under PnPRansac::compute's min_matches rule.
tests/test_pnp_edge_cases.py asserts from the oracle alone that each case reaches its regime;
tests/test_gpu_pnp_edges.py runs them on the device."""
import numpy as np

from pnp_cases import K_TUM, problem

F = np.float32
DEFAULTS = dict(iters=500, reproj=3.0, conf=0.85, min_matches=0)

SIZES = [5, 6, 7, 11, 12, 13, 36, 37, 48, 49, 60, 61, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4095, 4096]

# The chunk schedules (K0, K1) a context can be steered into by preceding solves, and the RANSAC iteration counts
# at which a problem's loop ends on the last iteration of a chunk or on the first of the next: the two device
# chunks, then the host's chunks of 2 K1, 4 K1, ...
SCHEDULES = {(8, 16): [8, 9, 24, 25, 56, 57, 120, 121, 248, 249],
             (4, 4): [4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257],
             (64, 64): [64, 65, 128, 129, 256, 257]}

# Searched on the oracle over problem(n, seed, outliers = o) with (n, o) in (24, 0.2), (40, 0.45), (48, 0.6),
# (64, 0.7), (60, 0.75), (80, 0.78) and seeds 0..1499, first hit in that order.
# ITER_TABLE[k] = (n, seed, o): the oracle ends ok after exactly k iterations.
ITER_TABLE = {4: (24, 1, 0.2), 5: (24, 2, 0.2), 8: (24, 53, 0.2), 9: (24, 0, 0.2), 16: (24, 295, 0.2),
              17: (24, 312, 0.2), 24: (24, 219, 0.2), 25: (24, 296, 0.2), 32: (24, 382, 0.2), 33: (40, 782, 0.45),
              56: (24, 151, 0.2), 57: (40, 164, 0.45), 64: (40, 496, 0.45), 65: (48, 719, 0.6), 120: (40, 386, 0.45),
              121: (40, 946, 0.45), 128: (40, 675, 0.45), 129: (40, 558, 0.45), 248: (48, 1115, 0.6),
              249: (40, 263, 0.45), 256: (48, 683, 0.6), 257: (40, 64, 0.45)}
# BEST_TABLE[b] = (n, seed, o, iterations): the best model is the b-th iteration's (b = the smallest iteration
# cap at which the oracle already returns the final mask and inlier count) and the loop runs on past it.
BEST_TABLE = {4: (24, 40, 0.2, 7), 5: (24, 61, 0.2, 7), 8: (24, 80, 0.2, 13), 9: (24, 11, 0.2, 10),
              16: (24, 1406, 0.2, 19), 17: (40, 16, 0.45, 136), 24: (24, 1353, 0.2, 27), 25: (40, 9, 0.45, 37),
              32: (40, 203, 0.45, 60), 33: (40, 32, 0.45, 255), 56: (40, 1096, 0.45, 102), 57: (40, 182, 0.45, 60),
              64: (40, 597, 0.45, 102), 65: (40, 200, 0.45, 78), 120: (40, 362, 0.45, 136), 121: (48, 409, 0.6, 194),
              128: (40, 768, 0.45, 184), 129: (40, 800, 0.45, 136), 248: (40, 56, 0.45, 360),
              249: (48, 608, 0.6, 255), 256: (48, 795, 0.6, 460), 257: (40, 545, 0.45, 500)}
FORCED_ITERS = [8, 24, 25]   # an all-outlier problem under these iteration caps runs exactly that many

PLACEMENTS = ["edges", "wave", "pass", "alt"]
PLACE_SIZES = [256, 600]
# the one-wave placements need a subset inside one wave: iteration 308 at 256 points, 5711 at 600 (subsets())
PLACE_ITERS = {"place_wave_256": 500, "place_wave_600": 6000}

DEGENERATE = ["collinear", "coplanar", "coplanar_jitter", "two_distinct", "every_twice", "behind", "behind_fit5",
              "zero_7th", "collinear_5", "coplanar_5", "all_outlier", "scale_1e4", "scale_1e-4"]
NF_N, NF_SEED = 40, 7
NF_IN = 5        # in the first subset drawn at 40 points: [5, 4, 20, 13, 31]
# searched on the oracle from 0 up: an index in no subset of the iterations the poisoned run makes
NF_OUT = {"nan_px_out": 1, "inf_px_out": 1, "nan_obj_out": 1}
NONFINITE = ["nan_px_in", "inf_px_in", "nan_obj_in"] + list(NF_OUT) + ["nan_px_5", "inf_5"]
PARAMS = ["reproj_0", "reproj_1e6", "conf_0", "conf_1", "iters_0", "iters_1", "iters_2", "iters_3000", "minm_count",
          "minm_count1"]

SIZE_NAMES = ["size_%d" % n for n in SIZES]
PLACE_NAMES = ["place_%s_%d" % (k, n) for k in PLACEMENTS for n in PLACE_SIZES]
ITER_NAMES = ["iters_eq_%d" % k for k in ITER_TABLE]
BEST_NAMES = ["best_eq_%d" % k for k in BEST_TABLE]
FORCED_NAMES = ["forced_%d" % k for k in FORCED_ITERS]
NAMES = SIZE_NAMES + PLACE_NAMES + ITER_NAMES + BEST_NAMES + FORCED_NAMES + DEGENERATE + NONFINITE + PARAMS


def schedule_names(schedule):
    """The boundary problems of one schedule: loop ends and best iterations on each of its hand-overs."""
    ks = SCHEDULES[schedule]
    return ["iters_eq_%d" % k for k in ks] + ["best_eq_%d" % k for k in ks]


# ------------------------------------------------------------------ cv::RNG((uint64)-1) and getSubset, restated
def subsets(count, k):
    """The first k 5-point subsets solvePnPRansac draws at `count` points (they depend on the count alone)."""
    state, out = (1 << 64) - 1, []
    for _ in range(k):
        cur = []
        while len(cur) < 5:
            state = (state & 0xffffffff) * 4164903690 + (state >> 32)
            v = (state & 0xffffffff) % count
            if v not in cur:
                cur.append(v)
        out.append(cur)
    return out


def project(P, R, t, K4=K_TUM):
    Xc = P.astype(np.float64) @ R.T + t
    return np.stack([K4[0] * Xc[:, 0] / Xc[:, 2] + K4[2], K4[1] * Xc[:, 1] / Xc[:, 2] + K4[3]], 1)


def placement_inliers(kind, n):
    """The hand-placed inlier indices of a placement case (every other pixel is moved by 60 px)."""
    if kind == "edges":   # the last / first lane of a wave and of a pass, plus the rest of one drawn subset
        fixed = {63, 64, 255, 256}
        sub = next(s for s in subsets(n, 500) if len(set(s) & fixed) == 1)
        return np.array(sorted({i for i in fixed if i < n} | set(sub)))
    if kind == "wave":    # one wave of a pass holds every inlier: the wave of the first subset that fits in one
        sub = next(s for s in subsets(n, PLACE_ITERS["place_wave_%d" % n]) if len({v // 64 for v in s}) == 1)
        w = sub[0] // 64
        return np.arange(64 * w, min(64 * w + 64, n))
    if kind == "pass":    # the first half (256: waves 0, 1; 600: all of pass 0) outliers, then a whole pass of inliers
        return np.arange(128, 256) if n == 256 else np.arange(256, 512)
    if kind == "alt":
        return np.arange(0, n, 2)
    raise KeyError(kind)


def _placed(kind, n):
    P, uv, *_ = problem(n, 700 + n, outliers=0.0, noise=0.0)
    out = np.ones(n, bool)
    out[placement_inliers(kind, n)] = False
    uv = uv.copy()
    ang = 2.4 * np.arange(n)   # 60 px each, no two neighbours the same way: the outliers share no pose
    uv[out] += (60 * np.stack([np.cos(ang), np.sin(ang)], 1)).astype(F)[out]
    return P, uv


def _pose(rs):
    from pnp_cases import rot
    return rot(rs.normal(size=3) * 0.15), rs.normal(size=3) * 0.15


def _all_outlier(n, rs):
    P = rs.uniform([-1.5, -1.2, 0.8], [1.5, 1.2, 4.5], size=(n, 3)).astype(F)
    return P, rs.uniform([0, 0], [640, 480], size=(n, 2)).astype(F)


def _degenerate(name, rs):
    R, t = _pose(rs)
    noise = lambda n: rs.normal(size=(n, 2)) * 0.5
    if name in ("collinear", "collinear_5"):
        n = 5 if name.endswith("_5") else 40
        s = rs.uniform(-1, 1, n)[:, None]
        # exactly collinear in f32 too: multiples of a direction of few mantissa bits from a dyadic origin
        P = (np.array([0.125, -0.25, 2.5], F) + np.round(s * 512).astype(F) / F(512) * np.array([1.0, 0.5, 0.75], F)).astype(F)
        return P, (project(P, R, t) + noise(n)).astype(F)
    if name in ("coplanar", "coplanar_5", "coplanar_jitter"):
        n = 5 if name.endswith("_5") else 40
        P = np.c_[rs.uniform(-1.5, 1.5, n), rs.uniform(-1.2, 1.2, n), np.full(n, 2.0)]
        if name == "coplanar_jitter":
            P[:, 2] += rs.uniform(-1e-4, 1e-4, n)
        P = P.astype(F)
        return P, (project(P, R, t) + noise(n)).astype(F)
    if name == "two_distinct":
        P = np.repeat(np.array([[0.3, -0.2, 2.0], [-0.6, 0.4, 3.0]], F), 20, 0)
        return P, project(P, R, t).astype(F)
    if name == "every_twice":
        P, uv, *_ = problem(20, 811, outliers=0.0)
        return np.repeat(P, 2, 0), np.repeat(uv, 2, 0)
    if name in ("behind", "behind_fit5"):   # without outliers one sample's model fits its own five points
        P, uv, *_ = problem(40, 812, outliers=0.3 if name == "behind" else 0.0)
        return P * np.array([1, 1, -1], F), uv
    if name == "zero_7th":
        P, uv, *_ = problem(70, 813, outliers=0.2)
        P = P.copy()
        P[::7] = 0
        return P, uv
    if name == "all_outlier":
        return _all_outlier(40, rs)
    if name.startswith("scale_"):
        P, uv, *_ = problem(60, 814, outliers=0.3)
        return (P * F(float(name[len("scale_"):]))).astype(F), uv
    raise KeyError(name)


def _nonfinite(name):
    if name in ("nan_px_5", "inf_5"):
        P, uv, *_ = problem(5, 820, outliers=0.0)
        P, uv = P.copy(), uv.copy()
        if name == "nan_px_5":
            uv[2, 0] = np.nan
        else:
            P[3, 1] = np.inf
        return P, uv
    P, uv, *_ = problem(NF_N, NF_SEED, outliers=0.3)
    P, uv = P.copy(), uv.copy()
    i = NF_IN if name.endswith("_in") else NF_OUT[name]
    if name.startswith("nan_px"):
        uv[i, 0] = np.nan
    elif name.startswith("inf_px"):
        uv[i, 1] = np.inf
    else:
        P[i, 2] = np.nan
    return P, uv


def case(name):
    prm = dict(DEFAULTS)
    rs = np.random.default_rng(3000 + NAMES.index(name))
    if name in SIZE_NAMES:
        n = int(name[len("size_"):])
        p3, p2, *_ = problem(n, 900 + n, outliers=0.3 if n > 12 else 0.0)
    elif name in PLACE_NAMES:
        _, kind, n = name.split("_")
        p3, p2 = _placed(kind, int(n))
        prm["iters"] = PLACE_ITERS.get(name, 500)
    elif name in ITER_NAMES:
        n, seed, o = ITER_TABLE[int(name[len("iters_eq_"):])]
        p3, p2, *_ = problem(n, seed, outliers=o)
    elif name in BEST_NAMES:
        n, seed, o, _ = BEST_TABLE[int(name[len("best_eq_"):])]
        p3, p2, *_ = problem(n, seed, outliers=o)
    elif name in FORCED_NAMES:
        p3, p2 = _all_outlier(40, np.random.default_rng(2999))
        prm["iters"] = int(name[len("forced_"):])
    elif name in DEGENERATE:
        p3, p2 = _degenerate(name, rs)
    elif name in NONFINITE:
        p3, p2 = _nonfinite(name)
    elif name == "iters_3000":
        p3, p2, *_ = problem(64, 3, outliers=0.85)
        prm["iters"] = 3000
    elif name in PARAMS:
        p3, p2, *_ = problem(60, 77, outliers=0.3)
        key, val = name.split("_")
        if key == "minm":
            prm["min_matches"] = 60 if val == "count" else 61
        else:
            prm[key] = float(val) if key != "iters" else int(val)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(p3, F), np.ascontiguousarray(p2, F), prm


def tiny(n):
    """The empty, 4-point and 5-point problems the schedule batches place between the boundary problems."""
    p3, p2, *_ = problem(12, 9, outliers=0.0)
    return p3[:n], p2[:n], dict(DEFAULTS)


# One batch for all three schedules: under each of them one problem ends in the second device chunk
# (K0 < iterations <= K0 + K1) and one in the host continuation (tests/test_pnp_edge_cases.py).
INDEPENDENCE = ["iters_eq_5", "iters_eq_8", "iters_eq_9", "iters_eq_17", "iters_eq_24", "iters_eq_25", "iters_eq_57",
                "iters_eq_65", "iters_eq_128", "iters_eq_129", "iters_eq_257", "best_eq_33"]
WAVE_TAIL = ["iters_eq_5", "iters_eq_9", "iters_eq_25", "iters_eq_57", "iters_eq_65", "iters_eq_129", "iters_eq_17"]
PRIME_SEEDS_4_4 = list(range(1000, 1010))   # problem(30, seed, outliers = 0): at most 3 iterations each


def prime(schedule):
    """The batch whose solve leaves a context in `schedule`, the way production gets there (none for the fresh
    context's (8, 16))."""
    if schedule == (8, 16):
        return []
    if schedule == (4, 4):
        return [problem(30, s, outliers=0.0)[:2] for s in PRIME_SEEDS_4_4]
    if schedule == (64, 64):
        return [_all_outlier(40, np.random.default_rng(2990 + i)) for i in range(4)]
    raise KeyError(schedule)


def adapted_chunks(iters):
    """pnp_host.cpp's adapt_chunk, restated: the schedule after a solve whose problems of five or more points ran
    `iters` iterations."""
    it = sorted(iters)
    pct = lambda q: it[min(len(it) - 1, len(it) * q // 100)]
    k0 = min(64, max(4, pct(90) + 1))
    return k0, min(64, max(4, (pct(99) + 2 - k0 + 3) & ~3))


def handovers(schedule, limit=500):
    """The iteration counts on which a chunk of `schedule` ends: K0, K0 + K1, then the host's 2 K1, 4 K1, ..."""
    k0, k1 = schedule
    out, at, chunk = [k0, k0 + k1], k0 + k1, 2 * k1
    while at + chunk < limit:
        at += chunk
        out.append(at)
        chunk *= 2
    return out


def expected(oracle, p3, p2, prm):
    """(ok, R, t, mask, n_inliers, iters) of the definition: the oracle's solvePnPRansac behind
    PnPRansac::compute's min_matches rule (fewer matches: no solve)."""
    if len(p3) < prm["min_matches"]:
        return False, np.eye(3), np.zeros(3), np.zeros(len(p3), bool), 0, 0
    return oracle.pnp_ransac(p3, p2, K_TUM, prm["iters"], prm["reproj"], prm["conf"])
