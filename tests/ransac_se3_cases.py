"""Seeded RansacSE3 inputs (test infrastructure), one per edge regime of csrc/ransac.hip and of the host control in
csrc/solver.cpp: match counts at the mask-word (32), chunk / fit-block (64) and capacity (2304) boundaries, the host's
second chunk of hypotheses and the workspace's growth, zero-weight points in a sample (the ballot compaction),
covariances of rank 0, 1 and 2 and the reflection branch of the fit, the identity fallback taken and refused, every
loop parameter away from Tracking's defaults, and odd but legal inputs.  case(name) returns (xyz1, xyz2, matches,
params, seed, sticky, update_f2): params are the arguments of ransac_params, sticky is the preset covariance or None,
update_f2 is 1 (flags passed and updated), 0 (flags passed, update off) or None (no flags).
tests/test_ransac_se3_cases.py asserts from the oracle alone that each case reaches its regime;
tests/test_gpu_ransac_edges.py runs them on the device."""
import ctypes as C

import numpy as np

from pnp_cases import rot

F = np.float32
DEFAULTS = (200, 10, 3.0, 4)   # iterations, min_inlier_th, max_mahalanobis, sample_size (System/Tracking.cpp)

SIZES = [31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 2303, 2304]
NOISY_SIZES = [64, 65, 129, 2304]
ITERATIONS = [-1, 0, 1, 23, 24, 25, 300, 1000]
SAMPLE_SIZES = [0, 1, 2, 3, 8]
STICKY_PRESETS = {"sticky_0": 0.0, "sticky_1e-12": 1e-12, "sticky_1e6": 1e6}
ZW_M = 200          # zero-weight cases: matches 1..40 get a NaN source z, 41..70 a +inf target z, 71..100 a +inf
ZW_ITERS = 6        # source z; iterations, few enough for a seed whose every consumed sample holds one of them
# searched on the oracle over seeds 1..400, first hit: ok, and every one of the ZW_ITERS consumed samples holds a
# zero-weight id (so the winning hypothesis's does)
ZW_SEEDS = {"zw_ss4": 1, "zw_ss8": 1}
# searched over seeds 1..400, first hit: the first consumed sample of four keeps exactly 2 / exactly 1 valid points
ZW_KEEP_SEEDS = {"zw_keep2": 1, "zw_keep1": 2}
IDENT_M, IDENT_STATIC = 150, 60
CONTAM_SEEDS = {"contam_2304": 1, "contam_257": 1}   # searched from 1 up: ok after more than 24 hypotheses
NEG_Z_SEED = 9      # searched from 1 up: ok, and the first of several consumed samples holds a source with negated z
ITERS_SEED = 39     # searched from 1 up: hypothesis 24, the first of the host's second chunk, is the first accepted

NAMES = (["size_%d" % m for m in SIZES] + ["size_%d_noisy" % m for m in NOISY_SIZES] + ["contam_2304", "contam_257"] +
         list(ZW_SEEDS) + list(ZW_KEEP_SEEDS) +
         ["all_identical", "exact_line", "exact_plane", "mirror_slab", "mirror_full"] +
         ["ident_it1", "ident_it3", "ident_refused"] + ["iters_%d" % i for i in ITERATIONS] +
         ["ss_%d" % s for s in SAMPLE_SIZES] + ["m_lt_ss", "maxd_0.5", "maxd_10", "minth_3", "minth_M"] +
         ["target_z0", "neg_z", "src_z0_all", "first20_invalid"] + list(STICKY_PRESETS) +
         ["dup_matches", "many_to_one", "equal_dist", "f2_off", "flags_none"])


def dmatch_dtype():
    import oracle_lib
    return oracle_lib.DMATCH_DTYPE


def motion():
    """About 0.03 rad and 3 cm."""
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot(np.array([0.012, -0.022, 0.016])), [0.018, -0.012, 0.02]
    return T


def frustum(n, rs):
    z = rs.uniform(0.6, 4.0, n)
    return np.c_[rs.uniform(-0.5, 0.5, n) * z, rs.uniform(-0.4, 0.4, n) * z, z].astype(F)


def moved(P, rs=None):
    """The target of P: the moved source rounded to f32; with rs, depth-quadratic noise of 0.002 z^2 on top."""
    T = motion()
    Q = P.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    if rs is not None:
        Q += rs.normal(size=Q.shape) * (0.002 * Q[:, 2:3] ** 2) * np.array([0.3, 0.3, 1.0])
    return Q.astype(F)


def matched(P, Q, rs, distance=None, anchor=False):
    """xyz1 = P, xyz2 = Q shuffled, match i = (i, where Q[i] went), distinct distances in shuffled order.  anchor: the
    smallest distance goes to the source nearest 1.2 m, whose depth then sets the sticky covariance (1.44 cm in
    depth: the noisy flavour's targets beyond about 3.5 m start to fall outside three of them)."""
    n = len(P)
    perm = rs.permutation(n)
    xyz2 = np.zeros_like(Q)
    xyz2[perm] = Q
    m = np.zeros(n, dmatch_dtype())
    m["queryIdx"], m["trainIdx"] = np.arange(n), perm
    d = rs.permutation(n).astype(F) if distance is None else distance
    if anchor:
        a, z = int(np.argmin(np.abs(P[:, 2] - 1.2))), int(np.argmin(d))
        d[[a, z]] = d[[z, a]]
    m["distance"] = d
    return np.ascontiguousarray(P, F), xyz2, m


def contaminate(Q, frac, rs):
    """frac of the targets permuted among themselves."""
    Q = Q.copy()
    k = rs.choice(len(Q), int(frac * len(Q)), replace=False)
    Q[k] = Q[np.roll(k, 1)]
    return Q


def odd_ids(name):
    """The matches (= sources) that target_z0 / neg_z alter."""
    return np.random.default_rng(len(name)).choice(120, 30 if name == "target_z0" else 10, replace=False)


def sorted_order(matches):
    import oracle_lib
    return oracle_lib.sort_dmatch(matches["distance"])


def zero_weight_ids(matches):
    """The zero-weight cases' bad matches as positions of the sorted order (what the sampler draws)."""
    order = sorted_order(matches)
    return np.nonzero(np.isin(order, zw_bad_matches()))[0]


def zw_bad_matches():
    return np.arange(1, 101)   # match 0 carries distance 0 and stays clean: it sets the sticky covariance


def _zero_weight(rs):
    P = frustum(ZW_M, rs)
    Q = moved(P)
    P[1:41, 2] = np.nan
    Q[41:71, 2] = np.inf
    P[71:101, 2] = np.inf
    d = np.r_[0, 1 + rs.permutation(ZW_M - 1)].astype(F)
    return matched(P, Q, rs, d)


def identity_static(rs):
    return np.sort(rs.choice(IDENT_M, IDENT_STATIC, replace=False))


def _identity(rs):
    P = frustum(IDENT_M, rs)
    d = rs.normal(size=P.shape)
    Q = (P + 0.5 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    st = identity_static(np.random.default_rng(77))
    Q[st] = P[st]
    return matched(P, Q, rs)


def case(name):
    prm = list(DEFAULTS)
    seed, sticky, update_f2 = 5, None, 1
    rs = np.random.default_rng(2000 + NAMES.index(name))
    rs120 = np.random.default_rng(2120)   # the 120-point clouds of the parameter and odd-input cases
    if name.startswith("size_"):
        M = int(name.split("_")[1])
        P = frustum(M, rs)
        noisy = name.endswith("_noisy")
        out = matched(P, moved(P, rs if noisy else None), rs, anchor=noisy)
    elif name.startswith("contam_"):
        P = frustum(int(name.split("_")[1]), rs)
        out = matched(P, contaminate(moved(P, rs), 0.7, rs), rs, anchor=True)
        seed = CONTAM_SEEDS[name]
    elif name in ZW_SEEDS:
        out = _zero_weight(np.random.default_rng(2300))
        prm[0], prm[3], seed = ZW_ITERS, int(name[len("zw_ss"):]), ZW_SEEDS[name]
    elif name in ZW_KEEP_SEEDS:
        out = _zero_weight(np.random.default_rng(2300))
        prm[0], seed = 3, ZW_KEEP_SEEDS[name]
    elif name == "all_identical":
        P = np.tile(np.array([0.3, -0.2, 2.0], F), (50, 1))
        out = matched(P, (P + np.array([0.015625, 0, 0], F)).astype(F), rs)
    elif name == "exact_line":
        P = np.c_[rs.uniform(-1, 1, 100), np.full(100, 0.25), np.full(100, 2.0)].astype(F)
        out = matched(P, (P + np.array([0.004, -0.003, 0.002], F)).astype(F), rs)
    elif name == "exact_plane":
        P = np.c_[rs.uniform(-1, 1, 200), rs.uniform(-0.8, 0.8, 200), np.full(200, 2.0)].astype(F)
        out = matched(P, (P + np.array([0, 0, 0.01], F)).astype(F), rs)
    elif name == "mirror_slab":
        P = frustum(200, rs)
        P[:, 0] = rs.uniform(-0.004, 0.004, 200).astype(F)
        out = matched(P, P * np.array([-1, 1, 1], F), rs)
    elif name == "mirror_full":
        P = frustum(120, rs)
        out = matched(P, P * np.array([-1, 1, 1], F), rs)
        prm[1] = 4
    elif name in ("ident_it1", "ident_it3", "ident_refused"):
        out = _identity(np.random.default_rng(2400))
        prm[0], prm[1] = (3 if name == "ident_it3" else 1), (IDENT_STATIC if name == "ident_refused" else 20)
    elif name.startswith("iters_"):
        prm[0] = int(name[len("iters_"):])
        P = frustum(120, rs120)
        Q = moved(P, rs120)
        # from 23 on the loop must not end early: 55 % of the targets permuted, so no model reaches M / 2
        out = matched(P, contaminate(Q, 0.55, rs120) if prm[0] >= 23 else Q, rs120, anchor=True)
        seed = ITERS_SEED if prm[0] >= 23 else seed
    elif name in ("maxd_0.5", "maxd_10", "minth_3", "minth_M", "f2_off", "flags_none") or name.startswith("ss_"):
        P = frustum(120, rs120)
        out = matched(P, moved(P, rs120), rs120, anchor=True)
        if name.startswith("ss_"):
            prm[3] = int(name[3:])
        elif name.startswith("maxd_"):
            prm[2] = float(name[5:])
        elif name.startswith("minth_"):
            prm[1] = 3 if name == "minth_3" else 120
        update_f2 = {"f2_off": 0, "flags_none": None}.get(name, 1)
    elif name == "m_lt_ss":
        P = frustum(5, rs)
        out = matched(P, moved(P), rs)
        prm[1], prm[3] = 3, 8
    elif name in STICKY_PRESETS:
        P = frustum(120, rs120)
        out = matched(P, moved(P), rs120)
        sticky = STICKY_PRESETS[name]
    else:
        P = frustum(120, rs120)
        Q = moved(P)
        if name == "target_z0":
            Q[odd_ids(name), 2] = 0
        elif name == "neg_z":
            P[odd_ids(name), 2] *= -1
            seed = NEG_Z_SEED
        elif name == "src_z0_all":
            P[:, 2] = 0
        if name == "many_to_one":
            # ORB's multi-level duplicates: twelve sources within a millimetre of each of ten points, one target each
            P = (P[np.arange(120) % 10] + rs.uniform(-5e-4, 5e-4, size=(120, 3)) * (np.arange(120) >= 10)[:, None]).astype(F)
            xyz1, xyz2, m = matched(P, moved(P), rs)
            m["trainIdx"] = m["trainIdx"][np.arange(120) % 10]
            out = xyz1, xyz2, m
        elif name == "equal_dist":
            out = matched(P, Q, rs, np.full(120, 30, F))
        elif name == "first20_invalid":
            xyz1, xyz2, m = matched(P, Q, rs)
            first = sorted_order(m)[:20]
            xyz1[m["queryIdx"][first[:7]], 2] = 0          # skipped before the covariance is touched
            xyz2[m["trainIdx"][first[7:14]], 0] = 0
            xyz1[m["queryIdx"][first[14:]], 2] = np.nan    # evaluated, but not touching
            out = xyz1, xyz2, m
        elif name == "dup_matches":
            xyz1, xyz2, m = matched(P, Q, rs)
            out = xyz1, xyz2, np.repeat(m, 2)
        elif name in ("target_z0", "neg_z", "src_z0_all"):
            out = matched(P, Q, rs)
        else:
            raise KeyError(name)
    xyz1, xyz2, m = out
    return xyz1, np.ascontiguousarray(xyz2, F), np.ascontiguousarray(m), tuple(prm), seed, sticky, update_f2


# ------------------------------------------------------------------ RansacSE3::sampleMatches, restated
def _random_int():
    import oracle_lib
    L = oracle_lib.lib()
    L.orc_random_int.restype = C.c_int
    L.orc_random_int.argtypes = [C.POINTER(oracle_lib.Rng), C.c_int, C.c_int]
    return L.orc_random_int


def rng_key(r):
    return tuple(r.state), r.f, r.r


def draw_sample(random_int, rng, M, SS):
    """One sampleMatches call with a set over Random::randomInt: (sorted ids, rand() calls made)."""
    ids, safety, calls = set(), 0, 0
    while len(ids) < SS and M >= SS:
        a, b = random_int(C.byref(rng), 0, M - 1), random_int(C.byref(rng), 0, M - 1)
        calls += 2
        ids.add(min(a, b))
        safety += 1
        if safety > 10000:
            break
    return sorted(ids), calls


def sample_model(oracle, seed, M, SS, nh):
    """RansacSE3::sampleMatches with a set, Random::randomInt from the oracle: (ids, rand() calls so far) per hypothesis"""
    random_int = _random_int()
    rng, calls, out = oracle.rng(seed), 0, []
    for _ in range(nh):
        ids, c = draw_sample(random_int, rng, M, SS)
        calls += c
        out.append((ids, calls))
    return out


def hypotheses_consumed(seed, M, SS, rng_after, limit=2000):
    """The samples (sorted ids, as positions of the sorted matches) of the loop iterations a call ran: drawn until
    the restated RNG state equals the oracle's state after the call.  A call that drew nothing (no iteration, SS = 0
    or M < SS) leaves the state where it was: []."""
    import oracle_lib
    random_int = _random_int()
    rng, want, out = oracle_lib.rng(seed), rng_key(rng_after), []
    while rng_key(rng) != want:
        assert len(out) < limit, "the oracle's RNG state is not on the sampler's path"
        out.append(draw_sample(random_int, rng, M, SS)[0])
    return out
