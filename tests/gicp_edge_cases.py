"""Seeded GICP inputs (test infrastructure), one per edge regime of csrc/gicp.hip: the rounds fallback of the
covariance k-NN in each of its eight instantiations, the cloud sizes at their boundaries, duplicate / coplanar /
collinear / identical neighbourhoods, exact distance ties in the 1-NN, the grid's full-scan branches and its
rim, correspondences at the max_corr boundary, the 4-correspondence abort at and after iteration 0, every
parameter away from Tracking's defaults.  case(name) returns (name, P, Q, guess, params); params holds the
rgbd_gicp_params fields.  tests/test_gicp_edge_cases.py asserts from the oracle and tests/gicp_path_model.py
alone that each case reaches its regime; tests/test_gpu_gicp_edges.py runs them on the device."""
import numpy as np

from gicp_cases import clouds
from pnp_cases import rot

F = np.float32
DEFAULTS = dict(max_iterations=10, k_correspondences=20, max_corr_dist=0.07, transformation_epsilon=1e-9,
                rotation_epsilon=2e-3, gicp_epsilon=1e-3, gn_iterations=4)   # Tracking's (System/Tracking.cpp:147-151)

ROUNDS_L = {4: 19, 8: 10, 12: 6, 16: 5, 20: 4, 24: 3, 28: 3, 32: 3}          # cluster lanes per NC (all < k = 20)
SIZE_NC = {63: 4, 64: 4, 65: 4, 256: 4, 257: 8, 512: 8, 513: 12, 2047: 32}   # cloud size -> NC
K_CASES = {"k1": (120, 1), "k2": (120, 2), "k3": (120, 3), "k5": (120, 5), "k32": (120, 32), "k32_M32": (32, 32),
           "k32_M31": (31, 32), "M1_k1": (1, 1)}                             # name -> (M, k_correspondences)
PARAM_CASES = {"mi1": dict(max_iterations=1, gn_iterations=4), "mi3_gn1": dict(max_iterations=3, gn_iterations=1),
               "mi50_gn8": dict(max_iterations=50, gn_iterations=8), "gn0": dict(max_iterations=10, gn_iterations=0),
               "loose_eps": dict(max_iterations=50, transformation_epsilon=1e-4, rotation_epsilon=1e-4)}
RIM_H = 1.01 * 0.07                                                          # the grid's cell at max_corr 0.07
LATE_ABORT_SEED = 138   # searched on the oracle: 5 correspondences at first, 3 left after four outer iterations

NAMES = (["rounds_nc%d" % nc for nc in ROUNDS_L] + ["total_64", "total_65"] + ["size_%d" % n for n in SIZE_NC] +
         ["dup_pairs", "dup_block25", "all_identical", "exact_plane", "exact_plane_moved", "exact_line", "lattice_half",
          "lattice_half_gridoff", "small_maxcorr", "query_far_mixed", "grid_rim", "grid_rim_out", "guess_far",
          "maxcorr_zero", "edge_ring", "four_eq", "four_below", "late_abort"] + list(K_CASES) + list(PARAM_CASES) +
         ["big_rot_guess"])


def make_params(mod, params):
    """params as the GicpParams of `mod` (the package or oracle_lib: the same leading fields)."""
    p = mod.gicp_params()
    for key, v in params.items():
        assert key in dict(p._fields_), key
        setattr(p, key, v)
    return p


def moved(P, T, noise, rs):
    return (P.astype(np.float64) @ T[:3, :3].T + T[:3, 3] + rs.normal(size=P.shape) * noise).astype(F)


def rounds_cluster(M, L):
    """The points a rounds_nc case moves into its cluster: those on the wave's first L lanes."""
    return np.nonzero(np.arange(M) % 64 < L)[0]


def _lattice(rs):
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(5), indexing="ij"), -1).reshape(-1, 3)
    P = (g / 16.0 + np.array([-0.25, -0.25, 1.5])).astype(F)   # every value exact in float
    Q = (P + np.array([1 / 32, 0, 0], F)).astype(F)
    return P[rs.permutation(len(P))], Q[rs.permutation(len(Q))]


def _four(last):
    """20 pairs 1 m apart along x except 0.01, 0.02, 0.03 and `last`; max_corr 0.0625 makes thr = 2^-8 exactly."""
    i = np.arange(20)
    P = np.stack([np.zeros(20), 0.5 * i, 2.0 + 0.25 * (i % 3)], 1).astype(F)
    Q = P.copy()
    Q[:, 0] = F(1.0)
    Q[[2, 7, 11], 0] = np.array([0.01, 0.02, 0.03], F)
    Q[16, 0] = last
    return P, Q


def late_abort(seed):
    rs = np.random.default_rng(seed)
    P = rs.uniform([-1, -1, 1.5], [1, 1, 3.0], size=(24, 3)).astype(F)
    Q = (P + np.array([1, 0, 0], F)).astype(F)
    near = rs.choice(24, 5, replace=False)
    d = rs.normal(size=(5, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    Q[near] = (P[near] + d * rs.uniform(0.05, 0.0699, size=(5, 1))).astype(F)
    return P, Q


def case(name):
    prm = dict(DEFAULTS)
    guess = np.eye(4, dtype=F)
    seed = 1000 + NAMES.index(name)
    rs = np.random.default_rng(seed)
    if name.startswith("rounds_nc"):
        nc = int(name[len("rounds_nc"):])
        M = 64 * nc - 5
        P, Q, T = clouds(M, 100 + nc)
        idx = rounds_cluster(M, ROUNDS_L[nc])
        P[idx] = (np.array([0.1, -0.2, 2.0]) + rs.normal(size=(len(idx), 3)) * 0.002).astype(F)
        Q[idx] = moved(P[idx], T, 0.001, rs)
    elif name in ("total_64", "total_65"):
        # a cluster of c points on 19 lanes leaves its points c + 1 candidates (k = 20: one far lane minimum):
        # 64 is the threshold path's last size (every lane of the sort used), 65 the rounds path's first
        c = int(name[len("total_"):]) - 1
        P, Q, T = clouds(251, 104)
        idx = rounds_cluster(251, 19)[:c]
        P[idx] = (np.array([0.1, -0.2, 2.0]) + rs.normal(size=(c, 3)) * 0.002).astype(F)
        Q[idx] = moved(P[idx], T, 0.001, rs)
    elif name.startswith("size_"):
        P, Q, _ = clouds(int(name[len("size_"):]), seed)
    elif name == "dup_pairs":   # ORB's multi-level duplicates: every point twice
        P, Q, _ = clouds(150, seed)
        P, Q = np.repeat(P, 2, axis=0), np.repeat(Q, 2, axis=0)
    elif name == "dup_block25":
        # 25 >= k copies of one point: all 20 neighbours coincide.  The point lies on the 1/64 lattice so that
        # PCL's float products are exact and the covariance is the zero matrix (svd3's scale == 0 branch), not
        # the float rounding of x * x
        P, Q, _ = clouds(200, seed)
        P[40:65] = np.round(P[40] * 64) / 64
        Q[40:65] = np.round(Q[40] * 64) / 64
    elif name == "all_identical":
        P = np.tile(np.array([0.3, -0.2, 2.1], F), (30, 1))
        Q = (P + np.array([0.01, 0, 0], F)).astype(F)
    elif name in ("exact_plane", "exact_plane_moved"):
        P = np.c_[rs.uniform(-1, 1, 300), rs.uniform(-0.8, 0.8, 300), np.full(300, 2.0)].astype(F)
        if name == "exact_plane":
            Q = (P + np.array([0.004, -0.003, 0.002], F)).astype(F)
        else:
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = rot(np.array([0.01, -0.015, 0.02])), [0.01, -0.008, 0.012]
            Q = moved(P, T, 0.001, rs)
    elif name == "exact_line":
        P = np.c_[rs.uniform(-1, 1, 200), np.full(200, 0.25), np.full(200, 2.0)].astype(F)
        Q = (P + np.array([0.004, -0.003, 0.002], F)).astype(F)
    elif name in ("lattice_half", "lattice_half_gridoff"):
        P, Q = _lattice(np.random.default_rng(1000 + NAMES.index("lattice_half")))
        if name == "lattice_half_gridoff":
            Q[0] = (0, 0, 40)
    elif name == "small_maxcorr":
        P, Q, _ = clouds(300, seed, noise=3e-4, motion=(5e-4, 5e-4))
        prm.update(max_corr_dist=0.004)
    elif name == "query_far_mixed":
        P, Q, _ = clouds(300, seed)
        P[7] = (0, 0, 40)
        P[200] = (-50, 0, 2)
    elif name in ("grid_rim", "grid_rim_out"):
        # targets in the grid's last valid cells (-511 and 510; 509 as well) on three axes, their sources where
        # the true motion puts them, the true motion as the guess; grid_rim_out adds the first cell outside (511)
        P, Q, T = clouds(300, 1000 + NAMES.index("grid_rim"))
        rim = [(0, -510.5), (1, 509.5), (2, 510.5)] + ([(0, 511.5)] if name == "grid_rim_out" else [])
        E = np.tile(np.array([0.1, -0.1, 2.0]), (len(rim), 1))
        for r, (axis, c) in enumerate(rim):
            E[r, axis] = c * RIM_H
        E = E.astype(F)
        Q = np.concatenate([Q, E])
        P = np.concatenate([P, ((E.astype(np.float64) - T[:3, 3]) @ T[:3, :3]).astype(F)])
        guess = T.astype(F)
    elif name == "guess_far":
        P, Q, _ = clouds(300, seed)
        guess[:3, 3] = 40.0
    elif name == "maxcorr_zero":
        P, Q, _ = clouds(100, seed)
        prm.update(max_corr_dist=0.0)
    elif name == "edge_ring":
        g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
        P = (g * 0.3 + np.array([-0.75, -0.75, 1.5]) + rs.uniform(-0.02, 0.02, size=g.shape)).astype(F)
        d = rs.normal(size=g.shape)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        # every other direction along an axis: only those can leave a 27-cell block whose cells are too small
        # (a random direction's largest component is rarely within a few per cent of its length)
        d[::2] = 0
        d[np.arange(0, len(g), 2), rs.integers(0, 3, len(g) // 2)] = rs.choice([-1.0, 1.0], len(g) // 2)
        Q = (P + d * (rs.uniform(0.97, 1.03, size=(len(g), 1)) * 0.07)).astype(F)
    elif name == "four_eq":
        P, Q = _four(F(0.0625))
        prm.update(max_corr_dist=0.0625)
    elif name == "four_below":
        P, Q = _four(np.nextafter(F(0.0625), F(0)))
        prm.update(max_corr_dist=0.0625)
    elif name == "late_abort":
        P, Q = late_abort(LATE_ABORT_SEED)
    elif name in K_CASES:
        M, k = K_CASES[name]
        P, Q, _ = clouds(M, seed)
        prm.update(k_correspondences=k)
    elif name in PARAM_CASES:
        P, Q, _ = clouds(300, seed)
        prm.update(PARAM_CASES[name])
    elif name == "big_rot_guess":
        P, _, _ = clouds(300, seed)
        T = big_rot_truth()
        Q = moved(P, T, 0.003, rs)
        guess = T.astype(F)
        guess[:3, 3] += np.array([0.006, -0.006, 0.005], F)
    else:
        raise KeyError(name)
    return name, np.ascontiguousarray(P, F), np.ascontiguousarray(Q, F), guess, prm


def big_rot_truth():
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot(np.array([0.3, -1.9, 0.8])), [0.4, -0.2, 0.3]
    return T
