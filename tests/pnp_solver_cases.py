"""TEST INFRASTRUCTURE ONLY: the inputs of the motion-only bundle adjustment tests (rgbd_pnp_solver*), each
built for one regime of DESIGN.md "Motion-only BA definition".  tests/test_pnp_solver_model.py asserts from the
model alone that every input is in the regime it is named for; tests/test_gpu_pnp_solver.py holds the device to
the model on the same inputs.  case(name) = dict(Xw (M, 3) f32, obs (M, 2) f32, K4, Tcw_in (4, 4) f32, prm = the
non-default parameters as a dict, plus what the regime test needs); model(name) = the model's result, computed
once."""
import functools
import math

import numpy as np

import pnp_solver_model as BA

K4 = np.array([517.3, 516.5, 318.6, 255.3], np.float32)       # fr1
K4_EXACT = np.array([512.0, 512.0, 320.0, 240.0], np.float32)  # projections that are exact in f32
W, H = 640, 480


def rodrigues(rv):
    rv = np.asarray(rv, np.float64)
    th = float(np.linalg.norm(rv))
    if th == 0:
        return np.eye(3)
    k = rv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)


def pose(rv, t):
    T = np.eye(4)
    T[:3, :3] = rodrigues(rv)
    T[:3, 3] = t
    return T


T_TRUE = pose([0.08, -0.12, 0.05], [0.30, -0.20, 0.50])
# 5 cm and 2 degrees off the planted pose
T_OFF = pose(np.deg2rad(2.0) * np.array([0.6, -0.64, 0.48]), [0.03, -0.032, 0.024])


def guess_of(T_true, off=T_OFF):
    return (off @ T_true).astype(np.float32)


def project(T, Xw, K=K4):
    p = (T[:3, :3] @ np.asarray(Xw, np.float64).T).T + T[:3, 3]
    fx, fy, cx, cy = [float(v) for v in K]
    return np.stack([p[:, 0] / p[:, 2] * fx + cx, p[:, 1] / p[:, 2] * fy + cy], 1)


def cloud(rng, n, T_true=T_TRUE, K=K4):
    """n world points (f32) seen by the planted pose at 0.5-4 m, and their f64 projections rounded to f32."""
    fx, fy, cx, cy = [float(v) for v in K]
    u = rng.uniform(20, W - 20, n)
    v = rng.uniform(20, H - 20, n)
    z = rng.uniform(0.5, 4.0, n)
    pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    Xw = ((pc - T_true[:3, 3]) @ T_true[:3, :3]).astype(np.float32)
    return Xw, project(T_true, Xw, K).astype(np.float32)


def move(rng, obs, idx, lo=20.0, hi=60.0):
    """obs with rows idx moved by lo..hi pixels in a random direction."""
    obs = obs.copy()
    a = rng.uniform(0, 2 * np.pi, len(idx))
    r = rng.uniform(lo, hi, len(idx))
    obs[idx] += np.stack([r * np.cos(a), r * np.sin(a)], 1).astype(np.float32)
    return obs


def _base(seed, n, frac=0.0, noise=0.0, T_true=T_TRUE, lo=20.0, hi=60.0):
    rng = np.random.default_rng(seed)
    Xw, obs = cloud(rng, n, T_true)
    if noise:
        obs = (obs + rng.normal(0, noise, obs.shape)).astype(np.float32)
    planted = np.zeros(n, np.uint8)
    if frac:
        idx = np.sort(rng.choice(n, int(round(frac * n)), replace=False))
        obs = move(rng, obs, idx, lo, hi)
        planted[idx] = 1
    return dict(Xw=Xw, obs=obs, K4=K4, Tcw_in=guess_of(T_true), prm={}, planted=planted, T_true=T_true)


def _trial_cap():
    """Round 0 without the Huber kernel ends by the trial cap: ten rejected trials, the last of them a step that
    still moves the estimate in its last bits."""
    c = _base(47, 40, noise=1.0)
    c["prm"] = dict(robust_rounds=0)
    return c


def _stale_error():
    """Quirk 3.  No Huber kernel (robust_rounds = 0), so round 0's optimisation does not read the threshold; the
    round ends on a rejected trial, and the threshold is put on the smaller of the two chi2 one active edge has at
    that trial and at the estimate: the edge's level then depends on which error the classification reads."""
    c = _trial_cap()
    r = BA.solve(c["Xw"], c["obs"], c["K4"], c["Tcw_in"], **c["prm"])
    r0 = r["rounds"][0]
    pr = BA.Problem(c["Xw"], c["obs"], c["K4"], 5.991)
    fin = pr.errors((list(r0["est"][:4]), list(r0["est"][4:])))[3]
    stale = r0["chi2"]
    differ = np.nonzero((stale != fin) & (fin > 0.5))[0]
    e = int(differ[0])
    c["prm"]["chi2_threshold"] = float(min(stale[e], fin[e]))
    c["edge"] = e
    return c


def _optimum(n):
    """An exact optimum: the identity pose and points whose projections are exact in f32, so err = 0, the step is
    0, the trial equals the estimate and rho_hat = 0 / 1e-3: one iteration, one rejected trial per round."""
    Xw = np.array([[0.5, 0.25, 1.0], [-0.5, 0.5, 2.0], [0.25, -0.75, 1.0], [1.0, 0.5, 2.0], [-0.25, 0.25, 1.0],
                   [0.5, -0.5, 4.0], [-1.0, -0.5, 2.0], [0.75, 0.25, 1.0], [-0.75, 0.125, 1.0], [0.125, 0.375, 0.5],
                   [1.5, 1.0, 4.0], [-0.125, -0.25, 0.5]], np.float32)[:n]
    obs = project(np.eye(4), Xw, K4_EXACT).astype(np.float32)
    return dict(Xw=Xw, obs=obs, K4=K4_EXACT, Tcw_in=np.eye(4, dtype=np.float32), prm={})


def _nan_edge():
    rng = np.random.default_rng(5)
    T_true = pose([0.0, 0.0, 0.0], [0.02, -0.01, 0.015])
    Xw, obs = cloud(rng, 12, T_true)
    Xw[0] = (0.0, 0.5, 0.0)   # under the identity guess: x_c = 0 and z_c = 0, so u = 0 / 0
    return dict(Xw=Xw, obs=obs, K4=K4, Tcw_in=np.eye(4, dtype=np.float32), prm={}, T_true=T_true)


def _nonorthonormal():
    c = _base(21, 60)
    A = pose([0.3, 0.2, -0.4], [0.1, 0.2, 0.3]).astype(np.float32)
    B = (np.linalg.inv(pose([0.3, 0.2, -0.4], [0.1, 0.2, 0.3])) @ T_OFF @ T_TRUE).astype(np.float32)
    G = np.zeros((4, 4), np.float32)   # the float gemm of two float poses (double sums, one rounding)
    for i in range(4):
        for j in range(4):
            G[i, j] = np.float32(sum(float(A[i, k]) * float(B[k, j]) for k in range(4)))
    c["Tcw_in"] = G
    return c


def _all_outliers():
    """Quirk 7: four points, each observed three times 100 px away in directions 120 degrees apart.  No pose
    explains any observation, so every edge leaves round 0 at level 1 and rounds 1-3 have no active edge."""
    c = _base(31, 4)
    ang = np.deg2rad(np.array([90.0, 210.0, 330.0]))
    offs = 100.0 * np.stack([np.cos(ang), np.sin(ang)], 1)
    c["Xw"] = np.repeat(c["Xw"], 3, axis=0)
    c["obs"] = (np.repeat(c["obs"], 3, axis=0) + np.tile(offs, (4, 1))).astype(np.float32)
    c["planted"] = np.ones(12, np.uint8)
    return c


_BUILD = {
    "clean_300": lambda: _base(1, 300),
    "outliers_30pct": lambda: _base(2, 300, frac=0.3),
    # 45 % of the pixels moved by 8-20 px: round 0 under the Huber kernel ends away from the guess
    # and two iterations per round leave every round short of convergence, so the starting point of a round shows
    "restart": lambda: dict(_base(3, 120, frac=0.45, noise=0.5, lo=8.0, hi=20.0), prm=dict(iterations=2)),
    "stale_error": _stale_error,
    # two iterations from the guess: round 3's edges are still far out on the Huber kernel's linear part
    "kernel_removed": lambda: dict(_base(4, 80, frac=0.2, noise=1.2, lo=3.0, hi=12.0), prm=dict(iterations=2)),
    "m9": lambda: _base(9, 9, noise=0.3),
    "m10": lambda: _base(9, 10, noise=0.3),
    "m2": lambda: _base(7, 2),
    "m3": lambda: _base(7, 3),
    "all_outliers_after_round0": _all_outliers,
    "nan_edge": _nan_edge,
    "ten_trials": _trial_cap,
    "rho_zero": lambda: _optimum(3),
    "nonorthonormal_guess": _nonorthonormal,
    "m255": lambda: _base(255, 255, frac=0.1, noise=0.5),
    "m256": lambda: _base(256, 256, frac=0.1, noise=0.5),
    "m257": lambda: _base(257, 257, frac=0.1, noise=0.5),
    "m4096": lambda: _base(4096, 4096, frac=0.1, noise=0.5),
    # every round is one rejected trial at an optimum: lambda = lambda_0 nu with the nu the rounds before left
    "nu_carry": lambda: _optimum(12),
}
NAMES = list(_BUILD)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILD[name]()


@functools.lru_cache(maxsize=None)
def model(name, **switches):
    c = case(name)
    return BA.solve(c["Xw"], c["obs"], c["K4"], c["Tcw_in"], **c["prm"], **switches)
