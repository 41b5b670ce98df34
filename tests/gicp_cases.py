"""Seeded synthetic GICP problems (test infrastructure): surface-like clouds (planes + a box) with a
known rigid motion, per-point noise, and an optional fraction of gross outliers."""
import numpy as np

from pnp_cases import rot


def clouds(n, seed, noise=0.003, outliers=0.0, motion=(0.02, 0.015)):
    rs = np.random.default_rng(seed)
    k = n // 3
    a = np.c_[rs.uniform(-1, 1, k), rs.uniform(-0.8, 0.8, k), 2.2 + 0.01 * rs.normal(size=k)]
    b = np.c_[rs.uniform(-1, 1, k), 0.9 + 0.01 * rs.normal(size=k), rs.uniform(1.2, 3.0, k)]
    m = n - 2 * k
    c = np.c_[-0.7 + 0.01 * rs.normal(size=m), rs.uniform(-0.8, 0.8, m), rs.uniform(1.2, 3.0, m)]
    P = np.concatenate([a, b, c]).astype(np.float32)
    R = rot(rs.normal(size=3) * motion[0])
    t = rs.normal(size=3) * motion[1]
    Q = P.astype(np.float64) @ R.T + t + rs.normal(size=P.shape) * noise
    bad = rs.random(n) < outliers
    Q[bad] += rs.uniform(-0.5, 0.5, size=(int(bad.sum()), 3))
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return P, Q.astype(np.float32), T


def np_covariances(P, k=20, eps=1e-3, idx=None):
    """PCL's covariance stage in an independent numpy formulation (lexsort k-NN, eigh instead of the SVD) for the
    points idx (default: all).  Defined where the covariance's smallest eigenvalue is simple."""
    P32 = P.astype(np.float32)
    out = []
    for i in (range(len(P32)) if idx is None else idx):
        d = P32 - P32[i]
        d2 = (((np.float32(0) + d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)
        nn = np.lexsort((np.arange(len(P32)), d2))[:k]
        X = P32[nn]
        mu = X.astype(np.float64).sum(0) / k
        # PCL accumulates float products (pt.y * pt.x) into double sums
        S = np.array([[(X[:, a] * X[:, b]).astype(np.float64).sum() for b in range(3)] for a in range(3)])
        C = S / k - np.outer(mu, mu)
        w, V = np.linalg.eigh(C)
        out.append(V @ np.diag([eps, 1.0, 1.0]) @ V.T)
    return np.array(out)
