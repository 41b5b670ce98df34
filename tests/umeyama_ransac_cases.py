"""TEST INFRASTRUCTURE ONLY: the inputs of the Umeyama RANSAC tests (rgbd_ransac_umeyama*), each built for one regime
of DESIGN.md "Umeyama RANSAC definition".  tests/test_umeyama_ransac_model.py asserts from the model alone that every
input is in the regime it is named for; tests/test_gpu_umeyama_ransac.py holds the device to the model on the same
inputs.  case(name) = dict(xyz1 (n1, 3) f32, xyz2 (n2, 3) f32, matches (DMATCH), prm (model.params), seed);
model(name) = the model's result on fresh flags and a generator seeded with the case's seed, computed once."""
import functools
import math

import numpy as np

import umeyama_ransac_model as UM

DMATCH = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
F = np.float32


def rodrigues(rv):
    rv = np.asarray(rv, np.float64)
    th = float(np.linalg.norm(rv))
    if th == 0:
        return np.eye(3)
    k = rv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)


R_TRUE = rodrigues([0.03, -0.05, 0.02])
T_TRUE = np.array([0.06, -0.03, 0.08])


def planted(seed, M, n_in, noise=0.0, outlier_spread=None, R=R_TRUE, t=T_TRUE, shuffle=True):
    """M matches: F2 points uniform in a 3 x 3 x (0.8..4) m box, F1 points = R p2 + t (+ gaussian noise); the
    matches past the first n_in get an F1 point elsewhere in the box (or within outlier_spread of the true one).
    The F2 cloud is stored permuted, so trainIdx != queryIdx."""
    g = np.random.default_rng(seed)
    p2 = np.stack([g.uniform(-1.5, 1.5, M), g.uniform(-1.5, 1.5, M), g.uniform(0.8, 4.0, M)], 1)
    p1 = p2 @ R.T + t + noise * g.standard_normal((M, 3))
    if outlier_spread is None:
        p1[n_in:] = np.stack([g.uniform(-1.5, 1.5, M - n_in), g.uniform(-1.5, 1.5, M - n_in), g.uniform(0.8, 4.0, M - n_in)], 1)
    else:
        p1[n_in:] += g.uniform(-outlier_spread, outlier_spread, (M - n_in, 3))
    order = g.permutation(M)                       # match order: inliers and outliers interleaved
    perm = g.permutation(M) if shuffle else np.arange(M)
    xyz1 = p1.astype(F)
    xyz2 = np.zeros((M, 3), F)
    xyz2[perm] = p2.astype(F)
    m = np.zeros(M, DMATCH)
    m["queryIdx"] = order
    m["trainIdx"] = perm[order]
    m["imgIdx"] = -1
    m["distance"] = g.uniform(10, 60, M).astype(F)
    return xyz1, xyz2, m


def _case(xyz1, xyz2, m, seed=1234, **prm):
    return dict(xyz1=np.ascontiguousarray(xyz1, F), xyz2=np.ascontiguousarray(xyz2, F), matches=m, prm=UM.params(**prm),
                seed=seed)


def _depth_gate():
    """pure x translation, so z1 == z2: rows 0 / 1 sit exactly on 0.1f / 6.0f, rows 2 / 3 one float outside"""
    xyz1, xyz2, m = planted(5, 16, 16, R=np.eye(3), t=np.array([0.05, 0.0, 0.0]), shuffle=False)
    m["queryIdx"] = np.arange(16)
    m["trainIdx"] = np.arange(16)
    z = [F(0.1), F(6.0), np.nextafter(F(0.1), F(0)), np.nextafter(F(6.0), F(7))]
    for i, v in enumerate(z):
        xyz1[i, 2] = xyz2[i, 2] = v
    return _case(xyz1, xyz2, m)


def _nan_z():
    xyz1, xyz2, m = planted(21, 12, 7)
    xyz2[m["trainIdx"][4], 2] = np.nan
    return _case(xyz1, xyz2, m)


def _too_few():
    xyz1, xyz2, m = planted(8, 12, 12)
    for i in range(4):
        xyz1[m["queryIdx"][2 * i], 2] = F(7.5)
    return _case(xyz1, xyz2, m)


def _duplicate_rows():
    xyz1, xyz2, m = planted(9, 20, 14)
    m[6] = m[5]
    return _case(xyz1, xyz2, m)


def _static_pair():
    xyz1, xyz2, m = planted(10, 64, 64, R=np.eye(3), t=np.zeros(3))
    return _case(xyz1, xyz2, m)


def _over_cap():
    xyz1, xyz2, m = planted(12, 4097, 4097, shuffle=False)
    return _case(xyz1, xyz2, m)


BUILDERS = {
    "clean": lambda: _case(*planted(1, 10, 10)),
    "half_outliers": lambda: _case(*planted(2, 64, 32)),
    "grow": lambda: _case(*planted(3, 64, 8)),
    "below_ratio": lambda: _case(*planted(4, 64, 4)),
    "refit_shrinks": lambda: _case(*planted(31, 257, 110, noise=0.015)),
    "reflection": lambda: _case(*planted(7, 10, 5)),
    "tie_keeps_first": lambda: _case(*planted(13, 64, 32), seed=99),
    "static_pair": _static_pair,
    "adaptive": lambda: _case(*planted(14, 64, 40, noise=0.012), error_version=UM.ADAPTIVE_ERROR, thr=0.015),
    "depth_gate": _depth_gate,
    "nan_z": _nan_z,
    "too_few": _too_few,
    "min_size": lambda: _case(*planted(15, 3, 3), min_matches=3),
    "duplicate_rows": _duplicate_rows,
    "pairs8": lambda: _case(*planted(16, 64, 40, noise=0.004), used_pairs=8),
    "saturate": lambda: _case(*planted(17, 2304, 300, outlier_spread=0.6)),
    "cap": lambda: _case(*planted(18, 4096, 2048)),
}
NAMES = list(BUILDERS)
CHAIN = ["half_outliers", "grow", "clean"]   # three calls on one generator


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def over_cap():
    return _over_cap()


def run_model(oracle, c, rng=None, flags2=None):
    rng = rng if rng is not None else oracle.rng(c["seed"])
    flags2 = flags2 if flags2 is not None else np.zeros(len(c["xyz2"]), np.uint8)
    out = UM.solve(oracle, c["xyz1"], c["xyz2"], c["matches"], c["prm"], rng, flags2)
    out["flags2"] = flags2
    out["rng"] = bytes(rng)
    return out


_MODEL = {}


def model(oracle, name):
    if name not in _MODEL:
        _MODEL[name] = run_model(oracle, case(name))
    return _MODEL[name]


_CHAIN = []


def chain_model(oracle):
    """the model's three results of CHAIN on one generator (seed 4242), state for state"""
    if not _CHAIN:
        rng = oracle.rng(4242)
        for name in CHAIN:
            _CHAIN.append(run_model(oracle, case(name), rng=rng))
    return _CHAIN
