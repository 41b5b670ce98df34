"""Inputs of the occupancy-map tests: the smallest scans at which each rule of DESIGN.md "Occupancy map definition" can
go wrong.  A case is (capacity, [scan, ...]); a scan is (points, Twc34, origin, maxrange), points being rgbd_points in
the camera frame.  Most cases use the identity pose, so their points are world coordinates."""
import numpy as np

F = np.float32
POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("pad", "u1")])
I34 = np.eye(4, dtype=F)[:3].copy()
O = np.array((0.04, 0.04, 0.04), F)
# the known-answer rays of tests/test_occmap_model.py
E_X, E_DIAG, E_NEG = (0.44, 0.04, 0.04), (0.20, 0.20, 0.20), (-0.12, 0.04, 0.20)


def pts(rows):
    """rows of (x, y, z) or (x, y, z, r, g, b); the default colour is (10, 20, 30)."""
    out = np.zeros(len(rows), POINT)
    for i, r in enumerate(rows):
        out[i]["x"], out[i]["y"], out[i]["z"] = r[0], r[1], r[2]
        out[i]["r"], out[i]["g"], out[i]["b"] = r[3:6] if len(r) >= 6 else (10, 20, 30)
    return out


def scan(rows, origin=O, maxrange=-1.0, T=I34):
    return (pts(rows) if not isinstance(rows, np.ndarray) else rows, np.asarray(T, F), np.asarray(origin, F), float(maxrange))


def _forty(reverse):
    rng = np.random.default_rng(40)
    rows = [(0.41 + 0.07 * rng.random(), 0.01 + 0.07 * rng.random(), 0.01 + 0.07 * rng.random(),
             int(rng.integers(256)), int(rng.integers(256)), int(rng.integers(256))) for _ in range(40)]
    return rows[::-1] if reverse else rows


def _random_cloud(seed, n, origin, spread=1.5):
    rng = np.random.default_rng(seed)
    p = pts([(0, 0, 0)] * n)
    xyz = (np.asarray(origin) + rng.normal(0, spread, (n, 3))).astype(F)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    col = rng.integers(0, 256, (n, 3))
    p["r"], p["g"], p["b"] = col[:, 0], col[:, 1], col[:, 2]
    return p


def _rot(axis, ang, t):
    a = np.asarray(axis, float)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    return np.concatenate([R, np.reshape(t, (3, 1))], 1).astype(F)


_FREE18 = [scan([(0.84, 0.04, 0.04)])] * 18     # the voxel of (0.44, 0.04, 0.04) is free 18 times: l_min

CASES = {
    # ray shapes, one point each
    "ray_x": (64, [scan([E_X])]),
    "ray_diag_ties": (64, [scan([E_DIAG])]),
    "ray_neg": (64, [scan([E_NEG])]),
    "same_voxel": (64, [scan([(0.05, 0.07, 0.01)])]),
    "zero_component": (64, [scan([(0.44, 0.30, 0.04)])]),
    "negative_steps": (64, [scan([(-0.50, -0.30, -0.21)])]),
    "posed": (256, [scan([(0.3, -0.2, 1.1), (-0.4, 0.1, 0.9)], origin=(0.5, -0.25, 0.125),
                         T=_rot((1, 2, 3), 0.7, (0.5, -0.25, 0.125)))]),
    # occupied beats free, once per scan
    "end_on_other_ray": (64, [scan([E_X, (0.84, 0.04, 0.04)])]),
    "end_on_other_ray_swapped": (64, [scan([(0.84, 0.04, 0.04), E_X])]),
    "forty_in_one_voxel": (64, [scan(_forty(False))]),
    "forty_in_one_voxel_reversed": (64, [scan(_forty(True))]),
    # colour: white counts as unset
    "white_then_colour": (64, [scan([E_X + (255, 255, 255), (0.45, 0.05, 0.05, 7, 90, 200)])]),
    # integer halving never reaches white from another colour, so a white voxel comes from a white point: the next
    # point sets the colour instead of averaging, the one after averages
    "white_voxel_hit_again": (64, [scan([E_X + (255, 255, 255)]), scan([E_X + (100, 50, 25)]), scan([E_X + (1, 2, 250)])]),
    "near_white_average": (64, [scan([E_X + (255, 255, 254), E_X + (255, 255, 255), E_X + (255, 255, 255)])]),
    # clamping
    "saturate_20": (64, [scan([E_X])] * 20),
    "hit_after_l_min": (64, _FREE18 + [scan([E_X])]),
    # maxrange: the voxel of the far point exists from the first scan, so its colour folds; nothing else is occupied
    "maxrange_far": (128, [scan([(2.04, 0.04, 0.04, 200, 100, 50)], origin=(1.96, 0.04, 0.04)),
                           scan([(2.04, 0.04, 0.04, 40, 60, 80), (0.04, 2.04, 0.04, 1, 2, 3)], maxrange=1.0)]),
    "maxrange_exact": (64, [scan([(1.5, 0.5, 0.5), (0.5, np.nextafter(F(1.5), F(2)), 0.5)], origin=(0.5, 0.5, 0.5),
                                 maxrange=1.0)]),
    # bad points are skipped whole
    "bad_points": (64, [scan([(3000.0, 0.0, 0.0), (np.nan, 0.1, 0.1), (0.1, np.inf, 0.1), (0.1, 0.1, -np.inf), E_X,
                              (0.0, -2700.0, 0.0)])]),
    "far_origin": (64, [scan([E_X], origin=(0.0, 0.0, 2700.0))]),
    # table limits: about 50 voxels in 64 slots
    "wrap_64": (64, [scan([(1.30, 0.40, 0.20), (0.04, 1.10, 0.30), (-0.9, -0.2, 0.04)])]),
    "random_cloud": (1 << 15, [   # about 22000 voxels: two thirds of the tablescan(_random_cloud(1, 300, (0, 0, 0)), origin=(0, 0, 0)),
                            scan(_random_cloud(2, 300, (0.5, 0, 0)), origin=(0.5, 0.1, 0), maxrange=2.0),
                            scan(_random_cloud(1, 300, (0, 0, 0)), origin=(0.1, -0.3, 0.2))]),
    "empty_scan": (64, [scan([]), scan([E_X]), scan([])]),
}

# a table of 64: the first scan takes about 30 voxels, the second needs more than the rest, the third fits again
OVERFLOW = (64, [scan([(1.30, 0.40, 0.20), (0.04, 1.10, 0.30)]),
                 scan([(-1.9, -0.2, 0.04), (0.04, -1.6, -0.9)]),
                 scan([(0.04, 0.04, 0.60)])])
