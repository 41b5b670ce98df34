"""Hand-placed inputs of the projection-match tests, shared by the CPU model tests and the GPU tests.

Camera fx = fy = 256, cx = 320, cy = 240 with identity poses and z = 1: a query point ((u - 320) / 256,
(v - 240) / 256, 1) projects to exactly (u, v) for u, v on the 1/256 grid, so the cases below are exact in f32.
An undistorted 640 x 480 frame: bounds (0, 640, 0, 480), wInv = hInv = 0.1f."""
import numpy as np

CAM = dict(fx=256.0, fy=256.0, cx=320.0, cy=240.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, factor=5000.0)
K4 = (256.0, 256.0, 320.0, 240.0)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
EYE = np.eye(4, dtype=np.float32)


def point(u, v, z=1.0):
    return [(u - 320.0) / 256.0 * z, (v - 240.0) / 256.0 * z, z]


def bits(n):
    """A descriptor with its first n bits set."""
    d = np.zeros(32, np.uint8)
    d[:n // 8] = 255
    if n % 8:
        d[n // 8] = (1 << (n % 8)) - 1
    return d


def case(queries, trains, th, qdesc=None, tdesc=None, tz=None, outlier=None, T1=EYE, T2=EYE):
    """queries: 3D points; trains: (x, y) undistorted keypoints.  Descriptors default to zeros, train z to 1."""
    n1, n2 = len(queries), len(trains)
    xyz2 = np.zeros((n2, 3), np.float32)
    xyz2[:, 2] = 1.0 if tz is None else np.asarray(tz, np.float32)
    t = np.asarray(trains, np.float32).reshape(n2, 2)
    return dict(xyz1=np.asarray(queries, np.float32).reshape(n1, 3),
                desc1=np.zeros((n1, 32), np.uint8) if qdesc is None else np.asarray(qdesc, np.uint8).reshape(n1, 32),
                outlier1=None if outlier is None else np.asarray(outlier, np.uint8),
                T1=np.asarray(T1, np.float32), x2=t[:, 0].copy(), y2=t[:, 1].copy(), xyz2=xyz2,
                desc2=np.zeros((n2, 32), np.uint8) if tdesc is None else np.asarray(tdesc, np.uint8).reshape(n2, 32),
                T2=np.asarray(T2, np.float32), th=th)


def M(*rows):
    """Expected matches: (queryIdx, trainIdx, distance) rows; imgIdx is -1."""
    from projection_model import DMATCH_DTYPE
    return np.array([(q, t, -1, float(d)) for q, t, d in rows], DMATCH_DTYPE)


def quirks():
    """name -> (case, expected matches), each worked out by hand from the definition."""
    out = {}
    # x = 635: (635 - 0) * 0.1f = 63.5 -> column 64, no cell: never found, although it is 0 px from the query;
    # x = 634 (column 63) is found
    out["x635_in_no_cell"] = (case([point(635, 100), point(634, 300)], [(635, 100), (634, 300)], 5.0), M((1, 1, 0)))
    # |dx| == th and |dy| == th are excluded, anything below is a candidate
    out["dx_equals_th"] = (case([point(100, 100), point(300, 100), point(100, 300), point(300, 300)],
                                [(105, 100), (304.5, 100), (100, 305), (300, 304.5)], 5.0), M((1, 1, 0), (3, 3, 0)))
    # u == max_x passes the bounds test (only u > max_x is skipped) and is searched
    out["u_equals_max_x"] = (case([point(640, 100)], [(634, 100)], 7.0), M((0, 0, 0)))
    # TH_HIGH is inclusive: 100 matches, 101 does not (and takes nothing: the next query still sees a free train)
    out["dist_100"] = (case([point(100, 100)], [(100, 100)], 5.0, tdesc=[bits(100)]), M((0, 0, 100)))
    out["dist_101"] = (case([point(100, 100), point(100, 100)], [(100, 100)], 5.0, qdesc=[bits(0), bits(1)],
                            tdesc=[bits(101)]), M((1, 0, 100)))
    # a tie: train 0 at x = 106 (column 11) is visited after train 1 at x = 94 (column 9), so train 1 wins
    out["tie_visiting_order"] = (case([point(100, 100)], [(106, 100), (94, 100)], 8.0, tdesc=[bits(7), bits(7)]),
                                 M((0, 1, 7)))
    return out


def cascade(extra=0, seed=5):
    """130 queries project to one spot where 130 trains sit with dist(q, t_j) = j: q_i -> t_i for i <= 100 and
    nothing after.  extra > 0 interleaves unrelated queries (each with its own train elsewhere, matched at 3)."""
    n = 130
    rs = np.random.default_rng(seed)
    slots = np.sort(rs.choice(n + extra, size=n, replace=False)) if extra else np.arange(n)
    is_main = np.zeros(n + extra, bool)
    is_main[slots] = True
    queries, qdesc, trains, tdesc, want = [], [], [(200.25, 150.5)] * n, [bits(j) for j in range(n)], []
    k = e = 0
    for i in range(n + extra):
        if is_main[i]:
            queries.append(point(200.25, 150.5))
            qdesc.append(bits(0))
            if k <= 100:
                want.append((i, k, k))
            k += 1
        else:
            u, v = 40.0 + 25.0 * (e % 20), 400.0
            queries.append(point(u, v))
            qdesc.append(bits(0))
            trains.append((u + 1.0, v - 1.0))
            tdesc.append(bits(3))
            want.append((i, n + e, 3))
            e += 1
    return case(queries, trains, 5.0, qdesc=qdesc, tdesc=tdesc), M(*want)


def run_model(c, K4=K4, bounds=BOUNDS, stats=None):
    import projection_model as PM
    return PM.projection_match(c["xyz1"], c["desc1"], c["outlier1"], c["T1"], c["x2"], c["y2"], c["xyz2"][:, 2], c["desc2"],
                               c["T2"], K4, bounds, c["th"], stats)
