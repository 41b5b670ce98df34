"""Matcher::projectionMatch (Features/Matcher.cpp:35-104) restated in numpy from DESIGN.md "Projection match
definition": np.float32 step by step, Python floats for the double sums of the cv::Mat gemms, round half
away from zero for posInGrid.  The candidate lists (geometry) and the serial greedy are offered separately.
Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
COLS, ROWS, TH_HIGH = 64, 48, 100
SEARCHED, OUTLIER, NO_DEPTH, BEHIND, OUTSIDE, NO_CELLS = range(6)
F = np.float32


def image_bounds(cam: dict, W=640, H=480):
    """computeImageBounds (Core/Frame.cpp:283-315) -> (min_x, max_x, min_y, max_y) as np.float32.  A distorted
    camera's corners go through the oracle's keypoint undistortion (orc_frame_geometry with the four corners as
    keypoints over a zero depth plane of (H + 1) x (W + 1), so the corner (W, H) reads inside the plane)."""
    if F(cam["k1"]) == F(0):
        return F(0), F(W), F(0), F(H)
    import oracle_lib as O
    L = O.lib()
    fn = L.orc_frame_geometry
    fn.restype = None
    fn.argtypes = [O.kpp, C.c_int, O.u16p, C.c_int, C.POINTER(O.Camera), O.kpp, O.f32p]
    kps = np.zeros(4, O.KEYPOINT_DTYPE)
    kps["x"] = [0, W, 0, W]
    kps["y"] = [0, 0, H, H]
    un = np.zeros(4, O.KEYPOINT_DTYPE)
    xyz = np.zeros((4, 3), np.float32)
    depth = np.zeros((H + 1, W + 1), np.uint16)
    oc = O.camera(cam)
    fn(kps, 4, depth, W + 1, C.byref(oc), un, xyz)
    x, y = un["x"], un["y"]
    return min(x[0], x[2]), max(x[1], x[3]), min(y[0], y[1]), max(y[2], y[3])


def _round(v):
    v = float(v)
    if math.isnan(v) or math.isinf(v):
        return v
    return math.copysign(math.floor(abs(v) + .5), v)


class Grid:
    """assignFeaturesToGrid / posInGrid (Core/Frame.cpp:75-89, :231-241) of F2's undistorted keypoints."""

    def __init__(self, x2, y2, bounds):
        self.min_x, self.max_x, self.min_y, self.max_y = (F(b) for b in bounds)
        self.winv = F(64.0) / (self.max_x - self.min_x)
        self.hinv = F(48.0) / (self.max_y - self.min_y)
        self.x = np.asarray(x2, np.float32)
        self.y = np.asarray(y2, np.float32)
        self.cells = [[[] for _ in range(ROWS)] for _ in range(COLS)]
        self.cell_of = []
        for i in range(len(self.x)):
            c = _round((self.x[i] - self.min_x) * self.winv)
            r = _round((self.y[i] - self.min_y) * self.hinv)
            if 0 <= c < COLS and 0 <= r < ROWS:   # false for NaN
                self.cells[int(c)][int(r)].append(i)
                self.cell_of.append((int(c), int(r)))
            else:
                self.cell_of.append(None)

    def window(self, u, v, th):
        """getFeaturesInArea's cell range (Core/Frame.cpp:185-199) or None on an early return."""
        th = F(th)
        c0 = math.floor(((u - self.min_x) - th) * self.winv)
        c1 = math.ceil(((u - self.min_x) + th) * self.winv)
        r0 = math.floor(((v - self.min_y) - th) * self.hinv)
        r1 = math.ceil(((v - self.min_y) + th) * self.hinv)
        c0, r0 = max(0, c0), max(0, r0)
        if c0 >= COLS or c1 < 0 or r0 >= ROWS or r1 < 0:
            return None
        return c0, min(COLS - 1, c1), r0, min(ROWS - 1, r1)

    def in_area(self, u, v, th):
        """vIndices2 in visiting order (default levels), or None when no cell range exists."""
        win = self.window(u, v, th)
        if win is None:
            return None
        c0, c1, r0, r1 = win
        th = F(th)
        out = []
        for ix in range(c0, c1 + 1):
            for iy in range(r0, r1 + 1):
                for j in self.cells[ix][iy]:
                    if abs(self.x[j] - u) < th and abs(self.y[j] - v) < th:
                        out.append(j)
        return out


def project(x, T1, T2, K4, bounds):
    """Steps 2-5 for one point: (status, u, v); u and v are None where not computed."""
    T1 = np.asarray(T1, np.float32).reshape(4, 4)
    T2 = np.asarray(T2, np.float32).reshape(4, 4)
    fx, fy, cx, cy = (F(k) for k in K4)
    min_x, max_x, min_y, max_y = (F(b) for b in bounds)
    xw = np.zeros(3, np.float32)
    for r in range(3):
        o = 0.0
        a = 0.0
        for k in range(3):
            o += float(T1[k, r]) * float(T1[k, 3])
            a += float(T1[k, r]) * float(x[k])
        Ow = F(o * -1.0)
        xw[r] = F(a + float(Ow))
    xc = np.zeros(3, np.float32)
    for r in range(3):
        a = 0.0
        for k in range(3):
            a += float(T2[r, k]) * float(xw[k])
        xc[r] = F(a + float(T2[r, 3]))
    with np.errstate(all="ignore"):
        inv = F(1.0) / xc[2]
        if inv < 0:
            return BEHIND, None, None
        u = (fx * xc[0]) * inv + cx
        v = (fy * xc[1]) * inv + cy
    if not (u >= min_x and u <= max_x and v >= min_y and v <= max_y):   # NaN: skipped (defined here)
        return OUTSIDE, u, v
    return SEARCHED, u, v


def candidates(xyz1, outlier1, T1, x2, y2, T2, K4, bounds, th, grid=None):
    """Per query: (status, u, v, vIndices2 in visiting order before the z and taken filters)."""
    grid = grid or Grid(x2, y2, bounds)
    xyz1 = np.asarray(xyz1, np.float32).reshape(-1, 3)
    out = []
    for i in range(len(xyz1)):
        if outlier1 is not None and outlier1[i]:
            out.append((OUTLIER, None, None, []))
            continue
        if not (xyz1[i, 2] > 0):
            out.append((NO_DEPTH, None, None, []))
            continue
        st, u, v = project(xyz1[i], T1, T2, K4, bounds)
        if st != SEARCHED:
            out.append((st, u, v, []))
            continue
        with np.errstate(all="ignore"):
            c = grid.in_area(u, v, th)
        if c is None:
            out.append((NO_CELLS, u, v, []))
        else:
            out.append((SEARCHED, u, v, c))
    return out


_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(d1, D2):
    return _POP[np.bitwise_xor(D2, d1[None, :])].sum(1)


def greedy(cands, desc1, desc2, z2, stats=None):
    """Step 8, serial: per query in order the smallest distance among the z-valid, untaken candidates, first in
    visiting order on ties, matched when <= TH_HIGH."""
    desc1 = np.asarray(desc1, np.uint8).reshape(-1, 32)
    desc2 = np.asarray(desc2, np.uint8).reshape(-1, 32)
    taken = set()
    out = []
    for i, (st, _, _, c) in enumerate(cands):
        if st != SEARCHED or not c:
            continue
        c = np.asarray(c, np.int64)
        d = hamming(desc1[i], desc2[c])
        best, bj, skipped, own = None, -1, False, None
        for k in range(len(c)):
            j = int(c[k])
            if not (z2[j] > 0):
                continue
            if own is None or d[k] < own[0]:
                own = (int(d[k]), j)   # the best candidate regardless of the taken set
            if j in taken:
                skipped = True
                continue
            if best is None or d[k] < best:
                best, bj = int(d[k]), j
        if best is not None and best <= TH_HIGH:
            out.append((i, bj, -1, float(best)))
            taken.add(bj)
            if stats is not None:
                stats["after_skip"] = stats.get("after_skip", 0) + int(skipped)
                stats["not_own_best"] = stats.get("not_own_best", 0) + int(own[1] != bj)
    return np.array(out, DMATCH_DTYPE)


def projection_match(xyz1, desc1, outlier1, T1, x2, y2, z2, desc2, T2, K4, bounds, th, stats=None):
    c = candidates(xyz1, outlier1, T1, x2, y2, T2, K4, bounds, th)
    return greedy(c, desc1, desc2, np.asarray(z2, np.float32), stats)


def brute_candidates(xyz1, outlier1, T1, x2, y2, T2, K4, bounds, th):
    """Grid-free candidate lists for keypoints that all lie inside the grid: every j with |dx| < th and
    |dy| < th, ordered by (cell column, cell row, index)."""
    g = Grid(x2, y2, bounds)
    assert all(c is not None for c in g.cell_of)
    order = sorted(range(len(g.x)), key=lambda j: (g.cell_of[j][0], g.cell_of[j][1], j))
    xyz1 = np.asarray(xyz1, np.float32).reshape(-1, 3)
    out = []
    for i in range(len(xyz1)):
        if (outlier1 is not None and outlier1[i]) or not (xyz1[i, 2] > 0):
            out.append([])
            continue
        st, u, v = project(xyz1[i], T1, T2, K4, bounds)
        if st != SEARCHED:
            out.append([])
            continue
        out.append([j for j in order if abs(g.x[j] - u) < F(th) and abs(g.y[j] - v) < F(th)])
    return out
