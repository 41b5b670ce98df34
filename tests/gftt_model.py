"""CPU model of the Shi-Tomasi GFTT + BRIEF extractor, Extractor(GFTT, BRIEF, NORMAL) of the reference
(Features/Extractor.cpp:50-61, 178-181: cv::GFTTDetector::create(nfeatures, 0.01, 3, 3, false, 0.04), retainBest,
BriefDescriptorExtractor), as DESIGN.md's "GFTT + BRIEF definition" states it: OpenCV 3.x's goodFeaturesToTrack
(cornerMinEigenVal with blockSize 3 and a 3x3 Sobel, threshold at quality_level of the frame's maximum, 3x3
dilate, sort by greaterThanPtr, the min-distance greedy) restated.  This file is the definition's executable
form; the device (csrc/gftt.hip) is held to it bit for bit by tests/test_gpu_gftt.py.

Several formulations are kept side by side and tests/test_gftt_model.py holds them equal:
  * the map: vectorised (eig_map) and a literal per-pixel restatement (eig_map_scalar);
  * the spacing: the brute-force distance test (select_brute), OpenCV's cvRound(minDistance) cell grid
    (select_grid) and the round-parallel form the device runs (select_rounds).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import oracle_lib as O
from adaptive_model import brief

KP = O.KEYPOINT_DTYPE
F32 = np.float32
SCALE = F32(1.0 / (4 * 3 * 255))   # 1 / ((1 << (ksize - 1)) * blockSize * 255), ksize = blockSize = 3


def params(nfeatures=1000, quality_level=0.01, min_distance=3.0):
    return dict(nfeatures=int(nfeatures), quality_level=float(quality_level), min_distance=float(min_distance))


# ------------------------------------------------------------------ the minimum-eigenvalue map
def eig_map(g: np.ndarray) -> np.ndarray:
    """e[y, x] (f32) of a u8 image: steps 2-5 of the definition."""
    P = np.pad(g.astype(np.int32), 1, mode="reflect")   # BORDER_REFLECT_101
    dx = (P[:-2, 2:] - P[:-2, :-2]) + 2 * (P[1:-1, 2:] - P[1:-1, :-2]) + (P[2:, 2:] - P[2:, :-2])
    dy = (P[2:, :-2] - P[:-2, :-2]) + 2 * (P[2:, 1:-1] - P[:-2, 1:-1]) + (P[2:, 2:] - P[:-2, 2:])
    Dx, Dy = dx.astype(F32) * SCALE, dy.astype(F32) * SCALE

    def box(m):   # unnormalised 3x3 sums in f64, rows first, REFLECT_101 on the product map, rounded once
        Q = np.pad(m, 1, mode="reflect").astype(np.float64)
        row = (Q[:, :-2] + Q[:, 1:-1]) + Q[:, 2:]
        return ((row[:-2] + row[1:-1]) + row[2:]).astype(F32)
    XX, XY, YY = box(Dx * Dx), box(Dx * Dy), box(Dy * Dy)
    a, b, c = XX * F32(0.5), XY, YY * F32(0.5)
    return ((a + c) - np.sqrt((a - c) * (a - c) + b * b)).astype(F32)


def _r101(i: int, n: int) -> int:
    return -i if i < 0 else (2 * n - 2 - i if i >= n else i)


def eig_map_scalar(g: np.ndarray) -> np.ndarray:
    """The same, one pixel at a time with explicit border arithmetic (slow: small images only)."""
    H, W = g.shape

    def px(y, x):
        return int(g[_r101(y, H), _r101(x, W)])

    def prod(y, x):   # the three covariance products at an in-image pixel
        dx = (px(y - 1, x + 1) - px(y - 1, x - 1)) + 2 * (px(y, x + 1) - px(y, x - 1)) + (px(y + 1, x + 1) - px(y + 1, x - 1))
        dy = (px(y + 1, x - 1) - px(y - 1, x - 1)) + 2 * (px(y + 1, x) - px(y - 1, x)) + (px(y + 1, x + 1) - px(y - 1, x + 1))
        Dx, Dy = F32(dx) * SCALE, F32(dy) * SCALE
        return Dx * Dx, Dx * Dy, Dy * Dy
    pr = [[prod(y, x) for x in range(W)] for y in range(H)]
    out = np.zeros((H, W), F32)
    for y in range(H):
        for x in range(W):
            s = []
            for k in range(3):
                rows = []
                for yy in (y - 1, y, y + 1):
                    r = pr[_r101(yy, H)]
                    rows.append((np.float64(r[_r101(x - 1, W)][k]) + np.float64(r[x][k])) + np.float64(r[_r101(x + 1, W)][k]))
                s.append(F32((rows[0] + rows[1]) + rows[2]))
            a, b, c = s[0] * F32(0.5), s[1], s[2] * F32(0.5)
            out[y, x] = (a + c) - np.sqrt(F32((a - c) * (a - c) + b * b))
    return out


# ------------------------------------------------------------------ threshold, 3x3 maximum, candidates
def candidates(e: np.ndarray, quality_level: float):
    """(M, thr, xy [n, 2] int32, val [n] f32) in raster order: steps 6-7."""
    H, W = e.shape
    M = F32(e.max())
    thr = F32(np.float64(M) * np.float64(quality_level))
    tv = np.where(e > thr, e, F32(0)).astype(F32)   # THRESH_TOZERO
    c = tv[1:-1, 1:-1]
    dil = c.copy()
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            np.maximum(dil, tv[dy:dy + H - 2, dx:dx + W - 2], out=dil)
    ys, xs = np.nonzero((c != 0) & (c == dil))
    xy = np.stack([xs + 1, ys + 1], 1).astype(np.int32)
    return M, thr, xy, e[ys + 1, xs + 1].astype(F32)


def rank(xy: np.ndarray, val: np.ndarray, W: int, higher_index_first=True) -> np.ndarray:
    """Step 8: descending value; equal values by raster index, the higher first (greaterThanPtr)."""
    idx = xy[:, 1].astype(np.int64) * W + xy[:, 0]
    return np.lexsort((idx if higher_index_first else -idx, np.asarray(val, F32)))[::-1].astype(np.int32)


# ------------------------------------------------------------------ the spacing, three ways
def select_brute(xy, order, min_distance: float, max_corners: int):
    """Step 9 as stated: (accepted indices into xy in acceptance order, ranks consumed)."""
    md2 = np.float64(min_distance) * np.float64(min_distance)
    ax = np.zeros(max(max_corners, 1), np.int64)
    ay = np.zeros(max(max_corners, 1), np.int64)
    out = []
    used = 0
    for i in order:
        if len(out) >= max_corners:
            break
        used += 1
        x, y = int(xy[i, 0]), int(xy[i, 1])
        m = len(out)
        if min_distance >= 1 and m:
            d2 = (ax[:m] - x) ** 2 + (ay[:m] - y) ** 2
            if np.any(d2.astype(np.float64) < md2):
                continue
        ax[m], ay[m] = x, y
        out.append(int(i))
    return np.array(out, np.int32), used


def select_grid(xy, order, W: int, H: int, min_distance: float, max_corners: int):
    """goodFeaturesToTrack's loop: a grid of cvRound(minDistance) cells, the 3 x 3 cells around a candidate
    searched.  min_distance >= 1 (below that OpenCV takes every candidate)."""
    assert min_distance >= 1
    cell = int(round(min_distance))   # cvRound: halves to even, as Python's round
    gw, gh = (W + cell - 1) // cell, (H + cell - 1) // cell
    grid = [[] for _ in range(gw * gh)]
    md2 = np.float64(min_distance) * np.float64(min_distance)
    out = []
    for i in order:
        x, y = int(xy[i, 0]), int(xy[i, 1])
        xc, yc = x // cell, y // cell
        good = True
        for yy in range(max(0, yc - 1), min(gh - 1, yc + 1) + 1):
            for xx in range(max(0, xc - 1), min(gw - 1, xc + 1) + 1):
                for (px, py) in grid[yy * gw + xx]:
                    dx, dy = F32(x) - F32(px), F32(y) - F32(py)   # Point2f arithmetic, exact on integers
                    if np.float64(dx * dx + dy * dy) < md2:
                        good = False
                        break
                if not good:
                    break
            if not good:
                break
        if good:
            grid[yc * gw + xc].append((x, y))
            out.append(int(i))
            if len(out) == max_corners:
                break
    return np.array(out, np.int32)


def select_rounds(xy, order, min_distance: float, max_corners: int):
    """The round-parallel form: a candidate is rejected once an accepted higher-ranked candidate lies within
    min_distance, accepted once no higher-ranked one within min_distance is undecided; rounds run until
    nothing is undecided.  The first max_corners accepted in rank order are kept.  Returns (indices, rounds)."""
    n = len(order)
    p = xy[order].astype(np.int64)
    if min_distance < 1:
        return np.asarray(order[:max_corners], np.int32), 0
    md2 = np.float64(min_distance) * np.float64(min_distance)
    d2 = (p[:, None, 0] - p[None, :, 0]) ** 2 + (p[:, None, 1] - p[None, :, 1]) ** 2
    near = (d2.astype(np.float64) < md2) & (np.arange(n)[None, :] < np.arange(n)[:, None])   # near[i, j]: j < i conflicts
    state = np.zeros(n, np.int8)   # 0 undecided, 1 accepted, 2 rejected
    rounds = 0
    while (state == 0).any():
        rounds += 1
        acc = near & (state == 1)[None, :]
        und = near & (state == 0)[None, :]
        has_acc, has_und = acc.any(1), und.any(1)
        new = state.copy()
        new[(state == 0) & has_acc] = 2
        new[(state == 0) & ~has_acc & ~has_und] = 1
        state = new
    return np.asarray(order, np.int32)[state == 1][:max_corners], rounds


# ------------------------------------------------------------------ the extractor
class Extractor:
    """Stateless from frame to frame."""

    def __init__(self, prm=None, W=640, H=480, pattern=None):
        self.prm = prm or params()
        self.W, self.H = W, H
        self.pattern = O.brief_default_pattern() if pattern is None else np.asarray(pattern, np.int8).reshape(256, 4)

    def detect(self, g: np.ndarray):
        """(keypoints before BRIEF, record): steps 2-10."""
        assert g.shape == (self.H, self.W)
        p = self.prm
        e = eig_map(g)
        M, thr, xy, val = candidates(e, p["quality_level"])
        order = rank(xy, val, self.W)
        sel, used = select_brute(xy, order, p["min_distance"], p["nfeatures"])
        kps = np.zeros(len(sel), KP)
        kps["x"], kps["y"], kps["size"], kps["angle"] = xy[sel, 0], xy[sel, 1], 3.0, -1.0
        kps["response"], kps["octave"], kps["class_id"] = 0.0, 0, -1
        return kps, dict(e=e, M=M, thr=thr, n_candidates=len(xy), corners=xy[sel].copy(), vals=val[sel].copy(), ranks=used)

    def detect_and_compute(self, g: np.ndarray):
        kps, rec = self.detect(np.ascontiguousarray(g))
        kps, desc = brief(g, kps, self.pattern)
        return kps, desc, rec

    def frame(self, bgr: np.ndarray, depth: np.ndarray, cam: dict):
        """Frame::Frame: gray, detectAndCompute, undistortKeyPoints + uprojectCamera (the oracle's)."""
        g = O.gray(bgr)
        kps, desc, rec = self.detect_and_compute(g)
        n = len(kps)
        kun = np.zeros(max(n, 1), KP)
        xyz = np.zeros((max(n, 1), 3), np.float32)
        oc = O.camera(cam)
        fn = O.lib().orc_frame_geometry
        fn.restype = None
        fn.argtypes = [O.kpp, C.c_int, O.u16p, C.c_int, C.POINTER(O.Camera), O.kpp, O.f32p]
        kin = np.ascontiguousarray(kps) if n else np.zeros(1, KP)
        fn(kin, n, np.ascontiguousarray(depth), depth.shape[1], C.byref(oc), kun, xyz)
        return dict(kps=kps, kps_un=kun[:n].copy(), desc=desc, xyz=xyz[:n].copy(), rec=rec)
