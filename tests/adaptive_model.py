"""CPU model of the adaptive FAST + BRIEF extractor, Extractor(FAST, BRIEF, ADAPTIVE) of the reference
(Features/Extractor.cpp:24-61, 82-109; DetectorAdjuster.cpp; VideoDynamicAdaptedFeatureDetector.cpp:24-44;
VideoGridAdaptedFeatureDetector.cpp:24-84), as DESIGN.md's "Adaptive FAST + BRIEF definition" states it.

Two formulations of one cell's detection:
  * literal: one cv::FAST (the oracle's orc_fast, called with the image's stride on the ROI) per try;
  * score map: the threshold-free score S = max(M, 1) - 1 once per frame, each ROI's strict 3x3 maxima, and
    the tries as counts of maxima with S >= t -- the form the device runs.
tests/test_adaptive_model.py holds them equal.  Everything else (keepStrongest's introselect, BRIEF-32) is
restated here and checked there against libstdc++ and the SVO oracle.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import oracle_lib as O

KP = O.KEYPOINT_DTYPE
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1),
        (-3, 0), (-3, 1), (-2, 2), (-1, 3)]   # (dx, dy), cv::FAST's 16-pixel ring in circular order


def params(nfeatures=1000, min_features=600, grid_rows=3, grid_cols=3, edge_threshold=31, iterations=5,
           init_thresh=20.0, min_thresh=2.0, max_thresh=10000.0, increase=1.3, decrease=0.7):
    return dict(nfeatures=nfeatures, min_features=min_features, grid_rows=grid_rows, grid_cols=grid_cols,
                edge_threshold=edge_threshold, iterations=iterations, init_thresh=float(init_thresh),
                min_thresh=float(min_thresh), max_thresh=float(max_thresh), increase=float(increase),
                decrease=float(decrease))


def derived(prm):
    """Extractor::createAdaptiveDetector :97-105 and VideoGridAdaptedFeatureDetector::detect :58, as the C++
    computes them: int maxFeatures = minFeatures * 1.7 (double), round(x / float(cells))."""
    cells = prm["grid_rows"] * prm["grid_cols"]
    max_features = int(prm["min_features"] * 1.7)
    f32 = np.float32

    def rnd(x):   # C round(): halves away from zero (x >= 0 here)
        return int(np.floor(np.float64(x) + 0.5))
    return dict(cells=cells, max_features=max_features, grid_min=rnd(f32(prm["min_features"]) / f32(cells)),
                grid_max=rnd(f32(max_features) / f32(cells)), max_per_cell=max_features // cells)


def rois(W, H, prm):
    """[(x0, y0, x1, y1)] row-major (VideoGridAdaptedFeatureDetector.cpp:62-69)."""
    r, c, e = prm["grid_rows"], prm["grid_cols"], prm["edge_threshold"]
    out = []
    for i in range(r):
        y0, y1 = max(i * H // r - e, 0), min(H, (i + 1) * H // r + e)
        for j in range(c):
            x0, x1 = max(j * W // c - e, 0), min(W, (j + 1) * W // c + e)
            out.append((x0, y0, x1, y1))
    return out


def clamp_t(thresh: float) -> int:
    """FastFeatureDetector::create((int)mThresh), cv::FAST's clamp to [0, 255]."""
    return min(max(int(thresh), 0), 255)


# ------------------------------------------------------------------ one cell's corners, two ways
def fast_literal(g: np.ndarray, roi, t: int) -> np.ndarray:
    """cv::FAST on the ROI as an image of its own: (x, y, score) in ROI coordinates, raster order."""
    H, W = g.shape
    x0, y0, x1, y1 = roi
    flat = g.reshape(-1)[y0 * W + x0:]
    cap = (x1 - x0) * (y1 - y0)
    out = np.zeros(cap * 3, np.int32)
    n = O.lib().orc_fast(flat, W, x1 - x0, y1 - y0, int(t), out, cap)
    return out[:3 * n].reshape(n, 3).copy()


def score_map(g: np.ndarray) -> np.ndarray:
    """S = max(M, 1) - 1 where the ring lies in the image, else 0; M = the largest, over the 16 arcs of 9
    ring pixels and both polarities, of the arc's smallest difference to the centre."""
    H, W = g.shape
    out = np.zeros((H, W), np.uint8)
    if H < 7 or W < 7:
        return out
    gi = g.astype(np.int16)
    v = gi[3:H - 3, 3:W - 3]
    d = np.stack([gi[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] - v for dx, dy in RING])
    d = np.concatenate([d, d[:8]])
    mn, mx = d[0:16].copy(), d[0:16].copy()
    for j in range(1, 9):
        np.minimum(mn, d[j:j + 16], out=mn)
        np.maximum(mx, d[j:j + 16], out=mx)
    M = np.maximum(mn.max(0), (-mx).max(0))
    out[3:H - 3, 3:W - 3] = (np.maximum(M, 1) - 1).astype(np.uint8)
    return out


def roi_maxima(S: np.ndarray, roi) -> np.ndarray:
    """The ROI's strict 3x3 maxima of S with S >= 1, (x, y, score) in ROI coordinates, raster order; scores
    outside the ROI's scan range [3, w-3) x [3, h-3) count as 0."""
    x0, y0, x1, y1 = roi
    w, h = x1 - x0, y1 - y0
    P = np.zeros((h + 2, w + 2), np.int16)
    P[4:h - 2, 4:w - 2] = S[y0 + 3:y1 - 3, x0 + 3:x1 - 3]
    c = P[1:-1, 1:-1]
    ok = c >= 1
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if dy != 1 or dx != 1:
                ok &= c > P[dy:dy + h, dx:dx + w]
    ys, xs = np.nonzero(ok)
    return np.stack([xs, ys, c[ys, xs]], 1).astype(np.int32)


def fast_from_maxima(mx: np.ndarray, t: int) -> np.ndarray:
    return mx[mx[:, 2] >= max(int(t), 1)]


# ------------------------------------------------------------------ keepStrongest: libstdc++'s introselect
def _adjust_heap(r, ix, first, hole, length, vr, vi):
    top, child = hole, hole
    while child < (length - 1) // 2:
        child = 2 * (child + 1)
        if r[first + child] > r[first + child - 1]:
            child -= 1
        r[first + hole], ix[first + hole] = r[first + child], ix[first + child]
        hole = child
    if (length & 1) == 0 and child == (length - 2) // 2:
        child = 2 * (child + 1)
        r[first + hole], ix[first + hole] = r[first + child - 1], ix[first + child - 1]
        hole = child - 1
    parent = (hole - 1) // 2
    while hole > top and r[first + parent] > vr:
        r[first + hole], ix[first + hole] = r[first + parent], ix[first + parent]
        hole = parent
        parent = (hole - 1) // 2
    r[first + hole], ix[first + hole] = vr, vi


def _swap(r, ix, a, b):
    r[a], r[b] = r[b], r[a]
    ix[a], ix[b] = ix[b], ix[a]


def _heap_select(r, ix, first, middle, last):
    length = middle - first
    if length >= 2:
        parent = (length - 2) // 2
        while True:
            _adjust_heap(r, ix, first, parent, length, r[first + parent], ix[first + parent])
            if parent == 0:
                break
            parent -= 1
    for i in range(middle, last):
        if r[i] > r[first]:
            vr, vi = r[i], ix[i]
            r[i], ix[i] = r[first], ix[first]
            _adjust_heap(r, ix, first, 0, length, vr, vi)


def _median_to_first(r, ix, result, a, b, c):
    if r[a] > r[b]:
        if r[b] > r[c]:
            _swap(r, ix, result, b)
        elif r[a] > r[c]:
            _swap(r, ix, result, c)
        else:
            _swap(r, ix, result, a)
    elif r[a] > r[c]:
        _swap(r, ix, result, a)
    elif r[b] > r[c]:
        _swap(r, ix, result, c)
    else:
        _swap(r, ix, result, b)


def _insertion_sort(r, ix, f, l):
    for i in range(f + 1, l):
        vr, vi = r[i], ix[i]
        j = i
        if vr > r[f]:
            while j > f:
                r[j], ix[j] = r[j - 1], ix[j - 1]
                j -= 1
        else:
            while vr > r[j - 1]:
                r[j], ix[j] = r[j - 1], ix[j - 1]
                j -= 1
        r[j], ix[j] = vr, vi


def nth_element(resp, nth: int, depth_limit: int = -1) -> np.ndarray:
    """std::nth_element(begin, begin + nth, end, a.response > b.response) (libstdc++ __introselect): the
    permutation it leaves, as original indices.  depth_limit < 0: 2 * lg(n)."""
    r = [float(x) for x in np.asarray(resp, np.float32)]
    n = len(r)
    ix = list(range(n))
    if n == 0 or nth >= n:
        return np.array(ix, np.int32)
    first, last = 0, n
    depth = depth_limit if depth_limit >= 0 else 2 * (n.bit_length() - 1)
    while last - first > 3:
        if depth == 0:
            _heap_select(r, ix, first, nth + 1, last)
            _swap(r, ix, first, nth)
            return np.array(ix, np.int32)
        depth -= 1
        mid = first + (last - first) // 2
        _median_to_first(r, ix, first, first + 1, mid, last - 1)
        lo, hi, p = first + 1, last, r[first]   # __unguarded_partition(first + 1, last, first)
        while True:
            while r[lo] > p:
                lo += 1
            hi -= 1
            while p > r[hi]:
                hi -= 1
            if not lo < hi:
                break
            _swap(r, ix, lo, hi)
            lo += 1
        if lo <= nth:
            first = lo
        else:
            last = lo
    _insertion_sort(r, ix, first, last)
    return np.array(ix, np.int32)


def keep_strongest(resp, N: int, depth_limit: int = -1) -> np.ndarray:
    """keepStrongest(N, keypoints) (VideoGridAdaptedFeatureDetector.cpp:24-31): indices kept, in order."""
    n = len(resp)
    if n <= N:
        return np.arange(n, dtype=np.int32)
    return nth_element(resp, N, depth_limit)[:N]


# ------------------------------------------------------------------ the threshold loop of one cell and frame
def cell_detect(count_at, thresh: float, prm, drv):
    """VideoDynamicAdaptedFeatureDetector::detect with DetectorAdjuster's tooFew / tooMany / good.
    count_at(t) = the number of corners cv::FAST finds at integer threshold t.  Returns (threshold used,
    tries, threshold after, branch of the last try: 'few' | 'many' | 'ok')."""
    it = prm["iterations"]
    tries = 0
    while True:
        t = clamp_t(thresh)
        n = count_at(t)
        tries += 1
        if n < drv["grid_min"]:
            thresh = thresh * prm["decrease"]
            if thresh < prm["min_thresh"]:
                thresh = prm["min_thresh"]
            branch = "few"
        elif n > drv["grid_max"]:
            thresh = thresh * prm["increase"]
            if thresh > prm["max_thresh"]:
                thresh = prm["max_thresh"]
            branch = "many"
            break
        else:
            branch = "ok"
            break
        it -= 1
        if not (it > 0 and prm["min_thresh"] < thresh < prm["max_thresh"]):
            break
    return t, tries, thresh, branch


# ------------------------------------------------------------------ BRIEF-32 (as "SVO + BRIEF definition")
def box_sums(g: np.ndarray) -> np.ndarray:
    """9x9 window sums (the integral image's four-corner differences), valid where the window fits."""
    H, W = g.shape
    ii = np.zeros((H + 1, W + 1), np.int64)
    ii[1:, 1:] = np.cumsum(np.cumsum(g.astype(np.int64), 0), 1)
    out = np.zeros((H, W), np.int64)
    out[4:H - 4, 4:W - 4] = ii[9:, 9:] - ii[9:, :-9] - ii[:-9, 9:] + ii[:-9, :-9]
    return out


def brief(g: np.ndarray, kps: np.ndarray, pattern: np.ndarray):
    """runByImageBorder(28) then pixelTests32: returns (kept keypoints, descriptors)."""
    H, W = g.shape
    b = 28
    if H <= 2 * b or W <= 2 * b:
        return kps[:0].copy(), np.zeros((0, 32), np.uint8)
    keep = (kps["x"] >= b) & (kps["x"] < W - b) & (kps["y"] >= b) & (kps["y"] < H - b)
    kps = kps[keep].copy()
    box = box_sums(g)
    x = (kps["x"] + np.float32(0.5)).astype(np.int32)
    y = (kps["y"] + np.float32(0.5)).astype(np.int32)
    p = np.asarray(pattern, np.int8).reshape(256, 4).astype(np.int32)
    a = box[y[:, None] + p[None, :, 0], x[:, None] + p[None, :, 1]]
    c = box[y[:, None] + p[None, :, 2], x[:, None] + p[None, :, 3]]
    return kps, np.packbits(a < c, axis=1)


# ------------------------------------------------------------------ the extractor
class Extractor:
    """Stateful: thresholds[cell] (f64) carry from frame to frame."""

    def __init__(self, prm=None, W=640, H=480, literal=False, pattern=None):
        self.prm = prm or params()
        p = self.prm
        assert p["min_thresh"] >= 1 and p["min_thresh"] <= p["init_thresh"] <= p["max_thresh"]
        self.drv = derived(p)
        self.W, self.H = W, H
        self.rois = rois(W, H, p)
        self.thresholds = np.full(self.drv["cells"], p["init_thresh"], np.float64)
        self.literal = literal
        self.pattern = O.brief_default_pattern() if pattern is None else np.asarray(pattern, np.int8).reshape(256, 4)
        self.max_stored = 0   # most maxima with S >= (int)min_thresh any cell has held (the device's cell_cap)

    def detect(self, g: np.ndarray):
        """VideoGridAdaptedFeatureDetector::detect + retainBest: (keypoints before BRIEF, per-cell record)."""
        assert g.shape == (self.H, self.W)
        p, drv = self.prm, self.drv
        S = None if self.literal else score_map(g)
        tmin = max(1, int(p["min_thresh"]))
        cells, parts = [], []
        for k, roi in enumerate(self.rois):
            before = float(self.thresholds[k])
            if self.literal:
                cache = {}

                def corners(t, roi=roi, cache=cache):
                    if t not in cache:
                        cache[t] = fast_literal(g, roi, t)
                    return cache[t]
                stored = None
            else:
                mx = roi_maxima(S, roi)
                stored = int(np.count_nonzero(mx[:, 2] >= tmin))
                self.max_stored = max(self.max_stored, stored)

                def corners(t, mx=mx):
                    return fast_from_maxima(mx, t)
            used, tries, after, branch = cell_detect(lambda t: len(corners(t)), before, p, drv)
            self.thresholds[k] = after
            raster = corners(used)
            kept = raster[keep_strongest(raster[:, 2].astype(np.float32), drv["max_per_cell"])]
            cells.append(dict(before=before, used=used, tries=tries, after=after, branch=branch, raster=raster, kept=kept,
                              stored=stored))
            parts.append(kept + np.array([roi[0], roi[1], 0], np.int32))
        allk = np.concatenate(parts) if parts else np.zeros((0, 3), np.int32)
        total = len(allk)
        if total > p["nfeatures"]:
            allk = allk[O.retain_best(allk[:, 2].astype(np.float32), p["nfeatures"])]
        kps = np.zeros(len(allk), KP)
        kps["x"], kps["y"], kps["size"], kps["angle"] = allk[:, 0], allk[:, 1], 7.0, -1.0
        kps["response"], kps["octave"], kps["class_id"] = allk[:, 2], 0, -1
        return kps, dict(cells=cells, total=total)

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
