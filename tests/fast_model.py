"""CPU model of the plain FAST extractor, Extractor(FAST, BRIEF, NORMAL) and Extractor(FAST, ORB, NORMAL) of the
reference (Features/Extractor.cpp:50-61, 168-171, 216-218, 224-226), as DESIGN.md's "Plain FAST definition" states it.

The detector in the device's form: the strict 3x3 maxima of the threshold-free score map S = max(M, 1) - 1 with
S >= t over the whole image (adaptive_model.score_map / roi_maxima), which tests/test_fast_model.py holds equal to
the oracle's cv::FAST.  retainBest is adaptive_model.nth_element plus the partition on >= the boundary response,
restated here and checked there against libstdc++.  BRIEF is adaptive_model.brief; the ORB branch is
cv::ORB::compute()'s provided-keypoints path with cvorb_model's pieces (border 31, the oracle's blur, rbrief at the
stored angle).  Parity with OpenCV itself is unpinned, as for the other extractors: OpenCV is not available here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import adaptive_model as A
import oracle_lib as O

KP = O.KEYPOINT_DTYPE
BRIEF_BORDER, ORB_BORDER = 28, 31


def params(nfeatures=1000, threshold=10, descriptor="brief"):
    assert descriptor in ("brief", "orb") and 1 <= threshold <= 255 and nfeatures >= 1
    return dict(nfeatures=nfeatures, threshold=threshold, descriptor=descriptor)


def corners(g: np.ndarray, t: int) -> np.ndarray:
    """cv::FAST(g, t, true, TYPE_9_16): (x, y, score) in raster order."""
    H, W = g.shape
    return A.fast_from_maxima(A.roi_maxima(A.score_map(g), (0, 0, W, H)), t)


def retain_best(resp, n_points: int, depth_limit: int = -1) -> np.ndarray:
    """cv::KeyPointsFilter::retainBest (OpenCV 3.4): the kept original indices in the order it leaves them."""
    r = np.asarray(resp, np.float32)
    n = len(r)
    if n_points < 0 or n <= n_points:
        return np.arange(n, dtype=np.int32)
    if n_points == 0:
        return np.zeros(0, np.int32)
    ix = [int(i) for i in A.nth_element(r, n_points - 1, depth_limit)]
    amb = r[ix[n_points - 1]]
    # std::partition(begin + n_points, end, response >= amb): forward-iterator form is not used for vectors; the
    # bidirectional one swaps the first failing element from the left with the last passing one from the right
    lo, hi = n_points, n
    while True:
        while lo != hi and r[ix[lo]] >= amb:
            lo += 1
        if lo == hi:
            break
        hi -= 1
        while lo != hi and not r[ix[hi]] >= amb:
            hi -= 1
        if lo == hi:
            break
        ix[lo], ix[hi] = ix[hi], ix[lo]
        lo += 1
    return np.array(ix[:lo], np.int32)


def orb_describe(g: np.ndarray, kps: np.ndarray):
    """cv::ORB::create()->compute(g, kps): runByImageBorder(31) on cvRound of the points, one level (every octave is
    0, so no regrouping), the blur, the steered tests at each keypoint's own angle.  Keypoint fields pass through."""
    import cvorb_model as CV
    H, W = g.shape
    keep = CV.border_filter(CV.cv_round(kps["x"]), CV.cv_round(kps["y"]), W, H, ORB_BORDER)
    kps = kps[keep].copy()
    desc = np.zeros((len(kps), 32), np.uint8)
    if len(kps):
        blurred = O.blur(np.ascontiguousarray(g))
        for i, k in enumerate(kps):
            desc[i] = CV.rbrief(blurred, int(CV.cv_round(k["x"])), int(CV.cv_round(k["y"])), k["angle"])
    return kps, desc


class Extractor:
    """Stateless from frame to frame."""

    def __init__(self, prm=None, pattern=None):
        self.prm = prm or params()
        self.pattern = O.brief_default_pattern() if pattern is None else np.asarray(pattern, np.int8).reshape(256, 4)

    def detect(self, g: np.ndarray):
        """(keypoints before the descriptor's border filter, dict(raster = cv::FAST's corners, kept = indices))."""
        p = self.prm
        raster = corners(g, p["threshold"])
        kept = np.arange(len(raster), dtype=np.int32)
        if len(raster) > p["nfeatures"]:   # Extractor::detectAndCompute :56-57
            kept = retain_best(raster[:, 2].astype(np.float32), p["nfeatures"])
        sel = raster[kept]
        kps = np.zeros(len(sel), KP)
        kps["x"], kps["y"], kps["size"], kps["angle"] = sel[:, 0], sel[:, 1], 7.0, -1.0
        kps["response"], kps["octave"], kps["class_id"] = sel[:, 2], 0, -1
        return kps, dict(raster=raster, kept=kept)

    def detect_and_compute(self, g: np.ndarray):
        g = np.ascontiguousarray(g)
        kps, rec = self.detect(g)
        if self.prm["descriptor"] == "orb":
            kps, desc = orb_describe(g, kps)
        else:
            kps, desc = A.brief(g, kps, self.pattern)
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
