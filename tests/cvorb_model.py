"""CPU model of the OpenCV ORB extractor, Extractor(ORB, ORB, NORMAL) of the reference (Features/Extractor.cpp:50-61,
163-166, 216-218: cv::ORB::create(nfeatures, scaleFactor, nlevels) as detector, cv::ORB::create() as descriptor), as
DESIGN.md's "OpenCV ORB definition" states it: OpenCV 3.4's orb.cpp restated (pyramid, whole-level cv::FAST,
runByImageBorder, retainBest(2 N) on the FAST score, the Harris response, retainBest(N), IC_Angle, the frame-level
retainBest, then the provided-keypoints compute path with the steered BRIEF of bit_pattern_31_).  This file is the
definition's executable form; the device (csrc/cvorb.hip) is held to it bit for bit by tests/test_gpu_cvorb.py.

The pyramid, cv::FAST, the blur, fastAtan2, the f32 cos / sin pair and retainBest are the oracle's (oracle_lib);
tests/test_cvorb_model.py holds the parts restated here (budgets, Harris, angle, rBRIEF) to independent forms.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

import oracle_lib as O

KP = O.KEYPOINT_DTYPE
F32 = np.float32
HARRIS_K = F32(0.04)
PATCH = 31
HALF_PATCH = 15
DESC_BORDER = 31           # cv::ORB::create()'s edgeThreshold: the descriptor side's runByImageBorder
_SC = F32(1.0) / (F32(4 * 7) * F32(255.0))
SSQ = _SC * _SC * _SC * _SC    # f32, left to right


def params(nfeatures=1000, scale_factor=1.2, nlevels=8, edge_threshold=31, fast_threshold=20):
    return dict(nfeatures=int(nfeatures), scale_factor=float(F32(scale_factor)), nlevels=int(nlevels),
                edge_threshold=int(edge_threshold), fast_threshold=int(fast_threshold))


def cv_round(v):
    """cvRound: to nearest, halves to even."""
    return np.rint(v).astype(np.int64)


def layer_scales(scale_factor: float, nlevels: int) -> np.ndarray:
    """layerScale[l] = (float)pow((double)scale_factor, (double)l), scale_factor held as a float."""
    sf = float(F32(scale_factor))
    return np.array([F32(sf ** float(l)) for l in range(nlevels)], F32)


def level_sizes(W: int, H: int, ls: np.ndarray):
    """(w, h) per level: cvRound of the f32 quotient."""
    return [(int(cv_round(F32(W) / s)), int(cv_round(F32(H) / s))) for s in ls]


def budgets(nfeatures: int, scale_factor: float, nlevels: int) -> list:
    """Step 2: the per-level keypoint budgets N_l (f32 arithmetic, the power in f64)."""
    factor = F32(1.0 / float(F32(scale_factor)))
    nd = F32(nfeatures) * (F32(1) - factor) / (F32(1) - F32(float(factor) ** float(nlevels)))
    out, total = [], 0
    for _ in range(nlevels - 1):
        out.append(int(cv_round(nd)))
        total += out[-1]
        nd = F32(nd * factor)
    out.append(max(nfeatures - total, 0))
    return out


def border_filter(xs, ys, w: int, h: int, e: int) -> np.ndarray:
    """runByImageBorder((w, h), e) on integer positions: the kept mask (an image of at most 2 e px keeps nothing)."""
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    if w <= 2 * e or h <= 2 * e:
        return np.zeros(len(xs), bool)
    return (xs >= e) & (xs < w - e) & (ys >= e) & (ys < h - e)


def retain_best(resp: np.ndarray, n_points: int) -> np.ndarray:
    """KeyPointsFilter::retainBest: the kept elements' indices in the order it leaves them (libstdc++'s)."""
    n = len(resp)
    if n <= n_points:
        return np.arange(n, dtype=np.int32)
    if n_points == 0:
        return np.zeros(0, np.int32)
    return O.retain_best(np.asarray(resp, F32), n_points)


# ------------------------------------------------------------------ the Harris response
def harris(img: np.ndarray, xs, ys) -> np.ndarray:
    """Step 6, vectorised: f32 responses at integer positions at least 4 px inside the image."""
    P = img.astype(np.int64)
    H, W = P.shape
    Ix = np.zeros((H, W), np.int64)
    Iy = np.zeros((H, W), np.int64)
    Ix[1:-1, 1:-1] = (P[1:-1, 2:] - P[1:-1, :-2]) * 2 + (P[:-2, 2:] - P[:-2, :-2]) + (P[2:, 2:] - P[2:, :-2])
    Iy[1:-1, 1:-1] = (P[2:, 1:-1] - P[:-2, 1:-1]) * 2 + (P[2:, :-2] - P[:-2, :-2]) + (P[2:, 2:] - P[:-2, 2:])
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    assert len(xs) == 0 or (xs.min() >= 4 and ys.min() >= 4 and xs.max() < W - 4 and ys.max() < H - 4)
    d = np.arange(-3, 4)
    yy = ys[:, None, None] + d[None, :, None]
    xx = xs[:, None, None] + d[None, None, :]
    gx, gy = Ix[yy, xx], Iy[yy, xx]
    a = (gx * gx).sum((1, 2)).astype(np.int32)
    b = (gy * gy).sum((1, 2)).astype(np.int32)
    c = (gx * gy).sum((1, 2)).astype(np.int32)
    return harris_from_sums(a, b, c)


def harris_from_sums(a, b, c) -> np.ndarray:
    """((float)a (float)b - (float)c (float)c - 0.04f ((float)a + (float)b) ((float)a + (float)b)) ssq, left to right."""
    fa, fb, fc = np.asarray(a).astype(F32), np.asarray(b).astype(F32), np.asarray(c).astype(F32)
    s = fa + fb
    return ((fa * fb - fc * fc) - (HARRIS_K * s) * s) * SSQ


def harris_literal(img: np.ndarray, x0: int, y0: int) -> np.float32:
    """Step 6 as the triple loop states it."""
    a = b = c = 0
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            def p(oy, ox):
                return int(img[y0 + dy + oy, x0 + dx + ox])
            ix = (p(0, 1) - p(0, -1)) * 2 + (p(-1, 1) - p(-1, -1)) + (p(1, 1) - p(1, -1))
            iy = (p(1, 0) - p(-1, 0)) * 2 + (p(1, -1) - p(-1, -1)) + (p(1, 1) - p(-1, 1))
            a += ix * ix
            b += iy * iy
            c += ix * iy
    return harris_from_sums(np.int32(a), np.int32(b), np.int32(c))[()]


# ------------------------------------------------------------------ angle and steered BRIEF
_UMAX = None
_DISK = None
_PATTERN = None


def umax() -> np.ndarray:
    global _UMAX
    if _UMAX is None:
        _UMAX = O.tables(O.orb_params(1000))["umax"].copy()
    return _UMAX


def _disk():
    global _DISK
    if _DISK is None:
        um = umax()
        v, u = np.mgrid[-HALF_PATCH:HALF_PATCH + 1, -HALF_PATCH:HALF_PATCH + 1]
        inside = np.abs(u) <= um[np.abs(v)]
        _DISK = ((u * inside).astype(np.int64), (v * inside).astype(np.int64))
    return _DISK


def ic_angle(img: np.ndarray, x: int, y: int) -> np.float32:
    """IC_Angle: integer moments over the radius-15 disk, then the oracle's fastAtan2 (degrees)."""
    U, V = _disk()
    patch = img[y - HALF_PATCH:y + HALF_PATCH + 1, x - HALF_PATCH:x + HALF_PATCH + 1].astype(np.int64)
    m10, m01 = int((U * patch).sum()), int((V * patch).sum())
    fn = O.lib().orc_fast_atan2
    return F32(fn(F32(m01), F32(m10)))


def pattern() -> np.ndarray:
    """bit_pattern_31_ as [256, 4] f32 (x0, y0, x1, y1): the data table the oracle and the device include."""
    global _PATTERN
    if _PATTERN is None:
        txt = open(os.path.join(O.ROOT, "rgbd-slam_amd", "csrc", "orb_pattern.inc")).read()
        nums = [int(v) for v in re.findall(r"-?\d+", "\n".join(l for l in txt.splitlines() if not l.startswith("//")))]
        assert len(nums) == 1024
        _PATTERN = np.array(nums, F32).reshape(256, 4)
    return _PATTERN


FACTOR_PI = F32(np.pi / 180.0)   # (float)(CV_PI / 180.f)


def rbrief(blurred: np.ndarray, cx: int, cy: int, angle_deg) -> np.ndarray:
    """The 256 steered tests around (cx, cy) of the blurred level: 32 bytes."""
    co, si = C.c_float(0), C.c_float(0)
    O.lib().orc_cos_sin(F32(F32(angle_deg) * FACTOR_PI), C.byref(co), C.byref(si))
    a, b = F32(co.value), F32(si.value)
    pt = pattern()
    v = []
    for k in (0, 2):
        X, Y = pt[:, k], pt[:, k + 1]
        r = cv_round(X * b + Y * a)
        c = cv_round(X * a - Y * b)
        v.append(blurred[cy + r, cx + c].astype(np.int32))
    bits = (v[0] < v[1]).astype(np.uint8).reshape(32, 8)
    return (bits << np.arange(8, dtype=np.uint8)).sum(1).astype(np.uint8)


# ------------------------------------------------------------------ the extractor
class Extractor:
    """Stateless from frame to frame."""

    def __init__(self, prm=None, W=640, H=480):
        self.prm = prm or params()
        self.W, self.H = W, H
        p = self.prm
        self.ls = layer_scales(p["scale_factor"], p["nlevels"])
        self.sizes = level_sizes(W, H, self.ls)
        self.N = budgets(p["nfeatures"], p["scale_factor"], p["nlevels"])
        self.orb = O.orb_params(p["nfeatures"], p["scale_factor"], p["nlevels"])
        t = O.tables(self.orb, W, H)
        assert self.sizes == [(int(a), int(b)) for a, b in zip(t["w"], t["h"])], "cv::ORB level sizes differ from the pyramid's"

    def detect_level(self, img: np.ndarray, l: int):
        """Steps 3-7 on one level: dict(n_fast, s1 [n1, 3] (x, y, score), h1 [n1] f32, s2 [n2, 3], h2 [n2] f32)."""
        p = self.prm
        h, w = img.shape
        e, N = p["edge_threshold"], self.N[l]
        k = O.fast(img, p["fast_threshold"])
        k = k[border_filter(k[:, 0], k[:, 1], w, h, e)]
        s1 = k[retain_best(k[:, 2].astype(F32), 2 * N)]
        h1 = harris(img, s1[:, 0], s1[:, 1]) if len(s1) else np.zeros(0, F32)
        o2 = retain_best(h1, N)
        return dict(n_fast=len(k), s1=s1, h1=h1, s2=s1[o2], h2=h1[o2])

    def detect(self, g: np.ndarray):
        """Steps 1-10: (keypoints with level positions, record).  Returns (kps, lx, ly, levels, rec)."""
        assert g.shape == (self.H, self.W)
        p = self.prm
        levels = O.pyramid(np.ascontiguousarray(g), self.orb)
        recs = [self.detect_level(levels[l], l) for l in range(p["nlevels"])]
        n = sum(len(r["s2"]) for r in recs)
        kps = np.zeros(n, KP)
        lx, ly = np.zeros(n, np.int64), np.zeros(n, np.int64)
        o = 0
        for l, r in enumerate(recs):
            m = len(r["s2"])
            sl = slice(o, o + m)
            lx[sl], ly[sl] = r["s2"][:, 0], r["s2"][:, 1]
            kps["x"][sl] = r["s2"][:, 0].astype(F32) * self.ls[l]
            kps["y"][sl] = r["s2"][:, 1].astype(F32) * self.ls[l]
            kps["size"][sl] = F32(PATCH) * self.ls[l]
            kps["angle"][sl] = [ic_angle(levels[l], int(x), int(y)) for x, y in r["s2"][:, :2]]
            kps["response"][sl] = r["h2"]
            kps["octave"][sl] = l
            o += m
        kps["class_id"] = -1
        frame_retain = n > p["nfeatures"]
        if frame_retain:   # Extractor::detectAndCompute :56-57
            o = retain_best(kps["response"], p["nfeatures"])
            kps, lx, ly = kps[o], lx[o], ly[o]
        rec = dict(levels=recs, total=n, frame_retain=frame_retain, n_detect=len(kps))
        return kps, lx, ly, levels, rec

    def detect_and_compute(self, g: np.ndarray):
        """Steps 1-11: (keypoints, descriptors, record)."""
        kps, lx, ly, levels, rec = self.detect(g)
        keep = border_filter(cv_round(kps["x"]), cv_round(kps["y"]), self.W, self.H, DESC_BORDER)
        kps, lx, ly = kps[keep], lx[keep], ly[keep]
        oc = kps["octave"]
        rec["regroup"] = bool(np.any(oc[1:] < oc[:-1]))
        if rec["regroup"]:
            o = np.argsort(oc, kind="stable")
            kps, lx, ly = kps[o], lx[o], ly[o]
        desc = np.zeros((len(kps), 32), np.uint8)
        blurred = {}
        for i, k in enumerate(kps):
            l = int(k["octave"])
            if l not in blurred:
                blurred[l] = O.blur(levels[l])
            s = F32(1.0) / self.ls[l]
            cx, cy = int(cv_round(k["x"] * s)), int(cv_round(k["y"] * s))
            assert (cx, cy) == (lx[i], ly[i])   # form (b): the centre is the level position
            desc[i] = rbrief(blurred[l], cx, cy, k["angle"])
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
