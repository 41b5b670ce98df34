"""Seeded inputs (test infrastructure), one per edge regime of the three newest extraction front ends:
Extractor::ADAPTIVE (csrc/adaptive.hip), Extractor::GFTT (csrc/gftt.hip) and Extractor::ORB (csrc/cvorb.hip).  Frame
shapes whose score / eigenvalue tiles are partial in x and y, a tile row one pixel high, x >= 1024 in the packed keys;
GFTT frames with one candidate, none (M == +0 from textured input), all-tied candidates, every corner dropped by BRIEF's
border; adaptive grids at the 7 x 7 ROI minimum, thresholds walking to cv::FAST's 255 clamp and back down to
min_thresh, cell_cap and nfeatures on their boundaries; cv::ORB levels with a zero budget, fewer rows than list strips,
one 16-px segment, the first segment on both sides of a 16 boundary, fast_threshold 1 / 254 / 255, saturated scores, and
n_fast / len(s1) on retainBest's boundaries.

case(name) returns a dict: ext ("gftt" | "adaptive" | "cvorb"), W, H, prm (the model's parameters), dev (device-only
parameters: cand_cap, cell_cap, max_keypoints), bgr [B, H, W, 3], depth [B, H, W], cam, flag (the frames expected to
raise the capacity flag: index -> fragment of the error), after (a frame extracted on its own after the batch, or None)
and regime.  model(name) runs the CPU model over the case once per session and keeps the result:
tests/test_extractor_edge_cases.py asserts from it that each case reaches its regime, tests/test_gpu_extractor_edges.py
holds the device to it.  Natural images are the fr1 synthetic frame tiled and cropped (svo_edge_cases.images); the
patterns are numpy from fixed seeds."""
import functools

import numpy as np

import svo_edge_cases as S

GFTT, ADAPTIVE, CVORB = "gftt", "adaptive", "cvorb"
CVORB_CAND_CAP = 12288      # the largest: level 0 at fast_threshold 1 holds more corners than the default 8192


# ------------------------------------------------------------------ images
def pattern(kind, W, H, seed=0):
    """A gray image [H, W] u8."""
    y, x = np.mgrid[0:H, 0:W]
    if kind == "flat":
        g = np.full((H, W), 128)
    elif kind == "pixel":            # one bright pixel on black
        g = np.zeros((H, W))
        g[H // 2, W // 2] = 255
    elif kind == "stripes45":
        g = ((x + y) // 4 % 2) * 255
    elif kind == "xramp":
        g = np.minimum(2 * x, 255)
    elif kind == "vstripes":
        g = (x // 4 % 2) * 255
    elif kind == "checker1":
        g = ((x + y) % 2) * 255
    elif kind == "checker8":
        g = ((x // 8 + y // 8) % 2) * 255
    elif kind == "noise":            # uniform noise
        g = np.random.RandomState(seed).randint(0, 256, size=(H, W))
    elif kind == "binary":           # 0 / 255 noise: every FAST corner scores 254
        g = np.random.RandomState(seed).randint(0, 2, size=(H, W)) * 255
    elif kind == "tiles16":          # a 16 x 16 block of 0 / 255 noise repeated: scores and Harris responses tie exactly
        blk = np.random.RandomState(seed).randint(0, 2, size=(16, 16)) * 255
        g = np.tile(blk, (H // 16 + 1, W // 16 + 1))[:H, :W]
    elif kind == "rim":              # noise within 24 px of the frame's edge, flat inside: BRIEF's border (28) drops all
        g = np.full((H, W), 128)
        n = np.random.RandomState(seed).randint(0, 256, size=(H, W))
        rim = (x < 24) | (x >= W - 24) | (y < 24) | (y >= H - 24)
        g[rim] = n[rim]
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(g.astype(np.uint8))


def gray3(g):
    """A BGR frame whose gray image is g."""
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


def image(spec, W, H):
    """(bgr, depth) of one frame: ("nat", shift) is the natural image cropped at column shift, (kind, seed) a pattern
    (over the natural image's depth)."""
    kind, arg = spec
    bgr, depth, _ = S.images(W, H, arg if kind == "nat" else 0)
    if kind != "nat":
        bgr = gray3(pattern(kind, W, H, arg))
    return bgr, depth


NAT = (("nat", 0),)

# ------------------------------------------------------------------ the case table
# name -> (extractor, W, H, frames, model parameter overrides, device parameters, flagged frames, after, regime)
_T = {}


def _add(name, ext, W, H, frames=NAT, over=None, dev=None, flag=None, after=None, regime=""):
    assert name not in _T and regime
    _T[name] = (ext, W, H, tuple(frames), dict(over or {}), dict(dev or {}), dict(flag or {}), after, regime)


# ---- shapes, all three extractors (W % 16 == 0, W >= 64, 64 < H <= 2 W, sides <= 2047: what the geometry accepts)
_SHAPE_REGIMES = {
    (368, 239): "W = 5 * 64 + 48, H = 14 * 16 + 15 = 7 * 32 + 15 = 59 * 4 + 3: partial tiles in x and y, an odd height",
    (400, 481): "W = 6 * 64 + 16, H = 30 * 16 + 1 = 15 * 32 + 1: a tile row one pixel high, whose REFLECT_101 partner "
                "H - 2 lies in the tile above",
    (336, 241): "a second one-row tile, with a 16-px last tile column",
    (2032, 239): "x >= 1024 in gftt_near's 11-bit fields and in adp_pack; 32 tiles across",
}
for (_w, _h), _r in _SHAPE_REGIMES.items():
    _add("gftt_%dx%d" % (_w, _h), GFTT, _w, _h, regime=_r)
    if (_w, _h) != (336, 241):
        _add("adaptive_%dx%d" % (_w, _h), ADAPTIVE, _w, _h, regime=_r)
_add("cvorb_368x239", CVORB, 368, 239, over=dict(nlevels=4), regime=_SHAPE_REGIMES[(368, 239)] + "; 4 levels")
_add("cvorb_400x481", CVORB, 400, 481, regime=_SHAPE_REGIMES[(400, 481)])
_add("gftt_noise_368x239", GFTT, 368, 239, [("noise", 31)],
     regime="candidates on the rows and columns next to every border (x = 1, y = 1, x = W - 2, y = H - 2)")

# ---- GFTT, 128 x 96 unless noted
_G = (GFTT, 128, 96)
_add("gftt_one_pixel", *_G, [("pixel", 0)], regime="exactly one candidate: a single bright pixel on black")
_add("gftt_stripes45", *_G, [("stripes45", 0)], regime="exactly one candidate from a 45-degree stripe pattern")
for _k in ("xramp", "vstripes", "checker1"):
    _add("gftt_zero_%s" % _k, *_G, [(_k, 0)], regime="M == +0.0 from textured but one-dimensional input: no candidates")
_add("gftt_tied_md3", *_G, [("checker8", 0)], regime="all candidates tied at one value: the raster index alone orders them")
_add("gftt_tied_md10", *_G, [("checker8", 0)], over=dict(min_distance=10.0),
     regime="all candidates tied, min_distance 10")
_add("gftt_border_drop", *_G, [("rim", 5)], regime="every accepted corner dropped by runByImageBorder(28)")
_add("gftt_nfeatures_1", *_G, over=dict(nfeatures=1), regime="nfeatures = 1")
GFTT_368_CANDIDATES = 2866     # the model's candidate count on the natural 368 x 239 frame
_add("gftt_cand_cap_at", GFTT, 368, 239, dev=dict(cand_cap=GFTT_368_CANDIDATES),
     regime="cand_cap exactly the candidate count: no flag")
_add("gftt_cand_cap_below", GFTT, 368, 239, dev=dict(cand_cap=GFTT_368_CANDIDATES - 1), flag={0: "cand_cap"},
     regime="cand_cap one below the candidate count: the frame is flagged")

# ---- adaptive
# An 8 x 8 grid without margin on 64 x 65: ROIs of 8 x 8 and 8 x 9 (rows 0, 8, 16, 24, 32, 40, 48, 56 | 65), scan
# ranges 2 x 2 and 2 x 3, one segment per row.  min_features 64: maxFeatures 108, maxPerCell 1, per-cell 1..2.
_MINROI = dict(grid_rows=8, grid_cols=8, edge_threshold=0, min_features=64)
_add("adaptive_min_roi", ADAPTIVE, 64, 65, [("noise", 3), ("binary", 4), ("nat", 40)], over=_MINROI,
     regime="ROIs of 8 x 8 and 8 x 9: scan ranges 2 x 2 and 2 x 3 (64 x 65 is accepted; 80 x 72 was not needed)")
_add("adaptive_overlap_e3", ADAPTIVE, 80, 72, [("noise", 6), ("nat", 40)], over=dict(_MINROI, edge_threshold=3),
     regime="an 8 x 8 grid with margin 3 on 80 x 72: overlapping 16 x 15 ROIs, adp_roi clamped at 0 and at W / H, on "
            "score tiles partial in x and y")
# The threshold walk, 320 x 240, one batch: 0 / 255 noise first (every corner scores 254, so every cell has more than
# grid_max corners at any threshold up to 254 and its threshold is multiplied by 1.3 per frame: 20, 26, 33.8, ...
# 275.7 before frame 10), then flat frames (tooFew on every try, down to min_thresh).  Uniform noise does not get
# there: its thresholds settle near 115, where a cell's count falls inside [grid_min, grid_max].  (int)275.7 is
# clamped to 255 by cv::FAST; no score reaches 255 (S <= 254), so a try at 255 is always tooFew: it is the last try
# of its frame, and so `used`, only when iterations is 1.  With more iterations the clamp still decides the first try
# of that frame (before > 255) and `used` is a later try's threshold (193 = (int)(275.7 * 0.7)).
WALK_NOISE, WALK_FLAT = 11, 16
_WALK = [("binary", 100 + i) for i in range(WALK_NOISE)] + [("flat", 0)] * WALK_FLAT
for _it in (5, 1, 32):
    _add("adaptive_walk_it%d" % _it, ADAPTIVE, 320, 240, _WALK, over=dict(iterations=_it),
         regime="thresholds climb past 255 (clamp_t) and fall to min_thresh over one batch, iterations %d" % _it)
# cell_cap: three natural frames from init_thresh = min_thresh = 2, so that frames 0 and 1 run at threshold 2 = tmin
# and a cell's count at the threshold used is its stored count (the flag compares those two).  Frame 1 stores the most.
ADAPTIVE_CAP_FRAMES = (("nat", 100), ("nat", 0), ("nat", 200))
ADAPTIVE_CAP_STORED = (1323, 1354, 1288)   # the largest `stored` of each frame (the model's)
_CAP = max(ADAPTIVE_CAP_STORED)
_CAP_AFTER = ("nat", 200)                  # the later extraction: frame 2 again (it fits both capacities), other thresholds
_add("adaptive_cell_cap_at", ADAPTIVE, 368, 239, ADAPTIVE_CAP_FRAMES, over=dict(init_thresh=2.0), dev=dict(cell_cap=_CAP),
     after=_CAP_AFTER, regime="cell_cap exactly the largest stored count of the batch: no flag")
_add("adaptive_cell_cap_below", ADAPTIVE, 368, 239, ADAPTIVE_CAP_FRAMES, over=dict(init_thresh=2.0),
     dev=dict(cell_cap=_CAP - 1), flag={ADAPTIVE_CAP_STORED.index(_CAP): "cell_cap"}, after=_CAP_AFTER,
     regime="cell_cap one below it: that frame alone is flagged; the frames after it and a later extraction equal the model")
ADAPTIVE_368_TOTAL = 1017                  # the sum of nsel on the natural 368 x 239 frame (9 cells x maxPerCell 113)
for _d, _nm in ((-1, "_minus_1"), (0, ""), (1, "_plus_1")):
    _add("adaptive_nfeatures_total" + _nm, ADAPTIVE, 368, 239, over=dict(nfeatures=ADAPTIVE_368_TOTAL + _d),
         regime="retainBest's n > nfeatures in k_adp_frame at nfeatures = total %+d" % _d)

# ---- cv::ORB
_add("cvorb_budget_5", CVORB, 640, 480, over=dict(nfeatures=5), regime="N = [1, 1, 1, 1, 1, 0, 0, 0]: zero budgets")
_add("cvorb_budget_1", CVORB, 640, 480, over=dict(nfeatures=1), regime="N = [0, ..., 0, 1]: one keypoint")
_add("cvorb_zero_row_strips", CVORB, 320, 256, over=dict(edge_threshold=48, nlevels=6),
     regime="level 5 is 129 x 103: its range has 7 rows, fewer than the 8 list strips (strips with r0 == r1)")
_add("cvorb_one_segment", CVORB, 400, 481, over=dict(edge_threshold=48, nlevels=8),
     regime="level 7 is 112 x 134: its range is 16 x 38, one segment per row, fewer corners than N")
for _e in (32, 47, 48):
    _add("cvorb_a0_e%d" % _e, CVORB, 320, 256, over=dict(edge_threshold=_e, nlevels=4),
         regime="a0 = e & ~15 with e = %d: %d masked columns in the first segment" % (_e, _e & 15))
_add("cvorb_thr_255", CVORB, 320, 256, over=dict(fast_threshold=255, nlevels=4), regime="fast_threshold 255: no corners")
_add("cvorb_thr_254_binary", CVORB, 320, 256, [("binary", 8)], over=dict(fast_threshold=254, nlevels=4),
     regime="fast_threshold 254 on 0 / 255 noise: every corner scores 254")
_add("cvorb_thr_1", CVORB, 320, 256, over=dict(fast_threshold=1, nlevels=4), regime="fast_threshold 1")
_add("cvorb_checker8", CVORB, 320, 240, [("checker8", 0)], over=dict(nlevels=4),
     regime="saturated input: level 0 has no corner, level 2's 1022 corners share 37 scores: retainBest(2 N) under ties "
            "(the frame keeps fewer than nfeatures at any budget, so the frame-level retainBest does not run on it)")
_add("cvorb_saturated_tiles", CVORB, 320, 240, [("tiles16", 1)], over=dict(nfeatures=300, nlevels=4),
     regime="a repeated 0 / 255 block: level 0's corners all score 254 and their Harris responses tie, so the level "
            "keeps more than N, the frame more than nfeatures: the frame-level retainBest and regroup run under ties")
# Selection boundaries on the natural 320 x 256 frame, 4 levels, fast_threshold 20, edge_threshold 31: the smallest
# nfeatures in 1..8192 at which some level (with N >= 2) has n_fast == 2 N, n_fast == 2 N + 1, len(s1) == N and
# len(s1) == N + 1, as search_selection_boundaries() below finds them (tests/test_extractor_edge_cases.py runs the
# search again).  All four boundaries exist.
CVORB_SELECTION = {"n_fast_2N": (1469, 3), "n_fast_2N_plus_1": (1953, 2), "s1_N_plus_1": (2934, 3), "s1_N": (2939, 3)}
for _what, (_nf, _l) in CVORB_SELECTION.items():
    _add("cvorb_sel_" + _what, CVORB, 320, 256, over=dict(nfeatures=_nf, nlevels=4),
         regime="level %d at nfeatures %d: %s" % (_l, _nf, _what))

NAMES = list(_T)
# the only cases that may end without keypoints (the stripes' one candidate lies at (W - 2, H - 2), inside BRIEF's
# border; it must still come out as the one accepted corner)
MAY_BE_EMPTY = {"gftt_zero_xramp", "gftt_zero_vstripes", "gftt_zero_checker1", "gftt_border_drop", "gftt_stripes45",
                "cvorb_thr_255"}
# cases whose regime itself caps the count below 20: name -> the keypoints the whole batch must still give
SMALL_BY_REGIME = {"gftt_one_pixel": 1, "gftt_nfeatures_1": 1, "cvorb_budget_5": 5, "cvorb_budget_1": 1,
                   "adaptive_min_roi": 1,       # BRIEF's border leaves 8 x 9 px of 64 x 65: four cells, one corner each
                   "adaptive_overlap_e3": 5}    # 24 x 16 px of 80 x 72
# the 368 x 239 case of each extractor: misaligned pointers, padded gray rows, stale state
SHARED = {GFTT: "gftt_368x239", ADAPTIVE: "adaptive_368x239", CVORB: "cvorb_368x239"}


# ------------------------------------------------------------------ parameters and models
def model_params(ext, over):
    if ext == GFTT:
        import gftt_model as G
        return G.params(**over)
    if ext == ADAPTIVE:
        import adaptive_model as A
        return A.params(**over)
    import cvorb_model as M
    return M.params(**over)


def make_model(ext, W, H, prm):
    if ext == GFTT:
        import gftt_model as G
        return G.Extractor(prm, W=W, H=H)
    if ext == ADAPTIVE:
        import adaptive_model as A
        return A.Extractor(prm, W=W, H=H)
    import cvorb_model as M
    return M.Extractor(prm, W=W, H=H)


def device_params(pkg, c):
    """The ctypes parameter block of the case's context, as the keyword Context takes it."""
    ext, prm, dev = c["ext"], c["prm"], c["dev"]
    if ext == GFTT:
        return dict(gftt=pkg.gftt_params(cand_cap=dev.get("cand_cap", 0), **prm))
    if ext == ADAPTIVE:
        return dict(adaptive=pkg.adaptive_params(cell_cap=dev.get("cell_cap", 0), **prm))
    return dict(cvorb=pkg.cvorb_params(cand_cap=dev.get("cand_cap", CVORB_CAND_CAP),
                                       max_keypoints=dev.get("max_keypoints", 0), **prm))


@functools.lru_cache(maxsize=None)
def case(name):
    ext, W, H, frames, over, dev, flag, after, regime = _T[name]
    imgs = [image(f, W, H) for f in frames]
    return dict(name=name, ext=ext, W=W, H=H, prm=model_params(ext, over), dev=dev, B=len(frames),
                bgr=np.stack([i[0] for i in imgs]), depth=np.stack([i[1] for i in imgs]), cam=S.images(W, H)[2],
                flag=flag, after=image(after, W, H) if after else None, regime=regime)


@functools.lru_cache(maxsize=None)
def model(name):
    """The CPU model over the case, once per session and left unchanged: dict(frames = the model's frame per batch
    frame, after = the model's frame of case["after"], thresholds / thresholds_after = the adaptive state (f64) after
    the batch / after the later extraction)."""
    c = case(name)
    m = make_model(c["ext"], c["W"], c["H"], c["prm"])
    out = dict(frames=[m.frame(c["bgr"][b], c["depth"][b], c["cam"]) for b in range(c["B"])], after=None)
    if c["ext"] == ADAPTIVE:
        out["thresholds"] = m.thresholds.copy()
    if c["after"] is not None:
        out["after"] = m.frame(c["after"][0], c["after"][1], c["cam"])
        if c["ext"] == ADAPTIVE:
            out["thresholds_after"] = m.thresholds.copy()
    return out


@functools.lru_cache(maxsize=None)
def shared_frames(ext, shifts=(0, 100, 200)):
    """(case, bgr [3, ...], depth [3, ...]) of the extractor's 368 x 239 case at three crops of the natural image."""
    c = case(SHARED[ext])
    imgs = [image(("nat", s), c["W"], c["H"]) for s in shifts]
    return c, np.stack([i[0] for i in imgs]), np.stack([i[1] for i in imgs])


@functools.lru_cache(maxsize=None)
def shared_model(ext, order):
    """The model's frames over shared_frames(ext) taken in `order` (indices; -1 is a flat frame), one model instance
    carried through them: (frames, thresholds after)."""
    c, bgr, depth = shared_frames(ext)
    m = make_model(ext, c["W"], c["H"], c["prm"])
    flat = np.full_like(bgr[0], 128)
    out = [m.frame(flat if i < 0 else bgr[i], depth[max(i, 0)], c["cam"]) for i in order]
    return out, (m.thresholds.copy() if ext == ADAPTIVE else None)


# ------------------------------------------------------------------ the cv::ORB selection-boundary search
@functools.lru_cache(maxsize=None)
def cvorb_level_scores(W=320, H=256, nlevels=4):
    """Per level of the natural frame, the FAST scores of its corners after the border filter (fast_threshold 20,
    edge_threshold 31), descending: n_fast is the list's length, and retainBest(2 N) keeps the 2 N best and every tie of
    the last of them."""
    import cvorb_model as M
    import oracle_lib as O
    m = M.Extractor(M.params(nlevels=nlevels), W=W, H=H)
    g = O.gray(S.images(W, H)[0])
    levels = O.pyramid(np.ascontiguousarray(g), m.orb)
    scores = []
    for l in range(nlevels):
        h, w = levels[l].shape
        k = O.fast(levels[l], 20)
        scores.append(np.sort(k[M.border_filter(k[:, 0], k[:, 1], w, h, 31)][:, 2])[::-1].copy())
    return scores


def search_selection_boundaries(lo=1, hi=8192):
    """The smallest nfeatures in lo..hi for which some level has n_fast == 2 N, n_fast == 2 N + 1, len(s1) == N and
    len(s1) == N + 1 (len(s1) = n_fast when n_fast <= 2 N, else the 2 N best plus the ties of the last score):
    boundary -> (nfeatures, level), the boundaries not found left out."""
    import cvorb_model as M
    scores = cvorb_level_scores()
    found = {}
    for nf in range(lo, hi + 1):
        N = M.budgets(nf, 1.2, len(scores))
        for l, sc in enumerate(scores):
            n = len(sc)
            n1 = n if n <= 2 * N[l] else (int(np.count_nonzero(sc >= sc[2 * N[l] - 1])) if N[l] > 0 else 0)
            for what, hit in (("n_fast_2N", n == 2 * N[l]), ("n_fast_2N_plus_1", n == 2 * N[l] + 1),
                              ("s1_N", n1 == N[l]), ("s1_N_plus_1", n1 == N[l] + 1)):
                if hit and N[l] >= 2 and what not in found:   # N >= 2: N + 1 is not 2 N
                    found[what] = (nf, l)
    return found
