"""Seeded SVO + BRIEF inputs (test infrastructure), one per edge regime of csrc/svo.hip and of svo_configure in
csrc/svo_host.cpp: frame sizes whose 128-px pyramid tiles and 64 x 32 detect tiles are partial, whose levels are not a
multiple of 4 wide where they still carry keypoints, whose key holds x >= 1024; grid cell sizes on every fill of
k_svo_select's threads (12 cells per thread down to one cell in all); FAST barriers on both sides of the reference's
hard-coded score floor of 20; nfeatures on both sides of retainBest's n > nfeatures; and the configurations
rgbd_create_svo refuses.  An SVO context inherits the ORB geometry's refusals (DESIGN.md "SVO + BRIEF definition"), so
only shapes that geometry accepts are used.

case(name) returns a dict: W, H, prm (the arguments of svo_params, max_keypoints included), bgr, depth, cam and
regime (what the case exists for).  The images are the fr1 synthetic frame tiled and cropped to the shape.
tests/test_svo_edge_cases.py asserts from the oracle alone that each case reaches its regime;
tests/test_gpu_svo_edges.py runs them on the device."""
import functools

import numpy as np

DEFAULTS = dict(nfeatures=1000, nlevels=5, cell_size=5, threshold=20, max_keypoints=0)
SMALL = (240, 239)   # the shape of the cell, barrier and nfeatures cases

# name -> (W, H, parameter overrides, regime)
SHAPES = {
    "x_partial_tiles": (368, 239, {}, "k_svo_pyramid's last tile 112 px wide (zero fill, x < W guards, lx0 + c < lw); "
                        "level 3 is 46 wide: unaligned detect staging with keypoints; detect tiles partial in x"),
    "x_partial_tiles_l1": (368, 239, dict(nlevels=1), "no halfSample level at a width with partial tiles"),
    "x_partial_tiles_l2": (368, 239, dict(nlevels=2), "one halfSample level, from G0 into A"),
    "x_partial_tiles_l4": (368, 239, dict(nlevels=4), "the unaligned level 3 is the last level"),
    "odd_height_unaligned_l3": (240, 239, {}, "heights 239 / 119 / 59 / 29 / 14; level 3 is 30 wide, level 4 starts "
                                "at an offset that is no multiple of 4"),
    "tall_one_row_tile": (400, 481, {}, "481 = 15 * 32 + 1: a detect tile row one pixel high; 481 = 3 * 128 + 97: a "
                          "pyramid tile row partial in y"),
    "wide_11bit": (2032, 239, dict(cell_size=8), "x >= 1024 in the cell key; 16 pyramid tiles across"),
}
# the octave whose level is not a multiple of 4 wide (k_svo_detect's byte-wise staging) and still holds keypoints:
# 46, 46, 30, 50 and 254 px
UNALIGNED_OCTAVE = {"x_partial_tiles": 3, "x_partial_tiles_l4": 3, "odd_height_unaligned_l3": 3,
                    "tall_one_row_tile": 3, "wide_11bit": 3}

# cell_size -> grid cells at 240 x 239 (kSvoSelThreads = 1024 threads, E = ceil(cells / 1024) cells per thread)
CELLS = {3: 6400, 5: 2304, 7: 1225, 8: 900, 40: 36, 240: 1, 1000: 1}
BARRIERS = [0, 5, 19, 20, 21, 60, 254]
SCORE_FLOOR = 20   # fast_corner_score_10(..., 20, ...): Features/SVOextractor.cpp:106-107

# the oracle's grid keypoint count (before retainBest) at 240 x 239, 5 levels, cell 5, barrier 20
N_GRID = 1479
NFEATURES = {"nfeatures_n_minus_1": dict(nfeatures=N_GRID - 1, max_keypoints=12288),
             "nfeatures_n": dict(nfeatures=N_GRID, max_keypoints=12288),
             "nfeatures_n_plus_1": dict(nfeatures=N_GRID + 1, max_keypoints=12288),
             "nfeatures_1_cell_40": dict(nfeatures=1, cell_size=40, max_keypoints=12288)}

CELL_NAMES = ["cell_%d" % c for c in CELLS]
BARRIER_NAMES = ["barrier_%d" % t for t in BARRIERS]
NAMES = list(SHAPES) + CELL_NAMES + BARRIER_NAMES + list(NFEATURES)
# the only cases that may end without keypoints
MAY_BE_EMPTY = {"barrier_254", "cell_1000"}

ARG, UNSUPPORTED = 1, 4   # rgbd_status
# (name, W, H, parameter overrides, status, a fragment of rgbd_last_error)
REFUSALS = [
    ("levels_6_odd_width", 240, 239, dict(nlevels=6), UNSUPPORTED, "odd level width"),   # level 4 is 15 wide, not last
    ("cell_2", 240, 239, dict(cell_size=2), UNSUPPORTED, "12288 grid cells"),            # 14400 cells
    ("wide_cell_5", 2032, 239, dict(cell_size=5), UNSUPPORTED, "12288 grid cells"),      # 407 x 48 cells
    ("side_2048", 2048, 240, {}, UNSUPPORTED, "sides 1..2047"),   # the ORB geometry accepts it: svo_configure's own check
    ("levels_0", 240, 239, dict(nlevels=0), UNSUPPORTED, "nlevels must be 1..8"),
    ("levels_9", 240, 239, dict(nlevels=9), UNSUPPORTED, "nlevels must be 1..8"),
    ("cell_0", 240, 239, dict(cell_size=0), ARG, "cell_size >= 1"),
    ("threshold_minus_1", 240, 239, dict(threshold=-1), ARG, "0 <= threshold <= 254"),
    ("threshold_255", 240, 239, dict(threshold=255), ARG, "0 <= threshold <= 254"),
]


@functools.lru_cache(maxsize=None)
def _source():
    import synth
    bgr, depth, _, cam = synth.sequence(1, seed=3, preset="fr1")
    return np.tile(bgr[0], (2, 4, 1)), np.tile(depth[0], (2, 4)), cam


def images(W, H, shift=0):
    """(bgr, depth, cam) of a W x H frame: the fr1 synthetic frame tiled, cropped at column `shift`."""
    bgr, depth, cam = _source()
    return (np.ascontiguousarray(bgr[:H, shift:shift + W]), np.ascontiguousarray(depth[:H, shift:shift + W]), cam)


def params(name):
    if name in SHAPES:
        W, H, over, regime = SHAPES[name]
    elif name in CELL_NAMES:
        c = int(name[len("cell_"):])
        (W, H), over = SMALL, dict(cell_size=c)
        regime = "%d grid cells in k_svo_select" % CELLS[c]
    elif name in BARRIER_NAMES:
        t = int(name[len("barrier_"):])
        (W, H), over = SMALL, dict(threshold=t)
        regime = "FAST barrier %d against the score floor %d" % (t, SCORE_FLOOR)
    elif name in NFEATURES:
        (W, H), over = SMALL, NFEATURES[name]
        regime = "retainBest's n > nfeatures at nfeatures %d" % over["nfeatures"]
    else:
        raise KeyError(name)
    return W, H, dict(DEFAULTS, **over), regime


def case(name):
    W, H, prm, regime = params(name)
    bgr, depth, cam = images(W, H)
    return dict(name=name, W=W, H=H, prm=prm, bgr=bgr, depth=depth, cam=cam, regime=regime)


def oracle_params(oracle, prm):
    return oracle.svo_params(prm["nfeatures"], prm["nlevels"], prm["cell_size"], prm["threshold"])


def grid_dims(W, H, cell):
    """(gcols, grows) of SVOextractor::detect :93-94."""
    return -(-W // cell), -(-H // cell)


def kp_cap(W, H, prm):
    """svo_configure's output capacity per frame."""
    gc, gr = grid_dims(W, H, prm["cell_size"])
    return min(gc * gr, prm["max_keypoints"] if prm["max_keypoints"] > 0 else prm["nfeatures"] + 64)
