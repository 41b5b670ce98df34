"""CPU checks of tests/gftt_model.py, the executable form of DESIGN.md's "GFTT + BRIEF definition": its
formulations agree with each other (vectorised map vs a literal per-pixel restatement; brute-force spacing vs
OpenCV's cell grid vs the round-parallel form the device runs), and the inputs the GPU tests rely on have the
properties those tests need (ties, full corner budgets), so they can neither go idle nor silently skip."""
import numpy as np
import pytest

from conftest import synth_seq
import gftt_model as G


def tiled_frame(W=320, H=256, seed=4):
    """A 32 x 32 block repeated over the frame: every candidate value away from the border occurs many times."""
    blk = np.random.RandomState(seed).randint(0, 256, size=(32, 32)).astype(np.uint8)
    return np.tile(blk, (H // 32, W // 32))


def test_map_equals_scalar_restatement():
    g = np.random.RandomState(2).randint(0, 256, size=(40, 48)).astype(np.uint8)   # texture up to all four borders
    a, b = G.eig_map(g), G.eig_map_scalar(g)
    assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # the border rule matters: the box filter reflects the product maps, not a Sobel of extended pixels
    assert a[0].max() > 0 and a[-1].max() > 0 and a[:, 0].max() > 0 and a[:, -1].max() > 0


def test_flat_frame_has_no_candidates():
    e = G.eig_map(np.full((64, 64), 128, np.uint8))
    M, thr, xy, val = G.candidates(e, 0.01)
    assert M == 0 and thr == 0 and len(xy) == 0


@pytest.mark.parametrize("md", [1, 2.5, 3, 3.9, 4.5, 10])
def test_grid_greedy_equals_brute_force(md):
    rs = np.random.RandomState(int(md * 10))
    W, H = 96, 80
    # dense clusters, so most candidates have accepted neighbours in adjacent cells
    pts = np.unique(rs.randint(0, [W, H], size=(2500, 2)), axis=0).astype(np.int32)
    val = rs.randint(1, 40, size=len(pts)).astype(np.float32)   # many ties
    order = G.rank(pts, val, W)
    for maxc in (50, 100000):
        brute, used = G.select_brute(pts, order, md, maxc)
        assert np.array_equal(G.select_grid(pts, order, W, H, md, maxc), brute)
        assert used <= len(pts) and (len(brute) == maxc or used == len(pts))
    # at min_distance 1 no two distinct pixels conflict (d2 >= 1); above it the spacing rejects
    assert len(brute) == len(pts) if md == 1 else 10 < len(brute) < len(pts)


@pytest.mark.parametrize("md", [0, 1, 2.5, 3, 3.9, 10])
def test_round_parallel_equals_sequential(md):
    rs = np.random.RandomState(7)
    W, H = 128, 96
    pts = np.unique(rs.randint(0, [W, H], size=(1500, 2)), axis=0).astype(np.int32)
    val = rs.randint(1, 25, size=len(pts)).astype(np.float32)
    order = G.rank(pts, val, W)
    for maxc in (1, 40, 100000):
        got, rounds = G.select_rounds(pts, order, md, maxc)
        assert np.array_equal(got, G.select_brute(pts, order, md, maxc)[0]), (md, maxc)
    # a monotone ridge along one row at spacing 2: every candidate waits for its left neighbour
    n = 150
    ridge = np.stack([2 * np.arange(n), np.full(n, 5)], 1).astype(np.int32)
    rv = (n - np.arange(n)).astype(np.float32)
    ro = G.rank(ridge, rv, 400)
    got, rounds = G.select_rounds(ridge, ro, 3.0, 1000)
    assert np.array_equal(got, G.select_brute(ridge, ro, 3.0, 1000)[0])
    assert np.array_equal(got, np.arange(0, n, 2)) and rounds >= n // 2


def test_tiled_frame_has_ties_and_the_tie_rule_shows():
    g = tiled_frame()
    e = G.eig_map(g)
    M, thr, xy, val = G.candidates(e, 0.01)
    print("tiled: %d candidates, %d distinct values" % (len(xy), len(np.unique(val))))
    assert len(xy) > 2000 and len(np.unique(val)) * 10 < len(xy)
    hi = G.rank(xy, val, 320, True)
    lo = G.rank(xy, val, 320, False)
    assert val[hi[0]] == val[lo[0]] and tuple(xy[hi[0]]) != tuple(xy[lo[0]])
    a = G.select_brute(xy, hi, 3.0, 1000)[0]
    b = G.select_brute(xy, lo, 3.0, 1000)[0]
    assert a[0] != b[0]
    # the higher raster index goes first
    assert xy[a[0], 1] * 320 + xy[a[0], 0] > xy[b[0], 1] * 320 + xy[b[0], 0]


@pytest.mark.parametrize("preset,seed", [("fr1", 3), ("lowtex", 7)])
def test_presets_fill_the_corner_budget(oracle, preset, seed):
    bgr, depth, _, cam = synth_seq(5, seed=seed, preset=preset)
    m = G.Extractor()
    f = m.frame(bgr[0], depth[0], cam)
    rec = f["rec"]
    print("%s: %d candidates, %d corners, %d ranks, %d keypoints" % (preset, rec["n_candidates"], len(rec["corners"]),
                                                                    rec["ranks"], len(f["kps"])))
    assert len(rec["corners"]) == 1000 and len(f["kps"]) > 700
    assert rec["n_candidates"] > 2000 and rec["ranks"] < rec["n_candidates"]
    assert (f["kps"]["response"] == 0).all() and (f["kps"]["size"] == 3).all()
    # acceptance order is descending value; every pair of corners is at least min_distance apart
    assert np.all(np.diff(rec["vals"]) <= 0)
    c = rec["corners"].astype(np.int64)
    d2 = ((c[:, None] - c[None]) ** 2).sum(-1)
    assert d2[~np.eye(len(c), dtype=bool)].min() >= 9
