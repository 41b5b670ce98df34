"""The SVO edge cases (tests/svo_edge_cases.py) reach their regimes: asserted from the oracle alone, so a change of the
synthetic frame or of a case cannot quietly move it off the edge that tests/test_gpu_svo_edges.py runs it for."""
import numpy as np
import pytest

import svo_edge_cases as E


@pytest.fixture(scope="module")
def results(oracle):
    """Every case run once by the oracle: name -> (case, grid keypoints before retainBest, final frame)."""
    out = {}
    for name in E.NAMES:
        c = E.case(name)
        p = E.oracle_params(oracle, c["prm"])
        out[name] = (c, oracle.svo_detect(oracle.gray(c["bgr"]), p),
                     oracle.svo_frame(c["bgr"], c["depth"], p, oracle.camera(c["cam"])))
    return out


def _level_dims(W, H, nlevels):
    dims = [(W, H)]
    for _ in range(1, nlevels):
        dims.append((dims[-1][0] // 2, dims[-1][1] // 2))
    return dims


def test_names_are_unique_and_buildable():
    assert len(set(E.NAMES)) == len(E.NAMES) and len(E.NAMES) >= 25
    for name in E.NAMES:
        c = E.case(name)
        assert c["bgr"].shape == (c["H"], c["W"], 3) and c["bgr"].dtype == np.uint8 and c["bgr"].flags.c_contiguous
        assert c["depth"].shape == (c["H"], c["W"]) and c["depth"].dtype == np.uint16
        assert set(c["prm"]) == set(E.DEFAULTS) and c["regime"]
        assert c["W"] % 16 == 0   # the inherited ORB refusal: only such widths make a context


def test_shapes_have_the_tiles_they_are_named_for():
    W, H, prm, _ = E.params("x_partial_tiles")
    assert W % 128 == 112 and W % 64 != 0
    assert [w % 4 for w, _ in _level_dims(W, H, prm["nlevels"])][:4] == [0, 0, 0, 2]   # 368, 184, 92, 46
    W, H, prm, _ = E.params("odd_height_unaligned_l3")
    assert [h for _, h in _level_dims(W, H, prm["nlevels"])] == [239, 119, 59, 29, 14]
    assert _level_dims(W, H, prm["nlevels"])[3][0] == 30
    offs = np.cumsum([0] + [w * h for w, h in _level_dims(W, H, prm["nlevels"])])
    assert offs[4] % 4 != 0
    W, H, prm, _ = E.params("tall_one_row_tile")
    assert H % 32 == 1 and H % 128 == 97
    W, H, prm, _ = E.params("wide_11bit")
    assert -(-W // 128) == 16 and W > 1024 + 64
    for n, name in ((1, "x_partial_tiles_l1"), (2, "x_partial_tiles_l2"), (4, "x_partial_tiles_l4")):
        assert E.params(name)[:2] == E.params("x_partial_tiles")[:2] and E.params(name)[2]["nlevels"] == n
        assert np.array_equal(E.case(name)["bgr"], E.case("x_partial_tiles")["bgr"])


@pytest.mark.parametrize("name", list(E.UNALIGNED_OCTAVE))
def test_unaligned_levels_carry_keypoints(results, name):
    """k_svo_detect stages a level byte by byte when its width (or its offset) is no multiple of 4: at 640 x 480 only
    levels too small for the Shi-Tomasi window.  Here such a level holds final keypoints (10, 12, 12, 12 and 6 when
    the cases were written)."""
    c, _, fr = results[name]
    L = E.UNALIGNED_OCTAVE[name]
    assert _level_dims(c["W"], c["H"], c["prm"]["nlevels"])[L][0] % 4 != 0
    assert np.count_nonzero(fr["kps"]["octave"] == L) >= 5


def test_wide_keys_hold_11_bit_x(results):
    c, grid, fr = results["wide_11bit"]
    assert np.count_nonzero(fr["kps"]["x"] >= 1024) >= 50
    assert np.count_nonzero((grid["octave"] == 0) & (grid["x"] >= 1024)) >= 50   # X itself, not X << L, is 11 bits


def test_tall_case_reaches_its_last_rows(results, oracle):
    """Row 480 is a detect tile row of its own, but h - 3 = 478: it can hold no corner, and the Shi-Tomasi window
    ends at row 475.  What is reachable: the oracle has level-0 NMS survivors, and grid keypoints in the last two
    cell rows (rows 475..480; 10 of them, all at y = 475, when the case was written).  Row 480 itself pins the
    staging and domain guards of a one-row tile only."""
    c, grid, _ = results["tall_one_row_tile"]
    assert len(oracle.fast10_corners(oracle.gray(c["bgr"]), c["prm"]["threshold"])) >= 1
    _, grows = E.grid_dims(c["W"], c["H"], c["prm"]["cell_size"])
    last = grid["y"].astype(np.int64) // c["prm"]["cell_size"] >= grows - 2
    assert np.count_nonzero(last) >= 1 and grid["y"].max() == c["H"] - 6


@pytest.mark.parametrize("cell", list(E.CELLS))
def test_cell_cases(results, cell):
    c, grid, _ = results["cell_%d" % cell]
    gc, gr = E.grid_dims(c["W"], c["H"], cell)
    assert gc * gr == E.CELLS[cell]
    assert len(grid) > 0
    if cell == 1000:
        assert len(grid) <= 1 and cell > max(c["W"], c["H"])
    # the fills of k_svo_select's 1024 threads
    E_ = -(-E.CELLS[cell] // 1024)
    assert E_ == {3: 7, 5: 3, 7: 2, 8: 1, 40: 1, 240: 1, 1000: 1}[cell]
    if cell == 7:
        assert E.CELLS[cell] % 1024 != 0 and E.CELLS[cell] % E_ != 0   # ragged: the last busy thread is half full
    if cell == 40:
        assert E.CELLS[cell] < 64


@pytest.mark.parametrize("t", [t for t in E.BARRIERS if t < E.SCORE_FLOOR])
def test_low_barriers_have_weak_unequal_neighbours(results, oracle, t):
    """Below the reference's score floor of 20 every weaker corner scores exactly 20, so 8-adjacent weak corners tie and
    suppress each other (fast_nonmax_3x3 compares with >=).  The floor is visible only where two 8-adjacent corners
    both have a true score (m - 1) below 20 and the two differ: the level-0 score map at the barrier holds such a
    pair.  At barrier 19 no such pair can exist (a corner there scores at least 19, so two scores below 20 are both
    19); there the floor shows in a corner of score 19 next to one of score exactly 20, which tie at 20.  Both kinds
    are pairs whose true scores differ and whose floored scores are equal: asserted at every barrier, and the
    narrower kind wherever it can exist."""
    c, _, _ = results["barrier_%d" % t]
    s = oracle.fast10_score_map(oracle.gray(c["bgr"]), t)
    corner = s >= max(t, 1)   # a corner at barrier t scores >= t (score 0: not a corner)
    fl = np.maximum(s, E.SCORE_FLOOR)
    both_weak = tied = 0
    for dy, dx in ((0, 1), (1, -1), (1, 0), (1, 1)):
        ya, yb = slice(0, s.shape[0] - dy), slice(dy, s.shape[0])
        xa, xb = slice(max(0, -dx), s.shape[1] - max(0, dx)), slice(max(0, dx), s.shape[1] - max(0, -dx))
        pair = corner[ya, xa] & corner[yb, xb] & (s[ya, xa] != s[yb, xb])
        tied += np.count_nonzero(pair & (fl[ya, xa] == fl[yb, xb]))
        both_weak += np.count_nonzero(pair & (s[ya, xa] < E.SCORE_FLOOR) & (s[yb, xb] < E.SCORE_FLOOR))
    assert tied >= 1
    if t < E.SCORE_FLOOR - 1:
        assert both_weak >= 1


def test_barrier_cases(results):
    assert len(results["barrier_254"][2]["kps"]) == 0 and len(results["barrier_254"][1]) == 0
    # the barrier changes the result on either side of 20: the cases are not copies of one another
    counts = {t: len(results["barrier_%d" % t][1]) for t in E.BARRIERS}
    assert len(set(counts.values())) == len(E.BARRIERS), counts


def test_nfeatures_cases(results):
    """n is the oracle's grid keypoint count: retainBest runs at n - 1 and not at n or n + 1."""
    for name in ("nfeatures_n_minus_1", "nfeatures_n", "nfeatures_n_plus_1"):
        c, grid, fr = results[name]
        assert len(grid) == E.N_GRID
    assert [E.NFEATURES[k]["nfeatures"] - E.N_GRID for k in ("nfeatures_n_minus_1", "nfeatures_n", "nfeatures_n_plus_1")] \
        == [-1, 0, 1]
    full = results["nfeatures_n"][2]["kps"]
    assert np.array_equal(full, results["nfeatures_n_plus_1"][2]["kps"])
    assert not np.array_equal(results["nfeatures_n_minus_1"][2]["kps"], full)   # retainBest cut or reordered them
    c, grid, fr = results["nfeatures_1_cell_40"]
    assert len(grid) > 1 and len(fr["kps"]) == 1


@pytest.mark.parametrize("name", E.NAMES)
def test_cases_are_not_empty_and_fit_their_capacity(results, name):
    """Only barrier_254 and cell_1000 may end without keypoints.  Every other case has at least 20 in the oracle,
    except the three whose regime itself caps the count below 20: one grid cell (cell_240, cell_1000) and nfeatures 1
    can keep one keypoint at most, and must keep it.  No case trips the capacity flag."""
    c, grid, fr = results[name]
    n = len(fr["kps"])
    gc, gr = E.grid_dims(c["W"], c["H"], c["prm"]["cell_size"])
    ceiling = min(gc * gr, c["prm"]["nfeatures"])
    if name not in E.MAY_BE_EMPTY:
        assert n >= min(20, ceiling), (name, n)
    assert n <= E.kp_cap(c["W"], c["H"], c["prm"])


def test_refusals_are_the_issue_list():
    assert len(E.REFUSALS) == 9 and len({r[0] for r in E.REFUSALS}) == 9
    for name, W, H, over, status, msg in E.REFUSALS:
        prm = dict(E.DEFAULTS, **over)
        gc, gr = (E.grid_dims(W, H, prm["cell_size"]) if prm["cell_size"] > 0 else (0, 0))
        widths = [w for w, _ in _level_dims(W, H, max(prm["nlevels"], 1))]
        why = {"odd level width": any(w & 1 for w in widths[:-1]), "12288 grid cells": gc * gr > 12288,
               "sides 1..2047": max(W, H) > 2047, "nlevels must be 1..8": not 1 <= prm["nlevels"] <= 8,
               "cell_size >= 1": prm["cell_size"] < 1, "0 <= threshold <= 254": not 0 <= prm["threshold"] <= 254}
        assert why[msg], name
        assert status == (E.ARG if msg in ("cell_size >= 1", "0 <= threshold <= 254") else E.UNSUPPORTED)
