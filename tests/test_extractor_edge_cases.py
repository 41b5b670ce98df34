"""The extractor edge cases (tests/extractor_edge_cases.py) reach their regimes: asserted from the CPU models alone
(tests/gftt_model.py, tests/adaptive_model.py, tests/cvorb_model.py over oracle.gray), so a change of the synthetic
frame, of a model or of a case cannot quietly move it off the edge that tests/test_gpu_extractor_edges.py runs it for.
The model frames are computed once (extractor_edge_cases.model) and shared with the GPU file."""
import numpy as np
import pytest

import adaptive_model as A
import cvorb_model as M
import extractor_edge_cases as E
import gftt_model as G

F32 = np.float32


def _frames(name):
    return E.model(name)["frames"]


def _gftt_candidates(name, b=0):
    """(xy, val) of every candidate of the model's frame."""
    c = E.case(name)
    _, _, xy, val = G.candidates(_frames(name)[b]["rec"]["e"], c["prm"]["quality_level"])
    return xy, val


# ------------------------------------------------------------------ the table itself
def test_names_are_unique_and_buildable(oracle):
    assert len(set(E.NAMES)) == len(E.NAMES) and len(E.NAMES) >= 45
    assert E.MAY_BE_EMPTY <= set(E.NAMES) and set(E.SMALL_BY_REGIME) <= set(E.NAMES)
    assert not E.MAY_BE_EMPTY & set(E.SMALL_BY_REGIME)
    for name in E.NAMES:
        c = E.case(name)
        W, H, B = c["W"], c["H"], c["B"]
        assert c["ext"] in (E.GFTT, E.ADAPTIVE, E.CVORB) and c["regime"]
        assert c["bgr"].shape == (B, H, W, 3) and c["bgr"].dtype == np.uint8 and c["bgr"].flags.c_contiguous
        assert c["depth"].shape == (B, H, W) and c["depth"].dtype == np.uint16
        # what the one-level and the ORB geometry accept
        assert W % 16 == 0 and W >= 64 and 64 < H <= 2 * W and max(W, H) <= 2047, name
        assert set(c["flag"]) <= set(range(B))
    for ext in E.SHARED:
        assert E.case(E.SHARED[ext])["ext"] == ext and (E.case(E.SHARED[ext])["W"], E.case(E.SHARED[ext])["H"]) == (368, 239)


@pytest.mark.parametrize("kind", ["pixel", "stripes45", "xramp", "vstripes", "checker1", "checker8", "noise", "binary", "tiles16", "rim"])
def test_patterns_survive_the_gray_conversion(oracle, kind):
    g = E.pattern(kind, 128, 96, 5)
    assert g.dtype == np.uint8 and np.array_equal(oracle.gray(E.gray3(g)), g)
    assert np.array_equal(g, E.pattern(kind, 128, 96, 5)) and g.max() > g.min()   # seeded, textured


def test_shapes_have_the_tiles_they_are_named_for():
    # GFTT 64 x 16, adaptive 64 x 32, cv::ORB 64 x 4 (over the range [e - 1, w - e] x [e - 1, h - e])
    W, H = 368, 239
    assert W % 64 == 48 and H % 16 == 15 and H % 32 == 15 and H % 2 == 1
    e = 31
    assert (W - 2 * e + 2) % 64 != 0 and (H - 2 * e + 2) % 4 != 0
    W, H = 400, 481
    assert W % 64 == 16 and H % 16 == 1 and H % 32 == 1
    W, H = 336, 241
    assert W % 64 == 16 and H % 16 == 1
    W, H = 2032, 239
    assert -(-W // 64) == 32 and W > 1024 + 64


# ------------------------------------------------------------------ GFTT
@pytest.mark.parametrize("name", ["gftt_368x239", "gftt_400x481", "gftt_336x241", "gftt_2032x239", "gftt_noise_368x239"])
def test_gftt_shapes(name):
    c = E.case(name)
    W, H = c["W"], c["H"]
    rec = _frames(name)[0]["rec"]
    xy, _ = _gftt_candidates(name)
    assert len(xy) == rec["n_candidates"] < 32768            # below the default cand_cap
    assert len(rec["corners"]) == 1000 and rec["ranks"] < rec["n_candidates"]
    lo = np.count_nonzero(xy[:, 0] == 1), np.count_nonzero(xy[:, 1] == 1)
    hi = np.count_nonzero(xy[:, 0] == W - 2), np.count_nonzero(xy[:, 1] == H - 2)
    print(name, rec["n_candidates"], "candidates; at x = 1, y = 1:", lo, "at x = W - 2, y = H - 2:", hi)
    assert max(lo) >= 1 and max(hi) >= 1
    if name == "gftt_noise_368x239":
        assert min(lo) >= 1 and min(hi) >= 1
    if H % 16 == 1:   # the one-row tile: candidates in the last rows, whose box sums reach row H - 1 and its partner H - 2
        assert hi[1] >= 1
    # the map has texture on every border (its bits are compared there too)
    e = rec["e"]
    assert e[0].max() > rec["thr"] and e[-1].max() > rec["thr"] and e[:, 0].max() > rec["thr"] and e[:, -1].max() > rec["thr"]
    if name == "gftt_368x239":
        assert rec["n_candidates"] == E.GFTT_368_CANDIDATES
    if name == "gftt_2032x239":
        assert np.count_nonzero(rec["corners"][:, 0] >= 1024) >= 50 and np.count_nonzero(xy[:, 0] >= 1024) >= 1000
        # accepted corners on both sides of x = 1024 within min_distance of it: gftt_near compares across the bit
        assert np.count_nonzero(np.abs(rec["corners"][:, 0] - 1024) <= 3) >= 1


def test_gftt_single_candidates():
    for name in ("gftt_one_pixel", "gftt_stripes45"):
        rec = _frames(name)[0]["rec"]
        assert rec["n_candidates"] == 1 and len(rec["corners"]) == 1 and rec["ranks"] == 1, name
    assert abs(float(_frames("gftt_stripes45")[0]["rec"]["M"]) - 0.1388889) < 1e-6
    c = E.case("gftt_stripes45")
    assert tuple(_frames("gftt_stripes45")[0]["rec"]["corners"][0]) == (c["W"] - 2, c["H"] - 2)
    assert len(_frames("gftt_one_pixel")[0]["kps"]) == 1 and len(_frames("gftt_stripes45")[0]["kps"]) == 0


@pytest.mark.parametrize("kind", ["xramp", "vstripes", "checker1"])
def test_gftt_zero_maximum_from_texture(oracle, kind):
    name = "gftt_zero_" + kind
    f = _frames(name)[0]
    g = oracle.gray(E.case(name)["bgr"][0])
    assert g.max() - g.min() >= 200                             # textured
    assert F32(f["rec"]["M"]).view(np.uint32) == 0              # +0.0, bit for bit
    assert f["rec"]["n_candidates"] == 0 and len(f["rec"]["corners"]) == 0 and len(f["kps"]) == 0
    assert f["rec"]["e"].min() <= 0 and f["rec"]["e"].max() == 0


@pytest.mark.parametrize("name", ["gftt_tied_md3", "gftt_tied_md10"])
def test_gftt_all_tied(name):
    c = E.case(name)
    rec = _frames(name)[0]["rec"]
    xy, val = _gftt_candidates(name)
    assert len(xy) == rec["n_candidates"] == 660 and len(np.unique(val.view(np.uint32))) == 1
    # the raster index alone decides: accepted in strictly descending raster order, the list exhausted
    idx = rec["corners"][:, 1].astype(np.int64) * c["W"] + rec["corners"][:, 0]
    assert np.all(np.diff(idx) < 0) and rec["ranks"] == 660 and idx[0] == (xy[:, 1].astype(np.int64) * c["W"] + xy[:, 0]).max()
    assert 20 < len(rec["corners"]) < 660                       # the spacing rejects
    assert len(_frames("gftt_tied_md3")[0]["rec"]["corners"]) > len(_frames("gftt_tied_md10")[0]["rec"]["corners"])


def test_gftt_border_drop_and_nfeatures_1():
    f = _frames("gftt_border_drop")[0]
    assert len(f["rec"]["corners"]) > 100 and len(f["kps"]) == 0
    f = _frames("gftt_nfeatures_1")[0]
    assert f["rec"]["n_candidates"] > 100 and len(f["rec"]["corners"]) == 1 and f["rec"]["ranks"] == 1 and len(f["kps"]) == 1


def test_gftt_cand_cap_cases():
    n = _frames("gftt_cand_cap_at")[0]["rec"]["n_candidates"]
    assert n == E.GFTT_368_CANDIDATES and n % 64 != 0
    assert E.case("gftt_cand_cap_at")["dev"]["cand_cap"] == n and not E.case("gftt_cand_cap_at")["flag"]
    assert E.case("gftt_cand_cap_below")["dev"]["cand_cap"] == n - 1 and E.case("gftt_cand_cap_below")["flag"] == {0: "cand_cap"}


# ------------------------------------------------------------------ adaptive
def _cells(name):
    return [f["rec"]["cells"] for f in _frames(name)]


@pytest.mark.parametrize("name", ["adaptive_368x239", "adaptive_400x481", "adaptive_2032x239"])
def test_adaptive_shapes(name):
    c = E.case(name)
    f = _frames(name)[0]
    stored = max(x["stored"] for x in f["rec"]["cells"])
    print(name, "largest stored", stored, "total", f["rec"]["total"], "keypoints", len(f["kps"]))
    assert stored <= 8192 and f["rec"]["total"] > c["prm"]["nfeatures"]   # below the default cell_cap; retainBest runs
    if name == "adaptive_2032x239":
        assert np.count_nonzero(f["kps"]["x"] >= 1024) >= 50
        assert any(np.count_nonzero(x["raster"][:, 0] + r[0] >= 1024) for x, r in zip(f["rec"]["cells"], A.rois(c["W"], c["H"], c["prm"])))


def test_adaptive_minimum_rois():
    c = E.case("adaptive_min_roi")
    rois = A.rois(c["W"], c["H"], c["prm"])
    sizes = {(x1 - x0, y1 - y0) for x0, y0, x1, y1 in rois}
    assert sizes == {(8, 8), (8, 9)} and len(rois) == 64
    assert {(w - 6, h - 6) for w, h in sizes} == {(2, 2), (2, 3)}          # the scan ranges: one segment per row
    assert A.derived(c["prm"])["max_per_cell"] == 1
    cells = _cells("adaptive_min_roi")
    assert sum(len(x["raster"]) for fc in cells for x in fc) >= 50
    assert {x["tries"] for fc in cells for x in fc} >= {1, 2, 5}           # the chain is not idle
    assert any(x["before"] == c["prm"]["min_thresh"] for x in cells[-1])
    c = E.case("adaptive_overlap_e3")
    rois = A.rois(c["W"], c["H"], c["prm"])
    assert c["W"] % 64 != 0 and c["H"] % 32 != 0
    assert {(x1 - x0, y1 - y0) for x0, y0, x1, y1 in rois} == {(13, 12), (16, 12), (13, 15), (16, 15)}
    assert rois[0][:2] == (0, 0) and rois[-1][2:] == (c["W"], c["H"])     # both clamps
    assert rois[1][0] < rois[0][2] and rois[8][1] < rois[0][3]             # neighbours overlap
    assert sum(len(x["raster"]) for fc in _cells("adaptive_overlap_e3") for x in fc) >= 200


@pytest.mark.parametrize("it", [5, 1, 32])
def test_adaptive_threshold_walk(it):
    name = "adaptive_walk_it%d" % it
    c = E.case(name)
    assert c["prm"]["iterations"] == it and c["prm"]["max_thresh"] > 255 and c["B"] == E.WALK_NOISE + E.WALK_FLAT
    cells = _cells(name)
    # the climb: every cell, every noise frame before the clamp: 20 * 1.3^k
    th = 20.0
    for b in range(E.WALK_NOISE - 1):
        assert all(x["before"] == th and x["branch"] == "many" and x["tries"] == 1 for x in cells[b]), (b, th)
        th = th * 1.3
    b = E.WALK_NOISE - 1
    assert th > 255 and all(x["before"] == th and A.clamp_t(x["before"]) == 255 for x in cells[b])
    if it == 1:   # the try at 255 is the only one: tooFew (no score reaches 255)
        assert all(x["used"] == 255 and x["branch"] == "few" and len(x["raster"]) == 0 for x in cells[b])
    else:         # a second try at (int)(275.7 * 0.7)
        assert all(x["used"] == 193 and x["tries"] == 2 for x in cells[b])
    # the fall: flat frames, down to min_thresh, and it stays there
    tmin = int(c["prm"]["min_thresh"])
    first = next(i for i in range(b + 1, c["B"]) if all(x["used"] == tmin for x in cells[i]))
    assert all(x["before"] > c["prm"]["min_thresh"] for x in cells[first]) or it == 1
    assert all(x["used"] == tmin and x["before"] == c["prm"]["min_thresh"] and x["tries"] == 1 for x in cells[-1])
    assert np.all(E.model(name)["thresholds"] == c["prm"]["min_thresh"])
    assert max(x["tries"] for fc in cells for x in fc) == {5: 5, 1: 1, 32: 14}[it]
    assert max(x["stored"] for fc in cells for x in fc) <= 8192


def test_adaptive_cell_cap_cases():
    for name in ("adaptive_cell_cap_at", "adaptive_cell_cap_below"):
        c = E.case(name)
        cells = _cells(name)
        stored = tuple(max(x["stored"] for x in fc) for fc in cells)
        assert stored == E.ADAPTIVE_CAP_STORED
        worst = stored.index(max(stored))
        assert 0 < worst < c["B"] - 1                                   # frames before and after it
        cap = c["dev"]["cell_cap"]
        tmin = max(1, int(c["prm"]["min_thresh"]))
        # the flag compares the list's count at the threshold used with the cell's: at used == tmin they are `stored`
        w = max(cells[worst], key=lambda x: x["stored"])
        assert w["used"] == tmin and len(w["raster"]) == w["stored"]
        if name.endswith("_at"):
            assert cap == max(stored) and not c["flag"]
        else:
            assert cap == max(stored) - 1 and c["flag"] == {worst: "cell_cap"}
            assert all(s <= cap for i, s in enumerate(stored) if i != worst)
        after = E.model(name)["after"]
        assert len(after["kps"]) > 100 and max(x["stored"] for x in after["rec"]["cells"]) <= cap   # it does not flag
        assert [x["used"] for x in after["rec"]["cells"]] != [x["used"] for x in cells[2]]          # not a replay


def test_adaptive_nfeatures_cases():
    tot = [_frames("adaptive_nfeatures_total" + s)[0]["rec"]["total"] for s in ("_minus_1", "", "_plus_1")]
    assert tot == [E.ADAPTIVE_368_TOTAL] * 3
    nf = [E.case("adaptive_nfeatures_total" + s)["prm"]["nfeatures"] for s in ("_minus_1", "", "_plus_1")]
    assert [n - E.ADAPTIVE_368_TOTAL for n in nf] == [-1, 0, 1]
    full = _frames("adaptive_nfeatures_total")[0]["kps"]
    assert np.array_equal(full, _frames("adaptive_nfeatures_total_plus_1")[0]["kps"])
    assert not np.array_equal(_frames("adaptive_nfeatures_total_minus_1")[0]["kps"], full)   # retainBest cut or reordered


# ------------------------------------------------------------------ cv::ORB
def _levels(name, b=0):
    return [(lr["n_fast"], len(lr["s1"]), len(lr["s2"])) for lr in _frames(name)[b]["rec"]["levels"]]


def _ext(name):
    c = E.case(name)
    return M.Extractor(c["prm"], W=c["W"], H=c["H"])


def _list_geometry(w, h, e):
    """k_cvorb_list's (range width, range height, a0, segments per row) of a level."""
    a0 = e & ~15
    return w - 2 * e, h - 2 * e, a0, (w - e - a0 + 15) // 16


def _masked_maxima(oracle, name, l):
    """What only k_cvorb_list's column test drops: strict 3 x 3 maxima of the stored score map (S >= t on
    [e - 1, w - e] x [e - 1, h - e], 0 elsewhere) in the columns e - 1 and w - e, rows [e, h - e)."""
    c = E.case(name)
    m = _ext(name)
    e, t = c["prm"]["edge_threshold"], c["prm"]["fast_threshold"]
    lv = oracle.pyramid(np.ascontiguousarray(oracle.gray(c["bgr"][0])), m.orb)[l]
    h, w = lv.shape
    S = A.score_map(lv).astype(np.int32)
    S[S < t] = 0
    st = np.zeros_like(S)
    st[e - 1:h - e + 1, e - 1:w - e + 1] = S[e - 1:h - e + 1, e - 1:w - e + 1]
    mx = A.roi_maxima(st.astype(np.uint8), (0, 0, w, h))
    rows = (mx[:, 1] >= e) & (mx[:, 1] < h - e)
    return int(np.count_nonzero(rows & (mx[:, 0] == e - 1))), int(np.count_nonzero(rows & (mx[:, 0] == w - e)))


def test_cvorb_shapes():
    assert _levels("cvorb_368x239") and all(n > 2 * N for (n, _, _), N in zip(_levels("cvorb_368x239"), _ext("cvorb_368x239").N))
    assert len(_frames("cvorb_368x239")[0]["kps"]) > 800 and len(_frames("cvorb_400x481")[0]["kps"]) > 800
    for name in ("cvorb_368x239", "cvorb_400x481"):
        assert max(n for n, _, _ in _levels(name)) <= E.CVORB_CAND_CAP
        odd = [(w, h) for w, h in _ext(name).sizes if (w - 60) % 64 and (h - 60) % 4]
        assert len(odd) >= 3   # partial score tiles in x and y on most levels


def test_cvorb_zero_budgets():
    assert _ext("cvorb_budget_5").N == [1, 1, 1, 1, 1, 0, 0, 0] and _ext("cvorb_budget_1").N == [0] * 7 + [1]
    for name in ("cvorb_budget_5", "cvorb_budget_1"):
        N = _ext(name).N
        lv = _levels(name)
        for l in range(8):
            assert lv[l][0] > 500                                    # corners on every level
            if N[l] == 0:
                assert lv[l][1:] == (0, 0)
            else:
                assert lv[l][2] == 1 and lv[l][1] >= 2
    assert len(_frames("cvorb_budget_5")[0]["kps"]) == 5 and len(_frames("cvorb_budget_1")[0]["kps"]) == 1
    assert _frames("cvorb_budget_1")[0]["kps"]["octave"][0] == 7


def test_cvorb_thin_levels():
    m = _ext("cvorb_zero_row_strips")
    assert m.sizes[5] == (129, 103)
    sw, shh, a0, segs = _list_geometry(129, 103, 48)
    assert (sw, shh) == (33, 7) and shh < 8 and segs == 3
    assert [shh * s // 8 == shh * (s + 1) // 8 for s in range(8)].count(True) == 1   # one strip without rows
    n5 = _levels("cvorb_zero_row_strips")[5]
    assert 0 < n5[0] <= m.N[5] and n5[0] == n5[2]
    m = _ext("cvorb_one_segment")
    assert m.sizes[7] == (112, 134)
    sw, shh, a0, segs = _list_geometry(112, 134, 48)
    assert (sw, shh, segs) == (16, 38, 1)
    n7 = _levels("cvorb_one_segment")[7]
    assert 0 < n7[0] < m.N[7] == 60 and n7[0] == n7[1] == n7[2]     # neither retainBest runs on that level


def test_cvorb_first_segment_column(oracle):
    for e, masked in ((32, 0), (47, 15), (48, 0)):
        name = "cvorb_a0_e%d" % e
        assert E.case(name)["prm"]["edge_threshold"] == e and e - (e & ~15) == masked
        assert all(n > 100 for n, _, _ in _levels(name))
        # corners in the first and in the last column of the range, on some level
        s = np.concatenate([np.stack([lr["s1"][:, 0] - e, w - e - 1 - lr["s1"][:, 0]], 1)
                            for lr, (w, h) in zip(_frames(name)[0]["rec"]["levels"], _ext(name).sizes)])
        print(name, "corners in the range's first / last column:", np.count_nonzero(s[:, 0] == 0), np.count_nonzero(s[:, 1] == 0))
        assert s.min() >= 0
    # maxima of the stored map that only the list's column test removes (it is not idle)
    left = sum(_masked_maxima(oracle, "cvorb_a0_e47", l)[0] for l in range(4))
    right = sum(_masked_maxima(oracle, "cvorb_a0_e47", l)[1] for l in range(4))
    print("e = 47: maxima in column e - 1:", left, "in column w - e:", right)
    assert left >= 1 and right >= 1


def test_cvorb_fast_thresholds():
    assert _levels("cvorb_thr_255") == [(0, 0, 0)] * 4 and len(_frames("cvorb_thr_255")[0]["kps"]) == 0
    lr = _frames("cvorb_thr_254_binary")[0]["rec"]["levels"]
    assert lr[0]["n_fast"] > 2 * _ext("cvorb_thr_254_binary").N[0] and np.all(lr[0]["s1"][:, 2] == 254)
    assert len(lr[0]["s1"]) == lr[0]["n_fast"]                     # all tied: retainBest(2 N) keeps every one
    assert len(_frames("cvorb_thr_254_binary")[0]["kps"]) > 200
    n1, n20 = _levels("cvorb_thr_1"), _levels("cvorb_a0_e32")
    assert all(a[0] <= E.CVORB_CAND_CAP for a in n1) and n1[0][0] > 2000
    f = _frames("cvorb_thr_1")[0]
    weak = sum(int(np.count_nonzero(l["s1"][:, 2] < 20)) for l in f["rec"]["levels"])
    print("fast_threshold 1:", [a[0] for a in n1], "corners;", weak, "of s1 score below 20")
    assert n20 and len(f["kps"]) > 800


def test_cvorb_saturated_input():
    lv = _levels("cvorb_checker8")
    assert [a[0] for a in lv] == [0, 14, 1022, 368]
    rec = _frames("cvorb_checker8")[0]["rec"]
    # level 2: more than 2 N corners sharing a few scores, so retainBest(2 N) keeps ties past 2 N
    N = _ext("cvorb_checker8").N
    assert lv[2][0] > 2 * N[2] and lv[2][1] > 2 * N[2] and lv[2][2] == N[2]
    assert len(np.unique(rec["levels"][2]["s1"][:, 2])) * 8 < lv[2][1] and not rec["frame_retain"]
    # the repeated block: one score on level 0, Harris ties at N, the frame stage under ties
    c = E.case("cvorb_saturated_tiles")
    lv = _levels("cvorb_saturated_tiles")
    rec = _frames("cvorb_saturated_tiles")[0]["rec"]
    N = _ext("cvorb_saturated_tiles").N
    assert np.all(rec["levels"][0]["s1"][:, 2] == 254) and lv[0][1] == lv[0][0] > 2 * N[0] and lv[0][2] > N[0]
    assert len(np.unique(rec["levels"][0]["h2"].view(np.uint32))) * 4 < lv[0][2]
    assert rec["total"] > c["prm"]["nfeatures"] and rec["frame_retain"] and rec["regroup"]
    n = len(_frames("cvorb_saturated_tiles")[0]["kps"])
    assert c["prm"]["nfeatures"] <= rec["n_detect"] <= c["prm"]["nfeatures"] + c["prm"]["nfeatures"] // 4 and n > 200


def test_cvorb_selection_boundaries():
    assert E.search_selection_boundaries() == E.CVORB_SELECTION and len(E.CVORB_SELECTION) == 4
    for what, (nf, l) in E.CVORB_SELECTION.items():
        name = "cvorb_sel_" + what
        N = _ext(name).N[l]
        n, n1, n2 = _levels(name)[l]
        want = {"n_fast_2N": n == 2 * N, "n_fast_2N_plus_1": n == 2 * N + 1, "s1_N": n1 == N, "s1_N_plus_1": n1 == N + 1}
        assert want[what] and N >= 2, (name, n, n1, N)
        assert n2 == N or n1 <= N


# ------------------------------------------------------------------ no case is idle
@pytest.mark.parametrize("name", E.NAMES)
def test_cases_are_not_empty(name):
    """Only the cases of MAY_BE_EMPTY may end without keypoints.  Every other case keeps at least 20 over its batch in
    the model, except those whose regime itself caps the count (SMALL_BY_REGIME), which must keep what it allows."""
    n = sum(len(f["kps"]) for f in _frames(name))
    if name in E.MAY_BE_EMPTY:
        return
    assert n >= E.SMALL_BY_REGIME.get(name, 20), (name, n)


@pytest.mark.parametrize("ext", [E.GFTT, E.ADAPTIVE, E.CVORB])
def test_shared_frames(ext):
    """The three crops of the misaligned-pointer and stale-state tests differ and are rich."""
    c, bgr, depth = E.shared_frames(ext)
    assert not np.array_equal(bgr[0], bgr[1]) and not np.array_equal(bgr[1], bgr[2])
    frames, _ = E.shared_model(ext, (0, 1, 2))
    assert all(len(f["kps"]) > 500 for f in frames)
    assert (c["W"] * c["H"] * 3) % 16 == 0 and (c["W"] * c["H"] * 2) % 4 == 0   # every frame as misaligned as the first
    # the stale-state order: [rich, rich'], [flat, rich''], [rich, flat]; no frame trips a capacity
    order = (0, 1, -1, 2, 0, -1)
    for o in (order, (0, 1, 2, 0, 1, 2)):
        frames, _ = E.shared_model(ext, o)
        for i, f in zip(o, frames):
            assert (len(f["kps"]) == 0) if i < 0 else (len(f["kps"]) > 500), (ext, i)
        for f in frames:
            if ext == E.ADAPTIVE:
                assert max(x["stored"] for x in f["rec"]["cells"]) <= 8192
            elif ext == E.GFTT:
                assert f["rec"]["n_candidates"] < 32768
            else:
                assert max(l["n_fast"] for l in f["rec"]["levels"]) <= E.CVORB_CAND_CAP
