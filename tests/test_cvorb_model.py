"""The CPU model of the OpenCV ORB extractor (tests/cvorb_model.py), held together on the CPU: the budgets and level
sizes, the forms the device rests on, the Harris response three ways, the restated angle and steered BRIEF against
the ORB2 oracle's, and the regimes the GPU tests' frames must show so that no path of the device is idle."""
import numpy as np
import pytest

from conftest import synth_seq
import adaptive_model as A
import cvorb_model as M

F32 = np.float32

# the GPU tests' contexts: (W, H, parameters)
SMALL = dict(W=320, H=248, prm=M.params(scale_factor=2.0, nlevels=3))   # the last level is 80 x 62: it keeps nothing
P300 = dict(W=320, H=256, prm=M.params(nfeatures=300, nlevels=3, scale_factor=1.5, edge_threshold=22, fast_threshold=7))
_MEMO = {}


def tie_frame(oracle):
    """A 16 x 16 block of the rich frame tiled over 640 x 480: level 0 repeats every corner, so its scores and
    Harris responses tie exactly."""
    if "tie" not in _MEMO:
        g = oracle.gray(synth_seq(5, seed=3, preset="fr1")[0][0])
        _MEMO["tie"] = np.ascontiguousarray(np.tile(g[100:116, 200:216], (30, 40)))
    return _MEMO["tie"]


def small_frame(oracle, preset="fr1", seed=3, W=320, H=248):
    import synth
    key = ("small", preset, seed, W, H)
    if key not in _MEMO:
        _MEMO[key] = synth.sequence(2, seed=seed, preset=preset, W=W, H=H)
    return _MEMO[key]


def model_run(key, g, prm=None, W=640, H=480):
    """detect_and_compute of the model, once per session."""
    key = ("run", key)
    if key not in _MEMO:
        _MEMO[key] = M.Extractor(prm, W=W, H=H).detect_and_compute(g)
    return _MEMO[key]


# ------------------------------------------------------------------ tables
def test_budgets():
    assert M.budgets(1000, 1.2, 8) == [217, 181, 151, 126, 105, 87, 73, 60]
    assert M.budgets(1000, 1.2, 1) == [1000] and M.budgets(37, 1.5, 1) == [37]
    assert sum(M.budgets(300, 1.5, 3)) == 300


@pytest.mark.parametrize("W,H,sf,nl", [(640, 480, 1.2, 8), (320, 248, 2.0, 3), (320, 256, 1.5, 3), (752, 480, 1.2, 8),
                                       (640, 480, 1.25, 5), (640, 480, 1.2, 12)])
def test_level_sizes_equal_the_pyramids(oracle, W, H, sf, nl):
    t = oracle.tables(oracle.orb_params(1000, sf, nl), W, H)
    assert M.level_sizes(W, H, M.layer_scales(sf, nl)) == [(int(a), int(b)) for a, b in zip(t["w"], t["h"])]


# ------------------------------------------------------------------ the forms the device rests on
@pytest.mark.parametrize("t", [1, 7, 20, 60])
def test_form_a_corners_are_the_maxima_of_the_score_map(oracle, t):
    """cv::FAST(level, t, nonmax) = the strict 3 x 3 maxima of the threshold-free score map with S >= t, and also of
    the map with every S < t set to 0 (what the device stores)."""
    g = oracle.gray(synth_seq(5, seed=3, preset="fr1")[0][0])
    lv = oracle.pyramid(g, oracle.orb_params(1000))[3]
    h, w = lv.shape
    want = oracle.fast(lv, t)
    S = A.score_map(lv)
    got = A.fast_from_maxima(A.roi_maxima(S, (0, 0, w, h)), t)
    assert len(want) > 500 and np.array_equal(got, want)
    cut = np.where(S >= t, S, 0).astype(np.uint8)
    assert np.array_equal(A.roi_maxima(cut, (0, 0, w, h)), want)


def test_form_b_level_positions_survive_the_scaling():
    """cvRound((x * layerScale) * (1.f / layerScale)) == x for every integer x < 2048, every level of the accepted
    scale factors: compute()'s centre is the detector's level position, so the device keeps level coordinates."""
    x = np.arange(2048)
    for sf in (1.2, 1.25, 1.3, 1.5, 2.0):
        for s in M.layer_scales(sf, 12):
            assert np.array_equal(M.cv_round((x.astype(F32) * s) * (F32(1.0) / s)), x), (sf, s)


def test_form_c_selection_orders(oracle):
    """The selection ranks the f32 responses themselves (no rank key): an integer FAST score is exact in f32.  The
    frame stage regroups by octave always: on a list whose octaves do not decrease that changes nothing, and on the
    tie frame it equals the model's conditional regrouping."""
    assert np.array_equal(np.arange(256).astype(F32).astype(np.int64), np.arange(256))
    oc = np.repeat(np.arange(8), [5, 0, 3, 9, 1, 0, 0, 4])
    assert np.array_equal(np.argsort(oc, kind="stable"), np.arange(len(oc)))
    kps, _, rec = model_run("tie", tie_frame(oracle))
    assert rec["regroup"] and np.all(np.diff(kps["octave"]) >= 0)
    m = M.Extractor()
    k0, lx, ly, _, _ = m.detect(tie_frame(oracle))
    keep = M.border_filter(M.cv_round(k0["x"]), M.cv_round(k0["y"]), 640, 480, M.DESC_BORDER)
    always = k0[keep][np.argsort(k0[keep]["octave"], kind="stable")]
    assert np.array_equal(always, kps)


# ------------------------------------------------------------------ Harris
def test_harris_three_ways(oracle):
    # a 9 x 9 vertical step edge, 0 | 100 between columns 3 and 4: Ix = 4 * 100 at block columns 3 and 4 of all 7
    # rows, Iy = 0, so a = 7 * 2 * 400^2, b = c = 0
    patch = np.zeros((9, 9), np.uint8)
    patch[:, 4:] = 100
    a = F32(7 * 2 * 400 * 400)
    sc = F32(1.0) / F32(4 * 7 * 255.0)
    want = ((a * F32(0) - F32(0) * F32(0)) - (F32(0.04) * (a + F32(0))) * (a + F32(0))) * (sc * sc * sc * sc)
    assert M.harris_literal(patch, 4, 4).view(np.uint32) == want.view(np.uint32)
    assert M.harris(patch, [4], [4]).view(np.uint32)[0] == want.view(np.uint32)
    assert want < 0
    g = oracle.gray(synth_seq(5, seed=3, preset="fr1")[0][0])
    rs = np.random.RandomState(2)
    xs, ys = rs.randint(4, 636, 200), rs.randint(4, 476, 200)
    v = M.harris(g, xs, ys)
    lit = np.array([M.harris_literal(g, int(x), int(y)) for x, y in zip(xs, ys)], F32)
    assert np.array_equal(v.view(np.uint32), lit.view(np.uint32)) and (v > 0).any() and (v < 0).any()


# ------------------------------------------------------------------ angle and rBRIEF against the ORB2 oracle
def test_angle_and_descriptor_equal_orb2s_at_shared_positions(oracle):
    g = oracle.gray(synth_seq(5, seed=3, preset="fr1")[0][0])
    p = oracle.orb_params(1000)
    ok, od = oracle.detect_and_compute(g, p)
    sc = oracle.tables(p)["scale"]
    kps, desc, _ = model_run("fr1", g)
    ls = M.layer_scales(1.2, 8)
    mine = {}
    for i, k in enumerate(kps):
        s = F32(1.0) / ls[k["octave"]]
        mine[(int(k["octave"]), int(M.cv_round(k["x"] * s)), int(M.cv_round(k["y"] * s)))] = i
    shared = 0
    for j, k in enumerate(ok):
        key = (int(k["octave"]), int(round(float(k["x"]) / float(sc[k["octave"]]))), int(round(float(k["y"]) / float(sc[k["octave"]]))))
        if key in mine:
            i = mine[key]
            shared += 1
            assert kps["angle"][i].view(np.uint32) == k["angle"].view(np.uint32), key
            assert np.array_equal(desc[i], od[j]), key
    assert shared >= 50, shared


# ------------------------------------------------------------------ the regimes of the GPU tests' frames
def _levels(rec):
    return [(lr["n_fast"], len(lr["s1"]), len(lr["s2"])) for lr in rec["levels"]]


def test_regimes(oracle):
    N = M.budgets(1000, 1.2, 8)
    # the rich frame: every level has n > 2 N; level 0's first selection keeps score ties (more than 2 N)
    _, _, rec = model_run("fr1", oracle.gray(synth_seq(5, seed=3, preset="fr1")[0][0]))
    lv = _levels(rec)
    assert all(n > 2 * N[l] and n2 == N[l] for l, (n, n1, n2) in enumerate(lv)) and lv[0][1] > 2 * N[0]
    assert 8192 < lv[0][0] <= 12288 and not rec["frame_retain"]      # above the default cand_cap
    # the low-texture frame: n <= N, no selection
    k, _, rec = model_run("lowtex", oracle.gray(synth_seq(5, seed=7, preset="lowtex")[0][0]))
    lv = _levels(rec)
    assert 0 < lv[0][0] <= N[0] and lv[0][0] == lv[0][1] == lv[0][2] and len(k) > 0
    # the tie frame: level 0 keeps Harris ties, the frame-level retainBest and the regrouping fire, and the frame
    # keeps more than nfeatures
    k, _, rec = model_run("tie", tie_frame(oracle))
    lv = _levels(rec)
    assert lv[0][2] > N[0] and rec["total"] > 1250 and rec["frame_retain"] and rec["regroup"]
    assert 1000 < len(k) <= 1250 and lv[0][0] <= 12288
    # a flat frame
    k, _, rec = model_run("flat", np.full((480, 640), 128, np.uint8))
    assert len(k) == 0 and rec["total"] == 0
    # 320 x 248 at 2.0 / 3: level 1 has N < n <= 2 N (the first selection idle, the second active); the last level
    # (80 x 62) is narrower than 2 * 31 + 1 and keeps nothing although it has corners
    g = oracle.gray(small_frame(oracle)[0][0])
    m = M.Extractor(SMALL["prm"], W=SMALL["W"], H=SMALL["H"])
    assert m.sizes[-1] == (80, 62)
    _, _, rec = model_run("small", g, SMALL["prm"], SMALL["W"], SMALL["H"])
    lv = _levels(rec)
    assert m.N[1] < lv[1][0] <= 2 * m.N[1] and lv[1][1] == lv[1][0] and lv[1][2] == m.N[1]
    assert lv[2] == (0, 0, 0) and len(oracle.fast(oracle.pyramid(g, m.orb)[2], 20)) > 0
    # nfeatures 300 at 1.5 / 3 with edge_threshold 22: the descriptor's 31-px border drops detected keypoints
    g = oracle.gray(small_frame(oracle, "fr3", 5, 320, 256)[0][0])
    k, _, rec = model_run("p300", g, P300["prm"], P300["W"], P300["H"])
    assert rec["n_detect"] == 300 and 200 < len(k) < 300
