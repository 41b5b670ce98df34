"""CPU: the model of the adaptive FAST + BRIEF extractor (tests/adaptive_model.py) against the oracle's cv::FAST,
libstdc++'s nth_element and the SVO oracle's BRIEF, and the shape of its threshold chain on the rendered
sequences the GPU tests use (so those cannot pass on a chain that never adapts)."""
import numpy as np
import pytest

from conftest import synth_seq
import adaptive_model as A
from test_gpu_svo import _adversarial


def _gray(oracle, preset, seed, n=2):
    bgr, _, _, _ = synth_seq(5, seed=seed, preset=preset)
    return [oracle.gray(bgr[f]) for f in range(n)]


def test_derived_constants():
    prm = A.params()
    d = A.derived(prm)
    assert d == dict(cells=9, max_features=1020, grid_min=67, grid_max=113, max_per_cell=113)
    assert 20 * 0.7 == 14.0 and 14.0 * 0.7 == 9.799999999999999 and 20 * 1.3 == 26.0
    assert A.clamp_t(9.799999999999999) == 9 and A.clamp_t(10000.0) == 255 and A.clamp_t(2.6) == 2
    r = A.rois(640, 480, prm)
    assert [(y0, y1) for _, y0, _, y1 in r[::3]] == [(0, 191), (129, 351), (289, 480)]
    assert [(x0, x1) for x0, _, x1, _ in r[:3]] == [(0, 244), (182, 457), (395, 640)]
    # neither side divisible by the grid
    assert A.rois(320, 256, A.params(grid_rows=2, grid_cols=4, edge_threshold=0))[5] == (80, 128, 160, 256)


def _frames(oracle):
    rs = np.random.RandomState(5)
    out = {"fr1": _gray(oracle, "fr1", 3, 1)[0], "lowtex": _gray(oracle, "lowtex", 7, 1)[0],
           "flat": np.full((480, 640), 128, np.uint8), "noise": rs.randint(0, 256, (480, 640)).astype(np.uint8)}
    return out


def test_literal_fast_equals_score_map(oracle):
    """One cv::FAST per try and ROI == the strict maxima of the threshold-free score map with S >= t, at every
    threshold the adjuster tries from the initial state and at 1, 2 and 254."""
    prm = A.params()
    drv = A.derived(prm)
    for name, g in _frames(oracle).items():
        S = A.score_map(g)
        for roi in A.rois(640, 480, prm):
            mx = A.roi_maxima(S, roi)
            tried = []

            def count(t):
                tried.append(t)
                return len(A.fast_from_maxima(mx, t))
            A.cell_detect(count, prm["init_thresh"], prm, drv)
            for t in sorted(set(tried) | {1, 2, 254}):
                want = A.fast_literal(g, roi, t)
                got = A.fast_from_maxima(mx, t)
                assert np.array_equal(got, want), (name, roi, t, len(got), len(want))
        # the whole image as one ROI: the corner count of the plain detector
        whole = (0, 0, 640, 480)
        assert np.array_equal(A.fast_from_maxima(A.roi_maxima(S, whole), 20), oracle.fast(g, 20)), name


def test_literal_extractor_equals_score_map_extractor(oracle):
    for preset, seed in (("fr1", 3), ("lowtex", 7)):
        a, b = A.Extractor(), A.Extractor(literal=True)
        for g in _gray(oracle, preset, seed, 2):
            ka, ra = a.detect(g)
            kb, rb = b.detect(g)
            assert np.array_equal(ka, kb) and len(ka) > 500
            for ca, cb in zip(ra["cells"], rb["cells"]):
                assert (ca["used"], ca["tries"], ca["after"]) == (cb["used"], cb["tries"], cb["after"])
                assert np.array_equal(ca["raster"], cb["raster"]) and np.array_equal(ca["kept"], cb["kept"])
        assert np.array_equal(a.thresholds.view(np.uint64), b.thresholds.view(np.uint64))


def test_brief_equals_svo_oracle(oracle):
    g = _gray(oracle, "fr1", 3, 1)[0]
    rnd = np.random.RandomState(9).randint(-24, 25, size=(256, 4)).astype(np.int8)
    for pat in (None, rnd):
        kps, desc = oracle.svo_detect_and_compute(g, oracle.svo_params(), pattern=pat)
        assert len(kps) > 500
        k2, d2 = A.brief(g, kps, oracle.brief_default_pattern() if pat is None else pat)
        assert np.array_equal(k2, kps) and np.array_equal(d2, desc)
    # the border filter: keypoints on both sides of 28 / W - 28
    k = np.zeros(4, A.KP)
    k["x"], k["y"] = [27, 28, 611, 612], [100, 100, 100, 100]
    assert list(A.brief(g, k, rnd)[0]["x"]) == [28, 611]


def test_keep_strongest_matches_libstdcxx(oracle):
    """keepStrongest's std::nth_element(begin, begin + N, end) is retainBest(N + 1)'s nth_element whenever
    n >= N + 2 (retainBest returns early at n <= N + 1), so the first N entries of the oracle's retainBest(N + 1)
    are libstdc++'s answer.  n == N + 1 is covered by the restatement alone (checked to be a permutation whose
    last element is a minimum)."""
    rs = np.random.RandomState(17)
    for n, N in [(5, 3), (115, 113), (200, 113), (1424, 113), (4096, 113), (3000, 1000), (64, 10)]:
        for r in _adversarial(n, rs):
            assert np.array_equal(A.keep_strongest(r, N), oracle.retain_best(r, N + 1)[:N]), (n, N)
            for depth in (0, 1, 3):
                assert np.array_equal(A.keep_strongest(r, N, depth), oracle.retain_best_depth(r, N + 1, depth)[:N]), (n, N, depth)
    for r in _adversarial(114, rs):
        got = A.nth_element(r, 113)
        assert sorted(got) == list(range(114)) and r[got[113]] == r.min()
    assert np.array_equal(A.keep_strongest(np.arange(7, dtype=np.float32), 113), np.arange(7))


def test_chain_shape_rich_sequence(oracle):
    """fr1 (seed 3): every cell takes tooMany every frame, 20 -> 26 -> 33 -> 43 -> 57; retainBest(1000) runs."""
    m = A.Extractor()
    for f, g in enumerate(_gray(oracle, "fr1", 3, 5)):
        kps, rec = m.detect(g)
        cells = rec["cells"]
        assert [c["used"] for c in cells] == [[20, 26, 33, 43, 57][f]] * 9
        assert all(c["tries"] == 1 and c["branch"] == "many" for c in cells)
        if f == 0:
            n20 = [len(c["raster"]) for c in cells]
            assert min(n20) == 1424 and max(n20) == 1966
        assert all(len(c["kept"]) == 113 for c in cells) and rec["total"] == 1017 > 1000
        assert 1000 <= len(kps) <= 1017
    assert np.all(m.thresholds == 20 * 1.3 * 1.3 * 1.3 * 1.3 * 1.3)


def test_chain_shape_lowtex_sequence(oracle):
    """lowtex (seed 7): three tries per cell on frame 0 (20 -> 14 -> 9), then one- and two-try cells whose
    thresholds diverge; retainBest never runs."""
    m = A.Extractor()
    totals, used, later = [], [], set()
    for f, g in enumerate(_gray(oracle, "lowtex", 7, 5)):
        kps, rec = m.detect(g)
        cells = rec["cells"]
        if f == 0:
            assert all(c["tries"] == 3 and c["used"] == 9 for c in cells)
        else:
            later |= {c["tries"] for c in cells}
            used += [c["used"] for c in cells]
        assert rec["total"] == len(kps) <= 1000
        totals.append(rec["total"])
    assert totals == [990, 904, 867, 795, 769]
    assert later == {1, 2} and min(used) == 8 and max(used) == 12
    assert len(set(m.thresholds)) > 3


def test_flat_frames_reach_min_thresh():
    """No corners: every cell walks down to exactly min_thresh = 2.0 and the loop ends by good()'s
    min_thresh < thresh test, not by the iteration count."""
    m = A.Extractor()
    g = np.full((480, 640), 128, np.uint8)
    tries = []
    for _ in range(3):
        kps, rec = m.detect(g)
        assert len(kps) == 0
        tries.append([c["tries"] for c in rec["cells"]])
        assert all(c["branch"] == "few" for c in rec["cells"])
    assert tries == [[5] * 9, [2] * 9, [1] * 9]
    assert np.all(m.thresholds == 2.0)
