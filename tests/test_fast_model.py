"""CPU: the model of the plain FAST extractor (tests/fast_model.py) against the oracle's cv::FAST, libstdc++'s
nth_element + partition at the sizes the whole-image detector produces, and cvorb_model's compute path; and the corner
counts of the frames the GPU tests use (so those cannot pass on an easy regime: every rich frame has more corners than
select_dev.h's 12,288-element LDS selection holds)."""
import numpy as np
import pytest

import adaptive_model as A
import cvorb_model as CV
import fast_cases as FC
import fast_model as F


@pytest.mark.parametrize("name", ["fr1", "lowtex", "flat", "noise", "binary"])
def test_detector_equals_cv_fast(oracle, name):
    g = FC.gray(name)
    for t in (1, 10, 20, 254):
        got, want = F.corners(g, t), oracle.fast(g, t)
        assert np.array_equal(got, want), (name, t, len(got), len(want))
    assert len(F.corners(g, 255)) == 0   # no score reaches 255


@pytest.mark.parametrize("name", sorted(FC.COUNTS))
def test_corner_counts(oracle, name):
    g = FC.gray(name)
    n1, n10, kept = FC.COUNTS[name]
    c10 = F.corners(g, 10)
    assert (len(F.corners(g, 1)), len(c10)) == (n1, n10)
    k, rec = F.Extractor().detect(g)
    assert len(k) == kept and np.array_equal(rec["raster"], c10)
    if n10 <= 1000:   # retainBest does not fire: raster order survives
        assert np.array_equal(rec["kept"], np.arange(n10))
    else:
        assert kept >= 1000 and k["response"][:kept].min() == np.sort(c10[:, 2])[::-1][999]


@pytest.mark.parametrize("name", ["fr1", "noise"])
def test_retain_best_matches_libstdcxx(oracle, name):
    """The restated nth_element + partition against libstdc++'s (the oracle's retainBest) on the detector's own
    responses: n = 13,715 and 31,337, nfeatures 1000, 1 and n - 1, and at forced depth limits."""
    r = F.corners(FC.gray(name), 10)[:, 2].astype(np.float32)
    n = len(r)
    assert n == FC.COUNTS[name][1]
    for keep in (1000, 1, n - 1):
        got, want = F.retain_best(r, keep), oracle.retain_best(r, keep)
        assert np.array_equal(got, want), (name, keep, len(got), len(want))
    for depth in (0, 1):
        assert np.array_equal(F.retain_best(r, 1000, depth), oracle.retain_best_depth(r, 1000, depth)), depth
    assert np.array_equal(F.retain_best(r, n), np.arange(n)) and len(F.retain_best(r, 0)) == 0


def test_orb_branch_equals_cvorb_compute_path(oracle):
    """cv::ORB::compute() on provided keypoints, two ways: fast_model.orb_describe and cvorb_model's own pieces called
    as its Extractor.detect_and_compute calls them for octave-0 keypoints (border 31 on cvRound, O.blur, rbrief at the
    keypoint's angle).  The angle is the stored -1, not IC_Angle's."""
    g = FC.gray("fr1")
    kps, _ = F.Extractor(F.params(descriptor="orb")).detect(g)
    got_k, got_d = F.orb_describe(g, kps)
    keep = CV.border_filter(CV.cv_round(kps["x"]), CV.cv_round(kps["y"]), 640, 480, CV.DESC_BORDER)
    want_k = kps[keep]
    blurred = oracle.blur(g)
    want_d = np.stack([CV.rbrief(blurred, int(k["x"]), int(k["y"]), k["angle"]) for k in want_k])
    assert np.array_equal(got_k, want_k) and np.array_equal(got_d, want_d) and 500 < len(got_k) < len(kps)
    assert np.all(got_k["angle"] == -1.0) and np.all(got_k["size"] == 7.0) and np.all(got_k["octave"] == 0)
    # a recomputed angle would give other descriptors
    ic = np.stack([CV.rbrief(blurred, int(k["x"]), int(k["y"]), CV.ic_angle(g, int(k["x"]), int(k["y"]))) for k in want_k[:50]])
    assert not np.array_equal(ic, want_d[:50])
    # BRIEF's border is 28, ORB's 31: the two descriptors keep different keypoints
    bk, _, _ = F.Extractor().detect_and_compute(g)
    assert len(bk) > len(got_k)
