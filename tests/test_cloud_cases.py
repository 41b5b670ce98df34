"""Every case of cloud_cases.py reaches the regime it is named for, asserted from the oracle alone: a case that
drifts out of its regime fails here, on the CPU, and cannot pass silently in test_gpu_cloud_cases.py."""
import numpy as np
import pytest

import cloud_cases as cc


def _s(oracle, name):
    return cc.case_stages(oracle, name), cc.case(name)[3]


def test_names_and_setup():
    assert len(set(cc.NAMES)) == len(cc.NAMES) == 15
    for name in cc.NAMES:
        bgr, depth, cam, kw = cc.case(name)
        assert bgr.shape == (128, 128, 3) and bgr.dtype == np.uint8
        assert depth.shape == (128, 128) and depth.dtype == np.uint16
        assert (cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["factor"]) == (128.0, 128.0, 64.0, 64.0, 5000.0)
        assert set(kw) == set(cc.DEFAULTS)
        assert 16384 >= ((128 + kw["stride"] - 1) // kw["stride"]) ** 2
    assert np.float32(5000) * cc.scale() + np.float32(0) == np.float32(1.0)


@pytest.mark.parametrize("name", ["empty_zero", "empty_range"])
def test_empty(oracle, name):
    s, _ = _s(oracle, name)
    assert len(s["cloud"]) == len(s["voxel"]) == len(s["out"]) == 0
    if name == "empty_range":   # valid depth, all of it below zmin
        d = cc.case(name)[1]
        assert np.all(d > 0) and np.all(cc.depth_f32(d) < np.float32(0.5))


def test_one_point(oracle):
    s, _ = _s(oracle, "one_point")
    assert len(s["cloud"]) == len(s["voxel"]) == len(s["out"]) == 1
    assert s["dist"][0] == 0.0


def test_two_points(oracle):
    s, kw = _s(oracle, "two_points")
    assert len(s["cloud"]) == len(s["voxel"]) == len(s["out"]) == 2
    assert np.all(s["dist"] > 10 * kw["leaf"] / kw["sor_k"])   # far apart


def test_few_points(oracle):
    s, kw = _s(oracle, "few_points")
    assert len(s["cloud"]) == len(s["voxel"]) == 9 < kw["sor_k"] + 1
    assert len(s["out"]) == 8


def test_plane_ties(oracle):
    """The (k+1)-th and (k+2)-th smallest float distances are equal: the cut falls inside a run of equal values."""
    s, kw = _s(oracle, "plane_ties")
    assert len(s["cloud"]) == 16384 and len(s["voxel"]) == 1024
    assert np.all(s["cloud"]["z"] == np.float32(1.0))
    d2 = np.sort(cc.sq_dist(s["voxel"]), axis=1)
    k = kw["sor_k"]
    tied = int(np.sum(d2[:, k] == d2[:, k + 1]))
    assert tied >= 512, tied
    assert 0 < len(s["out"]) < 1024


def test_plane_ties_k8(oracle):
    """Equal distances inside the k + 1 kept ones."""
    s, kw = _s(oracle, "plane_ties_k8")
    assert len(s["cloud"]) == 16384 and len(s["voxel"]) == 256
    d2 = np.sort(cc.sq_dist(s["voxel"]), axis=1)
    k = kw["sor_k"]
    inner = int(np.sum(np.any(d2[:, 1:k] == d2[:, 2:k + 1], axis=1)))
    assert inner >= 240, inner


def test_plane_ties_k63(oracle):
    """k + 1 = 64 values fill the lanes of the sort and the cut falls inside a run of equal values, so more than
    64 values are <= the 64th smallest: a selection that took them all would overflow the lanes."""
    s, kw = _s(oracle, "plane_ties_k63")
    assert kw["sor_k"] == 63 and len(s["voxel"]) == 1024
    d2 = np.sort(cc.sq_dist(s["voxel"]), axis=1)
    over = int(np.sum(np.sum(d2 <= d2[:, 63:64], axis=1) > 64))
    assert over >= 512, over
    assert 0 < len(s["out"]) < 1024


def test_tiny_leaf(oracle):
    s, _ = _s(oracle, "tiny_leaf")
    assert len(s["cloud"]) == 16384
    assert np.array_equal(s["voxel"].view(np.uint8), s["cloud"].view(np.uint8))   # 16384 points go into SOR
    p = s["cloud"]
    cells = 1
    for a in "xyz":   # VoxelGrid's own test: the voxel count over the bounds exceeds an int
        cells *= int((p[a].max() - p[a].min()) * (np.float32(1.0) / np.float32(1e-5))) + 1
    assert cells > 2 ** 31 - 1
    assert 0 < len(s["out"]) < 16384


def test_one_voxel(oracle):
    """leaf 100 puts every point into the voxel of its x / y signs (floor of a small negative is -1): at most
    four voxels, so one thread sums a run of at least 4096 points, four 1024-thread passes of the run scan."""
    s, _ = _s(oracle, "one_voxel")
    assert len(s["cloud"]) == 16384
    assert 1 <= len(s["voxel"]) <= 4
    assert 16384 // len(s["voxel"]) > 1024


def test_k63(oracle):
    s, kw = _s(oracle, "k63")
    assert kw["sor_k"] == 63 and len(s["voxel"]) > 64
    assert 0 < len(s["out"]) < len(s["voxel"])


def test_k1(oracle):
    s, kw = _s(oracle, "k1")
    assert kw["sor_k"] == 1 and len(s["voxel"]) > 2
    assert 0 < len(s["out"]) < len(s["voxel"])


def test_holes(oracle):
    s, _ = _s(oracle, "holes")
    assert 8192 < len(s["cloud"]) < 16384   # the sort is padded to 16384 keys
    assert 0 < len(s["out"]) < len(s["voxel"]) <= len(s["cloud"])


def test_limits(oracle):
    s, kw = _s(oracle, "limits")
    d = cc.case("limits")[1][::2, ::2]
    assert sorted(np.unique(d)) == [2499, 2500, 20000, 20001]
    assert len(s["cloud"]) == d.size // 2 == 2048   # exactly half: the two values on the limits
    assert set(np.unique(s["cloud"]["z"]).tolist()) == {0.5, 4.0}
    assert np.float32(kw["zmin"]) == np.float32(0.5) and np.float32(kw["zmax"]) == np.float32(4.0)


def test_std0(oracle):
    s, kw = _s(oracle, "std0")
    assert kw["sor_std"] == 0.0
    assert 0 < len(s["out"]) < len(s["voxel"])
