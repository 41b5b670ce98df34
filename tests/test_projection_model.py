"""CPU: the numpy restatement of Matcher::projectionMatch (tests/projection_model.py) against a grid-free brute
force, hand-computed quirk cases, the take-cascade and the conditions real frames put it under; and the C ABI's
argument validation without a device."""
import ctypes as C

import numpy as np
import pytest

import projection_cases as PC
import projection_model as PM


def test_model_equals_grid_free_brute_force():
    rs = np.random.default_rng(21)
    n = 300
    x2 = rs.uniform(2.0, 632.0, n).astype(np.float32)   # every keypoint inside the grid (column <= 63, row <= 47)
    y2 = rs.uniform(2.0, 472.0, n).astype(np.float32)
    z = rs.uniform(0.5, 4.0, n)
    u, v = rs.uniform(-30.0, 670.0, n), rs.uniform(-30.0, 510.0, n)
    xyz1 = np.stack([(u - 320.0) / 256.0 * z, (v - 240.0) / 256.0 * z, z], 1).astype(np.float32)
    xyz1[::17, 2] = 0.0
    outl = (rs.random(n) < 0.1).astype(np.uint8)
    T2 = np.eye(4, dtype=np.float32)
    T2[:3, 3] = [0.01, -0.02, 0.03]
    for th in (7.5, 30.0, 100.0):
        got = PM.candidates(xyz1, outl, PC.EYE, x2, y2, T2, PC.K4, PC.BOUNDS, th)
        want = PM.brute_candidates(xyz1, outl, PC.EYE, x2, y2, T2, PC.K4, PC.BOUNDS, th)
        assert [c for _, _, _, c in got] == want
        assert sum(len(c) for c in want) > (n if th == 100.0 else 20)   # not vacuous
    st = np.array([s for s, _, _, _ in got])
    assert {PM.SEARCHED, PM.OUTLIER, PM.NO_DEPTH, PM.OUTSIDE} <= set(st.tolist())


@pytest.mark.parametrize("name", sorted(PC.quirks()))
def test_quirk_cases(name):
    c, want = PC.quirks()[name]
    assert np.array_equal(PC.run_model(c), want), name


def test_x635_keypoint_is_in_no_cell():
    g = PM.Grid([635.0, 634.0], [100.0, 100.0], PC.BOUNDS)
    assert g.cell_of == [None, (63, 10)]
    assert g.in_area(np.float32(635), np.float32(100), 5.0) == [1]


@pytest.mark.parametrize("extra", [0, 20])
def test_cascade(extra):
    c, want = PC.cascade(extra)
    got = PC.run_model(c)
    assert np.array_equal(got, want)
    assert len(got) == 101 + extra


def test_real_frame_conditions(oracle, seq_fr1):
    """seq_fr1 frames 0 -> 1, th = 5, true poses: the greedy's take rule is no corner case on real frames."""
    bgr, depth, gt, cam = seq_fr1
    p, oc = oracle.orb_params(1000), oracle.camera(cam)
    f0, f1 = (oracle.frame(bgr[i], depth[i], p, oc) for i in range(2))
    K4 = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    stats = {}
    m = PM.projection_match(f0["xyz"], f0["desc"], None, gt[0], f1["kps_un"]["x"], f1["kps_un"]["y"], f1["xyz"][:, 2],
                            f1["desc"], gt[1], K4, PM.image_bounds(cam), 5.0, stats)
    print("matches %d, after a skip %d, not own best %d" % (len(m), stats["after_skip"], stats["not_own_best"]))
    assert len(m) >= 400
    assert stats["after_skip"] >= 100
    assert stats["not_own_best"] >= 25
    assert len(set(m["trainIdx"].tolist())) == len(m) and np.all(np.diff(m["queryIdx"]) > 0)


def test_argument_validation_without_device(pkg):
    lib = pkg.lib()
    m = C.c_int32(7)
    assert lib.rgbd_projection_match(None, None, None, None, 0, None, None, None, None, 0, None, None, C.c_float(5.0),
                                     None, 0, C.byref(m)) == 1
    assert lib.rgbd_image_bounds(None, None) == 1
    assert lib.rgbd_projection_match_batch(None, 0, None, None, None, None, C.c_float(5.0), None, None) == 1
    assert lib.rgbd_debug_projection(None, None, None, None, 0, None, None, None, None, 0, None, None, C.c_float(5.0),
                                     None, None, None, 0, None) == 1
    # a context whose creation stopped before the device (unsupported width) still validates th
    h = C.c_void_p()
    assert lib.rgbd_create(0, 650, 480, 1, C.byref(pkg.orb_params()), C.byref(pkg.camera(500, 500, 320, 240)),
                           C.byref(h)) == 4
    eye = np.eye(4, dtype=np.float32)
    for th in (-1.0, float("nan"), 65537.0, float("inf")):
        assert lib.rgbd_projection_match(h, None, None, None, 0, eye.ctypes.data, None, None, None, 0, eye.ctypes.data,
                                         None, C.c_float(th), None, 0, C.byref(m)) == 1, th
        assert b"th must be finite" in lib.rgbd_last_error(h)
        assert lib.rgbd_projection_match_batch(h, 0, None, None, None, None, C.c_float(th), None, None) == 1
    # empty inputs: RGBD_OK, no matches, nothing launched
    assert lib.rgbd_projection_match(h, None, None, None, 0, eye.ctypes.data, None, None, None, 0, eye.ctypes.data,
                                     None, C.c_float(5.0), None, 0, C.byref(m)) == 0 and m.value == 0
    b = pkg.Bounds()
    assert lib.rgbd_image_bounds(h, C.byref(b)) == 0   # k1 == 0: no device needed
    assert (b.min_x, b.max_x, b.min_y, b.max_y) == (0.0, 650.0, 0.0, 480.0)
    lib.rgbd_destroy(h)
