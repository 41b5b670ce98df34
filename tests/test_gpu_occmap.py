"""GPU: the occupancy map on real keyframe clouds.  The first three frames of the synthetic fr1 sequence, clouds from
ctx.keyframe_cloud with the default parameters, poses = the sequence's ground truth through occmap.sensor_pose: scan by
scan, as one batch, and the Python model (tests/occmap_model.py) agree bit for bit; MapBuilder rebuilds after a moved
big-change index like a fresh model build."""
import os
import subprocess

import numpy as np
import pytest

import occmap_model as M
from conftest import ROOT, synth_seq

pytestmark = pytest.mark.gpu

CAP = 1 << 16


def _rot(axis, ang):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


@pytest.fixture(scope="module")
def data(pkg):
    """(ctx, clouds, Tcw f32) of the three keyframes, and the model maps after each of them."""
    bgr, depth, poses, cam = synth_seq(4, seed=3, preset="fr1")
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"],
                   cam["factor"])
    ctx = pkg.Context(640, 480, max_batch=1, orb=pkg.orb_params(1000), cam=c)
    clouds = [ctx.keyframe_cloud(bgr[f], depth[f]) for f in range(3)]
    Tcw = [np.asarray(poses[f], np.float32) for f in range(3)]
    ref = M.Map(M.Params(capacity=CAP))
    want = []
    for cl, T in zip(clouds, Tcw):
        Twc, o = M.sensor_pose(T)
        assert ref.insert(cl, Twc, o)
        want.append(ref.leaves())
    yield ctx, clouds, Tcw, want
    ctx.close()


def assert_leaves(m, want, what):
    keys, lo, rgb = m.leaves()
    assert len(m) == len(want[0]) == len(keys), what
    assert np.array_equal(keys, want[0]), what
    assert np.array_equal(lo.view(np.uint32), want[1].view(np.uint32)), what
    assert np.array_equal(rgb, want[2]), what


def test_sensor_pose_equals_model(pkg, data):
    from rgbd_slam_amd import occmap
    _, _, Tcw, _ = data
    cases = list(Tcw)
    for ax, ang in (((0, 0, 1), 0.3), ((1, 0, 0), 3.0), ((0, 1, 0), 3.0), ((0, 0, 1), 3.0)):   # one per Shepperd branch
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = _rot(ax, ang).T
        T[:3, 3] = (0.3, -1.2, 0.7)
        cases.append(T)
    for T in cases:
        got, want = occmap.sensor_pose(T), M.sensor_pose(T)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        assert np.array_equal(got[0][:, 3], got[1])


def test_scan_by_scan_batch_and_model_agree(pkg, data):
    from rgbd_slam_amd import occmap
    ctx, clouds, Tcw, want = data
    assert all(1000 < len(c) <= 16384 for c in clouds)
    sp = [occmap.sensor_pose(T) for T in Tcw]
    m = pkg.OccupancyMap(ctx, pkg.occmap_params(capacity=CAP))
    try:
        for i in range(3):
            m.insert(clouds[i], sp[i][0], sp[i][1])
            assert_leaves(m, want[i], f"scan {i}")
        assert len(m) > 2000
        m.clear()
        assert m.insert_batch(clouds, [p[0] for p in sp], [p[1] for p in sp]) == 3
        assert_leaves(m, want[2], "batch")
        # the leaf query: what render draws
        centres, half, rgb, occ = occmap.render_leaves(m)
        keys, lo, col = want[2]
        sel = lo >= pkg.occmap_logodds(0.9)
        assert half == 0.04 and sel.any() and not sel.all()
        assert np.array_equal(centres, ((keys[sel].astype(np.float64) - 32768) + 0.5) * 0.08) and np.array_equal(rgb, col[sel])
        assert (occ >= 0.9 - 1e-7).all()
    finally:
        m.close()


def test_occmap_sequence_is_the_map_of_the_keyframes(pkg, data):
    """What tools/run_sequence.py --occmap writes: clouds and scans on the device, leaves as the model's."""
    from rgbd_slam_amd import occmap
    _, _, Tcw, want = data
    bgr, depth, _, cam = synth_seq(4, seed=3, preset="fr1")
    keys, prob, lo, rgb = occmap.occmap_sequence(pkg, lambda k: (bgr[k], depth[k]), cam, Tcw, [0, 1, 2], capacity=CAP)
    assert np.array_equal(keys, want[2][0]) and np.array_equal(rgb, want[2][2])
    assert np.array_equal(lo.view(np.uint32), want[2][1].view(np.uint32))
    assert prob.min() > 0.0009 and prob.max() < 0.9991 and ((prob > 0.5) == (lo > 0)).all()


def test_cpp_occmap_example(pkg, data, tmp_path):
    """examples/occmap_example.cpp (rgbd::OctomapDrawer of include/rgbd/frontend.hpp) prints the model's leaves."""
    exe = os.path.join(ROOT, "rgbd-slam_amd", "build", "occmap_example")
    assert os.path.exists(exe), "build() must compile examples/occmap_example.cpp"
    _, _, Tcw, want = data
    bgr, depth, _, cam = synth_seq(4, seed=3, preset="fr1")
    raw, pf = tmp_path / "frames.raw", tmp_path / "poses.raw"
    with open(raw, "wb") as f:
        for i in range(3):
            f.write(np.ascontiguousarray(bgr[i]).tobytes())
            f.write(np.ascontiguousarray(depth[i]).tobytes())
    np.stack(Tcw).astype(np.float32).tofile(pf)
    args = [exe, str(raw)] + ["%r" % float(cam[k]) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "factor")]
    out = subprocess.run(args + [str(pf), "3"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    assert lines[:4] == ["size %d" % len(w[0]) for w in want] + ["rebuilt %d" % len(want[2][0])]
    keys, lo, rgb = want[2]
    leaves = ["%d %d %d %08x %d %d %d" % (*k, b, *c) for k, b, c in zip(keys.tolist(), lo.view(np.uint32).tolist(), rgb.tolist())]
    assert lines[4:4 + len(leaves)] == leaves
    assert lines[4 + len(leaves)] == "render %d" % int((lo >= pkg.occmap_logodds(0.9)).sum())


def test_map_builder_rebuilds_on_big_change(pkg, data):
    from rgbd_slam_amd import occmap
    ctx, clouds, Tcw, want = data
    b = occmap.MapBuilder(ctx, pkg.occmap_params(capacity=CAP))
    try:
        assert b.update([(10, clouds[0], Tcw[0]), (14, clouds[1], Tcw[1])]) == 2
        assert_leaves(b.map, want[1], "two keyframes")
        # the ids already inserted are skipped, whatever their poses are now; a keyframe without a cloud is passed over
        moved = [T.copy() for T in Tcw]
        for k, T in enumerate(moved):
            T[:3, 3] += np.float32(0.013 * (k + 1))
            T[:3, :3] = (_rot((0.2, 1, 0.1), 0.01 * (k + 1)) @ T[:3, :3].astype(float)).astype(np.float32)
        kfs = [(10, clouds[0], moved[0]), (14, clouds[1], moved[1]), (15, None, moved[1]), (19, clouds[2], Tcw[2])]
        assert b.update(kfs) == 1
        assert_leaves(b.map, want[2], "third keyframe")
        assert b.update(kfs) == 0
        # a loop closure: the big-change index moves, the map is rebuilt from every keyframe at its corrected pose
        kfs[3] = (19, clouds[2], moved[2])
        assert b.update(kfs, big_change_idx=1) == 3
        ref = M.Map(M.Params(capacity=CAP))
        for (_, cl, T) in kfs:
            if cl is not None:
                assert ref.insert(cl, *M.sensor_pose(T))
        assert_leaves(b.map, ref.leaves(), "rebuilt")
        assert not np.array_equal(ref.leaves()[0], want[2][0])
        assert b.update(kfs, big_change_idx=1) == 0
    finally:
        b.close()
