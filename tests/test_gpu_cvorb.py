"""GPU parity: the OpenCV ORB front end (the reference's Extractor(ORB, ORB, NORMAL)) on gfx950 vs the CPU model
(tests/cvorb_model.py, held together by tests/test_cvorb_model.py), bit for bit: per (frame, level) the FAST count
after the border filter, the list after retainBest(2 N), its Harris responses and the list after retainBest(N); the
final keypoints / descriptors / undistorted keypoints / 3D points, batches, both per-frame capacity flags, the
refusals, and the tracking chains on a cv::ORB context.  Calls go through the C ABI; inputs are seeded synthetic
RGB-D frames.  The rich frames' level 0 holds more FAST corners than the default cand_cap (8192) stores, so the
contexts here take the largest one (12288) unless the test is about the cap."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, synth_seq
import chain_model
import cvorb_model as M
from test_cvorb_model import P300, SMALL, small_frame, tie_frame

pytestmark = pytest.mark.gpu

_MODEL = {}
CAP = 12288


def _cam(pkg, cam):
    return pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"],
                      cam["k3"], cam["factor"])


def _ctx(pkg, cam, max_batch=1, W=640, H=480, prm=None, cand_cap=CAP, max_keypoints=0):
    prm = prm or M.params()
    return pkg.Context(W, H, max_batch=max_batch, cam=_cam(pkg, cam),
                       cvorb=pkg.cvorb_params(cand_cap=cand_cap, max_keypoints=max_keypoints, **prm))


def _dev(bgr, depth):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(bgr)).cuda(),
            torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda())


def _want(key, bgr, depth, cam, prm=None):
    """The model's frame, computed once per test session and left unchanged."""
    if key not in _MODEL:
        H, W = bgr.shape[:2]
        _MODEL[key] = M.Extractor(prm, W=W, H=H).frame(bgr, depth, cam)
    return _MODEL[key]


def _same_frame(got, want, at=None):
    assert len(got["kps"]) == len(want["kps"]), (at, len(got["kps"]), len(want["kps"]))
    assert np.array_equal(got["kps"], want["kps"]), at
    assert np.array_equal(got["desc"], want["desc"]), at
    assert np.array_equal(got["kps_un"], want["kps_un"]), at
    assert np.array_equal(got["xyz"].view(np.uint32), want["xyz"].view(np.uint32)), at


def _same_levels(ctx, b, rec, at=None):
    """All four debug stages of every level of frame b."""
    for l, lr in enumerate(rec["levels"]):
        got = ctx.cvorb_debug_level(b, l)
        assert got["n_fast"] == lr["n_fast"], (at, l, got["n_fast"], lr["n_fast"])
        assert np.array_equal(got["s1"], lr["s1"]), (at, l, len(got["s1"]), len(lr["s1"]))
        assert np.array_equal(got["h1"].view(np.uint32), lr["h1"].view(np.uint32)), (at, l)
        assert np.array_equal(got["s2"], lr["s2"]), (at, l, len(got["s2"]), len(lr["s2"]))
        assert np.array_equal(got["h2"].view(np.uint32), lr["h2"].view(np.uint32)), (at, l)


def _gray3(g):
    """A BGR frame whose gray image is g."""
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


def _batch3(oracle):
    """[rich, lowtex, tie] at 640 x 480 with their model frames."""
    rb, rd, _, cam = synth_seq(5, seed=3, preset="fr1")
    lb, ld, _, _ = synth_seq(5, seed=7, preset="lowtex")
    tg = tie_frame(oracle)
    bgr = np.stack([rb[0], lb[0], _gray3(tg)])
    depth = np.stack([rd[0], ld[0], rd[0]])
    assert np.array_equal(oracle.gray(bgr[2]), tg)
    want = [_want(("batch3", b), bgr[b], depth[b], cam) for b in range(3)]
    return bgr, depth, cam, want


# ------------------------------------------------------------------ stages and whole frames
def test_stages_and_batch_equal_model_and_single_frames(pkg, oracle):
    bgr, depth, cam, want = _batch3(oracle)
    assert want[2]["rec"]["frame_retain"] and want[2]["rec"]["regroup"] and len(want[2]["kps"]) > 1000
    a = _ctx(pkg, cam, max_batch=3)
    b1 = _ctx(pkg, cam, max_batch=1)
    d_bgr, d_dep = _dev(bgr, depth)
    a.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 3)
    for b in range(3):
        _same_levels(a, b, want[b]["rec"], b)
        got = a.batch_frame(b)
        _same_frame(got, want[b], b)
        _same_frame(b1.frame(bgr[b], depth[b]), got, b)
        _same_levels(b1, 0, want[b]["rec"], ("single", b))
    a.close()
    b1.close()


@pytest.mark.parametrize("preset,seed", [("fr1", 3), ("fr3", 11), ("icl", 23)])
def test_frames_bit_exact(pkg, oracle, preset, seed):
    bgr, depth, _, cam = synth_seq(5 if preset == "fr1" else 3 if preset == "fr3" else 2, seed=seed, preset=preset)
    if preset == "fr1":
        assert cam["k1"] != 0   # the distorted camera: kps_un differ from kps
    ctx = _ctx(pkg, cam)
    for f in range(2):
        want = _want((preset, seed, f), bgr[f], depth[f], cam)
        assert len(want["kps"]) > 900
        got = ctx.frame(bgr[f], depth[f])
        _same_frame(got, want, (preset, f))
        _same_levels(ctx, 0, want["rec"], (preset, f))
        if preset == "fr1":
            assert not np.array_equal(got["kps_un"]["x"], got["kps"]["x"])
    # detect_and_compute from a gray image (Extractor::detectAndCompute)
    g = oracle.gray(bgr[0])
    k, d = ctx.detect_and_compute(g)
    wk, wd, _ = M.Extractor().detect_and_compute(g)
    assert np.array_equal(k, wk) and np.array_equal(d, wd)
    # it uses ORB's pattern: the BRIEF table entry points refuse it
    with pytest.raises(pkg.RgbdError, match="not an SVO"):
        ctx.set_brief_pattern(np.zeros((256, 4), np.int8))
    ctx.close()


def test_small_shape_with_an_empty_last_level(pkg, oracle):
    """320 x 248 at 2.0 / 3: the last level (80 x 62) is narrower than 2 * 31 + 1."""
    bgr, depth, _, cam = small_frame(oracle)
    W, H, prm = SMALL["W"], SMALL["H"], SMALL["prm"]
    ctx = _ctx(pkg, cam, max_batch=2, W=W, H=H, prm=prm)
    want = [_want(("small", b), bgr[b], depth[b], cam, prm) for b in range(2)]
    assert all(w["rec"]["levels"][2]["n_fast"] == 0 and len(w["kps"]) > 500 for w in want)
    d_bgr, d_dep = _dev(bgr, depth)
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 2)
    for b in range(2):
        _same_levels(ctx, b, want[b]["rec"], b)
        _same_frame(ctx.batch_frame(b), want[b], b)
    ctx.close()


def test_parameters(pkg, oracle):
    """nfeatures 300, 3 levels at 1.5, edge_threshold 22, fast_threshold 7."""
    bgr, depth, _, cam = small_frame(oracle, "fr3", 5, 320, 256)
    W, H, prm = P300["W"], P300["H"], P300["prm"]
    ctx = _ctx(pkg, cam, max_batch=2, W=W, H=H, prm=prm)
    assert ctx.kp_cap == 375
    want = [_want(("p300", b), bgr[b], depth[b], cam, prm) for b in range(2)]
    assert all(w["rec"]["n_detect"] == 300 and 200 < len(w["kps"]) < 300 for w in want)
    d_bgr, d_dep = _dev(bgr, depth)
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 2)
    for b in range(2):
        _same_levels(ctx, b, want[b]["rec"], b)
        _same_frame(ctx.batch_frame(b), want[b], b)
    ctx.close()


# ------------------------------------------------------------------ the capacity flags
def test_cand_cap_flag_per_frame(pkg, oracle):
    """cand_cap one below the rich frame's level-0 count: that frame alone overflows."""
    bgr, depth, cam, want = _batch3(oracle)
    n0 = want[0]["rec"]["levels"][0]["n_fast"]
    assert n0 > want[1]["rec"]["levels"][0]["n_fast"]
    lb, ld, _, _ = synth_seq(5, seed=7, preset="lowtex")
    bgr, depth = np.stack([lb[0], bgr[0], lb[1]]), np.stack([ld[0], depth[0], ld[1]])
    w2 = _want(("lowtex", 7, 1), lb[1], ld[1], cam)
    ctx = _ctx(pkg, cam, max_batch=3, cand_cap=n0 - 1)
    d_bgr, d_dep = _dev(bgr, depth)
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 3)
    _same_frame(ctx.batch_frame(0), want[1], 0)
    _same_frame(ctx.batch_frame(2), w2, 2)
    with pytest.raises(pkg.RgbdError, match="cand_cap"):
        ctx.batch_frame(1)
    assert ctx.cvorb_debug_level(1, 0)["n_fast"] == n0          # the count goes on past the cap
    with pytest.raises(pkg.RgbdError, match="cand_cap"):      # a tracking chain fails the whole call, same cause
        ctx.pnp_track_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 3, 0.9, pkg.pnp_params(), np.eye(4, dtype=np.float32))
    _same_frame(ctx.frame(lb[0], ld[0]), want[1], "after")      # flag cleared
    ctx.close()
    ctx = _ctx(pkg, cam, cand_cap=n0)                           # exactly the count: no overflow
    _same_frame(ctx.frame(bgr[1], depth[1]), want[0], "at the cap")
    ctx.close()


def test_max_keypoints_flag_per_frame(pkg, oracle):
    """The tie frame keeps more than nfeatures; with max_keypoints below its count it fails alone."""
    bgr, depth, cam, want = _batch3(oracle)
    n = len(want[2]["kps"])
    assert n > 1001
    ctx = _ctx(pkg, cam, max_batch=3, max_keypoints=n - 1)
    d_bgr, d_dep = _dev(bgr, depth)
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 3)
    for b in (0, 1):
        _same_frame(ctx.batch_frame(b), want[b], b)
    with pytest.raises(pkg.RgbdError, match="max_keypoints"):
        ctx.batch_frame(2)
    _same_frame(ctx.frame(bgr[0], depth[0]), want[0], "after")
    ctx.close()
    ctx = _ctx(pkg, cam, max_keypoints=n)
    _same_frame(ctx.frame(bgr[2], depth[2]), want[2], "at the cap")
    ctx.close()


# ------------------------------------------------------------------ refusals
def test_refusals(pkg):
    lib = pkg.lib()
    cam = pkg.camera(500, 500, 320, 240)
    bad = [dict(nfeatures=0), dict(nfeatures=8193), dict(fast_threshold=0), dict(fast_threshold=256),
           dict(edge_threshold=21), dict(edge_threshold=256), dict(cand_cap=12289), dict(cand_cap=-1),
           dict(nfeatures=1000, max_keypoints=999)]
    for kw in bad:
        h = C.c_void_p()
        st = lib.rgbd_create_cvorb(0, 640, 480, 1, C.byref(pkg.cvorb_params(**kw)), C.byref(cam), C.byref(h))
        assert st == 4 and b"cv::ORB" in lib.rgbd_last_error(h), (kw, st)
        lib.rgbd_destroy(h)
    # the ORB geometry's rules: a width that is no multiple of 16, too many levels, a level below 48 px
    for W, H, kw in ((650, 480, {}), (640, 480, dict(nlevels=13)), (320, 256, dict(nlevels=12))):
        h = C.c_void_p()
        assert lib.rgbd_create_cvorb(0, W, H, 1, C.byref(pkg.cvorb_params(**kw)), C.byref(cam), C.byref(h)) == 4, (W, H, kw)
        lib.rgbd_destroy(h)
    with pytest.raises(ValueError):
        pkg.Context(640, 480, cam=cam, cvorb=pkg.cvorb_params(), svo=pkg.svo_params())
    # the bounds themselves are accepted
    ctx = pkg.Context(640, 480, max_batch=1, cam=cam, cvorb=pkg.cvorb_params(nfeatures=8192, edge_threshold=22, cand_cap=12288))
    assert ctx.kp_cap == 8192 + 2048
    ctx.close()
    # the other extractors' contexts have no cv::ORB stage
    for kw in (dict(), dict(svo=pkg.svo_params()), dict(gftt=pkg.gftt_params())):
        ctx = pkg.Context(640, 480, max_batch=1, cam=cam, **kw)
        n = C.c_int32(0)
        assert lib.rgbd_cvorb_debug_level(ctx._h, 0, 0, 0, None, None, 0, C.byref(n)) == 1
        assert b"not a cv::ORB context" in lib.rgbd_last_error(ctx._h)
        ctx.close()


# ------------------------------------------------------------------ chains
def test_pnp_chain_matches_model(pkg, oracle):
    """Extract (cv::ORB) + Matcher + PnPRansac per consecutive pair, bit-exact vs the oracle chain over the model's
    frames."""
    B = 5
    bgr, depth, gt, cam = synth_seq(B, seed=21, preset="fr1")
    ctx = _ctx(pkg, cam, max_batch=B)
    d_bgr, d_dep = _dev(bgr, depth)
    pose0 = gt[0].astype(np.float32)
    poses, status, ninl, nm = ctx.pnp_track_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B, 0.9, pkg.pnp_params(), pose0)
    frames = [_want(("fr1", 21, i), bgr[i], depth[i], cam) for i in range(B)]
    K4 = np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], np.float32)
    wp, ws, wn, wm = chain_model.pnp_track(oracle, frames, pose0, K4)
    assert np.array_equal(nm, wm) and np.array_equal(status, ws) and np.array_equal(ninl, wn)
    assert np.array_equal(poses.view(np.uint32), wp.view(np.uint32))
    assert status.all()
    ctx.close()


@pytest.mark.parametrize("solver", ["pnp", "se3"])
def test_track_sequence_batches_equal_one_batch(pkg, tmp_path, solver):
    from rgbd_slam_amd import datasets as D
    from rgbd_slam_amd.sequence import track_sequence
    n = 7
    bgr, depth, gt, cam = synth_seq(n, seed=21, preset="fr1")
    base = str(tmp_path / "rgbd_dataset_freiburg1_seq") + os.sep
    D.write_dataset(base, bgr, depth, 100.0 + 0.033 * np.arange(n), gt)
    ds = D.open_dataset(base)
    p4, s4, i4 = track_sequence(pkg, ds, B=4, solver=solver, pose0=gt[0], extractor="cvorb")
    pn, sn, i_n = track_sequence(pkg, ds, B=n, solver=solver, pose0=gt[0], extractor="cvorb")
    assert np.array_equal(p4.view(np.uint32), pn.view(np.uint32))
    assert np.array_equal(s4, sn) and np.array_equal(i4, i_n) and sn[0] == 1 and sn.sum() > 1


def test_cpp_example_matches_python(pkg, oracle, tmp_path):
    """examples/cvorb_example.cpp (rgbd::Extractor(ORB, ORB, NORMAL) over include/rgbd/frontend.hpp) prints an FNV-1a
    hash of every frame's keypoints and descriptors; (ORB, BRIEF) and (ORB, ORB, ADAPTIVE) still throw."""
    exe = os.path.join(ROOT, "rgbd-slam_amd", "build", "cvorb_example")
    assert os.path.exists(exe), "build() must compile examples/cvorb_example.cpp"
    n = 3
    bgr, depth, _, cam = synth_seq(5, seed=3, preset="fr1")
    raw = tmp_path / "seq.raw"
    with open(raw, "wb") as f:
        for i in range(n):
            f.write(np.ascontiguousarray(bgr[i]).tobytes())
            f.write(np.ascontiguousarray(depth[i]).tobytes())
    args = [exe, str(raw), str(n)] + ["%r" % float(cam[k]) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2",
                                                                       "k3", "factor")]
    out = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[-2:] == ["ORB BRIEF: throws", "ORB ADAPTIVE: throws"]
    rows = [l.split() for l in lines[:-2]]
    assert len(rows) == n

    def fnv(*arrays):
        h = 0xcbf29ce484222325
        for a in arrays:
            for byte in np.ascontiguousarray(a).view(np.uint8).reshape(-1).tolist():
                h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
        return h
    ctx = _ctx(pkg, cam)
    for i in range(n):
        got = ctx.frame(bgr[i], depth[i])
        assert int(rows[i][1]) == len(got["kps"]) > 900
        assert int(rows[i][2], 16) == fnv(got["kps"], got["desc"]), i
        assert int(rows[i][3]) == ctx.cvorb_debug_level(0, 0)["n_fast"]
    ctx.close()
