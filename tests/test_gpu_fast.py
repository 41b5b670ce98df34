"""GPU parity: the plain FAST front end (the reference's Extractor(FAST, BRIEF, NORMAL) and Extractor(FAST, ORB, NORMAL),
csrc/fast.hip) vs the CPU model (tests/fast_model.py, itself held to the oracle's cv::FAST, libstdc++ and cvorb_model by
tests/test_fast_model.py), bit-exact and stage by stage: the raster corner list and its count, the kept keypoints in
retainBest's order, descriptors / undistorted keypoints / 3D points; k_fast_select's two-tier retainBest alone against
libstdc++ on up to 65,536 responses; frame shapes, thresholds and borders; the two capacity flags; the refusals; the PnP
chain; track_sequence; and examples/fast_example.cpp.  Calls go through the C ABI; inputs are seeded."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, synth_seq
import chain_model
import extractor_edge_cases as E
import fast_cases as FC
import fast_model as F
import svo_edge_cases as S
from test_gpu_svo import _adversarial

pytestmark = pytest.mark.gpu

ARG, CAPACITY, UNSUPPORTED = 1, 3, 4   # rgbd_status
TIER = 12288                           # kFastLdsTier: live ranges up to this are selected in LDS
DESCRIPTORS = ["brief", "orb"]


def _cam(pkg, cam):
    return pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"],
                      cam["k3"], cam["factor"])


def _ctx(pkg, cam, max_batch=1, W=640, H=480, **kw):
    return pkg.Context(W, H, max_batch=max_batch, cam=_cam(pkg, cam), fast=pkg.fast_params(**kw))


def _dev(bgr, depth):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(bgr)).cuda(),
            torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda())


def _same_corners(ctx, b, rec, what):
    n, xys = ctx.fast_debug_corners(b)
    assert n == len(rec["raster"]), f"{what}: {n} corners, model {len(rec['raster'])}"
    assert np.array_equal(xys, rec["raster"]), f"{what}: raster list"


def _same_frame(got, want, what):
    assert len(got["kps"]) == len(want["kps"]), f"{what}: {len(got['kps'])} keypoints, model {len(want['kps'])}"
    assert np.array_equal(got["kps"], want["kps"]), f"{what}: kps"
    assert np.array_equal(got["desc"], want["desc"]), f"{what}: desc"
    assert np.array_equal(got["kps_un"], want["kps_un"]), f"{what}: kps_un"
    assert np.array_equal(got["xyz"].view(np.uint32), want["xyz"].view(np.uint32)), f"{what}: xyz"


# ------------------------------------------------------------------ stages on the pinned 640 x 480 frames
@pytest.mark.parametrize("descriptor", DESCRIPTORS)
def test_frames_match_model(pkg, oracle, descriptor):
    """A batch of three different frames (fr1: 13,715 corners; lowtex: 656, fewer than nfeatures, so raster order
    survives; uniform noise: 31,337), then fr2 alone through rgbd_frame, then a gray image."""
    names = ["fr1", "lowtex", "noise"]
    want = [FC.model_frame(n, descriptor) for n in names]
    assert [len(w["rec"]["raster"]) for w in want] == [FC.COUNTS[n][1] for n in names]
    assert np.array_equal(want[1]["rec"]["kept"], np.arange(656))
    cam = FC.frame("fr1")[2]
    ctx = _ctx(pkg, cam, max_batch=3, descriptor=descriptor)
    d_bgr, d_dep = _dev(np.stack([FC.frame(n)[0] for n in names]), np.stack([FC.frame(n)[1] for n in names]))
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 3)
    for b, n in enumerate(names):
        _same_corners(ctx, b, want[b]["rec"], (descriptor, n))
        _same_frame(ctx.batch_frame(b), want[b], (descriptor, n))
        assert len(want[b]["kps"]) > 400
    ctx.close()
    bgr, depth, cam2 = FC.frame("fr2")
    assert cam2["k1"] != 0   # a distorted camera: kps_un differ from kps
    ctx = _ctx(pkg, cam2, descriptor=descriptor)
    w2 = FC.model_frame("fr2", descriptor)
    _same_frame(ctx.frame(bgr, depth), w2, (descriptor, "fr2"))
    _same_corners(ctx, 0, w2["rec"], (descriptor, "fr2"))
    assert not np.array_equal(w2["kps_un"]["x"], w2["kps"]["x"])
    k, d = ctx.detect_and_compute(FC.gray("fr2"))   # Extractor::detectAndCompute from a gray image
    assert np.array_equal(k, w2["kps"]) and np.array_equal(d, w2["desc"])
    ctx.close()


def test_brief_pattern_entry_points(pkg, oracle):
    bgr, depth, cam = FC.frame("lowtex")
    ctx = _ctx(pkg, cam)
    assert np.array_equal(ctx.brief_pattern(), oracle.brief_default_pattern())
    rnd = np.random.RandomState(9).randint(-24, 25, size=(256, 4)).astype(np.int8)
    ctx.set_brief_pattern(rnd)
    assert np.array_equal(ctx.brief_pattern(), rnd)
    want = F.Extractor(pattern=rnd).frame(bgr, depth, cam)
    _same_frame(ctx.frame(bgr, depth), want, "pattern")
    assert not np.array_equal(want["desc"], FC.model_frame("lowtex")["desc"])
    ctx.close()
    ctx = _ctx(pkg, cam, descriptor="orb")   # no BRIEF table behind the ORB descriptor
    with pytest.raises(pkg.RgbdError):
        ctx.brief_pattern()
    with pytest.raises(pkg.RgbdError):
        ctx.set_brief_pattern(rnd)
    ctx.close()


# ------------------------------------------------------------------ the selection alone
@pytest.fixture(scope="module")
def sel_ctx(pkg):
    ctx = _ctx(pkg, synth_seq(2, seed=3, preset="fr1")[3])
    yield ctx
    ctx.close()


def _two_values(n, rs):
    """Two distinct values, the boundary of retainBest(1000) inside the larger group."""
    r = np.full(n, 5.0, np.float32)
    r[rs.permutation(n)[:300]] = 9.0
    return r


@pytest.mark.parametrize("n", [1001, TIER, TIER + 1, 32768, 65536])
def test_retain_best_matches_libstdcxx(pkg, oracle, sel_ctx, n):
    """n = nfeatures + 1, the tier boundary and one above it, the default and the largest cand_cap.  The inputs: random,
    few distinct values, strictly increasing and decreasing, organ-pipe, all tied, two values."""
    rs = np.random.RandomState(17 + n)
    inc = np.arange(n, dtype=np.float32)
    for i, r in enumerate(_adversarial(n, rs) + [inc, inc[::-1].copy(), _two_values(n, rs)]):
        for keep in (1000, 1):
            got, want = sel_ctx.fast_retain_best(r, keep), oracle.retain_best(r, keep)
            assert len(got) == len(want) and np.array_equal(got, want), (n, i, keep, len(got), len(want))
    r = rs.rand(n).astype(np.float32)
    assert np.array_equal(sel_ctx.fast_retain_best(r, n - 1), oracle.retain_best(r, n - 1))
    assert np.array_equal(sel_ctx.fast_retain_best(r, n), np.arange(n))   # nothing to drop: the input order


@pytest.mark.parametrize("n", [3000, 20000, 40000])
def test_retain_best_depth_limits(pkg, oracle, sel_ctx, n):
    """depth_limit 0: heap-select at once, in LDS (n = 3000) and on the global tier (n > 12288).  depth_limit 1: one
    Hoare pass, then heap-select in LDS (20000: the pass leaves about half) or still on the global tier (40000)."""
    rs = np.random.RandomState(29 + n)
    for depth in (0, 1):
        for i, r in enumerate(_adversarial(n, rs)[:3]):
            got = sel_ctx.fast_retain_best(r, 1000, depth)
            want = oracle.retain_best_depth(r, 1000, depth)
            assert np.array_equal(got, want), (n, depth, i, len(got), len(want))


def test_retain_best_on_the_detector_s_responses(pkg, oracle, sel_ctx):
    for name in ("fr1", "noise"):
        r = FC.model_frame(name)["rec"]["raster"][:, 2].astype(np.float32)
        assert len(r) > TIER
        assert np.array_equal(sel_ctx.fast_retain_best(r, 1000), FC.model_frame(name)["rec"]["kept"])


# ------------------------------------------------------------------ shapes, thresholds, borders
def _shape_case(W, H, spec, **prm):
    bgr, depth = E.image(spec, W, H)
    return bgr, depth, S.images(W, H)[2], prm


@pytest.mark.parametrize("descriptor", DESCRIPTORS)
@pytest.mark.parametrize("W,H,spec,prm,least", [
    (64, 65, ("noise", 3), {}, 0),                        # the smallest accepted: 8 x 9 px inside BRIEF's border, 2 x 3 inside ORB's
    (368, 239, ("nat", 0), {}, 500),                      # partial score tiles in x and y, an odd height
    (400, 481, ("nat", 0), {}, 500),                      # a tile row one pixel high; the ORB pyramid's rows are padded (448)
    (2032, 239, ("nat", 0), {}, 500),                     # 11-bit x; 8 columns per k_fast_rows thread
    (368, 239, ("nat", 0), dict(threshold=1), 500),       # every strict maximum is a corner
    (368, 239, ("nat", 0), dict(threshold=255), 0),       # no score reaches 255
    (368, 239, ("binary", 4), dict(nfeatures=200), 200),  # every corner scores 254: retainBest keeps all of them
    (128, 96, ("flat", 0), {}, 0),
], ids=["64x65", "368x239", "400x481", "2032x239", "threshold1", "threshold255", "binary", "flat"])
def test_shapes_and_thresholds(pkg, oracle, descriptor, W, H, spec, prm, least):
    bgr, depth, cam, prm = _shape_case(W, H, spec, **prm)
    want = F.Extractor(F.params(descriptor=descriptor, **prm)).frame(bgr, depth, cam)
    n = len(want["rec"]["raster"])
    if prm.get("threshold") == 255 or spec[0] == "flat":
        assert n == 0
    elif spec[0] == "binary":
        assert n > 200 and len(want["rec"]["kept"]) == n and set(want["rec"]["raster"][:, 2]) == {254}
    elif W == 64:
        assert n > 100
    else:
        assert n > 1000   # retainBest runs
    assert len(want["kps"]) >= least
    ctx = _ctx(pkg, cam, W=W, H=H, descriptor=descriptor, max_keypoints=max(n, 1000) if spec[0] == "binary" else 0, **prm)
    got = ctx.frame(bgr, depth)
    _same_corners(ctx, 0, want["rec"], (descriptor, W, H, spec))
    _same_frame(got, want, (descriptor, W, H, spec))
    ctx.close()


@pytest.mark.parametrize("descriptor", DESCRIPTORS)
def test_corners_on_the_domain_s_edge(pkg, oracle, descriptor):
    """Bright single pixels at x or y = 3 and W - 4 or H - 4 are corners (score 254); one column or row further out they
    are not (cv::FAST scans [3, W - 3) x [3, H - 3)).  The descriptor's border drops them all, so the list is the check."""
    W, H = 400, 97   # the ORB pyramid pads these rows to 448
    g = np.zeros((H, W), np.uint8)
    inside = [(3, 3), (W - 4, 3), (200, 3), (3, 50), (W - 4, 50), (3, H - 4), (W - 4, H - 4), (201, H - 4)]
    for x, y in inside + [(2, 20), (W - 3, 20), (100, 2), (100, H - 3), (W - 1, 70), (0, 70)]:
        g[y, x] = 255
    want = F.Extractor(F.params(descriptor=descriptor)).detect(g)[1]["raster"]
    assert sorted(map(tuple, want[:, :2])) == sorted(inside) and set(want[:, 2]) == {254}
    _, depth, cam = S.images(W, H)
    ctx = _ctx(pkg, cam, W=W, H=H, descriptor=descriptor)
    got = ctx.frame(E.gray3(g), depth)
    n, xys = ctx.fast_debug_corners(0)
    assert n == len(inside) and np.array_equal(xys, want)
    assert len(got["kps"]) == 0
    ctx.close()


def _detect_padded(pkg, ctx, gray, pad):
    H, W = gray.shape
    wide = np.random.RandomState(7).randint(0, 256, size=(H, W + pad)).astype(np.uint8)
    wide[:, :W] = gray
    kps = np.zeros(ctx.kp_cap, pkg.KEYPOINT_DTYPE)
    desc = np.zeros((ctx.kp_cap, 32), np.uint8)
    n = C.c_int32(0)
    st = pkg.lib().rgbd_detect_and_compute(ctx._h, wide.ctypes.data_as(C.c_void_p), W + pad, kps.ctypes.data_as(C.c_void_p),
                                           desc.ctypes.data_as(C.c_void_p), ctx.kp_cap, C.byref(n))
    assert st == 0, pkg.lib().rgbd_last_error(ctx._h)
    return kps[:n.value].copy(), desc[:n.value].copy()


@pytest.mark.parametrize("descriptor", DESCRIPTORS)
def test_padded_rows_and_misaligned_pointers(pkg, oracle, descriptor):
    """A gray image inside rows 24 bytes longer (garbage in the padding) gives what the contiguous one gives; a 3-frame
    batch from device pointers offset by 1 byte (BGR) and 2 bytes (depth) gives what the model gives, and so does the
    same batch from aligned pointers afterwards."""
    import torch
    W, H = 368, 239
    imgs = [E.image(("nat", s), W, H) for s in (0, 100, 200)]
    bgr, depth, cam = np.stack([i[0] for i in imgs]), np.stack([i[1] for i in imgs]), S.images(W, H)[2]
    m = F.Extractor(F.params(descriptor=descriptor))
    want = [m.frame(bgr[b], depth[b], cam) for b in range(3)]
    ctx = _ctx(pkg, cam, max_batch=3, W=W, H=H, descriptor=descriptor)
    gray = oracle.gray(bgr[0])
    k0, d0 = ctx.detect_and_compute(gray)
    assert len(k0) > 500 and np.array_equal(k0, want[0]["kps"]) and np.array_equal(d0, want[0]["desc"])
    k1, d1 = _detect_padded(pkg, ctx, gray, 24)
    assert np.array_equal(k1, k0) and np.array_equal(d1, d0)
    _same_corners(ctx, 0, want[0]["rec"], "padded rows")
    raw_b = torch.zeros(bgr.size + 64, dtype=torch.uint8, device="cuda")
    raw_d = torch.zeros(depth.size + 32, dtype=torch.int16, device="cuda")
    for off in (1, 0):
        d_bgr, d_dep = raw_b[off:off + bgr.size], raw_d[off:off + depth.size]
        d_bgr.copy_(torch.from_numpy(bgr.reshape(-1)))
        d_dep.copy_(torch.from_numpy(np.ascontiguousarray(depth).view(np.int16).reshape(-1)))
        torch.cuda.synchronize()
        assert d_bgr.data_ptr() % 16 == off and d_dep.data_ptr() % 4 == 2 * off
        ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 3)
        for b in range(3):
            _same_corners(ctx, b, want[b]["rec"], (descriptor, off, b))
            _same_frame(ctx.batch_frame(b), want[b], (descriptor, off, b))
    ctx.close()


# ------------------------------------------------------------------ capacities
def test_cand_cap_flags_one_frame(pkg, oracle):
    """[natural, noise, natural] at 128 x 96: with cand_cap = the noise frame's corner count every frame passes; with one
    less the noise frame alone fails, its count still reported, and a later extraction is clean."""
    W, H = 128, 96
    imgs = [E.image(("nat", 0), W, H), E.image(("noise", 31), W, H), E.image(("nat", 40), W, H)]
    bgr, depth, cam = np.stack([i[0] for i in imgs]), np.stack([i[1] for i in imgs]), S.images(W, H)[2]
    m = F.Extractor(F.params(nfeatures=100))
    want = [m.frame(bgr[b], depth[b], cam) for b in range(3)]
    n = [len(w["rec"]["raster"]) for w in want]
    assert n[1] > max(n[0], n[2]) > 100
    d_bgr, d_dep = _dev(bgr, depth)
    for cap, flagged in ((n[1], False), (n[1] - 1, True)):
        ctx = _ctx(pkg, cam, max_batch=3, W=W, H=H, nfeatures=100, cand_cap=cap)
        ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 3)
        for b in range(3):
            if flagged and b == 1:
                with pytest.raises(pkg.RgbdError, match="cand_cap"):
                    ctx.batch_frame(b)
                cnt, xys = ctx.fast_debug_corners(b)
                assert cnt == n[1] and np.array_equal(xys, want[b]["rec"]["raster"][:cap])
            else:
                _same_corners(ctx, b, want[b]["rec"], (cap, b))
                _same_frame(ctx.batch_frame(b), want[b], (cap, b))
        _same_frame(ctx.frame(bgr[0], depth[0]), want[0], "after")   # flag cleared
        ctx.close()


def test_max_keypoints_flags_one_frame(pkg, oracle):
    """0 / 255 noise: every corner scores 254, so retainBest(100) keeps them all.  max_keypoints = that count passes, one
    less fails that frame alone."""
    W, H = 128, 96
    imgs = [E.image(("nat", 0), W, H), E.image(("binary", 4), W, H), E.image(("nat", 40), W, H)]
    bgr, depth, cam = np.stack([i[0] for i in imgs]), np.stack([i[1] for i in imgs]), S.images(W, H)[2]
    m = F.Extractor(F.params(nfeatures=100))
    want = [m.frame(bgr[b], depth[b], cam) for b in range(3)]
    kept = [len(w["rec"]["kept"]) for w in want]
    assert kept[1] == len(want[1]["rec"]["raster"]) and kept[1] - 1 > max(kept[0], kept[2], 100)
    d_bgr, d_dep = _dev(bgr, depth)
    for cap, flagged in ((kept[1], False), (kept[1] - 1, True)):
        ctx = _ctx(pkg, cam, max_batch=3, W=W, H=H, nfeatures=100, max_keypoints=cap)
        ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 3)
        for b in range(3):
            if flagged and b == 1:
                with pytest.raises(pkg.RgbdError, match="max_keypoints"):
                    ctx.batch_frame(b)
            else:
                _same_frame(ctx.batch_frame(b), want[b], (cap, b))
        ctx.close()


# ------------------------------------------------------------------ refusals
def test_refusals(pkg):
    lib = pkg.lib()
    cam = pkg.camera(500, 500, 320, 240)

    def create(W, H, **kw):
        h = C.c_void_p()
        st = lib.rgbd_create_fast(0, W, H, 1, C.byref(pkg.fast_params(**kw)), C.byref(cam), C.byref(h))
        msg = lib.rgbd_last_error(h)
        lib.rgbd_destroy(h)
        return st, msg
    for kw in [dict(nfeatures=0), dict(nfeatures=12289), dict(threshold=0), dict(threshold=256), dict(descriptor=2),
               dict(descriptor=-1), dict(cand_cap=-1), dict(cand_cap=65537), dict(max_keypoints=999), dict(max_keypoints=65537),
               dict(max_keypoints=-1)]:
        for d in ([kw.get("descriptor")] if "descriptor" in kw else DESCRIPTORS):
            st, msg = create(640, 480, **dict(kw, descriptor=d))
            assert st == UNSUPPORTED and b"FAST" in msg, (kw, d, st, msg)
    for d in DESCRIPTORS:
        st, msg = create(2064, 480, descriptor=d)                 # a side above 2047
        assert st == UNSUPPORTED and b"2047" in msg
        assert create(100, 96, descriptor=d)[0] == UNSUPPORTED    # the one-level ORB geometry's: width no multiple of 16
        assert create(48, 96, descriptor=d)[0] == UNSUPPORTED     # width below 64
        assert create(640, 480, descriptor=d, nfeatures=12288, cand_cap=65536, max_keypoints=65536)[0] == 0
    # wrong kinds of context, both ways
    ctx = pkg.Context(640, 480, max_batch=1, cam=cam)
    n = C.c_int32(0)
    assert lib.rgbd_fast_debug_corners(ctx._h, 0, C.byref(n), None, 0, None) == ARG and b"not a FAST context" in lib.rgbd_last_error(ctx._h)
    r, o = np.zeros(8, np.float32), np.zeros(8, np.int32)
    assert lib.rgbd_fast_retain_best(ctx._h, r.ctypes.data_as(C.c_void_p), 8, 4, -1, o.ctypes.data_as(C.c_void_p), C.byref(n)) == ARG
    ctx.close()
    ctx = pkg.Context(640, 480, max_batch=1, cam=cam, fast=pkg.fast_params())
    assert lib.rgbd_adaptive_rewind(ctx._h, 1) == ARG and b"not an adaptive context" in lib.rgbd_last_error(ctx._h)
    assert lib.rgbd_svo_retain_best(ctx._h, r.ctypes.data_as(C.c_void_p), 8, 4, -1, o.ctypes.data_as(C.c_void_p), C.byref(n)) == ARG
    assert b"not an SVO context" in lib.rgbd_last_error(ctx._h)
    assert lib.rgbd_cvorb_debug_level(ctx._h, 0, 0, 0, None, None, 0, C.byref(n)) == ARG and b"not a cv::ORB context" in lib.rgbd_last_error(ctx._h)
    assert lib.rgbd_gftt_debug_ranks(ctx._h, 0, C.byref(n)) != 0
    big = np.zeros(65537, np.float32)
    assert lib.rgbd_fast_retain_best(ctx._h, big.ctypes.data_as(C.c_void_p), 65537, 4, -1, o.ctypes.data_as(C.c_void_p), C.byref(n)) == UNSUPPORTED
    ctx.close()


# ------------------------------------------------------------------ the chain, the sequence driver, the C++ shim
def test_pnp_chain_matches_model(pkg, oracle):
    """Extract (FAST + BRIEF) + Matcher + PnPRansac per consecutive pair, bit-exact vs the oracle chain over the model's
    frames."""
    B = 4
    bgr, depth, gt, cam = synth_seq(5, seed=21, preset="fr1")
    ctx = _ctx(pkg, cam, max_batch=B)
    d_bgr, d_dep = _dev(bgr[:B], depth[:B])
    pose0 = gt[0].astype(np.float32)
    poses, status, ninl, nm = ctx.pnp_track_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B, 0.9, pkg.pnp_params(), pose0)
    m = F.Extractor()
    frames = [m.frame(bgr[i], depth[i], cam) for i in range(B)]
    assert all(len(f["rec"]["raster"]) > 1000 for f in frames)   # retainBest runs on every frame
    K4 = np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], np.float32)
    wp, ws, wn, wm = chain_model.pnp_track(oracle, frames, pose0, K4)
    assert np.array_equal(nm, wm) and np.array_equal(status, ws) and np.array_equal(ninl, wn)
    assert np.array_equal(poses.view(np.uint32), wp.view(np.uint32))
    assert status.all()
    ctx.close()


@pytest.mark.parametrize("extractor", ["fast", "fast-orb"])
def test_track_sequence(pkg, tmp_path, extractor):
    from rgbd_slam_amd import datasets as D
    from rgbd_slam_amd.sequence import track_sequence
    n = 3
    bgr, depth, gt, cam = synth_seq(5, seed=21, preset="fr1")
    base = str(tmp_path / "rgbd_dataset_freiburg1_seq") + os.sep
    D.write_dataset(base, bgr[:n], depth[:n], 100.0 + 0.033 * np.arange(n), gt[:n])
    ds = D.open_dataset(base)
    p2, s2, i2 = track_sequence(pkg, ds, B=2, solver="pnp", pose0=gt[0], extractor=extractor)
    p3, s3, i3 = track_sequence(pkg, ds, B=3, solver="pnp", pose0=gt[0], extractor=extractor)
    assert np.array_equal(p2.view(np.uint32), p3.view(np.uint32)) and np.array_equal(s2, s3) and np.array_equal(i2, i3)
    assert s3[0] == 1 and (extractor != "fast" or (s3.all() and i3[1:].min() >= 10))


def test_cpp_example_matches_python(pkg, oracle, tmp_path):
    """examples/fast_example.cpp (rgbd::Extractor(FAST, BRIEF, NORMAL) and (FAST, ORB, NORMAL) over
    include/rgbd/frontend.hpp) prints an FNV-1a hash of every frame's keypoints and descriptors for both pairs;
    Extractor(FAST, FREAK, NORMAL) throws."""
    exe = os.path.join(ROOT, "rgbd-slam_amd", "build", "fast_example")
    assert os.path.exists(exe), "build() must compile examples/fast_example.cpp"
    n = 2
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
    assert lines[-1] == "FAST FREAK: throws"
    rows = [l.split() for l in lines[:-1]]
    assert len(rows) == n

    def fnv(*arrays):
        h = 0xcbf29ce484222325
        for a in arrays:
            for byte in np.ascontiguousarray(a).view(np.uint8).reshape(-1).tolist():
                h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
        return h
    for col, descriptor in ((1, "brief"), (3, "orb")):
        ctx = _ctx(pkg, cam, descriptor=descriptor, cand_cap=65536)
        for i in range(n):
            got = ctx.frame(bgr[i], depth[i])
            assert int(rows[i][col]) == len(got["kps"]) > 500
            assert int(rows[i][col + 1], 16) == fnv(got["kps"], got["desc"]), (descriptor, i)
            assert int(rows[i][5]) == ctx.fast_debug_corners(0)[0] > TIER
        ctx.close()
