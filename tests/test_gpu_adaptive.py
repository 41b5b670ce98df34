"""GPU parity: the adaptive FAST + BRIEF front end (the reference's Extractor(FAST, BRIEF, ADAPTIVE)) on gfx950
vs the CPU model (tests/adaptive_model.py, itself held to the oracle's cv::FAST, libstdc++ and the SVO oracle's
BRIEF by tests/test_adaptive_model.py), bit-exact: every cell's threshold chain and raster corner list, the
final keypoints / descriptors / undistorted keypoints / 3D points, the carried thresholds over batches, rewinds
and single frames, the capacity flag, keepStrongest's libstdc++ order, and the PnP chain on an adaptive context.
Calls go through the C ABI; inputs are seeded synthetic RGB-D frames."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, synth_seq
import adaptive_model as A
import chain_model
from test_gpu_svo import _adversarial

pytestmark = pytest.mark.gpu


def _cam(pkg, cam):
    return pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"],
                      cam["k3"], cam["factor"])


def _ctx(pkg, cam, max_batch=6, W=640, H=480, **kw):
    return pkg.Context(W, H, max_batch=max_batch, cam=_cam(pkg, cam), adaptive=pkg.adaptive_params(**kw))


def _dev(bgr, depth):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(bgr)).cuda(),
            torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda())


def _same_frame(got, want, at=None):
    assert len(got["kps"]) == len(want["kps"]), (at, len(got["kps"]), len(want["kps"]))
    assert np.array_equal(got["kps"], want["kps"]), at
    assert np.array_equal(got["desc"], want["desc"]), at
    assert np.array_equal(got["kps_un"], want["kps_un"]), at
    assert np.array_equal(got["xyz"].view(np.uint32), want["xyz"].view(np.uint32)), at


def _same_cells(ctx, b, rec, at=None):
    for k, c in enumerate(rec["cells"]):
        before, used, tries, xys = ctx.adaptive_debug_cell(b, k)
        assert np.float64(before).view(np.uint64) == np.float64(c["before"]).view(np.uint64), (at, b, k)
        assert (used, tries) == (c["used"], c["tries"]), (at, b, k, used, tries, c["used"], c["tries"])
        assert np.array_equal(xys, c["raster"]), (at, b, k, len(xys), len(c["raster"]))


def _flat(like):
    return np.full_like(like, 128)


def _mixed(oracle):
    """[rich, flat, flat, flat, rich, lowtex]: the flats drive every threshold to 2.0, so the second rich frame
    runs at threshold 2."""
    rb, rd, _, cam = synth_seq(5, seed=3, preset="fr1")
    lb, ld, _, _ = synth_seq(5, seed=7, preset="lowtex")
    bgr = np.stack([rb[0], _flat(rb[0]), _flat(rb[0]), _flat(rb[0]), rb[0], lb[0]])
    depth = np.stack([rd[0], rd[0], rd[0], rd[0], rd[0], ld[0]])
    return bgr, depth, cam


@pytest.mark.parametrize("preset,seed", [("fr1", 3), ("lowtex", 7)])
def test_cells_match_model(pkg, oracle, preset, seed):
    """Every (frame, cell): the threshold before (f64 bits), the threshold used, the tries and the raster list."""
    B = 5
    bgr, depth, _, cam = synth_seq(B, seed=seed, preset=preset)
    m = A.Extractor()
    want = [m.frame(bgr[b], depth[b], cam) for b in range(B)]
    # the chain is exercised, not idle (tests/test_adaptive_model.py pins the exact shape)
    if preset == "fr1":
        assert all(c["branch"] == "many" for w in want for c in w["rec"]["cells"]) and want[4]["rec"]["cells"][0]["used"] == 57
        assert all(w["rec"]["total"] > 1000 for w in want)
    else:
        assert all(c["tries"] == 3 for c in want[0]["rec"]["cells"]) and len(set(m.thresholds)) > 3
    ctx = _ctx(pkg, cam, max_batch=B)
    d_bgr, d_dep = _dev(bgr, depth)
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B)
    for b in range(B):
        _same_cells(ctx, b, want[b]["rec"], preset)
        _same_frame(ctx.batch_frame(b), want[b], (preset, b))
    assert np.array_equal(ctx.adaptive_thresholds().view(np.uint64), m.thresholds.view(np.uint64))
    ctx.close()


@pytest.mark.parametrize("preset,seed", [("fr1", 3), ("fr3", 11), ("icl", 23)])
def test_frames_bit_exact(pkg, oracle, preset, seed):
    bgr, depth, _, cam = synth_seq(2, seed=seed, preset=preset)
    if preset == "fr1":
        assert cam["k1"] != 0   # the distorted camera: kps_un differ from kps
    ctx = _ctx(pkg, cam, max_batch=1)
    m = A.Extractor()
    for f in range(2):
        want = m.frame(bgr[f], depth[f], cam)
        assert len(want["kps"]) > 500
        _same_frame(ctx.frame(bgr[f], depth[f]), want, (preset, f))
    # detect_and_compute from a gray image (Extractor::detectAndCompute); the thresholds carry on
    g = oracle.gray(bgr[0])
    k, d = ctx.detect_and_compute(g)
    wk, wd, _ = m.detect_and_compute(g)
    assert np.array_equal(k, wk) and np.array_equal(d, wd)
    # a second BRIEF table
    assert np.array_equal(ctx.brief_pattern(), oracle.brief_default_pattern())
    rnd = np.random.RandomState(9).randint(-24, 25, size=(256, 4)).astype(np.int8)
    ctx.set_brief_pattern(rnd)
    m.pattern = rnd
    assert np.array_equal(ctx.brief_pattern(), rnd)
    _same_frame(ctx.frame(bgr[1], depth[1]), m.frame(bgr[1], depth[1], cam), (preset, "pattern"))
    ctx.close()


def test_batch_equals_single_frames(pkg, oracle):
    bgr, depth, cam = _mixed(oracle)
    m = A.Extractor()
    want = [m.frame(bgr[b], depth[b], cam) for b in range(6)]
    cells4 = want[4]["rec"]["cells"]
    # threshold 2 on the rich frame: 2416 corners in cell 0 (the oracle's cv::FAST on that ROI), 16037 on the whole frame
    assert all(c["used"] == 2 for c in cells4) and len(cells4[0]["raster"]) == 2416
    assert all(c["before"] == 2.0 for c in cells4)
    cap = m.max_stored              # the tightest capacity that holds every list
    assert 2416 <= cap <= 12288 and all(c["stored"] <= cap for w in want for c in w["rec"]["cells"])
    a = _ctx(pkg, cam, max_batch=6, cell_cap=cap)
    b1 = _ctx(pkg, cam, max_batch=1, cell_cap=cap)
    d_bgr, d_dep = _dev(bgr, depth)
    a.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 6)
    for b in range(6):
        got = a.batch_frame(b)
        _same_frame(got, want[b], b)
        _same_frame(b1.frame(bgr[b], depth[b]), got, b)
        _same_cells(a, b, want[b]["rec"])
    ta, tb = a.adaptive_thresholds(), b1.adaptive_thresholds()
    assert np.array_equal(ta.view(np.uint64), tb.view(np.uint64))
    assert np.array_equal(ta.view(np.uint64), m.thresholds.view(np.uint64))
    a.close()
    b1.close()


def test_state_roundtrip_and_rewind(pkg, oracle):
    n = 7
    bgr, depth, _, cam = synth_seq(n, seed=7, preset="lowtex")
    ctx = _ctx(pkg, cam, max_batch=n)
    th = np.random.RandomState(3).uniform(2.0, 10000.0, 9)
    th[0], th[1] = 2.0, 10000.0
    ctx.set_adaptive_thresholds(th)
    assert np.array_equal(ctx.adaptive_thresholds().view(np.uint64), th.view(np.uint64))
    with pytest.raises(pkg.RgbdError):
        ctx.set_adaptive_thresholds(np.full(9, 1.5))   # below min_thresh
    ctx.set_adaptive_thresholds(np.full(9, 20.0))
    d_bgr, d_dep = _dev(bgr, depth)
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), n)
    whole = [ctx.batch_frame(b) for b in range(n)]
    final = ctx.adaptive_thresholds()
    m = A.Extractor()
    for b in range(n):
        _same_frame(whole[b], m.frame(bgr[b], depth[b], cam), b)
    assert len(set(final)) > 3   # the cells' thresholds diverge: a rewind that is off by a frame shows
    with pytest.raises(pkg.RgbdError):
        ctx.adaptive_rewind(n + 1)
    for overlap in (1, 2):
        ctx.set_adaptive_thresholds(np.full(9, 20.0))
        s = 0
        while True:
            cnt = min(4, n - s)
            if s > 0:
                ctx.adaptive_rewind(overlap)
            ctx.extract_batch(d_bgr[s:s + cnt].contiguous().data_ptr(), d_dep[s:s + cnt].contiguous().data_ptr(), cnt)
            for b in range(cnt):
                _same_frame(ctx.batch_frame(b), whole[s + b], (overlap, s, b))
            if s + cnt >= n:
                break
            s += 4 - overlap
        assert np.array_equal(ctx.adaptive_thresholds().view(np.uint64), final.view(np.uint64)), overlap
    ctx.close()


@pytest.mark.parametrize("solver", ["pnp", "se3"])
def test_track_sequence_batches_equal_one_batch(pkg, tmp_path, solver):
    from rgbd_slam_amd import datasets as D
    from rgbd_slam_amd.sequence import track_sequence
    n = 7
    bgr, depth, gt, cam = synth_seq(n, seed=7, preset="lowtex")
    base = str(tmp_path / "rgbd_dataset_freiburg1_seq") + os.sep
    D.write_dataset(base, bgr, depth, 100.0 + 0.033 * np.arange(n), gt)
    ds = D.open_dataset(base)
    p4, s4, i4 = track_sequence(pkg, ds, B=4, solver=solver, pose0=gt[0], extractor="adaptive")
    pn, sn, i_n = track_sequence(pkg, ds, B=n, solver=solver, pose0=gt[0], extractor="adaptive")
    assert np.array_equal(p4.view(np.uint32), pn.view(np.uint32))
    assert np.array_equal(s4, sn) and np.array_equal(i4, i_n) and sn[0] == 1
    with pytest.raises(ValueError):
        track_sequence(pkg, ds, B=4, solver=solver, extractor="sift")


def test_capacity_flag_per_frame(pkg, oracle):
    """cell_cap 1024: the rich frame at threshold 2 alone overflows (2416 corners in cell 0); the frames after
    it in the batch still equal the model (the chain reads counts, not lists), and so does a later extraction."""
    rb, rd, _, cam = synth_seq(5, seed=3, preset="fr1")
    flat = _flat(rb[0])
    patch = flat.copy()
    patch[200:290, 250:400] = rb[0][200:290, 250:400]
    patch2 = flat.copy()
    patch2[60:150, 100:260] = rb[1][60:150, 100:260]
    bgr = np.stack([flat, flat, flat, rb[0], patch, patch2])
    depth = np.stack([rd[0]] * 6)
    m = A.Extractor()
    want = [m.frame(bgr[b], depth[b], cam) for b in range(6)]
    over = [max(c["stored"] for c in w["rec"]["cells"]) > 1024 for w in want]
    assert over == [False, False, False, True, False, False]
    assert len(want[4]["kps"]) > 50 and len(want[5]["kps"]) > 50
    ctx = _ctx(pkg, cam, max_batch=6, cell_cap=1024)
    d_bgr, d_dep = _dev(bgr, depth)
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 6)
    for b in (0, 1, 2, 4, 5):
        _same_frame(ctx.batch_frame(b), want[b], b)
        _same_cells(ctx, b, want[b]["rec"])
    with pytest.raises(pkg.RgbdError, match="cell_cap"):
        ctx.batch_frame(3)
    assert np.array_equal(ctx.adaptive_thresholds().view(np.uint64), m.thresholds.view(np.uint64))
    _same_frame(ctx.frame(patch, depth[0]), m.frame(patch, depth[0], cam), "after")   # flag cleared
    ctx.close()


def test_keep_strongest_matches_libstdcxx(pkg, oracle):
    """The device std::nth_element(begin, begin + N, end) against libstdc++'s: the first N entries of the
    oracle's retainBest(N + 1) (the same nth_element call whenever n >= N + 2)."""
    rs = np.random.RandomState(17)
    ctx = _ctx(pkg, synth_seq(2, seed=3, preset="fr1")[3], max_batch=1)
    N = 113
    for n in (N + 2, 200, 4096, 8192):
        for r in _adversarial(n, rs):
            assert np.array_equal(ctx.adaptive_keep_strongest(r, N), oracle.retain_best(r, N + 1)[:N]), n
        for depth in (0, 1, 3):
            for r in _adversarial(n, rs)[:3]:
                got = ctx.adaptive_keep_strongest(r, N, depth)
                assert np.array_equal(got, oracle.retain_best_depth(r, N + 1, depth)[:N]), (n, depth)
    # n == N + 1 and n <= N: the model's restatement (libstdc++ offers no second witness there)
    for r in _adversarial(N + 1, rs):
        assert np.array_equal(ctx.adaptive_keep_strongest(r, N), A.keep_strongest(r, N))
    r = rs.rand(50).astype(np.float32)
    assert np.array_equal(ctx.adaptive_keep_strongest(r, N), np.arange(50))
    ctx.close()


@pytest.mark.parametrize("W,H,kw", [(320, 256, {}),
                                    (640, 480, dict(grid_rows=2, grid_cols=4, edge_threshold=0, iterations=1, nfeatures=300)),
                                    (320, 256, dict(grid_rows=2, grid_cols=4, edge_threshold=0, nfeatures=300))])
def test_parameters_and_shapes(pkg, oracle, W, H, kw):
    import synth
    bgr, depth, _, cam = synth.sequence(3, seed=5, preset="fr3", W=W, H=H)
    ctx = _ctx(pkg, cam, max_batch=3, W=W, H=H, **kw)
    m = A.Extractor(A.params(**kw), W=W, H=H)
    want = [m.frame(bgr[b], depth[b], cam) for b in range(3)]
    assert len(want[0]["kps"]) > 100
    if kw.get("nfeatures") == 300:
        assert want[0]["rec"]["total"] > 300   # retainBest(300) runs
    d_bgr, d_dep = _dev(bgr, depth)
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 3)
    for b in range(3):
        _same_cells(ctx, b, want[b]["rec"])
        _same_frame(ctx.batch_frame(b), want[b], b)
    ctx.close()


def test_refusals(pkg):
    lib = pkg.lib()
    cam = pkg.camera(500, 500, 320, 240)
    bad = [dict(min_thresh=0.5), dict(min_thresh=0.0), dict(init_thresh=1.0), dict(init_thresh=20000.0),
           dict(decrease=1.0), dict(decrease=0.0), dict(increase=1.0), dict(iterations=0), dict(iterations=33),
           dict(grid_rows=0), dict(grid_cols=9), dict(edge_threshold=-1), dict(min_features=5),
           dict(cell_cap=12289), dict(min_features=8000)]
    for kw in bad:
        h = C.c_void_p()
        st = lib.rgbd_create_adaptive(0, 640, 480, 1, C.byref(pkg.adaptive_params(**kw)), C.byref(cam), C.byref(h))
        assert st == 4 and b"adaptive" in lib.rgbd_last_error(h), (kw, st)
        lib.rgbd_destroy(h)
    # a ROI below 7 x 7: an 8 x 8 grid without margin on 64 x 48 (8 x 6 cells)
    h = C.c_void_p()
    st = lib.rgbd_create_adaptive(0, 64, 48, 1, C.byref(pkg.adaptive_params(grid_rows=8, grid_cols=8, edge_threshold=0)),
                                  C.byref(cam), C.byref(h))
    assert st == 4 and b"7 x 7" in lib.rgbd_last_error(h)
    lib.rgbd_destroy(h)
    # the other extractors' contexts have no adaptive state
    ctx = pkg.Context(640, 480, max_batch=1, cam=cam)
    assert lib.rgbd_adaptive_rewind(ctx._h, 1) == 1 and b"not an adaptive context" in lib.rgbd_last_error(ctx._h)
    out = np.zeros(64, np.float64)
    assert lib.rgbd_adaptive_get_thresholds(ctx._h, C.c_void_p(out.ctypes.data)) == 1
    ctx.close()


def test_pnp_chain_matches_model(pkg, oracle):
    """Extract (adaptive FAST + BRIEF) + Matcher + PnPRansac per consecutive pair, bit-exact vs the oracle chain
    over the model's frames."""
    B = 5
    bgr, depth, gt, cam = synth_seq(B, seed=21, preset="fr1")
    ctx = _ctx(pkg, cam, max_batch=B)
    d_bgr, d_dep = _dev(bgr, depth)
    pose0 = gt[0].astype(np.float32)
    poses, status, ninl, nm = ctx.pnp_track_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B, 0.9, pkg.pnp_params(), pose0)
    m = A.Extractor()
    frames = [m.frame(bgr[i], depth[i], cam) for i in range(B)]
    K4 = np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], np.float32)
    wp, ws, wn, wm = chain_model.pnp_track(oracle, frames, pose0, K4)
    assert np.array_equal(nm, wm) and np.array_equal(status, ws) and np.array_equal(ninl, wn)
    assert np.array_equal(poses.view(np.uint32), wp.view(np.uint32))
    assert status.all()
    ctx.close()


def test_cpp_example_matches_python(pkg, oracle, tmp_path):
    """examples/adaptive_example.cpp (rgbd::Extractor(FAST, BRIEF, ADAPTIVE) over include/rgbd/frontend.hpp)
    prints an FNV-1a hash of every frame's keypoints and descriptors; Extractor(GFTT, BRIEF, ADAPTIVE) throws."""
    exe = os.path.join(ROOT, "rgbd-slam_amd", "build", "adaptive_example")
    assert os.path.exists(exe), "build() must compile examples/adaptive_example.cpp"
    n = 3
    bgr, depth, _, cam = synth_seq(5, seed=7, preset="lowtex")
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
    assert lines[-1] == "GFTT ADAPTIVE: throws"
    rows = [l.split() for l in lines[:-1]]
    assert len(rows) == n

    def fnv(*arrays):
        h = 0xcbf29ce484222325
        for a in arrays:
            for byte in np.ascontiguousarray(a).view(np.uint8).reshape(-1).tolist():
                h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
        return h
    ctx = _ctx(pkg, cam, max_batch=1)
    for i in range(n):
        got = ctx.frame(bgr[i], depth[i])
        assert int(rows[i][1]) == len(got["kps"]) > 500
        assert int(rows[i][2], 16) == fnv(got["kps"], got["desc"]), i
    ctx.close()
