"""GPU parity: the Shi-Tomasi GFTT + BRIEF front end (the reference's Extractor(GFTT, BRIEF, NORMAL)) on gfx950
vs the CPU model (tests/gftt_model.py, held together by tests/test_gftt_model.py), bit for bit: the raw
minimum-eigenvalue map, the frame maximum, the candidate count, the accepted corners with their eigenvalues, the
final keypoints / descriptors / undistorted keypoints / 3D points, batches, the per-frame capacity flag, the
rank + spacing stage on host lists (ties, dependency chains, chunk hand-overs), the refusals, and the tracking
chains on a GFTT context.  Calls go through the C ABI; inputs are seeded synthetic RGB-D frames."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, synth_seq
import chain_model
import gftt_model as G
from test_gftt_model import tiled_frame

pytestmark = pytest.mark.gpu

_MODEL = {}


def _cam(pkg, cam):
    return pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"],
                      cam["k3"], cam["factor"])


def _ctx(pkg, cam, max_batch=1, W=640, H=480, **kw):
    return pkg.Context(W, H, max_batch=max_batch, cam=_cam(pkg, cam), gftt=pkg.gftt_params(**kw))


def _dev(bgr, depth):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(bgr)).cuda(),
            torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda())


def _want(key, bgr, depth, cam, prm=None):
    """The model's frame, computed once per test session and left unchanged."""
    if key not in _MODEL:
        H, W = bgr.shape[:2]
        _MODEL[key] = G.Extractor(prm, W=W, H=H).frame(bgr, depth, cam)
    return _MODEL[key]


def _same_frame(got, want, at=None):
    assert len(got["kps"]) == len(want["kps"]), (at, len(got["kps"]), len(want["kps"]))
    assert np.array_equal(got["kps"], want["kps"]), at
    assert np.array_equal(got["desc"], want["desc"]), at
    assert np.array_equal(got["kps_un"], want["kps_un"]), at
    assert np.array_equal(got["xyz"].view(np.uint32), want["xyz"].view(np.uint32)), at


def _same_corners(ctx, b, rec, at=None):
    got = ctx.gftt_debug_corners(b)
    assert np.float32(got["M"]).view(np.uint32) == np.float32(rec["M"]).view(np.uint32), at
    assert got["n_candidates"] == rec["n_candidates"], (at, got["n_candidates"], rec["n_candidates"])
    assert np.array_equal(got["corners"], rec["corners"]), (at, len(got["corners"]), len(rec["corners"]))
    assert np.array_equal(got["vals"].view(np.uint32), rec["vals"].view(np.uint32)), at
    assert got["ranks"] == rec["ranks"], (at, got["ranks"], rec["ranks"])


def _gray3(g):
    """A BGR frame whose gray image is g."""
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


def _batch5(oracle):
    """[rich, flat 128, tiled, uniform noise, lowtex] at 640 x 480 (the tiled frame: a 32 x 32 block repeated
    over 320 x 256 on a flat background, so it stays below 16384 candidates)."""
    rb, rd, _, cam = synth_seq(5, seed=3, preset="fr1")
    lb, ld, _, _ = synth_seq(5, seed=7, preset="lowtex")
    flat = np.full_like(rb[0], 128)
    tg = np.full((480, 640), 128, np.uint8)
    tg[112:368, 160:480] = tiled_frame()
    noise = np.random.RandomState(12).randint(0, 256, size=(480, 640)).astype(np.uint8)
    bgr = np.stack([rb[0], flat, _gray3(tg), _gray3(noise), lb[0]])
    depth = np.stack([rd[0], rd[0], rd[0], rd[0], ld[0]])
    assert np.array_equal(oracle.gray(bgr[3]), noise) and np.array_equal(oracle.gray(bgr[2]), tg)
    want = [_want(("batch5", b), bgr[b], depth[b], cam) for b in range(5)]
    return bgr, depth, cam, want


# ------------------------------------------------------------------ the map
@pytest.mark.parametrize("case", ["fr3_320x256", "borders_320x256", "fr1_640x480"])
def test_map_matches_model(pkg, oracle, case):
    """The raw map's bits, M's bits and the candidate count."""
    import synth
    if case == "fr3_320x256":
        bgr, depth, _, cam = synth.sequence(2, seed=5, preset="fr3", W=320, H=256)
        g = oracle.gray(bgr[0])
    elif case == "borders_320x256":   # texture up to every border
        _, _, _, cam = synth.sequence(2, seed=5, preset="fr3", W=320, H=256)
        g = np.random.RandomState(31).randint(0, 256, size=(256, 320)).astype(np.uint8)
    else:
        bgr, depth, _, cam = synth_seq(5, seed=3, preset="fr1")
        g = oracle.gray(bgr[0])
    H, W = g.shape
    ctx = _ctx(pkg, cam, W=W, H=H)
    ctx.detect_and_compute(g)
    e = G.eig_map(g)
    M, thr, xy, val = G.candidates(e, 0.01)
    got = ctx.gftt_debug_eig(0)
    assert np.array_equal(got.view(np.uint32), e.view(np.uint32)), (case, int((got.view(np.uint32) != e.view(np.uint32)).sum()))
    rec = ctx.gftt_debug_corners(0)
    assert np.float32(rec["M"]).view(np.uint32) == np.float32(M).view(np.uint32)
    assert rec["n_candidates"] == len(xy) > 1000
    if case == "borders_320x256":
        assert e[0].max() > thr and e[:, 0].max() > thr and e[-1].max() > thr and e[:, -1].max() > thr
    ctx.close()


# ------------------------------------------------------------------ whole frames
@pytest.mark.parametrize("preset,seed", [("fr1", 3), ("lowtex", 7), ("icl", 23)])
def test_frames_bit_exact(pkg, oracle, preset, seed):
    bgr, depth, _, cam = synth_seq(5 if preset != "icl" else 2, seed=seed, preset=preset)
    if preset == "fr1":
        assert cam["k1"] != 0   # the distorted camera: kps_un differ from kps
    ctx = _ctx(pkg, cam)
    for f in range(2):
        want = _want((preset, seed, f), bgr[f], depth[f], cam)
        assert len(want["rec"]["corners"]) == 1000 and len(want["kps"]) > 700
        got = ctx.frame(bgr[f], depth[f])
        _same_frame(got, want, (preset, f))
        _same_corners(ctx, 0, want["rec"], (preset, f))
        if preset == "fr1":
            assert not np.array_equal(got["kps_un"]["x"], got["kps"]["x"])
    # detect_and_compute from a gray image (Extractor::detectAndCompute)
    g = oracle.gray(bgr[0])
    m = G.Extractor()
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
    bgr, depth, cam, want = _batch5(oracle)
    counts = [w["rec"]["n_candidates"] for w in want]
    assert counts[1] == 0 and len(want[1]["kps"]) == 0          # flat: M = 0, nothing, no error
    assert counts[3] > 16384 and counts[3] == max(counts)       # uniform noise
    cap = counts[3] + 1                                         # just above the model's count
    a = _ctx(pkg, cam, max_batch=5, cand_cap=cap)
    b1 = _ctx(pkg, cam, max_batch=1, cand_cap=cap)
    d_bgr, d_dep = _dev(bgr, depth)
    a.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 5)
    for b in range(5):
        got = a.batch_frame(b)
        _same_frame(got, want[b], b)
        _same_corners(a, b, want[b]["rec"], b)
        _same_frame(b1.frame(bgr[b], depth[b]), got, b)
    # the tiled frame's ties are decided by the raster index
    assert len(np.unique(want[2]["rec"]["vals"])) * 4 < len(want[2]["rec"]["vals"])
    a.close()
    b1.close()


def test_capacity_flag_per_frame(pkg, oracle):
    """cand_cap 16384: the noise frame alone overflows; the others equal the model, and so does a later extraction."""
    bgr, depth, cam, want = _batch5(oracle)
    over = [w["rec"]["n_candidates"] > 16384 for w in want]
    assert over == [False, False, False, True, False]
    ctx = _ctx(pkg, cam, max_batch=5, cand_cap=16384)
    d_bgr, d_dep = _dev(bgr, depth)
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 5)
    for b in (0, 1, 2, 4):
        _same_frame(ctx.batch_frame(b), want[b], b)
        _same_corners(ctx, b, want[b]["rec"], b)
    with pytest.raises(pkg.RgbdError, match="cand_cap"):
        ctx.batch_frame(3)
    assert ctx.gftt_debug_corners(3)["n_candidates"] == want[3]["rec"]["n_candidates"]   # the count goes on past the cap
    # a tracking chain fails the whole call and names the same cause
    with pytest.raises(pkg.RgbdError, match="cand_cap"):
        ctx.pnp_track_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 5, 0.9, pkg.pnp_params(), np.eye(4, dtype=np.float32))
    _same_frame(ctx.frame(bgr[0], depth[0]), want[0], "after")   # flag cleared
    ctx.close()


# ------------------------------------------------------------------ the selection stage alone
def _check_select(ctx, xy, val, W, H, md, maxc, chunk, memo=None, key=None):
    order = G.rank(xy, val, W)
    if memo is not None and key in memo:
        want = memo[key]
    else:
        want = G.select_brute(xy, order, md, maxc)[0]
        if memo is not None:
            memo[key] = want
    got = ctx.gftt_select(xy, val, W, H, md, maxc, chunk)
    assert np.array_equal(got, want), (key, md, maxc, chunk, len(got), len(want))
    return want


def _distinct(rs, n, W, H):
    idx = rs.choice(W * H, size=n, replace=False)
    return np.stack([idx % W, idx // W], 1).astype(np.int32)


def test_select_sizes(pkg):
    """n in {0, 1, 2, chunk - 1, chunk, chunk + 1, cand_cap}, for an explicit chunk and the default one."""
    cam = synth_seq(5, seed=3, preset="fr1")[3]
    ctx = _ctx(pkg, cam)
    rs = np.random.RandomState(41)
    W, H = 256, 192
    for chunk, eff in ((64, 64), (0, 2048)):   # the default chunk for 1000 corners is 2048
        for n in (0, 1, 2, eff - 1, eff, eff + 1, 32768):
            xy = _distinct(rs, n, W, H)
            val = rs.randint(1, 500, size=n).astype(np.float32) / np.float32(7)   # duplicates
            w = _check_select(ctx, xy, val, W, H, 3.0, 1000, chunk)
            assert len(w) == min(n, 1000) or n > 2
    ctx.close()


def test_select_ties_chains_and_staircase(pkg):
    cam = synth_seq(5, seed=3, preset="fr1")[3]
    ctx = _ctx(pkg, cam)
    rs = np.random.RandomState(43)
    for chunk in (64, 1000, 0):
        # all-equal values: pure address order, the higher raster index first
        xy = _distinct(rs, 700, 64, 48)
        w = _check_select(ctx, xy, np.full(700, 0.25, np.float32), 64, 48, 3.0, 1000, chunk)
        assert xy[w[0], 1] * 64 + xy[w[0], 0] == (xy[:, 1] * 64 + xy[:, 0]).max()
        # a monotone ridge along one row at spacing 2 over 300 px: a 150-long dependency chain
        n = 150
        ridge = np.stack([2 * np.arange(n) + 3, np.full(n, 9)], 1).astype(np.int32)
        w = _check_select(ctx, ridge, (n - np.arange(n)).astype(np.float32), 320, 32, 3.0, 1000, chunk)
        assert np.array_equal(w, np.arange(0, n, 2))
        # the same ridge descending from the right, and with ties in pairs
        _check_select(ctx, ridge, (1 + np.arange(n)).astype(np.float32), 320, 32, 3.0, 1000, chunk)
        _check_select(ctx, ridge, (1 + np.arange(n) // 2).astype(np.float32), 320, 32, 3.0, 1000, chunk)
        # a 2-D staircase: a spacing-2 lattice whose value falls with x + y (ties along the anti-diagonals)
        gx, gy = np.meshgrid(np.arange(30), np.arange(24))
        st = np.stack([2 * gx.ravel() + 1, 2 * gy.ravel() + 1], 1).astype(np.int32)
        sv = (100 - gx.ravel() - gy.ravel()).astype(np.float32)
        for md in (2.5, 3, 3.9, 10):
            _check_select(ctx, st, sv, 64, 52, md, 1000, chunk)
    ctx.close()


def test_select_random_lists(pkg):
    """Random lists with duplicate values over min_distance x max_corners x chunk."""
    cam = synth_seq(5, seed=3, preset="fr1")[3]
    ctx = _ctx(pkg, cam)
    rs = np.random.RandomState(47)
    W, H = 128, 96
    xy = _distinct(rs, 3000, W, H)
    val = rs.randint(1, 60, size=3000).astype(np.float32)
    order = G.rank(xy, val, W)
    memo = {}
    for md in (0, 1, 2.5, 3, 3.9, 10):
        yield1000 = len(G.select_brute(xy, order[:1000], md, 10 ** 6)[0])   # exactly what the first 1000 ranks yield
        total = len(G.select_brute(xy, order, md, 10 ** 6)[0])
        assert 0 < yield1000 <= total
        for maxc in (1, max(yield1000 // 2, 1), yield1000, min(total + 50, 12288)):   # the last exhausts the list
            for chunk in (64, 1000, 0):
                w = _check_select(ctx, xy, val, W, H, md, maxc, chunk, memo, (md, maxc))
                assert len(w) == min(maxc, total)
    ctx.close()


# ------------------------------------------------------------------ parameters
@pytest.mark.parametrize("kw", [dict(quality_level=0.05), dict(min_distance=0.0), dict(min_distance=1.0),
                                dict(min_distance=10.0), dict(nfeatures=300), dict(nfeatures=5000)])
def test_parameters_and_shapes(pkg, oracle, kw):
    import synth
    W, H = 320, 256
    bgr, depth, _, cam = synth.sequence(2, seed=5, preset="fr3", W=W, H=H)
    ctx = _ctx(pkg, cam, max_batch=2, W=W, H=H, **kw)
    m = G.Extractor(G.params(**kw), W=W, H=H)
    want = [m.frame(bgr[b], depth[b], cam) for b in range(2)]
    nf = kw.get("nfeatures", 1000)
    if nf == 5000:   # fewer than 5000 exist: the list is exhausted and every accepted corner comes out
        assert all(len(w["rec"]["corners"]) < 5000 and w["rec"]["ranks"] == w["rec"]["n_candidates"] for w in want)
    elif kw.get("min_distance") == 10.0:
        assert all(100 < len(w["rec"]["corners"]) for w in want)
    else:
        assert all(len(w["rec"]["corners"]) == nf for w in want)
    d_bgr, d_dep = _dev(bgr, depth)
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 2)
    for b in range(2):
        _same_corners(ctx, b, want[b]["rec"], (kw, b))
        _same_frame(ctx.batch_frame(b), want[b], (kw, b))
    ctx.close()


def test_refusals(pkg):
    lib = pkg.lib()
    cam = pkg.camera(500, 500, 320, 240)
    bad = [dict(nfeatures=0), dict(nfeatures=12289), dict(quality_level=0.0), dict(quality_level=1.0),
           dict(quality_level=float("nan")), dict(min_distance=-1.0), dict(min_distance=64.5),
           dict(min_distance=float("inf")), dict(min_distance=float("nan")), dict(cand_cap=-1), dict(cand_cap=(1 << 20) + 1)]
    for kw in bad:
        h = C.c_void_p()
        st = lib.rgbd_create_gftt(0, 640, 480, 1, C.byref(pkg.gftt_params(**kw)), C.byref(cam), C.byref(h))
        assert st == 4 and b"gftt" in lib.rgbd_last_error(h), (kw, st)
        lib.rgbd_destroy(h)
    for W, H in ((2048, 480), (640, 2048)):   # sides of at most 2047
        h = C.c_void_p()
        st = lib.rgbd_create_gftt(0, W, H, 1, C.byref(pkg.gftt_params()), C.byref(cam), C.byref(h))
        assert st == 4 and b"gftt" in lib.rgbd_last_error(h), (W, H, st)
        lib.rgbd_destroy(h)
    h = C.c_void_p()   # a one-level geometry refusal (the width is no multiple of 16)
    assert lib.rgbd_create_gftt(0, 650, 480, 1, C.byref(pkg.gftt_params()), C.byref(cam), C.byref(h)) == 4
    lib.rgbd_destroy(h)
    # a cand_cap of 65536 is within the bound
    ctx = pkg.Context(640, 480, max_batch=1, cam=cam, gftt=pkg.gftt_params(cand_cap=65536))
    ctx.close()
    # the other extractors' contexts have no GFTT stage
    ctx = pkg.Context(640, 480, max_batch=1, cam=cam)
    out = np.zeros((480, 640), np.float32)
    n = C.c_int32(0)
    assert lib.rgbd_gftt_debug_eig(ctx._h, 0, C.c_void_p(out.ctypes.data)) == 1 and b"not a GFTT context" in lib.rgbd_last_error(ctx._h)
    assert lib.rgbd_gftt_debug_corners(ctx._h, 0, None, None, None, None, 0, C.byref(n)) == 1
    xy = np.zeros((1, 2), np.int32)
    val = np.ones(1, np.float32)
    idx = np.zeros(1, np.int32)
    assert lib.rgbd_gftt_select(ctx._h, C.c_void_p(xy.ctypes.data), C.c_void_p(val.ctypes.data), 1, 64, 64, 3.0, 10, 0,
                                C.c_void_p(idx.ctypes.data), C.byref(n)) == 1
    ctx.close()


# ------------------------------------------------------------------ chains
def test_pnp_chain_matches_model(pkg, oracle):
    """Extract (GFTT + BRIEF) + Matcher + PnPRansac per consecutive pair, bit-exact vs the oracle chain over the
    model's frames."""
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
    bgr, depth, gt, cam = synth_seq(n, seed=7, preset="lowtex")
    base = str(tmp_path / "rgbd_dataset_freiburg1_seq") + os.sep
    D.write_dataset(base, bgr, depth, 100.0 + 0.033 * np.arange(n), gt)
    ds = D.open_dataset(base)
    p4, s4, i4 = track_sequence(pkg, ds, B=4, solver=solver, pose0=gt[0], extractor="gftt")
    pn, sn, i_n = track_sequence(pkg, ds, B=n, solver=solver, pose0=gt[0], extractor="gftt")
    assert np.array_equal(p4.view(np.uint32), pn.view(np.uint32))
    assert np.array_equal(s4, sn) and np.array_equal(i4, i_n) and sn[0] == 1 and sn.sum() > 1


def test_cpp_example_matches_python(pkg, oracle, tmp_path):
    """examples/gftt_example.cpp (rgbd::Extractor(GFTT, BRIEF, NORMAL) over include/rgbd/frontend.hpp) prints an
    FNV-1a hash of every frame's keypoints and descriptors; Extractor(GFTT, BRIEF, ADAPTIVE) still throws."""
    exe = os.path.join(ROOT, "rgbd-slam_amd", "build", "gftt_example")
    assert os.path.exists(exe), "build() must compile examples/gftt_example.cpp"
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
    ctx = _ctx(pkg, cam)
    for i in range(n):
        got = ctx.frame(bgr[i], depth[i])
        rec = ctx.gftt_debug_corners(0)
        assert int(rows[i][1]) == len(got["kps"]) > 700
        assert int(rows[i][2], 16) == fnv(got["kps"], got["desc"]), i
        assert int(rows[i][3]) == len(rec["corners"]) == 1000 and int(rows[i][4]) == rec["n_candidates"]
    ctx.close()
