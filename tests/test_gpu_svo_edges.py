"""GPU parity at the edge regimes of the SVO + BRIEF front end (csrc/svo.hip, csrc/svo_host.cpp): the cases of
tests/svo_edge_cases.py (frame sizes with partial tiles and unaligned levels, grid cell counts, FAST barriers around the
reference's score floor, nfeatures on retainBest's boundary), a batch from misaligned device pointers, gray images with
padded rows, and the refused configurations.  Bit-exact against the CPU oracle (oracle/orc_svo.cpp), stage by stage in
pipeline order so that a mismatch is named where it starts: pyramid levels, grid keypoints, then the frame.
tests/test_svo_edge_cases.py proves from the oracle alone that each case is in its regime."""
import ctypes as C

import numpy as np
import pytest

import svo_edge_cases as E

pytestmark = pytest.mark.gpu


def _cam(pkg, cam):
    return pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"],
                      cam["k3"], cam["factor"])


def _ctx(pkg, c, max_batch=1):
    ctx = pkg.Context(c["W"], c["H"], max_batch=max_batch, cam=_cam(pkg, c["cam"]), svo=pkg.svo_params(**c["prm"]))
    assert ctx.kp_cap == E.kp_cap(c["W"], c["H"], c["prm"])
    return ctx


def _same_levels(ctx, oracle, b, gray, nlevels, what):
    ref = oracle.svo_pyramid(gray, nlevels)
    for l in range(nlevels):
        got = ctx.svo_debug_level(b, l)
        assert got.shape == ref[l].shape, (what, l)
        assert np.array_equal(got, ref[l]), f"{what}: level {l}: {np.count_nonzero(got != ref[l])} px differ"


def _same_grid(ctx, oracle, b, gray, p, what):
    xyl, resp = ctx.svo_debug_grid(b)
    want = oracle.svo_detect(gray, p)
    assert len(xyl) == len(want), f"{what}: grid: {len(xyl)} keypoints, oracle {len(want)}"
    same = ((xyl[:, 0] == want["x"].astype(np.int32)) & (xyl[:, 1] == want["y"].astype(np.int32))
            & (xyl[:, 2] == want["octave"]) & (resp.view(np.uint32) == want["response"].view(np.uint32)))
    assert same.all(), f"{what}: grid: {np.count_nonzero(~same)} of {len(want)} keypoints differ"


def _same_frame(got, want, what):
    assert len(got["kps"]) == len(want["kps"]), f"{what}: frame: {len(got['kps'])} keypoints, oracle {len(want['kps'])}"
    assert np.array_equal(got["kps"], want["kps"]), f"{what}: kps"
    assert np.array_equal(got["desc"], want["desc"]), f"{what}: desc"
    assert np.array_equal(got["kps_un"], want["kps_un"]), f"{what}: kps_un"
    assert np.array_equal(got["xyz"].view(np.uint32), want["xyz"].view(np.uint32)), f"{what}: xyz"


def _check_stages(ctx, oracle, b, bgr, depth, c, got, what):
    p, oc = E.oracle_params(oracle, c["prm"]), oracle.camera(c["cam"])
    gray = oracle.gray(bgr)
    _same_levels(ctx, oracle, b, gray, c["prm"]["nlevels"], what)
    _same_grid(ctx, oracle, b, gray, p, what)
    _same_frame(got, oracle.svo_frame(bgr, depth, p, oc), what)


@pytest.mark.parametrize("name", E.NAMES)
def test_case_matches_oracle(pkg, oracle, name):
    c = E.case(name)
    ctx = _ctx(pkg, c)
    got = ctx.frame(c["bgr"], c["depth"])
    _check_stages(ctx, oracle, 0, c["bgr"], c["depth"], c, got, name)
    if name in E.SHAPES:   # Extractor::detectAndCompute from a gray image: k_svo_pyramid's src0 == nullptr branch
        gray = oracle.gray(c["bgr"])
        k, d = ctx.detect_and_compute(gray)
        p = E.oracle_params(oracle, c["prm"])
        _same_levels(ctx, oracle, 0, gray, c["prm"]["nlevels"], name + " (gray)")
        _same_grid(ctx, oracle, 0, gray, p, name + " (gray)")
        wk, wd = oracle.svo_detect_and_compute(gray, p)
        assert np.array_equal(k, wk) and np.array_equal(d, wd), name + " (gray)"
    ctx.close()


def test_misaligned_batch_then_aligned(pkg, oracle):
    """Frames at device addresses that are no multiple of 16 take k_svo_pyramid's scalar BGR loads (the context's
    width is always a multiple of 16, so only the pointer can be misaligned); the depth is read from an address that
    is no multiple of 4.  Then the same context runs from aligned pointers: k_svo_select reset every cell of the
    ragged grid (74 x 48 = 3552 cells, 4 per thread on 888 threads)."""
    import torch
    c = E.case("x_partial_tiles")
    W, H, B = c["W"], c["H"], 3
    frames = [E.images(W, H, shift=s)[:2] for s in (0, 100, 200)]
    bgr = np.stack([f[0] for f in frames])
    depth = np.stack([f[1] for f in frames])
    assert not np.array_equal(bgr[0], bgr[1]) and not np.array_equal(bgr[1], bgr[2])
    ctx = _ctx(pkg, c, max_batch=B)
    raw_b = torch.zeros(bgr.size + 64, dtype=torch.uint8, device="cuda")
    raw_d = torch.zeros(depth.size + 32, dtype=torch.int16, device="cuda")
    for off in (1, 0):
        d_bgr, d_dep = raw_b[off:off + bgr.size], raw_d[off:off + depth.size]
        d_bgr.copy_(torch.from_numpy(bgr.reshape(-1)))
        d_dep.copy_(torch.from_numpy(np.ascontiguousarray(depth).view(np.int16).reshape(-1)))
        torch.cuda.synchronize()
        assert d_bgr.data_ptr() % 16 == off and d_dep.data_ptr() % 4 == 2 * off
        assert (W * H * 3) % 16 == 0   # every frame of the batch starts as misaligned as the first
        ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B)
        for b in range(B):
            _check_stages(ctx, oracle, b, bgr[b], depth[b], c, ctx.batch_frame(b), "offset %d frame %d" % (off, b))
    ctx.close()


def _detect_padded(pkg, ctx, gray, pad):
    """rgbd_detect_and_compute on `gray` held in rows `pad` bytes longer, the padding filled with garbage."""
    H, W = gray.shape
    rs = np.random.RandomState(7)
    wide = rs.randint(0, 256, size=(H, W + pad)).astype(np.uint8)
    wide[:, :W] = gray
    kps = np.zeros(ctx.kp_cap, pkg.KEYPOINT_DTYPE)
    desc = np.zeros((ctx.kp_cap, 32), np.uint8)
    n = C.c_int32(0)
    st = pkg.lib().rgbd_detect_and_compute(ctx._h, wide.ctypes.data_as(C.c_void_p), W + pad,
                                           kps.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p), ctx.kp_cap,
                                           C.byref(n))
    assert st == 0, pkg.lib().rgbd_last_error(ctx._h)
    return kps[:n.value].copy(), desc[:n.value].copy()


def test_padded_gray_rows(pkg, oracle, seq_fr1):
    """rgbd_detect_and_compute takes a row step: an image inside a wider array (step = W + 24, garbage in the
    padding) gives what the contiguous image gives, on an SVO context and on an ORB context; a step below the width
    is refused before anything is launched."""
    c = E.case("x_partial_tiles")
    gray = oracle.gray(c["bgr"])
    ctx = _ctx(pkg, c)
    k0, d0 = ctx.detect_and_compute(gray)
    wk, wd = oracle.svo_detect_and_compute(gray, E.oracle_params(oracle, c["prm"]))
    assert len(k0) > 500 and np.array_equal(k0, wk) and np.array_equal(d0, wd)
    k1, d1 = _detect_padded(pkg, ctx, gray, 24)
    assert np.array_equal(k1, k0) and np.array_equal(d1, d0)
    _same_levels(ctx, oracle, 0, gray, c["prm"]["nlevels"], "padded rows")
    ctx.set_timing(True)
    ctx.reset_timing()
    n = C.c_int32(0)
    st = pkg.lib().rgbd_detect_and_compute(ctx._h, gray.ctypes.data_as(C.c_void_p), c["W"] - 1, None, None, 0, C.byref(n))
    assert st == E.ARG and ctx.timings() == {}
    ctx.close()

    bgr, _, _, cam = seq_fr1
    gray = oracle.gray(bgr[0])
    ctx = pkg.Context(640, 480, max_batch=1, orb=pkg.orb_params(1000), cam=_cam(pkg, cam))
    k0, d0 = ctx.detect_and_compute(gray)
    wk, wd = oracle.detect_and_compute(gray, oracle.orb_params(1000))
    assert len(k0) > 500 and np.array_equal(k0, wk) and np.array_equal(d0, wd)
    k1, d1 = _detect_padded(pkg, ctx, gray, 24)
    assert np.array_equal(k1, k0) and np.array_equal(d1, d0)
    ctx.close()


@pytest.mark.parametrize("name", [r[0] for r in E.REFUSALS])
def test_refusals(pkg, name):
    """A refused configuration never gets as far as the device: rgbd_create_svo returns the status from
    svo_configure, before the context has a stream or a buffer, so its timing table (the record of every launch a
    context makes) is empty and stays empty, and the Python wrapper raises."""
    _, W, H, over, status, msg = next(r for r in E.REFUSALS if r[0] == name)
    prm = dict(E.DEFAULTS, **over)
    cam = _cam(pkg, E.images(W, H)[2])
    svo = pkg.svo_params(**prm)
    L = pkg.lib()
    h = C.c_void_p()
    st = L.rgbd_create_svo(0, W, H, 1, C.byref(svo), C.byref(cam), C.byref(h))
    try:
        assert st == status, (st, L.rgbd_last_error(h))
        assert h.value and msg in L.rgbd_last_error(h).decode()
        assert L.rgbd_set_timing(h, 1) == 0
        assert L.rgbd_timing_count(h) == 0   # nothing launched
    finally:
        if h.value:
            L.rgbd_destroy(h)
    with pytest.raises(pkg.RgbdError, match=r"status %d" % status):
        pkg.Context(W, H, max_batch=1, cam=cam, svo=svo)
