"""GPU parity at the edge regimes of the adaptive FAST, GFTT and cv::ORB front ends (csrc/adaptive.hip, csrc/gftt.hip,
csrc/cvorb.hip): the cases of tests/extractor_edge_cases.py (frame shapes with partial and one-row tiles and 11-bit x,
single / no / all-tied GFTT candidates, minimum adaptive ROIs, the threshold walk to cv::FAST's clamp and down to
min_thresh, capacities and nfeatures on their boundaries, cv::ORB zero budgets, thin levels, first-segment columns, FAST
thresholds 1 / 254 / 255, saturated input, retainBest's boundaries), batches from misaligned device pointers, gray images
with padded rows, and slots that held a rich frame and then receive a flat one.  Bit-exact against the CPU models
through the C ABI, stage by stage in pipeline order so that a mismatch is named where it starts:
  GFTT      the eigenvalue map's bits, then M / candidate count / corners / values / ranks, then the frame;
  adaptive  every cell's threshold before (f64 bits) / threshold used / tries / raster list, the carried thresholds,
            then the frame;
  cv::ORB   per level the FAST count, s1 / h1 and s2 / h2, then the frame.
tests/test_extractor_edge_cases.py proves from the models alone that each case is in its regime; the model frames are
computed once there (extractor_edge_cases.model) and reused here."""
import ctypes as C

import numpy as np
import pytest

import extractor_edge_cases as E

pytestmark = pytest.mark.gpu

ARG = 1   # rgbd_status


def _cam(pkg, cam):
    return pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"],
                      cam["k3"], cam["factor"])


def _ctx(pkg, c, max_batch=None):
    return pkg.Context(c["W"], c["H"], max_batch=max_batch or c["B"], cam=_cam(pkg, c["cam"]), **E.device_params(pkg, c))


def _dev(bgr, depth):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(bgr)).cuda(),
            torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda())


# ------------------------------------------------------------------ the stages, in pipeline order
def _same_frame(got, want, what):
    assert len(got["kps"]) == len(want["kps"]), f"{what}: frame: {len(got['kps'])} keypoints, model {len(want['kps'])}"
    assert np.array_equal(got["kps"], want["kps"]), f"{what}: kps"
    assert np.array_equal(got["desc"], want["desc"]), f"{what}: desc"
    assert np.array_equal(got["kps_un"], want["kps_un"]), f"{what}: kps_un"
    assert np.array_equal(got["xyz"].view(np.uint32), want["xyz"].view(np.uint32)), f"{what}: xyz"


def _gftt_map(ctx, b, rec, what):
    got, e = ctx.gftt_debug_eig(b), rec["e"]
    bad = got.view(np.uint32) != e.view(np.uint32)   # borders included
    assert not bad.any(), f"{what}: map: {np.count_nonzero(bad)} px differ, the first at (y, x) = {tuple(np.argwhere(bad)[0])}"


def _gftt_corners(ctx, b, rec, what, flagged=False):
    got = ctx.gftt_debug_corners(b)
    assert np.float32(got["M"]).view(np.uint32) == np.float32(rec["M"]).view(np.uint32), f"{what}: M {got['M']!r}, model {rec['M']!r}"
    assert got["n_candidates"] == rec["n_candidates"], f"{what}: {got['n_candidates']} candidates, model {rec['n_candidates']}"
    if flagged:   # the list was cut: only the count (it goes on past the cap) is defined
        return
    assert np.array_equal(got["corners"], rec["corners"]), f"{what}: corners ({len(got['corners'])}, model {len(rec['corners'])})"
    assert np.array_equal(got["vals"].view(np.uint32), rec["vals"].view(np.uint32)), f"{what}: corner values"
    assert got["ranks"] == rec["ranks"], f"{what}: ranks {got['ranks']}, model {rec['ranks']}"


def _adaptive_cells(ctx, b, rec, what, cut=None):
    """cut: the frame was flagged with this cell_cap, so a list holds the model's first `cut` maxima (raster order)."""
    for k, c in enumerate(rec["cells"]):
        before, used, tries, xys = ctx.adaptive_debug_cell(b, k)
        assert np.float64(before).view(np.uint64) == np.float64(c["before"]).view(np.uint64), \
            f"{what}: cell {k}: before {before!r}, model {c['before']!r}"
        assert (used, tries) == (c["used"], c["tries"]), f"{what}: cell {k}: used / tries {(used, tries)}, model {(c['used'], c['tries'])}"
        want = c["raster"] if cut is None else c["raster"][:cut]
        assert np.array_equal(xys, want), f"{what}: cell {k}: raster list ({len(xys)}, model {len(want)})"


def _cvorb_levels(ctx, b, rec, what):
    for l, lr in enumerate(rec["levels"]):
        got = ctx.cvorb_debug_level(b, l)
        assert got["n_fast"] == lr["n_fast"], f"{what}: level {l}: {got['n_fast']} FAST corners, model {lr['n_fast']}"
        assert np.array_equal(got["s1"], lr["s1"]), f"{what}: level {l}: s1 ({len(got['s1'])}, model {len(lr['s1'])})"
        assert np.array_equal(got["h1"].view(np.uint32), lr["h1"].view(np.uint32)), f"{what}: level {l}: h1"
        assert np.array_equal(got["s2"], lr["s2"]), f"{what}: level {l}: s2 ({len(got['s2'])}, model {len(lr['s2'])})"
        assert np.array_equal(got["h2"].view(np.uint32), lr["h2"].view(np.uint32)), f"{what}: level {l}: h2"


def _check_stages(ctx, c, b, want, what, flagged=False):
    """Every debug stage of frame b of the last batch against the model's frame `want`."""
    rec = want["rec"]
    if c["ext"] == E.GFTT:
        _gftt_map(ctx, b, rec, what)
        _gftt_corners(ctx, b, rec, what, flagged)
    elif c["ext"] == E.ADAPTIVE:
        _adaptive_cells(ctx, b, rec, what, c["dev"]["cell_cap"] if flagged else None)
    else:
        _cvorb_levels(ctx, b, rec, what)


def _same_thresholds(ctx, want, what):
    got = ctx.adaptive_thresholds()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), f"{what}: carried thresholds {got}, model {want}"


# ------------------------------------------------------------------ the case table
@pytest.mark.parametrize("name", E.NAMES)
def test_case_matches_model(pkg, oracle, name):
    c, m = E.case(name), E.model(name)
    ctx = _ctx(pkg, c)
    d_bgr, d_dep = _dev(c["bgr"], c["depth"])
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), c["B"])
    for b in range(c["B"]):
        what = "%s frame %d" % (name, b)
        _check_stages(ctx, c, b, m["frames"][b], what, flagged=b in c["flag"])
        if b in c["flag"]:
            with pytest.raises(pkg.RgbdError, match=c["flag"][b]):
                ctx.batch_frame(b)
        else:   # no flag: a flagged frame raises
            _same_frame(ctx.batch_frame(b), m["frames"][b], what)
    if c["ext"] == E.ADAPTIVE:
        _same_thresholds(ctx, m["thresholds"], name)
    if c["after"] is not None:   # a later extraction: the flag is cleared, the state carried on
        _same_frame(ctx.frame(*c["after"]), m["after"], name + " after")
        _check_stages(ctx, c, 0, m["after"], name + " after")
        if c["ext"] == E.ADAPTIVE:
            _same_thresholds(ctx, m["thresholds_after"], name + " after")
    ctx.close()


# ------------------------------------------------------------------ shared: pointers, row steps, stale state
EXTRACTORS = [E.GFTT, E.ADAPTIVE, E.CVORB]


@pytest.mark.parametrize("ext", EXTRACTORS)
def test_misaligned_batch_then_aligned(pkg, oracle, ext):
    """A 3-frame batch from device pointers offset by 1 byte (BGR) and 2 bytes (depth): the BGR frames start at
    addresses that are no multiple of 16 (k_svo_pyramid's / k_pyramid's scalar loads), the depth at one that is no
    multiple of 4.  Then the same context runs the batch from aligned pointers.  An adaptive context carries its
    thresholds from the first run into the second; the model does the same."""
    import torch
    c, bgr, depth = E.shared_frames(ext)
    B = 3
    want, th = E.shared_model(ext, (0, 1, 2, 0, 1, 2))
    ctx = _ctx(pkg, c, max_batch=B)
    raw_b = torch.zeros(bgr.size + 64, dtype=torch.uint8, device="cuda")
    raw_d = torch.zeros(depth.size + 32, dtype=torch.int16, device="cuda")
    for run, off in enumerate((1, 0)):
        d_bgr, d_dep = raw_b[off:off + bgr.size], raw_d[off:off + depth.size]
        d_bgr.copy_(torch.from_numpy(bgr.reshape(-1)))
        d_dep.copy_(torch.from_numpy(np.ascontiguousarray(depth).view(np.int16).reshape(-1)))
        torch.cuda.synchronize()
        assert d_bgr.data_ptr() % 16 == off and d_dep.data_ptr() % 4 == 2 * off
        ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B)
        for b in range(B):
            what = "%s offset %d frame %d" % (ext, off, b)
            _check_stages(ctx, c, b, want[3 * run + b], what)
            _same_frame(ctx.batch_frame(b), want[3 * run + b], what)
    if ext == E.ADAPTIVE:
        _same_thresholds(ctx, th, ext)
    ctx.close()


def _detect_padded(pkg, ctx, gray, pad):
    """rgbd_detect_and_compute on `gray` held in rows `pad` bytes longer, the padding filled with garbage."""
    H, W = gray.shape
    wide = np.random.RandomState(7).randint(0, 256, size=(H, W + pad)).astype(np.uint8)
    wide[:, :W] = gray
    kps = np.zeros(ctx.kp_cap, pkg.KEYPOINT_DTYPE)
    desc = np.zeros((ctx.kp_cap, 32), np.uint8)
    n = C.c_int32(0)
    st = pkg.lib().rgbd_detect_and_compute(ctx._h, wide.ctypes.data_as(C.c_void_p), W + pad,
                                           kps.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p), ctx.kp_cap,
                                           C.byref(n))
    assert st == 0, pkg.lib().rgbd_last_error(ctx._h)
    return kps[:n.value].copy(), desc[:n.value].copy()


@pytest.mark.parametrize("ext", EXTRACTORS)
def test_padded_gray_rows(pkg, oracle, ext):
    """rgbd_detect_and_compute takes a row step: the image inside a wider array (step W + 24, garbage in the padding)
    gives what the contiguous image gives, stage by stage; a step below the width is refused before anything is
    launched.  An adaptive context is put back to its initial thresholds before each call, so both start alike."""
    c = E.case(E.SHARED[ext])
    gray = oracle.gray(c["bgr"][0])
    m = E.make_model(ext, c["W"], c["H"], c["prm"])
    wk, wd, rec = m.detect_and_compute(gray)
    want = dict(rec=rec)
    ctx = _ctx(pkg, c, max_batch=1)
    th0 = ctx.adaptive_thresholds() if ext == E.ADAPTIVE else None
    k0, d0 = ctx.detect_and_compute(gray)
    assert len(k0) > 500 and np.array_equal(k0, wk) and np.array_equal(d0, wd), ext + ": contiguous"
    _check_stages(ctx, c, 0, want, ext + " contiguous")
    if ext == E.ADAPTIVE:
        ctx.set_adaptive_thresholds(th0)
    k1, d1 = _detect_padded(pkg, ctx, gray, 24)
    assert np.array_equal(k1, k0) and np.array_equal(d1, d0), ext + ": padded rows"
    _check_stages(ctx, c, 0, want, ext + " padded rows")
    ctx.set_timing(True)
    ctx.reset_timing()
    n = C.c_int32(0)
    st = pkg.lib().rgbd_detect_and_compute(ctx._h, gray.ctypes.data_as(C.c_void_p), c["W"] - 1, None, None, 0, C.byref(n))
    assert st == ARG and ctx.timings() == {}
    ctx.close()


def _assert_flat_stages(ctx, c, b, what):
    """Every debug stage of a flat frame reports zeros, whatever the slot held before."""
    if c["ext"] == E.GFTT:
        assert not ctx.gftt_debug_eig(b).view(np.uint32).any(), what + ": map"
        got = ctx.gftt_debug_corners(b)
        assert np.float32(got["M"]).view(np.uint32) == 0 and got["n_candidates"] == 0 and len(got["corners"]) == 0 \
            and got["ranks"] == 0, what
    elif c["ext"] == E.ADAPTIVE:
        for k in range(ctx.adaptive_cells):
            assert len(ctx.adaptive_debug_cell(b, k)[3]) == 0, "%s: cell %d" % (what, k)
    else:
        for l in range(c["prm"]["nlevels"]):
            got = ctx.cvorb_debug_level(b, l)
            assert got["n_fast"] == 0 and len(got["s1"]) == 0 and len(got["s2"]) == 0, "%s: level %d" % (what, l)


@pytest.mark.parametrize("ext", EXTRACTORS)
def test_stale_state(pkg, oracle, ext):
    """A max_batch = 2 context runs [rich, rich'], then [flat, rich''] and [rich, flat] in the same slots: the flat
    frame returns nothing and every debug stage of its slot reports zeros (score / nstrip / keys / ncand / maxkey /
    list / nge hold nothing of the rich frame before it); the rich frames equal the model."""
    c, bgr, depth = E.shared_frames(ext)
    order = (0, 1, -1, 2, 0, -1)
    want, th = E.shared_model(ext, order)
    flat = np.full_like(bgr[0], 128)
    ctx = _ctx(pkg, c, max_batch=2)
    for run in range(3):
        idx = order[2 * run:2 * run + 2]
        d_bgr, d_dep = _dev(np.stack([flat if i < 0 else bgr[i] for i in idx]), np.stack([depth[max(i, 0)] for i in idx]))
        ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 2)
        for b, i in enumerate(idx):
            what = "%s run %d slot %d" % (ext, run, b)
            w = want[2 * run + b]
            _check_stages(ctx, c, b, w, what)
            got = ctx.batch_frame(b)
            _same_frame(got, w, what)
            if i < 0:
                assert len(got["kps"]) == 0, what
                _assert_flat_stages(ctx, c, b, what)
            else:
                assert len(got["kps"]) > 500, what
    if ext == E.ADAPTIVE:
        _same_thresholds(ctx, th, ext)
    ctx.close()
