"""GPU parity: k_fast's gathered segments and its survivor lists at the edge shapes (bit-exact vs the oracle).

k_fast packs the leftover cells of a level's cell rows into full waves (gathered segments, each slot staged
from its own cell, cells of different cell rows side by side in one wave); the candidate lists keep their
layout and order.  The shapes reach what 640 x 480 does not:

  368 x 240   16, 18, 19 and 20 lanes per cell; cell interiors of 26 .. 42 rows (42 = the 48-px ROI limit:
              more than 32 rows per cell); leftover cells in every cell row of levels 0-3; a single
              cell row on levels 6 and 7 (the width is a multiple of 16, as rgbd_create demands: 376 is refused)
  512 x 384   leftovers on levels 1-6, 17-19 lanes per cell on levels 2-3 and 5-7, none on level 0

Frames: uniform noise (the densest survivor pattern the NMS allows: the emission ranks and the cell_cap
bound), low-contrast noise (100 .. 118: no corner at iniThFAST = 20, so every cell takes the minThFAST
fallback), left half noise / right half low contrast (fallback and non-fallback cells side by side in a wave,
and mixed across cell rows by the gathered segments), and a constant frame (empty lists).  Every level's
candidate list is compared in order, then the whole frame.  One more case runs a 640 x 480 pair through
extract_batch (the per-frame slot bases).
"""
import numpy as np
import pytest

from conftest import synth_seq

pytestmark = pytest.mark.gpu

SHAPES = [(368, 240), (512, 384)]
KINDS = ["noise", "lowcontrast", "halves", "constant"]


def _gray_frame(kind, W, H):
    rng = np.random.default_rng(W * 31 + H)
    noise = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    low = rng.integers(100, 119, size=(H, W)).astype(np.uint8)
    if kind == "noise":
        return noise
    if kind == "lowcontrast":
        return low
    if kind == "halves":
        return np.concatenate([noise[:, :W // 2], low[:, W // 2:]], axis=1)
    return np.full((H, W), 93, np.uint8)


def _cam_dict(W, H):
    return dict(fx=525.0, fy=525.0, cx=W / 2.0, cy=H / 2.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, factor=5000.0)


def _assert_frame_equal(got, want, tag):
    assert len(got["kps"]) == len(want["kps"]), f"{tag} count {len(got['kps'])} vs {len(want['kps'])}"
    for name in ("kps", "kps_un"):
        for fld in got[name].dtype.names:
            assert np.array_equal(got[name][fld], want[name][fld]), f"{tag} {name}.{fld}"
    assert np.array_equal(got["desc"], want["desc"]), f"{tag} desc"
    assert np.array_equal(got["xyz"].view(np.uint32), want["xyz"].view(np.uint32)), f"{tag} xyz"


def _assert_candidates(ctx, oracle, b, gray, p, tag):
    ref = oracle.pyramid(gray, p)
    total = 0
    for l in range(p.nlevels):
        want = oracle.level_candidates(ref[l], p)
        got = ctx.debug_candidates(b, l)
        assert got.shape == want.shape, f"{tag} level {l}: {len(got)} vs {len(want)} candidates"
        assert np.array_equal(got, want), f"{tag} level {l}"
        total += len(want)
    return total


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "%dx%d" % s)
def shape_ctx(request, pkg):
    W, H = request.param
    cd = _cam_dict(W, H)
    cam = pkg.camera(cd["fx"], cd["fy"], cd["cx"], cd["cy"], cd["k1"], cd["k2"], cd["p1"], cd["p2"], cd["k3"],
                     cd["factor"])
    ctx = pkg.Context(W, H, max_batch=1, orb=pkg.orb_params(1000, 1.2, 8), cam=cam)
    yield W, H, ctx
    ctx.close()


@pytest.mark.parametrize("kind", KINDS)
def test_candidates_and_frame_bit_exact(pkg, oracle, shape_ctx, kind):
    W, H, ctx = shape_ctx
    gray = _gray_frame(kind, W, H)
    bgr = np.ascontiguousarray(np.repeat(gray[:, :, None], 3, axis=2))
    depth = np.full((H, W), 5000, np.uint16)
    p = oracle.orb_params(1000, 1.2, 8)
    assert np.array_equal(oracle.gray(bgr), gray)
    got = ctx.frame(bgr, depth)
    total = _assert_candidates(ctx, oracle, 0, gray, p, f"{W}x{H} {kind}")
    assert (total == 0) == (kind == "constant"), total
    _assert_frame_equal(got, oracle.frame(bgr, depth, p, oracle.camera(_cam_dict(W, H))), f"{W}x{H} {kind}")


def test_lowcontrast_cells_take_the_fallback(oracle):
    """The low-contrast frames hold no corner at iniThFAST and many at minThFAST (what the case above relies on)."""
    for W, H in SHAPES:
        gray = _gray_frame("lowcontrast", W, H)
        assert int(gray.max()) - int(gray.min()) < 20
        assert len(oracle.level_candidates(gray, oracle.orb_params(1000, 1.2, 8, 20, 20))) == 0
        assert len(oracle.level_candidates(gray, oracle.orb_params(1000, 1.2, 8))) > 100


def test_batch_pair_candidates_and_keypoints(pkg, oracle):
    """640 x 480, B = 2 through extract_batch: both frames' candidate lists and selected keypoints."""
    import torch
    bgr, depth, _, cam = synth_seq(2, seed=3, preset="fr1")
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"],
                   cam["k3"], cam["factor"])
    ctx = pkg.Context(640, 480, max_batch=2, orb=pkg.orb_params(1000), cam=c)
    d_bgr = torch.from_numpy(np.ascontiguousarray(bgr)).cuda()
    d_dep = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda()
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 2)
    p, oc = oracle.orb_params(1000), oracle.camera(cam)
    for f in range(2):
        assert _assert_candidates(ctx, oracle, f, oracle.gray(bgr[f]), p, f"batch frame {f}") > 1000
        _assert_frame_equal(ctx.batch_frame(f), oracle.frame(bgr[f], depth[f], p, oc), f"batch frame {f}")
    ctx.close()
