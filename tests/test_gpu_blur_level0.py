"""GPU parity: blurred level 0 from the matrix-core level blur (k_fast's blur_tile_walk), bit-exact against
oracle.blur(oracle.gray(frame)); every other level of the same call is compared too.

Level 0 of a multi-level pyramid is blurred by the tile waves like levels 1 and up (k_pyramid blurs nothing).
Shapes, asserted from oracle.tables before the GPU is touched:
  - the smallest accepted two-level frames that put level 0's REFLECT_101 rows across the 32-row block borders
    (h mod 32 in 0..3 and in 29..31) and that hold both widths a level 0 can have mod 32: a frame is a multiple
    of 16 px wide, so w mod 32 is 0 or 16 (a whole last tile, half a last tile) and never 29..31;
  - a frame exactly 64 px wide: two column tiles, the first and the last table and no interior one (its level 1
    must still hold one 30-px FAST cell column, which takes a scale factor near 1);
  - 272 x 500: 16 level-0 row blocks, more than the 13 (RGBD_BLUR_MS) one wave walks, so two strips of 8 whose
    second warm-up block lies inside the image;
  - 640 x 480, the benchmark's frame: 15 row blocks, strips of 8 and 7.
Contents: noise, all 0, all 255 and a 0/255 checkerboard.  Batches: 3 (2-D grid, two calls so that every content
is seen) and 16 (XCD-mapped 1-D grid; frames 0, 8, 9 and 15 are compared).
A one-level pyramid keeps the blur_thread path: its descriptors, through ctx.frame, must still match the oracle."""
import numpy as np
import pytest

from test_gpu_blur_tiles import BLUR_MS, _frames, level_sizes

pytestmark = pytest.mark.gpu

SMALL = [(80, 93, 2, 1.2), (96, 96, 2, 1.2)]   # W, H, levels, scale factor
W64 = (64, 65, 2, 1.03)
TALL = (272, 500, 2, 1.2)
BENCH = (640, 480, 8, 1.2)
SHAPES = SMALL + [W64, TALL, BENCH]


def _strips(h):
    """(strips, blocks per strip) of a level of h rows: ceil(nb / 13) strips of near-equal length."""
    nb = (h + 31) // 32
    strips = (nb + BLUR_MS - 1) // BLUR_MS
    return strips, (nb + strips - 1) // strips


def _assert_coverage(oracle):
    for s in SHAPES:
        w, h = level_sizes(oracle, *s)[0]
        assert (w, h) == s[:2] and w >= 64 and h >= 32 and s[2] > 1, s   # level 0 is one for the tile path
    small = [level_sizes(oracle, *s)[0] for s in SMALL]
    assert {w % 32 for w, h in small} == {0, 16}, small
    assert any(h % 32 <= 3 for w, h in small) and any(h % 32 >= 29 for w, h in small), small
    assert level_sizes(oracle, *W64)[0][0] == 64
    assert _strips(TALL[1]) == (2, 8)       # the second strip's warm-up block starts at row 32 * 8 - 4 = 252
    assert _strips(BENCH[1]) == (2, 8) and (BENCH[1] + 31) // 32 == 15


@pytest.mark.parametrize("W,H,nlevels,scale,B", [s + (b,) for b in (3, 16) for s in SHAPES])
def test_blurred_level0_bit_exact(pkg, oracle, W, H, nlevels, scale, B):
    import torch
    _assert_coverage(oracle)
    sizes = level_sizes(oracle, W, H, nlevels, scale)
    p = oracle.orb_params(1000, scale, nlevels)
    ctx = pkg.Context(W, H, max_batch=B, orb=pkg.orb_params(1000, scale, nlevels), cam=pkg.camera(525.0, 525.0, W / 2.0, H / 2.0))
    d_dep = torch.zeros((B, H, W), dtype=torch.int16).cuda()
    for call in range(2 if B == 3 else 1):
        fb = np.ascontiguousarray(np.roll(_frames(W, H, max(B, 4), 13 * W + H + B + call), -call, axis=0)[:B])
        d_bgr = torch.from_numpy(fb).cuda()
        ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B)
        torch.cuda.synchronize()
        for b in (range(B) if B == 3 else (0, 8, 9, 15)):
            g = oracle.gray(fb[b])
            ref = oracle.pyramid(g, p)
            assert np.array_equal(ref[0], g)
            for l, (w, h) in enumerate(sizes):
                got = ctx.debug_blurred(b, l, w, h)
                want = oracle.blur(g if l == 0 else ref[l])
                bad = np.argwhere(got != want)
                assert bad.size == 0, f"call {call} frame {b} level {l} ({w} x {h}): {len(bad)} px differ, first (y, x) {bad[0]}"
    ctx.close()


def test_one_level_pyramid_keeps_blur_thread(pkg, oracle, seq_fr1):
    bgr, depth, _, cam = seq_fr1
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"],
                   cam["factor"])
    ctx = pkg.Context(640, 480, max_batch=1, orb=pkg.orb_params(1000, 1.2, 1), cam=c)
    got = ctx.frame(bgr[0], depth[0])
    want = oracle.frame(bgr[0], depth[0], oracle.orb_params(1000, 1.2, 1), oracle.camera(cam))
    assert len(got["kps"]) == len(want["kps"]) > 100, (len(got["kps"]), len(want["kps"]))
    assert np.array_equal(got["kps"]["x"], want["kps"]["x"]) and np.array_equal(got["kps"]["y"], want["kps"]["y"])
    assert np.array_equal(got["desc"], want["desc"])
    g = oracle.gray(bgr[0])
    assert np.array_equal(ctx.debug_blurred(0, 0, 640, 480), oracle.blur(g))
    ctx.close()
