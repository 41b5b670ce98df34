"""GPU parity: the blurred pyramid at the tile borders of the matrix-core level blur (k_fast's blur_tile_walk),
bit-exact against oracle.blur(oracle.pyramid(...)[l]) for every level.

Shapes are the smallest 3- and 8-level frames the context accepts (W % 16 == 0, every level a whole grid of FAST
cells of at most 48 px) that have a level below 64 px wide, which keeps the blur_walk fallback (the scale factors
1.23 and 1.26 are what makes such a level possible), and whose levels put the REFLECT_101 columns and rows across
the 32-px tile borders: over the levels the tile path takes (level >= 1, at least 64 x 32) w mod 32 and h mod 32
each fall in {0..3} and in {29..31}.  The residues are asserted from oracle.tables before the GPU is touched.
Contents: noise, all 0, all 255 and a 0/255 checkerboard (the extremes reach the ends of the signed byte split).
Batches: 3 (2-D grid) and 16 (XCD-mapped 1-D grid; the second group of eight is compared).
One more frame, 272 x 500 with two levels (the smallest accepted one: a frame may be at most twice as tall as
wide), has a level 1 of 14 row blocks, more than the 13 (RGBD_BLUR_MS) one wave walks, so its columns are split
into two strips and the second strip's warm-up block lies inside the image."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(96, 114, 3, 1.23), (320, 314, 8, 1.26)]   # W, H, levels, scale factor
TALL = (272, 500, 2, 1.2)
BLUR_MS = 13   # RGBD_BLUR_MS (csrc/rgbd_internal.h)


def level_sizes(oracle, W, H, nlevels, scale):
    t = oracle.tables(oracle.orb_params(1000, scale, nlevels), W, H)
    return [(int(w), int(h)) for w, h in zip(t["w"], t["h"])]


def tiled(sizes):
    return [(w, h) for w, h in sizes[1:] if w >= 64 and h >= 32]   # (level 0 is blurred inside k_pyramid)


def _assert_coverage(oracle):
    tl = []
    for W, H, n, sc in SHAPES:
        sizes = level_sizes(oracle, W, H, n, sc)
        assert tiled(sizes), (W, H, n, sizes)
        assert any(w < 64 for w, h in sizes[1:]), ("no fallback level", W, H, n, sizes)
        tl += tiled(sizes)
    assert (level_sizes(oracle, *TALL)[1][1] + 31) // 32 > BLUR_MS
    for k, name in ((0, "w"), (1, "h")):
        assert any(s[k] % 32 <= 3 for s in tl), (name, "mod 32 in 0..3", tl)
        assert any(s[k] % 32 >= 29 for s in tl), (name, "mod 32 in 29..31", tl)


def _frames(W, H, B, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((B, H, W, 3), np.uint8)
    for b in range(B):
        kind = b % 4
        if kind == 0:
            out[b] = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        elif kind == 1:
            out[b] = (((xx + yy + b // 4) & 1) * 255).astype(np.uint8)[:, :, None]
        elif kind == 2:
            out[b] = 255
    return out


@pytest.mark.parametrize("W,H,nlevels,scale,B", [s + (b,) for b in (3, 16) for s in SHAPES] + [TALL + (3,)])
def test_blurred_levels_bit_exact(pkg, oracle, W, H, nlevels, scale, B):
    import torch
    _assert_coverage(oracle)
    sizes = level_sizes(oracle, W, H, nlevels, scale)
    p = oracle.orb_params(1000, scale, nlevels)
    ctx = pkg.Context(W, H, max_batch=B, orb=pkg.orb_params(1000, scale, nlevels), cam=pkg.camera(525.0, 525.0, W / 2.0, H / 2.0))
    d_dep = torch.zeros((B, H, W), dtype=torch.int16).cuda()
    # B = 3 holds three of the four contents per call: a second call rotates them
    for call in range(2 if B == 3 else 1):
        fb = np.roll(_frames(W, H, max(B, 4), 11 * W + B + call), -call, axis=0)[:B]
        fb = np.ascontiguousarray(fb)
        d_bgr = torch.from_numpy(fb).cuda()
        ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B)
        torch.cuda.synchronize()
        for b in (range(B) if B == 3 else (0, 8, 9, 10, 11, 15)):
            ref = oracle.pyramid(oracle.gray(fb[b]), p)
            for l, (w, h) in enumerate(sizes):
                got = ctx.debug_blurred(b, l, w, h)
                want = oracle.blur(ref[l])
                bad = np.argwhere(got != want)
                assert bad.size == 0, f"call {call} frame {b} level {l} ({w} x {h}): {len(bad)} px differ, first (y, x) {bad[0]}"
    ctx.close()
