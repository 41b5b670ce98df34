"""Kernel times of the OpenCV ORB extraction (Extractor(ORB, ORB, NORMAL)) next to the ORB2 extraction's on the same
frames and in the same run (64 frames per batch, HIP events per kernel): one JSON line per preset.

    python tools/cvorb_prof.py [frames per batch] [preset ...]      (default: 64 fr1 lowtex)

Both contexts share the pyramid and the blur; "k_fast(blur)" is the k_fast grid launched with its blur blocks alone.
The cv::ORB context stores up to 12288 FAST corners per level (the rich frames' level 0 holds more than the default
8192)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from conftest import load_pkg  # noqa: E402
import synth  # noqa: E402
import torch  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
PRESETS = sys.argv[2:] or ["fr1", "lowtex"]
R = 10
pkg = load_pkg()


def timed(ctx, d_bgr, d_dep):
    for _ in range(3):
        ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B)
    ctx.synchronize()
    ctx.reset_timing()
    ctx.set_timing(True)
    for _ in range(R):
        ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B)
    ctx.synchronize()
    t = ctx.timings()
    us = {k: round(v[0] * 1e3 / max(v[1], 1), 1) for k, v in sorted(t.items())}
    us["total"] = round(sum(us.values()), 1)
    return us


def span(v):
    return [int(min(v)), int(max(v))]


for preset in PRESETS:
    bgr, depth, gt, cam = synth.sequence(B, seed=1000, preset=preset)
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"],
                   cam["factor"])
    d_bgr = torch.from_numpy(bgr).cuda()
    d_dep = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda()
    cctx = pkg.Context(640, 480, max_batch=B, cam=c, cvorb=pkg.cvorb_params(1000, cand_cap=12288))
    c_us = timed(cctx, d_bgr, d_dep)
    c_kept = [len(cctx.batch_frame(b)["kps"]) for b in range(B)]
    recs = [cctx.cvorb_debug_level(b, 0) for b in range(B)]
    cctx.close()
    octx = pkg.Context(640, 480, max_batch=B, cam=c, orb=pkg.orb_params(1000))
    o_us = timed(octx, d_bgr, d_dep)
    o_kept = [len(octx.batch_frame(b)["kps"]) for b in range(B)]
    octx.close()
    print(json.dumps({"preset": preset, "frames": B, "repeats": R, "cvorb_us_per_launch": c_us, "orb2_us_per_launch": o_us,
                      "cvorb_kept_min_max": span(c_kept), "orb2_kept_min_max": span(o_kept),
                      "cvorb_level0_fast_min_max": span([r["n_fast"] for r in recs]),
                      "cvorb_level0_first_selection_min_max": span([len(r["s1"]) for r in recs])}))
