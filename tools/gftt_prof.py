"""Kernel times of the Shi-Tomasi GFTT + BRIEF extraction alone, next to the SVO + BRIEF and the adaptive FAST +
BRIEF extractors' on the same frames and in the same run (64 frames per batch, HIP events per kernel): one JSON
line per preset.

    python tools/gftt_prof.py [frames per batch] [preset ...]      (default: 64 fr1 lowtex)

The adaptive extractor's thresholds are reset before every timed batch, so each repeat walks the same chain."""
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


def timed(ctx, d_bgr, d_dep, reset=None):
    for _ in range(3):
        if reset:
            reset()
        ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B)
    ctx.synchronize()
    ctx.reset_timing()
    ctx.set_timing(True)
    for _ in range(R):
        if reset:
            reset()
        ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B)
    ctx.synchronize()
    t = ctx.timings()
    us = {k: round(v[0] * 1e3 / max(v[1], 1), 1) for k, v in sorted(t.items())}
    us["total"] = round(sum(us.values()), 1)
    return us


for preset in PRESETS:
    bgr, depth, gt, cam = synth.sequence(B, seed=1000, preset=preset)
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"],
                   cam["factor"])
    d_bgr = torch.from_numpy(bgr).cuda()
    d_dep = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda()
    gctx = pkg.Context(640, 480, max_batch=B, cam=c, gftt=pkg.gftt_params(1000))
    g_us = timed(gctx, d_bgr, d_dep)
    recs = [gctx.gftt_debug_corners(b) for b in range(B)]
    g_kept = [len(gctx.batch_frame(b)["kps"]) for b in range(B)]
    gctx.close()
    sctx = pkg.Context(640, 480, max_batch=B, cam=c, svo=pkg.svo_params(1000))
    s_us = timed(sctx, d_bgr, d_dep)
    s_kept = [len(sctx.batch_frame(b)["kps"]) for b in range(min(B, 8))]
    sctx.close()
    actx = pkg.Context(640, 480, max_batch=B, cam=c, adaptive=pkg.adaptive_params(1000))
    init = actx.adaptive_thresholds()
    a_us = timed(actx, d_bgr, d_dep, reset=lambda: actx.set_adaptive_thresholds(init))
    a_kept = [len(actx.batch_frame(b)["kps"]) for b in range(min(B, 8))]
    actx.close()

    def span(v):
        return [int(min(v)), int(max(v))]
    print(json.dumps({"preset": preset, "frames": B, "repeats": R, "gftt_us_per_launch": g_us, "svo_us_per_launch": s_us,
                      "adaptive_us_per_launch": a_us, "gftt_kept_min_max": span(g_kept),
                      "gftt_corners_min_max": span([len(r["corners"]) for r in recs]),
                      "gftt_candidates_min_max": span([r["n_candidates"] for r in recs]),
                      "gftt_ranks_min_max": span([r["ranks"] for r in recs]),
                      "svo_kept": s_kept, "adaptive_kept": a_kept}))
