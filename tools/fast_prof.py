"""Kernel times of the plain FAST extraction alone (both descriptors), next to the ORB2, the adaptive FAST + BRIEF and
the cv::ORB extractors' on the same frames and in the same run (64 frames per batch, HIP events per kernel): one JSON
line per preset.  "noise" is uniform noise, a different seed per frame, over the fr1 depth images.

    python tools/fast_prof.py [frames per batch] [preset ...]      (default: 64 fr1 lowtex noise)

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
PRESETS = sys.argv[2:] or ["fr1", "lowtex", "noise"]
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


def span(v):
    return [int(min(v)), int(max(v))]


for preset in PRESETS:
    bgr, depth, gt, cam = synth.sequence(B, seed=1000, preset="fr1" if preset == "noise" else preset)
    if preset == "noise":
        g = np.stack([np.random.RandomState(5 + b).randint(0, 256, (480, 640)).astype(np.uint8) for b in range(B)])
        bgr = np.ascontiguousarray(np.repeat(g[:, :, :, None], 3, axis=3))
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"],
                   cam["factor"])
    d_bgr = torch.from_numpy(bgr).cuda()
    d_dep = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda()
    out = {"preset": preset, "frames": B, "repeats": R}
    for d in ("brief", "orb"):
        fctx = pkg.Context(640, 480, max_batch=B, cam=c, fast=pkg.fast_params(1000, descriptor=d, cand_cap=65536))
        us = timed(fctx, d_bgr, d_dep)
        out["fast_%s_us_per_launch" % d] = us
        out["fast_%s_select_share" % d] = round(us.get("k_fast_select", 0.0) / max(us["total"], 1e-9), 3)
        out["fast_%s_kept_min_max" % d] = span([len(fctx.batch_frame(b)["kps"]) for b in range(B)])
        if d == "brief":
            out["fast_candidates_min_max"] = span([fctx.fast_debug_corners(b)[0] for b in range(B)])
        fctx.close()
    octx = pkg.Context(640, 480, max_batch=B, cam=c, orb=pkg.orb_params(1000))
    out["orb2_us_per_launch"] = timed(octx, d_bgr, d_dep)
    octx.close()
    actx = pkg.Context(640, 480, max_batch=B, cam=c, adaptive=pkg.adaptive_params(1000))
    init = actx.adaptive_thresholds()
    out["adaptive_us_per_launch"] = timed(actx, d_bgr, d_dep, reset=lambda: actx.set_adaptive_thresholds(init))
    actx.close()
    try:
        cctx = pkg.Context(640, 480, max_batch=B, cam=c, cvorb=pkg.cvorb_params(1000, cand_cap=12288))
        out["cvorb_us_per_launch"] = timed(cctx, d_bgr, d_dep)
        flagged = 0
        for b in range(B):
            try:
                cctx.batch_frame(b)
            except pkg.RgbdError:
                flagged += 1
        out["cvorb_frames_over_capacity"] = flagged   # their times still count: the kernels ran
        cctx.close()
    except pkg.RgbdError as e:
        out["cvorb_us_per_launch"] = str(e)
    print(json.dumps(out), flush=True)
