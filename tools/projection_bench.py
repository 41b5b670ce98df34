"""Time projection-guided matching (rgbd_projection_match_batch) on the benchmark's shape: B synthetic fr1 frames
at 1000 keypoints, the B - 1 consecutive pairs with their true poses, th 5 and 15; per kernel (k_proj_grid,
k_proj_search, k_proj_assign), and in the same process k_knn2 over the same pairs through the existing tracking
path (rgbd_pnp_track_batch).  Warm-up, then --reps timed repetitions: median, min and max per kernel, one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def pingpong(n, U):
    """0 .. U-1, U-2 .. 0, 1 ..: every consecutive pair is a neighbouring-frame pair of the rendered sequence."""
    period = np.concatenate([np.arange(U), np.arange(U - 2, 0, -1)])
    return period[np.arange(n) % len(period)]


def stats(v):
    v = np.asarray(v)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--unique", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import synth
    bgr, depth, gt, cam = synth.sequence(args.unique, seed=1000, preset="fr1")
    import torch
    from conftest import load_pkg
    pkg = load_pkg()
    B = args.batch
    src = pingpong(B, args.unique)
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"],
                   cam["factor"])
    ctx = pkg.Context(640, 480, max_batch=B, orb=pkg.orb_params(1000), cam=c)
    d_bgr = torch.from_numpy(np.ascontiguousarray(bgr[src])).cuda()
    d_dep = torch.from_numpy(np.ascontiguousarray(depth[src]).view(np.int16)).cuda()
    poses = np.ascontiguousarray(np.asarray(gt, np.float32)[src])
    qf, tf = np.arange(B - 1, dtype=np.int32), np.arange(1, B, dtype=np.int32)
    out = {"frames": B, "pairs": B - 1, "unique_frames": args.unique, "reps": args.reps, "kernel_ms": {}}

    # k_knn2 through the existing path: the tracking step's matcher over the same pairs
    ctx.set_timing(True)
    ctx.set_timing_filter("k_knn2")
    knn = []
    for r in range(args.warmup + args.reps):
        ctx.reset_timing()
        ctx.pnp_track_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B, 0.9, pose0=poses[0].reshape(4, 4))
        t = ctx.timings()["k_knn2"]
        if r >= args.warmup:
            knn.append(t[0])
    out["kernel_ms"]["k_knn2"] = stats(knn)
    ctx.set_timing_filter(None)

    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B)
    ctx.synchronize()
    for th in (5.0, 15.0):
        per = {k: [] for k in ("k_proj_grid", "k_proj_search", "k_proj_assign")}
        nm = 0
        for r in range(args.warmup + args.reps):
            ctx.reset_timing()
            m = ctx.projection_match_batch(qf, tf, poses, th)
            t = ctx.timings()
            nm = int(np.mean([len(x) for x in m]))
            if r >= args.warmup:
                for k in per:
                    per[k].append(t[k][0])
        tot = np.sum([per[k] for k in per], 0)
        out["kernel_ms"]["th%g" % th] = dict({k: stats(v) for k, v in per.items()}, total=stats(tot),
                                             matches_per_pair=nm)
    ctx.set_timing(False)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
