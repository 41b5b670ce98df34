"""Time the Umeyama RANSAC (rgbd_ransac_umeyama_frames) on the benchmark's shape: B synthetic fr1 frames at 1000
keypoints (a few rendered frames walked back and forth), the B - 1 consecutive pairs' Matcher::match lists, one
generator per pair; per kernel (k_umeyama, k_umeyama_gather) and the call's wall time.  Beside it, as the yardstick,
rgbd_ransac_se3 on the same pairs and matches, one call per pair (it has no batched form outside the tracking
chain): the sum of its k_ransac_hyp kernel times and of the calls' wall times.  Warm-up, then --reps timed
repetitions: median, min and max, one JSON line."""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--se3-reps", type=int, default=3)
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
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B)
    ctx.synchronize()
    qf, tf = np.arange(B - 1, dtype=np.int32), np.arange(1, B, dtype=np.int32)
    # the match list of a pair depends on the rendered frames alone: one Matcher::match per distinct (a, b)
    first = {}
    for b in range(B):
        first.setdefault(int(src[b]), b)
    fr = {u: ctx.batch_frame(b) for u, b in first.items()}
    cache, matches = {}, []
    for p in range(B - 1):
        a, b = int(src[p]), int(src[p + 1])
        if (a, b) not in cache:
            cache[(a, b)] = ctx.match(fr[a]["desc"], fr[b]["desc"], np.zeros(len(fr[a]["kps"]), np.uint8), fr[a]["xyz"][:, 2],
                                      fr[b]["xyz"][:, 2], 0.9)
        matches.append(cache[(a, b)])
    out = {"frames": B, "pairs": B - 1, "unique_frames": args.unique, "reps": args.reps, "kernel_ms": {},
           "matches_per_pair": round(float(np.mean([len(m) for m in matches])), 1)}
    prm = pkg.umeyama_params()
    ctx.set_timing(True)
    per = {k: [] for k in ("k_umeyama", "k_umeyama_gather")}
    wall = []
    for r in range(args.warmup + args.reps):
        rngs = [pkg.rng(1000 + p) for p in range(B - 1)]
        ctx.reset_timing()
        t0 = time.perf_counter()
        got = ctx.ransac_umeyama_frames(qf, tf, matches, prm, rngs)
        t1 = time.perf_counter()
        t = ctx.timings()
        if r >= args.warmup:
            wall.append((t1 - t0) * 1e3)
            for k in per:
                per[k].append(t[k][0])
    out["kernel_ms"].update({k: stats(v) for k, v in per.items()})
    out["frames_call_wall_ms"] = stats(wall)
    out["iterations_per_pair"] = round(float(np.mean([g["iterations"] for g in got])), 2)
    out["iterations_max"] = int(max(g["iterations"] for g in got))
    out["inliers_per_pair"] = round(float(np.mean([g["n_inliers"] for g in got])), 1)
    out["ok_pairs"] = int(sum(g["ok"] for g in got))

    # the yardstick: RansacSE3 (200 hypotheses, 19-step refinement chains) on the same pairs, one call each
    sprm = pkg.ransac_params()
    se3_k, se3_wall, se3_in = [], [], []
    for r in range(1 + args.se3_reps):
        rng, st = pkg.rng(1000), pkg.Sticky()
        ctx.reset_timing()
        t0 = time.perf_counter()
        nin = []
        for p in range(B - 1):
            a, b = int(src[p]), int(src[p + 1])
            ok, T, inl, rmse = ctx.ransac_se3(fr[a]["xyz"], fr[b]["xyz"], matches[p], sprm, rng, st)
            nin.append(len(inl))
        t1 = time.perf_counter()
        if r >= 1:
            se3_wall.append((t1 - t0) * 1e3)
            se3_k.append(ctx.timings()["k_ransac_hyp"][0])
            se3_in = nin
    out["ransac_se3"] = dict(k_ransac_hyp_ms=stats(se3_k), calls_wall_ms=stats(se3_wall),
                             inliers_per_pair=round(float(np.mean(se3_in)), 1))
    ctx.set_timing(False)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
