"""Time the motion-only bundle adjustment (rgbd_pnp_solver_frames) on the benchmark's shape: B synthetic fr1
frames at 1000 keypoints, the B - 1 consecutive pairs' th = 5 projection matches (found under the true poses),
every frame's pose then moved by one fixed offset (1 cm, 0.5 degrees) so that each pair's guess is off its
optimum; per kernel (k_pnpba, k_pnpba_gather).  Beside it: the wall and kernel time of one single-problem call,
the LM iterations per round of a sample of pairs (debug hook on host-gathered edges), and in the same process
k_pnp_refine -- the existing 10-step Gauss-Newton on the tracking step's matches of the same pairs -- for scale.
Warm-up, then --reps timed repetitions: median, min and max, one JSON line."""
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
    ap.add_argument("--sample", type=int, default=32, help="pairs whose rounds are read through the debug hook")
    args = ap.parse_args()
    import synth
    bgr, depth, gt, cam = synth.sequence(args.unique, seed=1000, preset="fr1")
    import torch
    import chain_model
    import pnp_solver_cases as Cs
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

    # k_pnp_refine through the existing path: the tracking step's PnPRansac over the same pairs
    ctx.set_timing(True)
    ctx.set_timing_filter("k_pnp_refine")
    ref = []
    for r in range(args.warmup + args.reps):
        ctx.reset_timing()
        _, _, ninl, nm = ctx.pnp_track_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B, 0.9, pose0=poses[0].reshape(4, 4))
        t = ctx.timings()["k_pnp_refine"]
        if r >= args.warmup:
            ref.append(t[0])
    out["kernel_ms"]["k_pnp_refine"] = stats(ref)
    out["pnp_refine_matches_per_pair"] = round(float(np.mean(nm[1:])), 1)
    out["pnp_refine_inliers_per_pair"] = round(float(np.mean(ninl[1:])), 1)
    ctx.set_timing_filter(None)

    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B)
    ctx.synchronize()
    matches = ctx.projection_match_batch(qf, tf, poses, 5.0)
    off = Cs.pose(np.deg2rad(0.5) * np.array([0.6, -0.64, 0.48]), [0.006, -0.0064, 0.0048])
    guess = np.stack([(off @ p.reshape(4, 4).astype(np.float64)).astype(np.float32) for p in poses]).reshape(B, 16)
    out["edges_per_pair"] = round(float(np.mean([len(m) for m in matches])), 1)
    per = {k: [] for k in ("k_pnpba", "k_pnpba_gather")}
    wall = []
    for r in range(args.warmup + args.reps):
        ctx.reset_timing()
        t0 = time.perf_counter()
        got = ctx.pnp_solver_frames(qf, tf, guess, matches, False)
        t1 = time.perf_counter()
        t = ctx.timings()
        if r >= args.warmup:
            wall.append((t1 - t0) * 1e3)
            for k in per:
                per[k].append(t[k][0])
    out["kernel_ms"].update({k: stats(v) for k, v in per.items()})
    out["frames_call_wall_ms"] = stats(wall)
    out["inliers_per_pair"] = round(float(np.mean([g["n_inliers"] for g in got if g["ok"]])), 1)

    # one single-problem call, and the rounds of a sample of pairs
    K4 = np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], np.float32)
    G = guess.reshape(B, 4, 4)
    iters, trials, one_wall, one_k = [], [], [], []
    for p in range(min(args.sample, B - 1)):
        fa, fb, m = ctx.batch_frame(int(qf[p])), ctx.batch_frame(int(tf[p])), matches[p]
        Xw = np.stack([chain_model.unproject_world(G[qf[p]], fa["xyz"][i]) for i in m["queryIdx"]])
        ku = fb["kps_un"][m["trainIdx"]]
        obs = np.stack([ku["x"], ku["y"]], 1).astype(np.float32)
        d = ctx.debug_pnp_solver(Xw, obs, K4, G[tf[p]])
        iters.append(d["iters"][:d["rounds_run"]])
        trials.append(d["trials"][:d["rounds_run"]])
        if p == 0:
            for r in range(args.warmup + args.reps):
                ctx.reset_timing()
                t0 = time.perf_counter()
                ctx.pnp_solver(Xw, obs, K4, G[tf[p]])
                t1 = time.perf_counter()
                if r >= args.warmup:
                    one_wall.append((t1 - t0) * 1e3)
                    one_k.append(ctx.timings()["k_pnpba"][0])
            out["single_call"] = dict(edges=len(m), wall_ms=stats(one_wall), k_pnpba_ms=stats(one_k))
    out["lm_iterations_per_round"] = round(float(np.mean(np.concatenate(iters))), 2)
    out["lm_trials_per_round"] = round(float(np.mean(np.concatenate(trials))), 2)
    ctx.set_timing(False)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
