"""Occupancy map timings for profiles/occmap/README.md: the per-kernel times of one scan and of an insert_batch rebuild
of 8 keyframes (synthetic fr1 frames, clouds with the default cloud parameters, ground-truth poses), from the context's
own timing table, and the wall time of both calls with the timing off.  Prints one JSON line.

  python tools/occmap_bench.py [--keyframes 8] [--capacity 262144]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=8)
    ap.add_argument("--capacity", type=int, default=1 << 18)
    args = ap.parse_args()
    from conftest import load_pkg, synth_seq
    pkg = load_pkg()
    from rgbd_slam_amd import occmap
    N = args.keyframes
    bgr, depth, poses, cam = synth_seq(N, seed=3, preset="fr1")
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"],
                   cam["factor"])
    ctx = pkg.Context(640, 480, max_batch=1, cam=c)
    clouds = [ctx.keyframe_cloud(bgr[f], depth[f]) for f in range(N)]
    sp = [occmap.sensor_pose(np.asarray(poses[f], np.float32)) for f in range(N)]
    T, o = [p[0] for p in sp], [p[1] for p in sp]
    m = pkg.OccupancyMap(ctx, pkg.occmap_params(capacity=args.capacity))
    out = {"points": [len(x) for x in clouds]}
    for _ in range(3):      # warm-up: code objects, buffers
        m.clear()
        m.insert_batch(clouds, T, o)
    out["voxels_after_batch"] = len(m)
    # wall time, timing off: a host clock around calls that end in a stream synchronise
    wall1, walln = [], []
    for _ in range(5):
        m.clear()
        ctx.synchronize()
        t0 = time.perf_counter()
        m.insert(clouds[0], T[0], o[0])
        wall1.append((time.perf_counter() - t0) * 1e3)
        m.clear()
        ctx.synchronize()
        t0 = time.perf_counter()
        m.insert_batch(clouds, T, o)
        walln.append((time.perf_counter() - t0) * 1e3)
    out["wall_ms_one_scan"] = wall1
    out["wall_ms_batch"] = walln
    # kernel times, timing on (an event pair per launch)
    ctx.set_timing(True)
    m.clear()
    ctx.reset_timing()
    m.insert(clouds[0], T[0], o[0])
    out["kernels_one_scan_ms"] = {k: v for k, v in ctx.timings().items() if k.startswith("k_occ")}
    out["voxels_after_one_scan"] = len(m)
    m.clear()
    ctx.reset_timing()
    m.insert_batch(clouds, T, o)
    out["kernels_batch_ms"] = {k: v for k, v in ctx.timings().items() if k.startswith("k_occ")}
    ctx.set_timing(False)
    m.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
