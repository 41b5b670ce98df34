"""Kernel times of the bag-of-words place recognition (profiles/bow/README.md records a run).

  * rgbd_bow_transform_frames over 1024 extracted frames (the four synthetic frames tiled on the device) and
    rgbd_bow_transform_batch over 1024 frames of random descriptors (every descent a different path), against a
    generated k = 10, L = 6 vocabulary (a full tree of random descriptors, built here, 1,111,111 nodes);
  * one rgbd_loopdb_query against 4096 entries;
  * one keyframe's transform and its two database queries, to name the kernel that bounds an insertion;
  * for scale, the same descent by tests/bow_model.py's inner loop on one host core.
Kernel times are HIP-event times around the launches (Context.timings()).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK = 8.0e12   # bytes / s


def full_tree(V, k, L, seed):
    rng = np.random.default_rng(seed)
    n = (k ** (L + 1) - 1) // (k - 1)
    parent = (np.arange(n, dtype=np.int64) - 1) // k      # breadth-first ids: the children of i are k i + 1 .. k i + k
    parent[0] = 0
    first_leaf = (k ** L - 1) // (k - 1)
    leaf = (np.arange(n) >= first_leaf).astype(np.uint8)
    word = np.where(leaf == 1, np.arange(n) - first_leaf, -1)
    weight = np.where(leaf == 1, rng.random(n) * 5.0 + 0.01, 0.0)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return V.Vocabulary(k, L, parent, desc, weight, leaf, word)


def timed(ctx, fn, reps):
    fn()                                                   # warm: allocations, code objects
    ctx.set_timing(True)
    ctx.reset_timing()
    for _ in range(reps):
        fn()
    t = ctx.timings()
    ctx.set_timing(False)
    return {k: v[0] / v[1] for k, v in t.items() if k.startswith("k_bow")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--entries", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from conftest import load_pkg, synth_seq
    pkg = load_pkg()
    import importlib
    V = importlib.import_module("rgbd_slam_amd.vocabulary")
    import bow_model as M

    k, L = 10, 6
    voc = full_tree(V, k, L, 1)
    bgr, depth, gt, cam = synth_seq(4, seed=3, preset="fr1")
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"], cam["factor"])
    B, ctx = a.frames, None
    while ctx is None:   # one context addresses at most 4 GiB of pyramids: the largest extraction batch it takes
        try:
            ctx = pkg.Context(640, 480, max_batch=B, orb=pkg.orb_params(1000), cam=c)
        except pkg.RgbdError:
            if B == 1:
                raise
            B //= 2
    ctx.voc_set(voc)
    out = dict(k=k, L=L, nodes=voc.n_nodes, descriptor_mb=voc.n_nodes * 32 / 1e6, frames=a.frames, extracted_frames=B)

    reps = (B + 3) // 4
    d_bgr = torch.from_numpy(np.ascontiguousarray(bgr)).cuda().repeat(reps, 1, 1, 1)[:B].contiguous()
    d_dep = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda().repeat(reps, 1, 1)[:B].contiguous()
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B)
    counts = [len(ctx.batch_frame(b)["desc"]) for b in range(4)]
    n_desc = sum(counts[b % 4] for b in range(B))
    frames = np.arange(B, dtype=np.int32)
    t = timed(ctx, lambda: ctx.bow_transform_frames(frames, 4), a.reps)
    gather = n_desc * L * k * 32
    out["frames_tiled"] = dict(descriptors=n_desc, ms=t, gather_bytes=gather,
                               gather_tb_s=gather / (t["k_bow_words"] * 1e-3) / 1e12,
                               hbm_peak_fraction=gather / (t["k_bow_words"] * 1e-3) / HBM_PEAK)

    rng = np.random.default_rng(2)
    B = a.frames
    descs = [rng.integers(0, 256, (1000, 32), dtype=np.uint8) for _ in range(B)]
    t = timed(ctx, lambda: ctx.bow_transform_batch(descs, 4), a.reps)
    gather = B * 1000 * L * k * 32
    out["batch_random"] = dict(descriptors=B * 1000, ms=t, gather_bytes=gather,
                               gather_tb_s=gather / (t["k_bow_words"] * 1e-3) / 1e12,
                               hbm_peak_fraction=gather / (t["k_bow_words"] * 1e-3) / HBM_PEAK)

    # one host core, the model's inner loop, on a sample of one frame's descriptors
    sample, children = descs[0][:200], voc.children()
    t0 = time.perf_counter()
    for d in sample:
        M.descend(voc, children, d, 4)
    per = (time.perf_counter() - t0) / len(sample)
    out["host_model"] = dict(us_per_descriptor=per * 1e6, s_for_batch=per * B * 1000)

    # the database: vectors of real frames' size over the vocabulary's words
    one = ctx.bow_transform(ctx.batch_frame(0)["desc"], 4)
    nw = len(one["ids"])
    for _ in range(a.entries):
        ids = np.sort(rng.choice(voc.n_words, nw, replace=False)).astype(np.uint32)
        v = rng.random(nw)
        ctx.loopdb_add(ids, v / v.sum())
    t = timed(ctx, lambda: ctx.loopdb_query(one["ids"], one["vals"], True), a.reps)
    out["query"] = dict(entries=a.entries, words_per_entry=nw, ms=t)

    # a keyframe insertion: one frame's transform, then the two queries of obtainCandidates
    desc0 = ctx.batch_frame(0)["desc"]
    t1 = timed(ctx, lambda: ctx.bow_transform(desc0, 4), a.reps)
    out["insertion"] = dict(transform_ms=t1, queries_ms=2 * t["k_bow_score"],
                            bound_by="k_bow_score" if 2 * t["k_bow_score"] > sum(t1.values()) else "k_bow_words + k_bow_vector")
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
