"""GPU parity of k_distribute's pyramid path (count / best-key pyramids over the depth-5 bins of a one-root level, the
division rounds on nodes alone) against the oracle's DistributeOctTree, with the path every tree took read through
debug_dist_path: 0 per-key state, 1 pyramid path, 2 pyramid path abandoned, 3 pyramid path skipped.  The paths are
also those of the Python model (quadtree_hist_model), level by level.

Frames are 640 x 480 unless said; the oracle side of every frame is computed once per module.
"""
import numpy as np
import pytest

import quadtree_hist_model as hm
import test_gpu_quadtree_state as qs
from conftest import synth_seq

pytestmark = pytest.mark.gpu

NFEAT = qs.NFEAT


def _oracle_case(oracle, bgr, depth, cam, nfeat=NFEAT):
    """(bgr, depth, cam, per-level candidates, per-level oracle selection, oracle frame, per-level model path)"""
    h, w = depth.shape
    p = oracle.orb_params(nfeat)
    t = oracle.tables(p, w, h)
    ref = oracle.pyramid(oracle.gray(bgr), p)
    cands, want, paths = [], [], []
    for l in range(8):
        c = oracle.level_candidates(ref[l], p)
        box = (16, int(t["w"][l]) - 16, 16, int(t["h"][l]) - 16)
        cands.append(c)
        want.append(oracle.distribute(c, *box, int(t["nfeat"][l])))
        paths.append(hm.distribute(c, *box, int(t["nfeat"][l]))[1])
    return (bgr, depth, cam, cands, want, oracle.frame(bgr, depth, p, oracle.camera(cam)), paths)


@pytest.fixture(scope="module")
def cases(oracle):
    bgr, depth, _, cam = synth_seq(4, seed=3, preset="fr1")
    cb, cd, _, ccam = synth_seq(2, seed=7, preset="corbs")
    flat = np.full((480, 640, 3), qs.FLAT, np.uint8)
    dot = flat.copy()
    dot[200, 300] = 200
    frames = {
        "fr1_0": (bgr[0], depth[0], cam),
        "fr1_1": (bgr[1], depth[1], cam),
        "corbs1": (cb[1], cd[1], ccam),
        "corner": (qs._block_frame(bgr[0], qs.CORNER_AT), depth[0], cam),
        "chain": (qs._block_frame(bgr[0], qs.CORNER_AT, qs.CHAIN_PATCHES), depth[0], cam),
        "deep": (hm.deep_frame(bgr[0], qs.FLAT), depth[0], cam),
        "flat": (flat, depth[0], cam),
        "dot": (dot, depth[0], cam),
    }
    return {name: _oracle_case(oracle, *f) for name, f in frames.items()}


def _paths(ctx, b):
    return [ctx.debug_dist_path(b, l) for l in range(8)]


def _check_single(pkg, case, tag):
    bgr, depth, cam, _, want, want_f, model_paths = case
    ctx = qs._ctx(pkg, cam)
    got_f = ctx.frame(bgr, depth)
    qs._assert_levels_equal(ctx, 0, want, tag)
    qs._assert_frame_equal(got_f, want_f, tag)
    paths = _paths(ctx, 0)
    ctx.close()
    assert paths == model_paths, (tag, paths, model_paths)
    return paths


@pytest.mark.parametrize("name", ["fr1_0", "corbs1"])
def test_rich_frames_take_the_pyramid_path(pkg, cases, name):
    """Every level of a rich frame (9-11k keys on level 0, the cell lists of CORBS past the gather's preloaded
    trips) completes on the pyramids."""
    assert _check_single(pkg, cases[name], name) == [hm.PATH_PYRAMID] * 8


def test_chain_is_not_run_on_the_pyramids(pkg, cases):
    """chain: a tree of 10 rounds on level 0 that splits one node off per round, far below depth 5; its 40-odd keys
    cannot fill the level, so the attempt is skipped (or abandoned)."""
    paths = _check_single(pkg, cases["chain"], "chain")
    assert paths[0] in (hm.PATH_ABANDONED, hm.PATH_SKIPPED), paths


def test_deep_tree_abandons_the_pyramids(pkg, cases):
    """deep: more keys than the budget on levels 0-4, in a region so small that nodes at depth 5 divide: the
    attempt is abandoned mid-rounds and nothing of it shows in the result."""
    ns = [len(c) for c in cases["deep"][3]]
    paths = _check_single(pkg, cases["deep"], "deep")
    assert paths[0] == hm.PATH_ABANDONED and ns[0] > len(cases["deep"][4][0]), (paths, ns)


def test_no_rounds(pkg, cases):
    """flat (no key on any level) and dot (levels of one key): no division round."""
    assert [len(c) for c in cases["flat"][3]] == [0] * 8
    assert max(len(c) for c in cases["dot"][3]) == 1
    assert _check_single(pkg, cases["flat"], "flat") == [hm.PATH_SKIPPED] * 8
    assert _check_single(pkg, cases["dot"], "dot") == [hm.PATH_SKIPPED] * 8


def test_mixed_batch(pkg, cases):
    """One extract_batch of 8 frames on the XCD-mapped grid mixing rich, chain, corner, deep, flat and dot frames:
    every frame equals its single-frame result and the oracle, and one launch holds completed, abandoned and
    skipped trees."""
    import torch
    names = ["fr1_0", "chain", "corner", "flat", "deep", "dot", "fr1_1", "chain"]
    cam = cases["fr1_0"][2]
    fb = np.ascontiguousarray(np.stack([cases[n][0] for n in names]))
    fd = np.ascontiguousarray(np.stack([cases[n][1] for n in names]))
    single = qs._ctx(pkg, cam)
    singles = [single.frame(fb[f], fd[f]) for f in range(8)]
    single.close()
    ctx = qs._ctx(pkg, cam, max_batch=8)
    d_bgr = torch.from_numpy(fb).cuda()
    d_dep = torch.from_numpy(fd.view(np.int16)).cuda()
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 8)
    seen = set()
    for f, n in enumerate(names):
        qs._assert_levels_equal(ctx, f, cases[n][4], f"batch {n}")
        got = ctx.batch_frame(f)
        qs._assert_frame_equal(got, cases[n][5], f"batch {n} vs oracle")
        qs._assert_frame_equal(got, singles[f], f"batch {n} vs single")
        paths = _paths(ctx, f)
        assert paths == cases[n][6], (n, paths, cases[n][6])
        seen.update(paths)
    ctx.close()
    assert seen == {hm.PATH_PYRAMID, hm.PATH_ABANDONED, hm.PATH_SKIPPED}, seen


def test_2000_features(pkg, oracle):
    """The rich frame at 2000 features (node capacity 512): the node arrays alone pass the workgroup's LDS budget,
    so no pyramid fits beside them at unchanged residency and every level stays on the per-key state."""
    bgr, depth, _, cam = synth_seq(4, seed=3, preset="fr1")
    _, _, _, _, want, want_f, _ = _oracle_case(oracle, bgr[0], depth[0], cam, nfeat=2000)
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"],
                   cam["k3"], cam["factor"])
    ctx = pkg.Context(640, 480, max_batch=1, orb=pkg.orb_params(2000), cam=c)
    got_f = ctx.frame(bgr[0], depth[0])
    qs._assert_levels_equal(ctx, 0, want, "2000")
    qs._assert_frame_equal(got_f, want_f, "2000")
    paths = _paths(ctx, 0)
    ctx.close()
    assert paths == [hm.PATH_KEYS] * 8, paths


def test_several_roots_stay_on_the_key_state(pkg, oracle):
    """640 x 336 (the top rows of a rich frame; a height whose every level fits the 30-px cell grid): every level
    starts from round(dX / dY) = 2 roots, which have no pyramid path."""
    bgr, depth, _, cam = synth_seq(4, seed=3, preset="fr1")
    b = np.ascontiguousarray(bgr[0][:336])
    d = np.ascontiguousarray(depth[0][:336])
    _, _, _, _, want, want_f, model_paths = _oracle_case(oracle, b, d, cam)
    assert model_paths == [hm.PATH_KEYS] * 8, model_paths
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"],
                   cam["k3"], cam["factor"])
    ctx = pkg.Context(640, 336, max_batch=1, orb=pkg.orb_params(NFEAT), cam=c)
    got_f = ctx.frame(b, d)
    qs._assert_levels_equal(ctx, 0, want, "640x336")
    qs._assert_frame_equal(got_f, want_f, "640x336")
    paths = _paths(ctx, 0)
    ctx.close()
    assert paths == [hm.PATH_KEYS] * 8, paths
