"""GPU parity of k_distribute's per-key round state (node index + quadrant, one destination table per round, no
root pass on one-root levels) against the oracle's DistributeOctTree, in the regimes the rich frames of
test_gpu_extract.py do not reach: sparse levels and deep trees, cell lists longer than the gather's preloaded
trips, a batch that mixes all of them on the XCD-mapped grid, and roots with one key or none.

All frames are 640 x 480.  Every level is compared through debug_selected with oracle.distribute and the frame
with oracle.frame; the oracle side of every frame is computed once per module.
"""
import numpy as np
import pytest

import quadtree_model as qm
from conftest import synth_seq

pytestmark = pytest.mark.gpu

NFEAT = 1000
FLAT = 90                      # gray level of the flat frames
BLOCK_SRC = (300, 200)         # (x, y) in fr1 seed 3 frame 0 of the 48 x 48 textured block
CORNER_AT = (20, 20)           # block near the top-left corner: bordered (4, 4) .. (52, 52), one root quadrant
# block centred on the level-0 root's midpoint, bordered (304, 224) = image (320, 240): all four root quadrants
STRADDLE_AT = (296, 216)
# A block inside one quadrant ends its tree in the first round (one child: the list does not grow), so a deep tree
# needs keys that split off round after round: 12 x 12 patches in the opposite quadrant of the block's box of
# rounds 1, 2 and 3 (bordered boxes 608 x 448, 304 x 224, 152 x 112); from round 4 on the block itself divides.
CHAIN_PATCHES = ((416, 316), (216, 166), (116, 96))
PATCH = 12


def _model_rounds(c, w, h, N):
    """List length after every round of quadtree_model's formulation (one root, its rules and helpers)."""
    n = len(c)
    if n == 0:
        return []
    nodes = [dict(box=(0, 0, w - 32, h - 32), keys=list(range(n)), cid=0)]
    nxt, phase, lens = 1, 1, []
    while True:
        prev = len(nodes)
        S = [i for i, nd in enumerate(nodes) if len(nd["keys"]) > 1]
        if phase == 2:
            S.sort(key=lambda i: (len(nodes[i]["keys"]), nodes[i]["cid"]), reverse=True)
        kids, run, napply = {}, prev, len(S)
        for j, i in enumerate(S):
            qs = {}
            for k in nodes[i]["keys"]:
                qs.setdefault(qm.quad(c[k, 0], c[k, 1], nodes[i]["box"]), []).append(k)
            kids[i] = qs
            run += len(qs) - 1
            if phase == 2 and run >= N:
                napply = j + 1
                break
        new = []
        for i in S[:napply]:
            for q in sorted(kids[i]):
                new.append(dict(box=qm.child_box(nodes[i]["box"], q), keys=kids[i][q], cid=nxt))
                nxt += 1
        new.reverse()
        applied = set(S[:napply])
        T = len(new)
        nodes = new + [nd for i, nd in enumerate(nodes) if i not in applied]
        lens.append(len(nodes))
        if len(nodes) >= N or len(nodes) == prev:
            return lens
        if phase == 1 and len(nodes) + 3 * sum(1 for nd in nodes[:T] if len(nd["keys"]) > 1) > N:
            phase = 2


def _block_frame(tex, at, patches=()):
    fr = np.full((480, 640, 3), FLAT, np.uint8)
    sx, sy = BLOCK_SRC
    fr[at[1]:at[1] + 48, at[0]:at[0] + 48] = tex[sy:sy + 48, sx:sx + 48]
    for x, y in patches:
        fr[y:y + PATCH, x:x + PATCH] = tex[sy + 60:sy + 60 + PATCH, sx + 60:sx + 60 + PATCH]
    return fr


@pytest.fixture(scope="module")
def cases(oracle):
    """name -> (bgr, depth, cam, per-level candidates, per-level oracle selection, oracle frame)."""
    bgr, depth, _, cam = synth_seq(4, seed=3, preset="fr1")
    cb, cd, _, ccam = synth_seq(2, seed=7, preset="corbs")
    flat = np.full((480, 640, 3), FLAT, np.uint8)
    dot = flat.copy()
    dot[200, 300] = 200        # one isolated corner
    frames = {
        "corner": (_block_frame(bgr[0], CORNER_AT), depth[0], cam),
        "straddle": (_block_frame(bgr[0], STRADDLE_AT), depth[0], cam),
        "chain": (_block_frame(bgr[0], CORNER_AT, CHAIN_PATCHES), depth[0], cam),
        "flat": (flat, depth[0], cam),
        "dot": (dot, depth[0], cam),
        "corbs1": (cb[1], cd[1], ccam),
        "fr1_0": (bgr[0], depth[0], cam),
        "fr1_1": (bgr[1], depth[1], cam),
        "fr1_2": (bgr[2], depth[2], cam),
    }
    p = oracle.orb_params(NFEAT)
    t = oracle.tables(p)
    out = {}
    for name, (b, d, c) in frames.items():
        ref = oracle.pyramid(oracle.gray(b), p)
        cands = [oracle.level_candidates(ref[l], p) for l in range(8)]
        want = [oracle.distribute(cands[l], 16, int(t["w"][l]) - 16, 16, int(t["h"][l]) - 16, int(t["nfeat"][l]))
                for l in range(8)]
        out[name] = (b, d, c, cands, want, oracle.frame(b, d, p, oracle.camera(c)))
    return out


def _ctx(pkg, cam, max_batch=1):
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"],
                   cam["k3"], cam["factor"])
    return pkg.Context(640, 480, max_batch=max_batch, orb=pkg.orb_params(NFEAT), cam=c)


def _assert_frame_equal(got, want, tag):
    assert len(got["kps"]) == len(want["kps"]), f"{tag} count {len(got['kps'])} vs {len(want['kps'])}"
    for name in ("kps", "kps_un"):
        for fld in got[name].dtype.names:
            bad = np.flatnonzero(got[name][fld] != want[name][fld])
            assert len(bad) == 0, f"{tag} {name}.{fld}: {len(bad)} differ, first {bad[:5]}"
    assert np.array_equal(got["desc"], want["desc"]), f"{tag} desc"
    assert np.array_equal(got["xyz"].view(np.uint32), want["xyz"].view(np.uint32)), f"{tag} xyz"


def _assert_levels_equal(ctx, b, want, tag):
    for l in range(8):
        got = ctx.debug_selected(b, l)
        assert len(got) == len(want[l]), f"{tag} level {l}: sel_count {len(got)} vs {len(want[l])}"
        assert np.array_equal(got, want[l]), f"{tag} level {l}"


def _check_single(pkg, case, tag):
    bgr, depth, cam, _, want, want_f = case
    ctx = _ctx(pkg, cam)
    got_f = ctx.frame(bgr, depth)
    _assert_levels_equal(ctx, 0, want, tag)
    _assert_frame_equal(got_f, want_f, tag)
    ctx.close()
    return got_f


@pytest.mark.parametrize("name", ["corner", "straddle", "chain"])
def test_sparse_levels_and_deep_trees(pkg, oracle, cases, name):
    """A flat frame with one 48 x 48 textured block: few candidates per level, lists of one to four nodes.
    corner: the block in one root quadrant (every tree ends in its first round with one node; levels with no
    candidate, with exactly one and with 1 < n < N).  straddle: the block over the level-0 root's midpoint (four
    children, then no growth).  chain: the corner block plus CHAIN_PATCHES, a tree that splits one node off per
    round (lists of 2, 3, 4 nodes) and then divides the block: 10 rounds on level 0 against the 4 of a rich frame."""
    t = oracle.tables(oracle.orb_params(NFEAT))
    cands, want = cases[name][3], cases[name][4]
    ns = [len(c) for c in cands]
    N = [int(v) for v in t["nfeat"]]
    lens0 = _model_rounds(cands[0], int(t["w"][0]), int(t["h"][0]), N[0])
    assert lens0[-1] == len(want[0]), (lens0, len(want[0]))   # the model's rounds end on the oracle's list
    assert any(2 <= n < N[l] for l, n in enumerate(ns)), ns
    if name == "corner":
        assert 0 in ns and 1 in ns, ns        # [34, 25, 10, 6, 2, 1, 1, 0]
        assert lens0 == [1], lens0
    elif name == "straddle":
        assert lens0 == [4, 4], lens0
    else:
        assert len(lens0) > 4 and lens0[:3] == [2, 3, 4], lens0
    _check_single(pkg, cases[name], name)


def test_long_cell_lists(pkg, cases):
    """CORBS seed 7 frame 1: a level-0 cell with more than 64 candidates (71), so the gather's trips run past the
    four it preloads; level 0's 11.2k candidates keep their state in LDS and their keys in the HBM scratch."""
    c0 = cases["corbs1"][3][0]
    # level 0: 20 x 14 cells of 31 x 32 from bordered (3, 3) (FAST's 3-pixel margin inside each cell's window)
    cell = ((c0[:, 1] - 3) // 32) * 20 + np.minimum((c0[:, 0] - 3) // 31, 19)
    assert np.bincount(cell).max() > 64, np.bincount(cell).max()
    assert len(c0) > 11000, len(c0)
    _check_single(pkg, cases["corbs1"], "corbs1")


def test_one_key_and_no_key_roots(pkg, cases):
    """A flat frame (no candidate on any level: L = 0, no round) and a flat frame with one isolated corner (levels
    with exactly one candidate: L = 1, a first round that divides nothing)."""
    assert [len(c) for c in cases["flat"][3]] == [0] * 8
    ns = [len(c) for c in cases["dot"][3]]
    assert 1 in ns and 0 in ns and max(ns) == 1, ns
    got = _check_single(pkg, cases["flat"], "flat")
    assert len(got["kps"]) == 0
    got = _check_single(pkg, cases["dot"], "dot")
    assert len(got["kps"]) == sum(ns)   # every level's one candidate is its tree's one node


def test_mixed_batch(pkg, cases):
    """One extract_batch of 8 frames (the XCD-mapped grid) mixing rich fr1 frames, the sparse frames, a flat frame
    and the one-corner frame: every frame equals its single-frame result and the oracle, every level's selection
    and count included."""
    import torch
    names = ["fr1_0", "corner", "fr1_1", "flat", "straddle", "chain", "dot", "fr1_2"]
    cam = cases["fr1_0"][2]
    fb = np.ascontiguousarray(np.stack([cases[n][0] for n in names]))
    fd = np.ascontiguousarray(np.stack([cases[n][1] for n in names]))
    single = _ctx(pkg, cam)
    singles = [single.frame(fb[f], fd[f]) for f in range(8)]
    single.close()
    ctx = _ctx(pkg, cam, max_batch=8)
    d_bgr = torch.from_numpy(fb).cuda()
    d_dep = torch.from_numpy(fd.view(np.int16)).cuda()
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 8)
    for f, n in enumerate(names):
        _assert_levels_equal(ctx, f, cases[n][4], f"batch {n}")
        got = ctx.batch_frame(f)
        _assert_frame_equal(got, cases[n][5], f"batch {n} vs oracle")
        _assert_frame_equal(got, singles[f], f"batch {n} vs single")
    ctx.close()
