"""CPU check of the pyramid formulation of DistributeOctTree (quadtree_hist_model, what k_distribute runs on
one-root levels) against the oracle's literal restatement, and of its path tables against a literal descent with
quadtree_model's quad / child_box."""
import numpy as np
import pytest

import quadtree_hist_model as hm
import quadtree_model as qm
import test_gpu_quadtree_state as qs
from conftest import synth_seq

RICH = ("fr1_0", "fr1_1", "fr1_2", "corbs1", "lowtex0")


@pytest.fixture(scope="module")
def frames():
    bgr, _, _, _ = synth_seq(4, seed=3, preset="fr1")
    cb, _, _, _ = synth_seq(2, seed=7, preset="corbs")
    lt, _, _, _ = synth_seq(1, seed=1251, preset="lowtex")
    flat = np.full((480, 640, 3), qs.FLAT, np.uint8)
    dot = flat.copy()
    dot[200, 300] = 200
    return {"fr1_0": bgr[0], "fr1_1": bgr[1], "fr1_2": bgr[2], "corbs1": cb[1], "lowtex0": lt[0],
            "corner": qs._block_frame(bgr[0], qs.CORNER_AT), "straddle": qs._block_frame(bgr[0], qs.STRADDLE_AT),
            "chain": qs._block_frame(bgr[0], qs.CORNER_AT, qs.CHAIN_PATCHES), "flat": flat, "dot": dot,
            "deep": hm.deep_frame(bgr[0], qs.FLAT)}


def _literal_code(v, hi, depth, axis):
    """The path of coordinate v by descending boxes with quad / child_box (the other axis held at 0)."""
    box, code = (0, 0, hi, hi), 0
    for _ in range(depth):
        q = qm.quad(v, 0, box) if axis == 0 else qm.quad(0, v, box)
        code = 2 * code + ((q & 1) if axis == 0 else (q >> 1))
        box = qm.child_box(box, q)
    return code


def test_path_tables_equal_literal_descent(oracle):
    t = oracle.tables(oracle.orb_params(1000))
    his = set()
    for l in range(8):
        his.update((int(t["w"][l]) - 32, int(t["h"][l]) - 32))
    for hi in sorted(his):
        tab = hm.path_table(hi)
        for axis in (0, 1):
            assert [_literal_code(v, hi, hm.D, axis) for v in range(hi + 1)] == list(tab), (hi, axis)
    # intervals that degenerate to width 1 ([a, a + 1]: the left child is the interval itself) and width 0 before
    # the last bit
    for hi in range(0, 40):
        for depth in (1, 3, 5, 8):
            tab = hm.path_table(hi, depth)
            for axis in (0, 1):
                assert [_literal_code(v, hi, depth, axis) for v in range(hi + 1)] == list(tab), (hi, depth, axis)


def test_bins_equal_two_axis_descent():
    """x and y together: the depth-D bin of a key is the node a literal 2-D descent reaches."""
    rng = np.random.default_rng(5)
    for X1, Y1 in ((608, 448), (101, 70), (37, 5), (1, 0)):
        xc, yc = hm.path_table(X1), hm.path_table(Y1)
        for _ in range(300):
            x, y = int(rng.integers(0, X1 + 1)), int(rng.integers(0, Y1 + 1))
            box, ix, iy = (0, 0, X1, Y1), 0, 0
            for _d in range(hm.D):
                q = qm.quad(x, y, box)
                ix, iy = 2 * ix + (q & 1), 2 * iy + (q >> 1)
                box = qm.child_box(box, q)
            assert (ix, iy) == (xc[x], yc[y]), (X1, Y1, x, y)


@pytest.mark.parametrize("nfeat", [1000, 2000])
def test_model_equals_oracle(oracle, frames, nfeat):
    p = oracle.orb_params(nfeat)
    t = oracle.tables(p)
    paths = {}
    for name, bgr in frames.items():
        ref = oracle.pyramid(oracle.gray(bgr), p)
        paths[name] = []
        for l in range(8):
            cands = oracle.level_candidates(ref[l], p)
            box = (16, int(t["w"][l]) - 16, 16, int(t["h"][l]) - 16)
            N = int(t["nfeat"][l])
            want = oracle.distribute(cands, *box, N)
            got, path = hm.distribute(cands, *box, N)
            paths[name].append(path)
            assert len(got) == len(want), (name, l, path)
            assert np.array_equal(got, want), (name, l, path)
            if path == hm.PATH_ABANDONED:
                # too shallow a pyramid is abandoned, never wrong: depth 3 on the same keys
                got3, path3 = hm.distribute(cands, *box, N, depth=3)
                assert np.array_equal(got3, want), (name, l, path3)
    print(nfeat, paths)
    for name in RICH:
        assert hm.PATH_ABANDONED not in paths[name], (name, paths[name])
    for name in ("fr1_0", "fr1_1", "fr1_2", "corbs1"):
        assert paths[name] == [hm.PATH_PYRAMID] * 8, (name, paths[name])
    assert paths["flat"] == [hm.PATH_SKIPPED] * 8 and paths["dot"] == [hm.PATH_SKIPPED] * 8
    assert paths["chain"][0] in (hm.PATH_ABANDONED, hm.PATH_SKIPPED), paths["chain"]
    if nfeat == 1000:
        assert paths["deep"][0] == hm.PATH_ABANDONED, paths["deep"]   # n > N and a node divided at depth D


def test_shallow_pyramid_is_abandoned(oracle, frames):
    """Depth 3 on a rich frame: levels 0-6 divide a node at depth 3 and abandon; the selection is the oracle's."""
    p = oracle.orb_params(1000)
    t = oracle.tables(p)
    ref = oracle.pyramid(oracle.gray(frames["fr1_0"]), p)
    for l in range(7):
        cands = oracle.level_candidates(ref[l], p)
        box = (16, int(t["w"][l]) - 16, 16, int(t["h"][l]) - 16)
        got, path = hm.distribute(cands, *box, int(t["nfeat"][l]), depth=3)
        assert path == hm.PATH_ABANDONED, l
        assert np.array_equal(got, oracle.distribute(cands, *box, int(t["nfeat"][l]))), l
