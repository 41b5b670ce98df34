"""GPU: loop detection in the pose graph (posegraph.PoseGraph.detect_loop) against a Python restatement of
PoseGraph::detectLoop / LoopDetector::obtainCandidates that drives tests/bow_model.py and the oracle's Matcher and
RansacSE3.  Eighteen hand-placed keyframes, 1 m apart (no local edges), frame ids 12 apart, whose features cycle over
the four frames of the synthetic sequence: the fifteenth keyframe is the first allowed to look for a loop, and the
keyframes four, eight and twelve places before it hold the very features it holds."""
import numpy as np
import pytest

import bow_cases as BC
import bow_model as M
from conftest import synth_seq

pytestmark = pytest.mark.gpu

N_KF, STEP, MEAN_INLIERS = 18, 12, 150


def pose(i):
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = -1.0 * i          # the camera centre at x = i metres
    return T


def expected(oracle, feats, voc):
    """The restatement over keyframes 0 .. N_KF - 1: (index of the keyframe that detects, candidates, attempts, edge)."""
    bows = [M.transform(voc, f["desc"], 4) for f in feats]
    vec = lambda i: (bows[i % 4]["ids"], bows[i % 4]["vals"])
    rng, sticky = oracle.rng(0), oracle.Sticky()
    th = int(float(MEAN_INLIERS) * 0.20)
    prm = oracle.ransac_params(200, th, 3.0, 4)
    counter, out = 0, []
    edges = set()
    for i in range(N_KF):
        counter += 1
        if i:
            edges.add((i, i - 1))
        if counter < 15:
            continue
        conn = sorted({b for a, b in edges if a == i} | {a for a, b in edges if b == i})
        skip = np.zeros(i + 1, np.uint8)
        skip[conn + [i]] = 1
        kept, ms, sc = M.obtain_candidates(vec(i), STEP * i, [vec(j) for j in range(i + 1)], [STEP * j for j in range(i + 1)],
                                           skip, [vec(j) for j in conn])
        attempts, edge = [], None
        for k in kept:
            fk, fc = feats[k % 4], feats[i % 4]
            m = oracle.match(fk["desc"], fc["desc"], np.zeros(len(fk["desc"]), np.uint8), fk["xyz"][:, 2], fc["xyz"][:, 2], 0.9)
            if len(m) < th:
                attempts.append((k, m, None))
                continue
            ok, T, inl, rmse = oracle.ransac_se3(fk["xyz"], fc["xyz"], m, prm, rng, sticky)
            attempts.append((k, m, dict(ok=ok, T21=np.asarray(T, np.float32), inliers=inl, rmse=rmse,
                                        rng=list(rng.state) + [rng.f, rng.r], sticky=(sticky.cov, sticky.set))))
            if ok:
                edge = (i, k, np.asarray(T, np.float32))
                edges.add((i, k))
                counter = 0
                break
        out.append((i, kept, attempts, edge))
    return out


@pytest.fixture(scope="module")
def world(pkg):
    bgr, depth, gt, cam = synth_seq(4, seed=3, preset="fr1")
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"],
                   cam["factor"])
    ctx = pkg.Context(640, 480, max_batch=1, orb=pkg.orb_params(1000), cam=c)
    feats = [ctx.frame(bgr[i], depth[i]) for i in range(4)]
    yield ctx, feats
    ctx.close()


def test_loop_detected_as_restated(pkg, oracle, world):
    from rgbd_slam_amd.posegraph import PoseGraph
    ctx, feats = world
    voc = BC.tree("k10_L3")
    want = expected(oracle, feats, voc)
    g = PoseGraph(pkg, ctx, vocabulary=voc, mean_inliers=MEAN_INLIERS)
    closed = []
    for i in range(N_KF):
        f = feats[i % 4]
        before = g.kfs_from_last_loop
        closed.append(g.insert_keyframe(STEP * i, pose(i), xyz=f["xyz"], desc=f["desc"]))
        if i < 14:
            assert not closed[-1] and g.kfs_from_last_loop == before + 1 and not g.loop_queries   # the counter is below 15
    assert not g.attempts                                              # centres 1 m apart: no local edge was tried
    # the restatement: one detection, at the fifteenth keyframe, of a keyframe with the same features
    assert [w[0] for w in want] == [14] and want[0][3] is not None
    i, kept, attempts, edge = want[0]
    assert edge[1] % 4 == i % 4 and edge[1] < i
    assert closed == [k == 14 for k in range(N_KF)]
    assert g.loop_queries == [(STEP * 14, [STEP * k for k in kept])]
    assert g.loops == [(STEP * 14, STEP * edge[1])]
    assert len(g.loop_attempts) == len(attempts)
    for (kid, cur, m, th, res), (k, mw, rw) in zip(g.loop_attempts, attempts):
        assert (kid, cur, th) == (STEP * k, STEP * 14, 30) and np.array_equal(m, mw)
        assert (res is None) == (rw is None)
        if res is not None:
            assert res["ok"] == rw["ok"] and np.array_equal(res["T21"].view(np.uint32), rw["T21"].view(np.uint32))
            assert np.array_equal(res["inliers"], rw["inliers"]) and np.float32(res["rmse"]) == np.float32(rw["rmse"])
            assert res["rng"] == rw["rng"] and res["sticky"] == rw["sticky"]
    # the edge, the connections and the counter
    loop_edges = [e for e in g.edges if e[2] is not None]
    assert len(loop_edges) == 1 and loop_edges[0][:2] == (STEP * 14, STEP * edge[1])
    assert np.array_equal(loop_edges[0][2], edge[2].astype(np.float64))
    assert g.exist_edge(STEP * 14, STEP * edge[1])
    assert STEP * edge[1] in g.connections[STEP * 14] and STEP * 14 in g.connections[STEP * edge[1]]
    assert g.kfs_from_last_loop == N_KF - 15                           # reset at the loop, three insertions since
    # optimize(20) ran at the loop: the measured identity pulled the two keyframes, 12 m apart as placed, together
    gap = np.linalg.norm(g.vertex_twc(STEP * 14)[:3, 3] - g.vertex_twc(STEP * edge[1])[:3, 3])
    assert gap < 11.0, gap
    assert np.allclose(g.kf[STEP * 14]["Tcw"], g.pose(STEP * 14), atol=1e-5)   # Frame::correctPose of optimize
    g.close()


def test_without_vocabulary_the_graph_is_todays(pkg, world):
    from rgbd_slam_amd.posegraph import PoseGraph
    ctx, feats = world
    g = PoseGraph(pkg, ctx)
    for i in range(N_KF):
        f = feats[i % 4]
        assert g.insert_keyframe(STEP * i, pose(i), xyz=f["xyz"], desc=f["desc"]) is False
    assert [(a, b) for a, b, Z in g.edges] == [(STEP * i, STEP * (i - 1)) for i in range(1, N_KF)]
    assert all(Z is None for _, _, Z in g.edges) and not g.loops and not g.loop_queries and not g.attempts
    assert g.detect_loop() is False
    g.close()
