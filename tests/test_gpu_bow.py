"""GPU: the bag-of-words place recognition (rgbd_voc_set, rgbd_bow_transform and its batch / frames / debug entries,
rgbd_bow_score, rgbd_loopdb_*) against the numpy restatement of tests/bow_model.py on the inputs of
tests/bow_cases.py.  Every comparison is bit for bit: word, weight, node and path per descriptor, the ids and f64
values of the BoW vector, the feature vector, and the scores."""
import functools
import os
import subprocess

import numpy as np
import pytest

import bow_cases as BC
import bow_model as M
from conftest import ROOT, synth_seq

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(640, 480, max_batch=1, orb=pkg.orb_params(1000), cam=pkg.camera(517.3, 516.5, 318.6, 255.3))
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def model(name):
    tname, desc, levelsup = BC.frame(name)
    w = M.words(BC.tree(tname), desc, levelsup)
    return w, M.vectors_from_words(w["word"], w["weight"], w["node"])


def assert_vectors(got, want, what):
    assert np.array_equal(got["ids"], want["ids"]), what
    assert np.array_equal(bits(got["vals"]), bits(want["vals"])), what
    assert np.array_equal(got["fv_node"], want["fv_node"]) and np.array_equal(got["fv_idx"], want["fv_idx"]), what


_loaded = [None]


def use_tree(ctx, name):
    if _loaded[0] != name:
        ctx.voc_set(BC.tree(name))
        _loaded[0] = name


@pytest.mark.parametrize("name", BC.FRAMES)
def test_frame_equals_model(ctx, name):
    tname, desc, levelsup = BC.frame(name)
    use_tree(ctx, tname)
    w, v = model(name)
    got = ctx.debug_bow_words(desc, levelsup)
    assert np.array_equal(got["path"], w["path"]), name            # first: a mismatch is named at the descent
    assert np.array_equal(got["word"], w["word"]) and np.array_equal(got["node"], w["node"]), name
    assert np.array_equal(bits(got["weight"]), bits(w["weight"])), name
    assert_vectors(ctx.bow_transform(desc, levelsup), v, name)


def test_batch_equals_model_in_one_launch_each(ctx):
    names = ["size_65", "size_0", "size_2000", "size_1", "levelsup_0"]   # levelsup 1 for all: model again for the last
    use_tree(ctx, "k10_L3")
    descs = [BC.frame(n)[1] for n in names]
    ctx.set_timing(True)
    ctx.reset_timing()
    got = ctx.bow_transform_batch(descs, 1)
    t = ctx.timings()
    ctx.set_timing(False)
    assert t["k_bow_words"][1] == 1 and t["k_bow_vector"][1] == 1, t
    for n, d, g in zip(names, descs, got):
        want = model(n)[1] if BC.frame(n)[2] == 1 else M.transform(BC.tree("k10_L3"), d, 1)
        assert_vectors(g, want, n)


def test_frames_equal_model(pkg):
    import torch
    bgr, depth, gt, cam = synth_seq(4, seed=3, preset="fr1")
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"],
                   cam["factor"])
    ctx = pkg.Context(640, 480, max_batch=3, orb=pkg.orb_params(1000), cam=c)
    voc = BC.tree("k10_L3")
    ctx.voc_set(voc)
    d_bgr = torch.from_numpy(np.ascontiguousarray(bgr[:3])).cuda()
    d_dep = torch.from_numpy(np.ascontiguousarray(depth[:3]).view(np.int16)).cuda()
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 3)
    ctx.set_timing(True)
    ctx.reset_timing()
    got = ctx.bow_transform_frames([2, 0], 1)
    t = ctx.timings()
    ctx.set_timing(False)
    assert t["k_bow_words"][1] == 1 and t["k_bow_vector"][1] == 1, t
    for g, b in zip(got, (2, 0)):
        desc = ctx.batch_frame(b)["desc"]
        assert len(desc) > 500
        assert_vectors(g, M.transform(voc, desc, 1), b)
    with pytest.raises(pkg.RgbdError, match=r"status 1"):
        ctx.bow_transform_frames([3], 1)
    ctx.close()


@pytest.mark.parametrize("name", sorted(BC.score_pairs()))
def test_score_equals_model_both_orders(ctx, name):
    a, b = BC.score_pairs()[name]
    for x, y in ((a, b), (b, a)):
        got, want = ctx.bow_score(x, y), M.score(x, y)
        assert bits(got) == bits(want), (name, got, want)          # the sign of -0.0 included


@pytest.mark.parametrize("name", BC.DATABASES)
def test_database_equals_model(pkg, ctx, name):
    d = BC.database(name)
    ctx.loopdb_clear()
    for i, (ids, vals) in enumerate(d["entries"]):
        assert ctx.loopdb_add(ids, vals) == i
    E = len(d["entries"])
    q = d["query"]
    ctx.set_timing(True)
    ctx.reset_timing()
    sc, ns, mw = ctx.loopdb_query(q[0], q[1], True)
    t = ctx.timings()
    ctx.set_timing(False)
    assert len(sc) == E
    assert ("k_bow_score" in t) == (E > 0) and (E == 0 or t["k_bow_score"][1] == 1), t
    want = [M.score(q, v) for v in d["entries"]]
    assert np.array_equal(bits(sc), bits(want)), name
    sh = [M.shared(q[0], v[0]) for v in d["entries"]]
    assert ns.tolist() == [s[0] for s in sh] and mw.tolist() == [s[1] for s in sh], name
    rev, _, _ = ctx.loopdb_query(q[0], q[1], False)                # LoopDetector.cpp:43's order
    assert np.array_equal(bits(rev), bits([M.score(v, q) for v in d["entries"]])), name
    # obtainCandidates from the three arrays
    skip = np.zeros(E, np.uint8)
    skip[d["connected"]] = 1
    if d["query_entry"] is not None:
        skip[d["query_entry"]] = 1
    kept, min_score, _ = M.obtain_candidates(q, d["query_id"], d["entries"], d["frame_ids"], skip,
                                             [d["entries"][e] for e in d["connected"]])
    if d["connected"]:
        ms = min(float(rev[e]) for e in d["connected"])
        assert bits(ms) == bits(min_score) or (ms == 0.0 and min_score == 0.0)
        got = pkg.loop_candidates(sc, ns, mw, d["frame_ids"], skip, d["query_id"], ms, 10)
        assert got.tolist() == kept, name
    ctx.loopdb_clear()


def test_database_grows_between_queries(ctx):
    d = BC.database("tied_sort")
    ctx.loopdb_clear()
    q = d["query"]
    for lo, hi in ((0, 3), (3, 40), (40, 70)):
        for ids, vals in d["entries"][lo:hi]:
            ctx.loopdb_add(ids, vals)
        sc, _, _ = ctx.loopdb_query(q[0], q[1], True)
        assert np.array_equal(bits(sc), bits([M.score(q, v) for v in d["entries"][:hi]])), hi
    ctx.loopdb_clear()


def test_limits(pkg, ctx):
    import importlib
    V = importlib.import_module("rgbd_slam_amd.vocabulary")
    b = BC.tree("k3_L2")

    def voc(**kw):
        f = dict(k=b.k, L=b.L, parent=b.parent.copy(), descriptor=b.descriptor.copy(), weight=b.weight.copy(),
                 is_leaf=b.is_leaf.copy(), word_id=b.word_id.copy(), weighting=V.TF_IDF, scoring=V.L1_NORM)
        f.update(kw)
        return V.Vocabulary(**f)
    leaf = int(np.flatnonzero(b.is_leaf == 1)[0])
    no_children = voc()
    no_children.is_leaf[leaf] = 0                                   # an inner node without children
    deep = voc(L=1)                                                 # nodes below level L
    w_nan, w_neg, w_inf = voc(), voc(), voc()
    w_nan.weight[leaf], w_neg.weight[leaf], w_inf.weight[leaf] = np.nan, -1.0, np.inf
    many = voc(k=2)                                                 # the root has three children
    wide = voc(descriptor=np.zeros((b.n_nodes, 64), np.uint8))
    bad = [voc(k=1), voc(k=33), voc(L=0), voc(L=11), no_children, deep, w_nan, w_neg, w_inf, many, wide,
           voc(weighting=V.TF), voc(weighting=V.BINARY), voc(scoring=V.L2_NORM), voc(scoring=V.DOT_PRODUCT)]
    ctx.set_timing(True)
    ctx.reset_timing()
    for i, v in enumerate(bad):
        with pytest.raises(pkg.RgbdError, match=r"status 4"):
            ctx.voc_set(v)
    # a node count of 2^31: refused from the count alone, before an array is read
    one = np.zeros(1, np.int32)
    st = pkg.lib().rgbd_voc_set(ctx._h, 3, 2, 0, 0, 32, 1 << 31, one.ctypes.data, one.ctypes.data, one.ctypes.data,
                                one.ctypes.data, one.ctypes.data)
    assert st == 4
    use_tree(ctx, "k3_L2")
    _loaded[0] = None
    with pytest.raises(pkg.RgbdError, match=r"status 4"):
        ctx.bow_transform(np.zeros((4097, 32), np.uint8), 1)
    with pytest.raises(pkg.RgbdError, match=r"status 4"):
        ctx.bow_transform_batch([np.zeros((3, 32), np.uint8), np.zeros((4097, 32), np.uint8)], 1)
    with pytest.raises(pkg.RgbdError, match=r"status 4"):
        ctx.debug_bow_words(np.zeros((4097, 32), np.uint8), 1)
    ids = np.arange(4097, dtype=np.uint32)
    with pytest.raises(pkg.RgbdError, match=r"status 4"):
        ctx.bow_score((ids, np.ones(4097)), (ids[:3], np.ones(3)))
    t = ctx.timings()
    ctx.set_timing(False)
    assert not [k for k in t if k.startswith("k_bow")], t          # nothing launched
    ctx.voc_clear()
    with pytest.raises(pkg.RgbdError, match=r"status 1"):
        ctx.bow_transform(np.zeros((3, 32), np.uint8), 1)


# ---------------------------------------------------------------- C++ surface
def test_cpp_loop_example(pkg, tmp_path):
    import importlib
    V = importlib.import_module("rgbd_slam_amd.vocabulary")
    exe = os.path.join(ROOT, "rgbd-slam_amd", "build", "loop_example")
    assert os.path.exists(exe), "build() must compile examples/loop_example.cpp"
    bgr, depth, gt, cam = synth_seq(4, seed=3, preset="fr1")
    raw = tmp_path / "frames.raw"
    with open(raw, "wb") as f:
        for i in range(4):
            f.write(np.ascontiguousarray(bgr[i]).tobytes())
            f.write(np.ascontiguousarray(depth[i]).tobytes())
    voc = BC.tree("k10_L3")
    yml = tmp_path / "voc.yml"
    V.save_dbow3_yaml(voc, yml)
    K = 16
    args = [exe, str(raw)] + ["%r" % float(cam[k]) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "factor")]
    out = subprocess.run(args + [str(yml), "4", str(K)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    # the model on the same frames
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"],
                   cam["factor"])
    ctx = pkg.Context(640, 480, max_batch=1, orb=pkg.orb_params(1000), cam=c)
    bows = [M.transform(voc, ctx.frame(bgr[i], depth[i])["desc"], 4) for i in range(4)]
    ctx.close()
    for i in range(K):
        b = bows[i % 4]
        assert lines[i].split() == ["bow", str(12 * i), str(len(b["ids"])), str(len(b["fv_idx"]))], i
    last = bows[(K - 1) % 4]
    nw = len(last["ids"])
    got = [l.split() for l in lines[K:K + nw]]
    assert [int(g[0]) for g in got] == last["ids"].tolist()
    assert [int(g[1], 16) for g in got] == bits(last["vals"]).tolist()
    vec = lambda i: (bows[i % 4]["ids"], bows[i % 4]["vals"])
    skip = np.zeros(K, np.uint8)
    skip[[K - 2, K - 1]] = 1
    kept, ms, sc = M.obtain_candidates(vec(K - 1), 12 * (K - 1), [vec(j) for j in range(K)], [12 * j for j in range(K)], skip,
                                       [vec(K - 2)])
    # the three keyframes of the same frame score 1 and lead; keyframes of another frame score above the connected
    # one's too, so more than five are kept and the sort cuts them to five
    assert len(kept) == 5 and sorted(kept[:3]) == [3, 7, 11] and lines[K + nw].split() == ["candidates", "5"]
    cand = [l.split() for l in lines[K + nw + 1:]]
    assert [int(g[0]) for g in cand] == [12 * k for k in kept]
    assert [int(g[1], 16) for g in cand] == bits([sc[k] for k in kept]).tolist()
