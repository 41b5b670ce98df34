"""CPU: the named bag-of-words cases reach the regimes they are named for (asserted from the model), the DBoW3 YAML
round trip keeps every bit, and the host candidate rule of the library equals the model's."""
import numpy as np
import pytest

import bow_cases as BC
import bow_model as M


@pytest.fixture(scope="module")
def V(pkg):
    import importlib
    return importlib.import_module("rgbd_slam_amd.vocabulary")


def levels(voc):
    lv = np.zeros(voc.n_nodes, np.int32)
    for i in range(1, voc.n_nodes):
        assert voc.parent[i] < i
        lv[i] = lv[voc.parent[i]] + 1
    return lv


@pytest.mark.parametrize("name", BC.TREES)
def test_tree_shapes(name):
    voc = BC.tree(name)
    lv, ch = levels(voc), voc.children()
    nch = np.array([len(c) for c in ch])
    assert lv.max() <= voc.L and np.all((nch == 0) == (voc.is_leaf == 1)) and nch.max() <= voc.k
    assert sorted(voc.word_id[voc.is_leaf == 1]) == list(range(voc.n_words))
    assert np.all(np.isfinite(voc.weight)) and np.all(voc.weight >= 0)
    if name == "k3_L2":
        assert (voc.k, voc.L) == (3, 2) and lv.max() == 2
    if name == "k10_L3":
        assert (voc.k, voc.L) == (10, 3) and lv.max() == 3 and voc.n_words > 300
        bfs = [0]
        for u in bfs:
            bfs.extend(ch[u])
        assert bfs != list(range(voc.n_nodes))                       # node ids are not breadth first
        assert np.any(voc.weight[voc.is_leaf == 1] > 0) and len(np.unique(voc.weight)) > 3
    if name == "k32_L1":
        assert (voc.k, voc.L) == (32, 1) and nch[0] == 32
    if name == "unbalanced":
        assert np.any((voc.is_leaf == 1) & (lv == 1)) and np.any((voc.is_leaf == 1) & (lv == 3))   # a leaf at level 1
        assert np.any((nch > 0) & (nch < voc.k))                     # an inner node with fewer than k children
        assert np.array_equal(voc.descriptor[6], voc.descriptor[7]) and voc.parent[6] == voc.parent[7]
    if name == "zero_word":
        assert np.sum(voc.weight[voc.is_leaf == 1] == 0) == 1


@pytest.mark.parametrize("name", BC.FRAMES)
def test_frame_regimes(name):
    tname, desc, levelsup = BC.frame(name)
    voc = BC.tree(tname)
    w = M.words(voc, desc, levelsup)
    v = M.vectors_from_words(w["word"], w["weight"], w["node"])
    assert np.all(np.diff(v["ids"].astype(np.int64)) > 0)
    if len(v["ids"]):
        assert abs(v["vals"].sum() - 1.0) < 1e-12
    if name.startswith("size_"):
        assert len(desc) == int(name[5:])
        if len(desc) == 2000:
            assert len(v["ids"]) < len(v["fv_idx"])                  # words hit more than once
    if name.startswith("levelsup_"):
        lv = levels(voc)
        if levelsup >= voc.L:
            assert np.all(w["node"] == 0)
        else:
            assert np.all(lv[w["node"]] == voc.L - levelsup) and len(np.unique(w["node"])) > 1
        if levelsup == 0:
            assert np.all(voc.is_leaf[w["node"]] == 1)
    if name == "unbalanced":
        assert np.all(w["path"][:8, :2] == [2, 0])                   # the twin's first child, not the second
        assert np.all(w["path"][8:12, 0] == 0) and np.all(w["path"][8:12, 1] == 255)   # the level-1 leaf
        assert np.all(w["node"][8:12] == 0)                          # the leaf lies above level L - levelsup = 2
        assert np.any(w["path"][:, 2] != 255)
    if name == "one_word_130":
        assert len(desc) == 130 and len(v["ids"]) == 1 and len(v["fv_idx"]) == 130
    if name == "zero_alone":
        assert np.all(w["weight"] == 0) and len(v["ids"]) == 0 and len(v["fv_idx"]) == 0
    if name == "zero_mixed":
        z = int(np.sum(w["weight"] == 0))
        assert 0 < z < len(desc) and len(v["fv_idx"]) == len(desc) - z and 0 not in v["ids"]


def test_in_order_sum_differs_from_a_product():
    """The sequential sum of one word's weights is not n * w: the order of the additions is observable."""
    tname, desc, levelsup = BC.frame("size_2000")
    w = M.words(BC.tree(tname), desc, levelsup)
    cnt = {}
    for k, wt in zip(w["word"], w["weight"]):
        cnt.setdefault(int(k), [0, float(wt)])[0] += 1
    diff = 0
    for n, wt in cnt.values():
        s = 0.0
        for _ in range(n):
            s += wt
        diff += s != n * wt
    assert diff > 0


def test_score_regimes():
    P = BC.score_pairs()
    s = M.score(*P["disjoint"])
    assert s == 0.0 and np.signbit(s)                                # -0.0
    assert np.signbit(M.score(*P["empty_a"])) and np.signbit(M.score(*P["empty_b"]))
    assert abs(M.score(*P["identical"]) - 1.0) < 1e-12
    assert M.shared(P["one_common"][0][0], P["one_common"][1][0]) == (1, 9)
    assert M.shared(P["many_common"][0][0], P["many_common"][1][0])[0] > 64
    a, b = P["order_matters"]
    assert M.score(a, b) != M.score(b, a)                            # the argument order reaches the last bits


def _case(name):
    d = BC.database(name)
    E = len(d["entries"])
    skip = np.zeros(E, np.uint8)
    for e in d["connected"]:
        skip[e] = 1
    if d["query_entry"] is not None:
        skip[d["query_entry"]] = 1
    conn = [d["entries"][e] for e in d["connected"]]
    kept, min_score, scores = M.obtain_candidates(d["query"], d["query_id"], d["entries"], d["frame_ids"], skip, conn)
    return d, skip, kept, min_score, scores


def test_database_regimes():
    assert _case("empty")[2] == [] and _case("one")[2] == [] and _case("no_connection")[2] == []
    assert len(BC.database("one")["entries"]) == 1
    d, skip, kept, ms, sc = _case("single")
    assert kept == []                                                # its only other entry is connected
    d, skip, kept, ms, sc = _case("tied_sort")
    assert len(d["entries"]) == 70 and np.signbit(ms) and ms == 0.0
    cand = [e for e in range(70) if not skip[e] and sc[e] > ms]
    assert len(cand) == 20 and len(kept) == 5 and kept[0] == 63
    assert sc[0] == sc[49] and sc[7] == sc[56] and {0, 49} <= set(kept)   # ties among the five
    assert kept != sorted(kept, key=lambda e: (-sc[e], e))           # the sort is not the stable one
    first_word = {e: M.shared(d["query"][0], d["entries"][e][0])[1] for e in cand}
    assert first_word[1] == 100 and first_word[7] == 0               # entry 7 is discovered before entry 1
    d, skip, kept, ms, sc = _case("exactly_five")
    assert kept == [35, 42, 49, 56, 63] and sc[63] > sc[35]          # discovery order, not score order
    d, skip, kept, ms, sc = _case("interval")
    assert int(np.argmax(np.where(skip, -1.0, sc))) == 63 and 63 not in kept and len(kept) == 5
    d, skip, kept, ms, sc = _case("connected")
    assert 63 not in kept and len(kept) == 5 and np.signbit(ms)


@pytest.mark.parametrize("name", BC.DATABASES)
def test_host_candidate_rule_equals_the_model(pkg, name):
    d, skip, kept, ms, sc = _case(name)
    if not d["connected"]:
        return                                                       # obtainCandidates returns before the rule
    sh = [M.shared(d["query"][0], v[0]) for v in d["entries"]]
    got = pkg.loop_candidates(sc, [s[0] for s in sh], [s[1] for s in sh], d["frame_ids"], skip, d["query_id"], ms, 10)
    assert list(got) == kept


def test_std_sort_model_small_is_stable_insertion():
    assert M.std_sort_desc([1.0, 3.0, 3.0, 2.0]) == [1, 2, 3, 0]


@pytest.mark.parametrize("gz", [False, True])
@pytest.mark.parametrize("name", ["k3_L2", "unbalanced", "zero_word"])
def test_yaml_round_trip(V, tmp_path, name, gz):
    voc = BC.tree(name)
    path = tmp_path / ("voc.yml.gz" if gz else "voc.yml")
    V.save_dbow3_yaml(voc, path)
    raw = open(path, "rb").read(2)
    assert (raw == b"\x1f\x8b") == gz
    back = V.load_dbow3_yaml(path)
    assert back.equal(voc) and back.n_nodes == voc.n_nodes
