"""Named inputs of the bag-of-words tests, and a seeded test-only vocabulary builder (hierarchical k-medians cut
short: the centres of a cluster are the first k distinct descriptors of a seeded permutation of it, assignment is by
Hamming distance with the first centre winning a tie, the recursion stops at depth L or at a cluster of one; weights
are log(N / n_i) over a seeded image set, computed here on the host)."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_pkg  # noqa: E402

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def _voc_mod():
    load_pkg()
    import importlib
    return importlib.import_module("rgbd_slam_amd.vocabulary")


def _dist(D, c):
    return _POP[np.bitwise_xor(D, c[None, :])].sum(1)


def random_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def noisy(rng, base, flips):
    """base with `flips` random bits toggled per row."""
    out = base.copy()
    for r in range(len(out)):
        for b in rng.integers(0, 256, flips):
            out[r, b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def build_vocabulary(seed, k, L, n_train, n_images=12, per_image=60):
    """Node ids as DBoW3's HKmeansStep hands them out: the children of a node are created together, then each is
    descended into, so ids are not breadth first below level 2."""
    V = _voc_mod()
    rng = np.random.default_rng(seed)
    base = random_desc(rng, max(4, n_train // 6))
    train = noisy(rng, base[rng.integers(0, len(base), n_train)], 24)
    parent, desc, leaf = [0], [np.zeros(32, np.uint8)], [0]

    def step(node, rows, level):
        D = train[rows]
        centres = []
        for r in rng.permutation(len(rows)):
            if not any(np.array_equal(D[r], c) for c in centres):
                centres.append(D[r])
                if len(centres) == k:
                    break
        dist = np.stack([_dist(D, c) for c in centres], 1)
        assign = dist.argmin(1)            # the first minimum
        kids = []
        for c in range(len(centres)):
            parent.append(node)
            desc.append(centres[c])
            leaf.append(0)
            kids.append(len(parent) - 1)
        for c, kid in enumerate(kids):
            sub = rows[assign == c]
            if level + 1 == L or len(sub) <= 1:
                leaf[kid] = 1
            else:
                step(kid, sub, level + 1)

    step(0, np.arange(n_train), 0)
    n = len(parent)
    word = np.full(n, -1, np.int32)
    word[np.flatnonzero(leaf)] = np.arange(int(np.sum(leaf)))
    voc = V.Vocabulary(k, L, np.array(parent), np.stack(desc), np.zeros(n), np.array(leaf, np.uint8), word)
    # IDF over a seeded image set
    import bow_model
    seen = np.zeros(voc.n_words, np.int64)
    for _ in range(n_images):
        img = noisy(rng, train[rng.integers(0, n_train, per_image)], 6)
        seen[np.unique(bow_model.words(voc, img, 0)["word"])] += 1
    for i in np.flatnonzero(leaf):
        ni = seen[word[i]]
        voc.weight[i] = math.log(n_images / ni) if ni > 0 else 0.0
    voc.train = train
    return voc


@functools.lru_cache(maxsize=None)
def tree(name):
    V = _voc_mod()
    if name == "k3_L2":
        return build_vocabulary(11, 3, 2, 40)
    if name == "k10_L3":
        return build_vocabulary(12, 10, 3, 3000, n_images=20, per_image=150)
    if name == "k32_L1":
        return build_vocabulary(13, 32, 1, 200)
    if name == "unbalanced":
        # k = 3, L = 3: node 1 a leaf at level 1; node 2 an inner node with two children (fewer than k); node 3 an
        # inner node whose children 6, 7 carry the same descriptor (the first must win)
        rng = np.random.default_rng(14)
        d = random_desc(rng, 12)
        d[7] = d[6]
        d[3] = d[6]    # and their parent's, so that a copy of it descends to them
        parent = [0, 0, 0, 0, 2, 2, 3, 3, 3, 4, 4, 4]
        leaf = [0, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1]
        word = np.full(12, -1, np.int32)
        word[np.flatnonzero(leaf)] = np.arange(int(np.sum(leaf)))[::-1]   # word ids not in node order
        weight = np.where(np.array(leaf) == 1, np.linspace(0.3, 1.7, 12), 0.0)
        voc = V.Vocabulary(3, 3, np.array(parent), d, weight, np.array(leaf, np.uint8), word)
        voc.train = d[1:]
        return voc
    if name == "zero_word":
        # k3_L2 with the weight of word 0 set to zero
        b = tree("k3_L2")
        w = b.weight.copy()
        w[np.flatnonzero(b.word_id == 0)] = 0.0
        w[(b.is_leaf == 1) & (b.word_id != 0) & (w == 0.0)] = 0.5
        voc = V.Vocabulary(b.k, b.L, b.parent, b.descriptor, w, b.is_leaf, b.word_id)
        voc.train = b.train
        return voc
    raise KeyError(name)


TREES = ("k3_L2", "k10_L3", "k32_L1", "unbalanced", "zero_word")
FRAME_SIZES = (0, 1, 2, 63, 64, 65, 2000)


@functools.lru_cache(maxsize=None)
def frame(name):
    """(tree name, descriptors, levelsup) of a named frame."""
    if name.startswith("size_"):
        n = int(name[5:])
        voc = tree("k10_L3")
        rng = np.random.default_rng(100 + n)
        return "k10_L3", noisy(rng, voc.train[rng.integers(0, len(voc.train), n)], 10) if n else np.zeros((0, 32), np.uint8), 1
    if name.startswith("levelsup_"):
        rng = np.random.default_rng(21)
        voc = tree("k10_L3")
        return "k10_L3", noisy(rng, voc.train[rng.integers(0, len(voc.train), 70)], 10), int(name[9:])
    if name in ("k3_L2", "k32_L1", "unbalanced"):
        rng = np.random.default_rng(22)
        voc = tree(name)
        d = noisy(rng, voc.train[rng.integers(0, len(voc.train), 90)], 12)
        if name == "unbalanced":   # exact copies of the twin descriptor and of the level-1 leaf among them
            d[:8] = voc.descriptor[6]
            d[8:12] = voc.descriptor[1]
        return name, d, 1
    if name == "one_word_130":     # one word hit by 130 features: the in-order sum crosses two wave boundaries
        voc = tree("k10_L3")
        return "k10_L3", np.repeat(voc.train[5:6], 130, 0), 1
    if name == "zero_alone":       # every descriptor on the zero-weight word: empty vectors
        voc = tree("zero_word")
        leaf = int(np.flatnonzero(voc.word_id == 0)[0])
        return "zero_word", np.repeat(voc.descriptor[leaf][None], 7, 0), 1
    if name == "zero_mixed":
        voc = tree("zero_word")
        rng = np.random.default_rng(23)
        leaf = int(np.flatnonzero(voc.word_id == 0)[0])
        d = noisy(rng, voc.train[rng.integers(0, len(voc.train), 40)], 8)
        d[::3] = voc.descriptor[leaf]
        return "zero_word", d, 1
    raise KeyError(name)


FRAMES = tuple(f"size_{n}" for n in FRAME_SIZES) + ("levelsup_0", "levelsup_2", "levelsup_3", "levelsup_4", "k3_L2", "k32_L1",
                                                    "unbalanced", "one_word_130", "zero_alone", "zero_mixed")


def _vec(ids, vals):
    return np.array(ids, np.uint32), np.array(vals, np.float64)


@functools.lru_cache(maxsize=None)
def score_pairs():
    """name -> (a, b) BoW vectors."""
    rng = np.random.default_rng(31)

    def rnd(ids):
        v = rng.random(len(ids)) + 0.01
        return _vec(ids, v / v.sum())
    a = rnd([1, 4, 9, 200, 3000])
    big_a = rnd(sorted(rng.choice(5000, 700, replace=False)))
    big_b = rnd(sorted(rng.choice(5000, 900, replace=False)))
    return {
        "disjoint": (a, rnd([0, 2, 5, 201])),
        "identical": (a, a),
        "one_common": (a, rnd([0, 9, 10])),
        "empty_a": (_vec([], []), a),
        "empty_b": (a, _vec([], [])),
        "many_common": (big_a, big_b),       # more than 64 common words: the sum crosses chunks of the entry
        # values far apart in magnitude: (|vi - wi| - |vi|) - |wi| rounds differently from (|wi - vi| - |wi|) - |vi|
        "order_matters": (_vec([3, 7, 8], [8.438395169341328e-05, 0.0009146632393196584, 0.0009458634295956662]),
                          _vec([3, 7, 8], [0.0009513545278912554, 0.00018908225305181082, 5.7680143001136665e-05])),
    }


@functools.lru_cache(maxsize=None)
def database(name):
    """dict(entries [(ids, vals)], frame_ids, query (ids, vals), query_id, query_entry or None, connected [entry
    indices]) of a named database case.  Vectors are made of a few shared 'places' so that scores tie exactly."""
    rng = np.random.default_rng(41)

    def place(lo):
        ids = np.arange(lo, lo + 40, 3)
        v = rng.random(len(ids)) + 0.05
        return _vec(ids, v / v.sum())
    places = [place(100 * i) for i in range(8)]

    def mix(p, extra, mass=None, also=()):
        """Place p's words, the words `also` at a mass of 0.01 each, and one private word: entries of one place share
        its words and differ in the private word's mass alone, so equal masses give exactly equal scores."""
        if mass is None:
            mass = 0.025 if extra == 9 else 0.05 * (1 + extra % 7)
        ids = np.concatenate([places[p][0], np.array(also, np.uint32), [5000 + extra]])
        v = np.concatenate([places[p][1], np.full(len(also), 0.01), [mass]])
        o = np.argsort(ids, kind="stable")
        ids, v = ids[o].astype(np.uint32), v[o]
        return ids, v / v.sum()
    plain = mix(0, 999, 0.02)
    query = mix(0, 999, 0.02, also=(100, 103))   # two words of place 1 as well: its entries are discovered later
    if name == "empty":
        return dict(entries=[], frame_ids=[], query=query, query_id=500, query_entry=None, connected=[])
    if name == "one":             # one entry, the query not among them and connected to nothing
        return dict(entries=[mix(0, 1)], frame_ids=[0], query=query, query_id=500, query_entry=None, connected=[])
    if name == "single":
        return dict(entries=[mix(0, 1), query], frame_ids=[0, 500], query=query, query_id=500, query_entry=1, connected=[0])
    # 70 entries, the query last: place i % 7, so ten entries of each of places 0..5; among place 0's (0, 7, .., 63)
    # entry 63 scores highest and (0, 49), (7, 56) tie exactly
    entries = [mix(i % 7, i // 7) for i in range(69)]
    frame_ids = [12 * i for i in range(70)]
    base = dict(entries=entries + [query], frame_ids=frame_ids, query=query, query_id=12 * 69, query_entry=69)
    if name == "tied_sort":        # twenty candidates (places 0 and 1), tied scores among them: the sort decides
        return dict(base, connected=[68])                       # place 5 shares no word: minScore = -0.0
    if name == "exactly_five":     # the plain query; five of place 0's ten entries are connected: five candidates
        return dict(base, entries=entries + [plain], query=plain, connected=[0, 7, 14, 21, 28, 68])
    if name == "interval":         # the query's frame id is 10 from the best entry's: the interval removes it
        return dict(base, frame_ids=frame_ids[:69] + [frame_ids[63] + 10], query_id=frame_ids[63] + 10, connected=[68])
    if name == "connected":        # the best entry is connected: skipped
        return dict(base, connected=[68, 63])
    if name == "no_connection":
        return dict(base, connected=[])
    raise KeyError(name)


DATABASES = ("empty", "one", "single", "tied_sort", "exactly_five", "interval", "connected", "no_connection")
