"""Numpy / plain-Python restatement of DESIGN.md "Bag-of-words and loop detection definition": the descent of a
descriptor through the vocabulary tree, the TF-IDF / L1 BoW vector and the feature vector of a frame, the L1 score,
and LoopDetector::obtainCandidates with libstdc++'s std::sort.  Every double operation is a Python float (IEEE
binary64) operation in the order of the definition."""
import numpy as np

import lane_sort_model

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


def descend(voc, children, d, levelsup):
    """Vocabulary::transform(feature, id, w, &nid, levelsup): (word, weight, nid, path)."""
    nid_level = voc.L - levelsup
    cur, nid, level, path = 0, 0, 0, []
    while True:
        level += 1
        kids = children[cur]
        best, best_d = 0, hamming(d, voc.descriptor[kids[0]])
        for c in range(1, len(kids)):
            dist = hamming(d, voc.descriptor[kids[c]])
            if dist < best_d:          # strict: the first child wins a tie
                best, best_d = c, dist
        cur = kids[best]
        path.append(best)
        if level == nid_level:
            nid = cur
        if voc.is_leaf[cur]:
            break
    return int(voc.word_id[cur]), float(voc.weight[cur]), nid, path


def words(voc, desc, levelsup=4):
    """Per descriptor: word i32, weight f64, node i32, path (n, 10) u8 (255 below the leaf)."""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    ch = voc.children()
    n = len(desc)
    word, node = np.zeros(n, np.int32), np.zeros(n, np.int32)
    weight, path = np.zeros(n, np.float64), np.full((n, 10), 255, np.uint8)
    for i in range(n):
        w, wt, nid, p = descend(voc, ch, desc[i], levelsup)
        word[i], weight[i], node[i] = w, wt, nid
        path[i, :len(p)] = p
    return dict(word=word, weight=weight, node=node, path=path)


def vectors_from_words(word, weight, node):
    """transform(features, BowVector, FeatureVector, levelsup) after the descents: additions in feature order, L1 norm
    in ascending word order, the division when the norm is above zero."""
    bow, fv = {}, {}
    for i in range(len(word)):
        w = float(weight[i])
        if w > 0:
            k = int(word[i])
            bow[k] = bow[k] + w if k in bow else w
            fv.setdefault(int(node[i]), []).append(i)
    ids = sorted(bow)
    norm = 0.0
    for k in ids:
        norm += abs(bow[k])
    vals = [bow[k] / norm if norm > 0.0 else bow[k] for k in ids]
    fvn = [nd for nd in sorted(fv) for _ in fv[nd]]
    fvi = [i for nd in sorted(fv) for i in fv[nd]]
    return dict(ids=np.array(ids, np.uint32), vals=np.array(vals, np.float64), fv_node=np.array(fvn, np.int32),
                fv_idx=np.array(fvi, np.int32))


def transform(voc, desc, levelsup=4):
    w = words(voc, desc, levelsup)
    return vectors_from_words(w["word"], w["weight"], w["node"])


def score(a, b):
    """L1Scoring::score(v = a, w = b) over (ids, vals) vectors."""
    ia, va, ib, vb = a[0], a[1], b[0], b[1]
    i = j = 0
    s = 0.0
    while i < len(ia) and j < len(ib):
        if ia[i] == ib[j]:
            vi, wi = float(va[i]), float(vb[j])
            s += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1
            j += 1
        elif ia[i] < ib[j]:
            i += 1
        else:
            j += 1
    return -s / 2.0


def shared(a_ids, b_ids):
    """(number of shared words, smallest shared word or -1)."""
    c = np.intersect1d(a_ids, b_ids)
    return len(c), (int(c[0]) if len(c) else -1)


def std_sort_desc(scores):
    """The order std::sort(first, last, CompareBoWscore) (score descending, unstable) leaves indices 0..n-1 in:
    libstdc++'s introsort as lane_sort_model restates it, over the dense ranks of the negated scores (comp(a, b) =
    a.score > b.score is rank(a) < rank(b), ties included)."""
    neg = [-float(s) for s in scores]
    rank = {v: r for r, v in enumerate(sorted(set(neg)))}
    return [int(i) for i in lane_sort_model.lane_sort([rank[v] for v in neg])]


def obtain_candidates(query, query_id, entries, frame_ids, skip, connected, interval=10):
    """LoopDetector::obtainCandidates.  query: (ids, vals); entries: the database vectors in add() order; skip[e]: the
    query itself or a connected keyframe; connected: the connected keyframes' vectors (the query's own excluded).
    Returns (entry indices in the returned order, minScore, scores of score(query, entry))."""
    if not connected:
        return [], None, []
    min_score = np.finfo(np.float64).max
    for c in connected:
        s = score(c, query)                      # LoopDetector.cpp:43
        if s < min_score:
            min_score = s
    disc = []
    for e, v in enumerate(entries):
        ns, mw = shared(query[0], v[0])
        if ns > 0 and not skip[e]:
            disc.append((mw, e))
    disc.sort()                                  # inverted-file order: smallest shared word, then insertion
    scores = [score(query, v) for v in entries]  # :70
    kept = [e for _, e in disc if scores[e] > min_score and abs(int(frame_ids[e]) - int(query_id)) > interval]
    if len(kept) > 5:
        order = std_sort_desc([scores[e] for e in kept])
        kept = [kept[i] for i in order][:5]
    return kept, min_score, scores
