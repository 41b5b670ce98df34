"""Python model of k_distribute's pyramid path on one-root levels (test infrastructure).

The quadtree's geometry does not depend on the keys: quad / child_box (quadtree_model) split x and y separately
and a midpoint depends on its own interval alone, so a node at depth d is a pair (ix, iy) of d-bit paths in two
1-D interval trees over [0, rootX1] and [0, rootY1].  One histogram of the keys over the depth-D bins, reduced
upward, gives every node's size (count pyramid) and its best key (best pyramid); the rounds of quadtree_model then
run on the nodes alone.  A round that would divide a node at depth D abandons the attempt (path 2), a tree of
n <= N keys is not attempted (path 3), and a level with several roots has no pyramid path (path 0): those are
quadtree_model.distribute.
"""
import numpy as np

import quadtree_model as qm

D = 5
PATH_KEYS, PATH_PYRAMID, PATH_ABANDONED, PATH_SKIPPED = 0, 1, 2, 3


def deep_frame(tex, gray=90):
    """A 640 x 480 frame whose trees have more keys than their budget and still go deeper than D: a 136 x 100
    block of the textured frame `tex` near the top-left corner and two 12 x 12 patches in the opposite quadrant of
    the block's box of rounds 1 and 2 (as test_gpu_quadtree_state's chain), so the block divides from round 3 on
    inside a box of 152 x 112: 264 keys for level 0's 217 nodes, which takes nodes below depth 5."""
    fr = np.full((480, 640, 3), gray, np.uint8)
    fr[20:120, 20:156] = tex[200:300, 300:436]
    for x, y in ((416, 316), (216, 166)):
        fr[y:y + 12, x:x + 12] = tex[260:272, 360:372]
    return fr


def path_table(hi, depth=D):
    """code[v], v = 0 .. hi: the depth-bit path (first split in the top bit) of v in the interval tree over [0, hi]."""
    code = np.zeros(hi + 1, np.int32)
    for v in range(hi + 1):
        a, e, c = 0, hi, 0
        for _ in range(depth):
            m = a + (e - a + 1) // 2
            if v >= m:
                c, a = 2 * c + 1, m
            else:
                c, e = 2 * c, m
        code[v] = c
    return code


def pyramids(cands, rootX1, rootY1, depth=D):
    """cnt[d][iy, ix] and best[d][iy, ix] = (score, -k) of the node's best key (None: empty), d = 0 .. depth."""
    xc, yc = path_table(rootX1, depth), path_table(rootY1, depth)
    side = 1 << depth
    cnt = [None] * (depth + 1)
    best = [None] * (depth + 1)
    cnt[depth] = np.zeros((side, side), np.int64)
    best[depth] = np.empty((side, side), object)
    for k, (x, y, s) in enumerate(cands):
        iy, ix = yc[min(int(y), rootY1)], xc[min(int(x), rootX1)]
        cnt[depth][iy, ix] += 1
        key = (int(s), -k)
        if best[depth][iy, ix] is None or key > best[depth][iy, ix]:
            best[depth][iy, ix] = key
    for d in range(depth - 1, -1, -1):
        c = cnt[d + 1]
        cnt[d] = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
        best[d] = np.empty((1 << d, 1 << d), object)
        for iy in range(1 << d):
            for ix in range(1 << d):
                ks = [best[d + 1][2 * iy + a, 2 * ix + b] for a in (0, 1) for b in (0, 1)]
                ks = [k for k in ks if k is not None]
                best[d][iy, ix] = max(ks) if ks else None
    return cnt, best


def _rounds(cnt, best, N, depth):
    """quadtree_model's rounds on nodes (d, ix, iy) alone; None when a node at `depth` would be divided."""
    nodes = [dict(pos=(0, 0, 0), size=int(cnt[0][0, 0]), cid=0)]
    next_cid, phase = 1, 1
    while nodes:
        L = prev = len(nodes)

        def childcnt(nd):
            d, ix, iy = nd["pos"]
            return [int(cnt[d + 1][2 * iy + (q >> 1), 2 * ix + (q & 1)]) for q in range(4)]

        S = [i for i in range(L) if nodes[i]["size"] > 1]
        if phase == 2:
            S.sort(key=lambda i: (nodes[i]["size"], nodes[i]["cid"]), reverse=True)
        napply, run = len(S), L
        cc = {}
        for j, i in enumerate(S):
            if nodes[i]["pos"][0] >= depth:
                return None           # every node up to the first that reaches N is divided: this one too
            cc[i] = childcnt(nodes[i])
            run += np.count_nonzero(cc[i]) - 1
            if phase == 2 and run >= N:
                napply = j + 1
                break
        new_children = []
        for i in S[:napply]:
            d, ix, iy = nodes[i]["pos"]
            for q in range(4):
                if cc[i][q] > 0:
                    new_children.append(dict(pos=(d + 1, 2 * ix + (q & 1), 2 * iy + (q >> 1)), size=cc[i][q],
                                             cid=next_cid + len(new_children)))
        T = len(new_children)
        applied = set(S[:napply])
        nodes = new_children[::-1] + [nd for i, nd in enumerate(nodes) if i not in applied]
        n_expand = sum(1 for nd in nodes[:T] if nd["size"] > 1)
        next_cid += T
        if len(nodes) >= N or len(nodes) == prev:
            break
        if phase == 1 and len(nodes) + 3 * n_expand > N:
            phase = 2
    return [best[d][iy, ix] for d, ix, iy in (nd["pos"] for nd in nodes)]


def distribute(cands, minX, maxX, minY, maxY, N, depth=D):
    """(selection, path): the selection in list order as quadtree_model.distribute, and the path taken."""
    n = len(cands)
    nIni = int(np.round(np.float32(maxX - minX) / np.float32(maxY - minY)))
    if nIni != 1:
        return qm.distribute(cands, minX, maxX, minY, maxY, N), PATH_KEYS
    if n <= N:
        return qm.distribute(cands, minX, maxX, minY, maxY, N), PATH_SKIPPED
    rootX1 = int(np.float32(maxX - minX) / np.float32(nIni))
    cnt, best = pyramids(cands, rootX1, maxY - minY, depth)
    sel = _rounds(cnt, best, N, depth)
    if sel is None:
        return qm.distribute(cands, minX, maxX, minY, maxY, N), PATH_ABANDONED
    return np.array([cands[-k[1]] for k in sel], np.int32).reshape(-1, 3), PATH_PYRAMID
