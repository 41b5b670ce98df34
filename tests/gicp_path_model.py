"""Python model of the path decisions of csrc/gicp.hip (test infrastructure, numpy only).

The kernels replace the oracle's two brute-force searches:

  gicp_knn          covariance k-NN.  Keys (float bits of dist2f << 32) | j; lane l of the wave holds the keys
                    of j % 64 == l; t = the k-th smallest lane minimum; the keys <= t are the candidates.  At most
                    64 of them: compacted and sorted (threshold path); more: k rounds of wave minimum (rounds
                    path).  Instantiated for NC = 4, 8, ..., 32 key slots per lane.
  gicp_align_block  correspondence 1-NN.  Uniform grid of 1.01 max_corr cells over the target, cells valid in
                    (-512, 511); a query whose cell is valid searches the 27 cells around it, ties by (d, j); one
                    target outside the range (grid_ok = 0) or a query outside it: the full scan.

knn_paths / grid_stats / nn_ties say which of these an input reaches, so tests/test_gicp_edge_cases.py can
assert that every case of tests/gicp_edge_cases.py is in the regime it is named after; grid_nn / full_nn restate
the two searches themselves in float32 so the grid's equivalence argument is checked against brute force on the
CPU.  Every float operation below is a single IEEE float32 operation in the device's order."""
import numpy as np

F = np.float32
GRID_HALF = 512
CELL_MARGIN = 1.01


def dist2f(a, b):
    """FLANN L2_Simple<float>: ((0 + dx^2) + dy^2) + dz^2 in float32, broadcasting over leading axes."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    r = F(0) + dx * dx
    r = r + dy * dy
    return r + dz * dz


def knn_keys(P):
    """(M, M) uint64: row i = the keys of every j as point i's search forms them."""
    P = np.ascontiguousarray(P, F).reshape(-1, 3)
    d = np.ascontiguousarray(dist2f(P[:, None, :], P[None, :, :]))
    return (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(P), dtype=np.uint64)[None, :]


def knn_nc(M):
    """Key slots per lane of the instantiation gicp_knn_any picks."""
    need = (M + 63) // 64
    return next(nc for nc in range(4, 33, 4) if nc >= need)


def knn_totals(P, k):
    """Per point: the number of keys at or below the k-th smallest lane minimum."""
    keys = knn_keys(P)
    M = keys.shape[0]
    slots = (M + 63) // 64
    pad = np.full((M, slots * 64), ~np.uint64(0), np.uint64)
    pad[:, :M] = keys
    lane_min = pad.reshape(M, slots, 64).min(axis=1)
    t = np.sort(lane_min, axis=1)[:, k - 1]
    assert (t != ~np.uint64(0)).all()   # k <= min(M, 64) lanes hold a key
    return (keys <= t[:, None]).sum(axis=1)


def knn_paths(P, k):
    """(NC, n_rounds, n_threshold, max_total) of one cloud's covariance k-NN."""
    total = knn_totals(P, k)
    rounds = int((total > 64).sum())
    return knn_nc(len(total)), rounds, len(total) - rounds, int(total.max())


def knn_ref(P, k):
    """(M, k) neighbour ids, ascending (distance, index): what either path must return."""
    return (np.sort(knn_keys(P), axis=1)[:, :k] & np.uint64(0xffffffff)).astype(np.int64)


def grid_hinv(max_corr, margin=CELL_MARGIN):
    thr = np.float64(max_corr) * np.float64(max_corr)
    with np.errstate(divide="ignore"):
        return F(1) / F(np.sqrt(thr) * margin)


def grid_cells(v, hinv):
    """(cells as float32, valid): floor(v * hinv) per coordinate; valid inside (-512, 511)."""
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor(np.asarray(v, F) * hinv)
    return c, (c > -F(GRID_HALF)) & (c < F(GRID_HALF - 1))


def xform_f(T, p):
    """((m0 x + m1 y) + m2 z) + m3 per row, float32."""
    T, p = np.asarray(T, F).reshape(4, 4), np.ascontiguousarray(p, F).reshape(-1, 3)
    return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], 1)


def queries(P, guess):
    """The 1-NN queries of outer iteration 0: transformation_ (identity) * (guess * source)."""
    return xform_f(np.eye(4, dtype=F), xform_f(guess, P))


def grid_stats(P, Q, guess, max_corr):
    """(grid_ok, n_in_grid, n_full_scan) of outer iteration 0."""
    hinv = grid_hinv(max_corr)
    _, tv = grid_cells(np.ascontiguousarray(Q, F).reshape(-1, 3), hinv)
    grid_ok = bool(tv.all())
    _, qv = grid_cells(queries(P, guess), hinv)
    n_in = int(qv.all(axis=1).sum()) if grid_ok else 0
    return grid_ok, n_in, len(qv) - n_in


def full_nn(q, tgt):
    """The oracle's scan: (best, bd) with the first index on ties."""
    d = dist2f(np.asarray(q, F)[None, :], np.ascontiguousarray(tgt, F).reshape(-1, 3))
    j = int(np.argmin(d))   # first occurrence of the minimum
    return j, d[j]


def nn_dists(P, Q, guess):
    """(M, M) float32 distances of iteration 0's queries to every target."""
    return dist2f(queries(P, guess)[:, None, :], np.ascontiguousarray(Q, F).reshape(-1, 3)[None, :, :])


def nn_ties(P, Q, guess):
    """Queries of iteration 0 whose minimum float distance is attained by more than one target."""
    d = nn_dists(P, Q, guess)
    return int(((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())


def corr0(P, Q, guess, max_corr):
    """Iteration 0 by the oracle's rule: (nn index, float squared distance, has correspondence) per query."""
    d = nn_dists(P, Q, guess)
    j = d.argmin(axis=1)
    bd = d[np.arange(len(j)), j]
    return j, bd, bd.astype(np.float64) < np.float64(max_corr) * np.float64(max_corr)


class Grid:
    """The target's cell table; nn(q) is the 27-cell search of one in-grid query (None: the query is outside
    the grid and the device takes the full scan).  margin: the cell size in units of max_corr (device: 1.01)."""

    def __init__(self, tgt, max_corr, margin=CELL_MARGIN):
        self.tgt = np.ascontiguousarray(tgt, F).reshape(-1, 3)
        self.hinv = grid_hinv(max_corr, margin)
        c, v = grid_cells(self.tgt, self.hinv)
        self.ok = bool(v.all())
        self.cells = {}
        if self.ok:
            for j, key in enumerate(map(tuple, c.astype(np.int64))):
                self.cells.setdefault(key, []).append(j)

    def nn(self, q):
        q = np.asarray(q, F)
        c, v = grid_cells(q, self.hinv)
        if not (self.ok and v.all()):
            return None
        cx, cy, cz = (int(x) for x in c)
        cand = sorted(j for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
                      for j in self.cells.get((cx + dx, cy + dy, cz + dz), ()))
        if not cand:
            return -1, F(0)
        d = dist2f(q[None, :], self.tgt[cand])
        i = int(np.argmin(d))   # ascending j: the first minimum is the smallest (d, j)
        return cand[i], d[i]


def device_corr(q, grid, thr):
    """The device's decision for one query: the correspondence index, or -1."""
    r = grid.nn(q)
    best, bd = full_nn(q, grid.tgt) if r is None else r
    return best if best >= 0 and np.float64(bd) < thr else -1
