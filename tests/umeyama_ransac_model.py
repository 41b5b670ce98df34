"""numpy restatement of DESIGN.md "Umeyama RANSAC definition" (Ransac::compute, Solver/Ransac.cpp:46-181).

Every operation is f32 in the order the definition fixes (numpy's float32 +, -, *, / and sqrt are the correctly
rounded IEEE operations, one rounding each, like the device's under -ffp-contract=off).  The fit and the scoring run
on a batch axis (one entry per hypothesis): the same scalar sequence per entry, branches taken with np.where.
rand() is the oracle's orc_random_int, pinned to the reference's own System/Random.cpp by tests/test_oracle_ref.py.
"""
import ctypes as C
import math

import numpy as np

F = np.float32
FLT_MIN = F(1.17549435e-38)
FLT_EPS = F(1.1920929e-07)
ITERS0 = 487
EUCLIDEAN_ERROR, REPROJECTION_ERROR, EUCLIDEAN_AND_REPROJECTION_ERROR, MAHALANOBIS_ERROR, ADAPTIVE_ERROR = range(5)
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def params(error_version=EUCLIDEAN_ERROR, used_pairs=3, min_matches=10, thr=0.03, min_inlier_ratio=0.1):
    return dict(error_version=error_version, used_pairs=used_pairs, min_matches=min_matches, thr=float(thr),
                min_inlier_ratio=float(min_inlier_ratio))


# ------------------------------------------------------------------ iteration bounds (:449-454), double, libm
def _log(x):
    return -math.inf if x == 0.0 else math.log(x)


def iters(r):
    """int(log(1 - 0.98) / log(1 - pow(r, 3))), the conversion saturating (a deviation: DESIGN.md)."""
    den = _log(1 - math.pow(r, 3))
    num = math.log(1 - 0.98)
    if den == 0.0:
        q = math.copysign(math.inf, -num) if math.copysign(1.0, den) < 0 else math.copysign(math.inf, num)
    else:
        q = num / den
    if q != q:
        return INT_MIN
    if q >= 2147483648.0:
        return INT_MAX
    if q <= -2147483649.0:
        return INT_MIN
    return int(q)


def ratio(c, M):
    return float(F(c) / F(M))


def bound_table(M, min_ratio):
    cap = iters(min_ratio)
    return [min(cap, iters(ratio(c, M))) for c in range(M + 1)]


# ------------------------------------------------------------------ the sampler (:183-208)
def sample(oracle, rng, M, n):
    """n distinct positions in draw order; returns (positions, rand() calls)."""
    f = oracle.lib().orc_random_int
    pos, calls = [], 0
    while len(pos) < n:
        i = f(C.byref(rng), 0, M - 1)
        calls += 1
        if i not in pos:
            pos.append(i)
    return pos, calls


def copy_rng(oracle, r):
    return oracle.Rng.from_buffer_copy(bytes(r))


# ------------------------------------------------------------------ Eigen 3.3 JacobiSVD<Matrix3f> on a batch
def _make_jacobi(x, y, z, dt):
    one = dt(1)
    deno = dt(2) * np.abs(y)
    skip = deno < np.finfo(dt).tiny
    tau = (x - z) / deno
    w = np.sqrt(tau * tau + one)
    t = np.where(tau > 0, one / (tau + w), one / (tau - w))
    sign_t = np.where(t > 0, one, -one).astype(dt)
    n = one / np.sqrt(t * t + one)
    s = ((-sign_t * np.copysign(one, y)) * np.abs(t)) * n
    return np.where(skip, one, n).astype(dt), np.where(skip, dt(0), s).astype(dt)


def _rot_rows(A, p, q, c, s, on):
    """x' = c x + s y, y' = -s x + c y on rows p, q where `on` and the rotation is not the identity."""
    act = on & ~((c == 1) & (s == 0))
    for i in range(3):
        xi, yi = A[:, p, i].copy(), A[:, q, i].copy()
        A[:, p, i] = np.where(act, c * xi + s * yi, xi)
        A[:, q, i] = np.where(act, -s * xi + c * yi, yi)


def _rot_cols(A, p, q, c, s, on):
    """applyOnTheRight(p, q, j): the transposed rotation (c, -s) on columns p, q."""
    s = -s
    act = on & ~((c == 1) & (s == 0))
    for i in range(3):
        xi, yi = A[:, i, p].copy(), A[:, i, q].copy()
        A[:, i, p] = np.where(act, c * xi + s * yi, xi)
        A[:, i, q] = np.where(act, -s * xi + c * yi, yi)


def svd3(Min, dt=F):
    """Min (H, 3, 3) -> U, S, V (full, sorted); the sweeps of oracle/orc_solver.cpp svd3 in dtype dt."""
    Min = np.asarray(Min, dt)
    H = len(Min)
    one, zero = dt(1), dt(0)
    tiny, eps = np.finfo(dt).tiny, np.finfo(dt).eps
    with np.errstate(all="ignore"):
        a = np.abs(Min).reshape(H, 9)
        finite = np.all(a <= np.finfo(dt).max, axis=1)
        scale = np.zeros(H, dt)
        for k in range(9):
            scale = np.where(a[:, k] > scale, a[:, k], scale)
        scale = np.where(scale == 0, one, scale).astype(dt)
        W = (Min / scale[:, None, None]).astype(dt)
        U = np.tile(np.eye(3, dtype=dt), (H, 1, 1))
        V = U.copy()
        maxDiag = np.maximum(np.maximum(np.abs(W[:, 0, 0]), np.abs(W[:, 1, 1])), np.abs(W[:, 2, 2]))
        live = finite.copy()
        for _ in range(64):
            any_rot = np.zeros(H, bool)
            for p in range(1, 3):
                for q in range(p):
                    thr = np.maximum(tiny, (dt(2) * eps) * maxDiag)
                    on = live & ((np.abs(W[:, p, q]) > thr) | (np.abs(W[:, q, p]) > thr))
                    if not on.any():
                        continue
                    any_rot |= on
                    m00, m01, m10, m11 = W[:, p, p].copy(), W[:, p, q].copy(), W[:, q, p].copy(), W[:, q, q].copy()
                    t = m00 + m11
                    d = m10 - m01
                    small = np.abs(d) < tiny
                    u = t / d
                    tmp = np.sqrt(one + u * u)
                    r1s = np.where(small, zero, one / tmp).astype(dt)
                    r1c = np.where(small, one, u / tmp).astype(dt)
                    app = ~((r1c == 1) & (r1s == 0))
                    a0, b0 = r1c * m00 + r1s * m10, -r1s * m00 + r1c * m10
                    a1, b1 = r1c * m01 + r1s * m11, -r1s * m01 + r1c * m11
                    m00, m10 = np.where(app, a0, m00), np.where(app, b0, m10)
                    m01, m11 = np.where(app, a1, m01), np.where(app, b1, m11)
                    jrc, jrs = _make_jacobi(m00, m01, m11, dt)
                    jtc, jts = jrc, -jrs
                    jlc = r1c * jtc - r1s * jts
                    jls = r1c * jts + r1s * jtc
                    _rot_rows(W, p, q, jlc, jls, on)
                    _rot_cols(U, p, q, jlc, -jls, on)
                    _rot_cols(W, p, q, jrc, jrs, on)
                    _rot_cols(V, p, q, jrc, jrs, on)
                    md = np.maximum(maxDiag, np.maximum(np.abs(W[:, p, p]), np.abs(W[:, q, q])))
                    maxDiag = np.where(on, md, maxDiag)
            live = live & any_rot
            if not live.any():
                break
        S = np.zeros((H, 3), dt)
        for i in range(3):
            d = W[:, i, i]
            S[:, i] = np.abs(d)
            U[:, :, i] = np.where((d < 0)[:, None], -U[:, :, i], U[:, :, i])
        S = (S * scale[:, None]).astype(dt)
        for h in range(H):   # the selection sort of the singular values (after rescaling), per entry
            for i in range(3):
                pos, mx = i, S[h, i]
                for j in range(i + 1, 3):
                    if S[h, j] > mx:
                        mx, pos = S[h, j], j
                if mx == 0:
                    break
                if pos != i:
                    S[h, [i, pos]] = S[h, [pos, i]]
                    U[h][:, [i, pos]] = U[h][:, [pos, i]]
                    V[h][:, [i, pos]] = V[h][:, [pos, i]]
        U[~finite] = np.nan
        V[~finite] = np.nan
        S[~finite] = np.nan
    return U, S, V


def _det3(A):
    return ((A[:, 0, 0] * (A[:, 1, 1] * A[:, 2, 2] - A[:, 1, 2] * A[:, 2, 1])
             - A[:, 0, 1] * (A[:, 1, 0] * A[:, 2, 2] - A[:, 1, 2] * A[:, 2, 0]))
            + A[:, 0, 2] * (A[:, 1, 0] * A[:, 2, 1] - A[:, 1, 1] * A[:, 2, 0]))


def _seqsum(x, axis):
    """sequential f32 sum in index order, the first term taken as it is"""
    return np.add.accumulate(x, axis=axis, dtype=F).take(-1, axis=axis)


def umeyama(dst, src):
    """Eigen::umeyama(src, dst, false) on a batch: dst, src (H, n, 3) f32, n >= 1.
    Returns R (H, 3, 3), t (H, 3), valid (H,) [not isnan(T(0, 0))], sneg (H,)."""
    dst, src = np.asarray(dst, F), np.asarray(src, F)
    H, n, _ = dst.shape
    with np.errstate(all="ignore"):
        inv_n = F(1) / F(n)
        dm = _seqsum(dst, 1) * inv_n
        sm = _seqsum(src, 1) * inv_n
        dd = dst - dm[:, None, :]
        sd = src - sm[:, None, :]
        sigma = np.zeros((H, 3, 3), F)
        for a in range(3):
            for b in range(3):
                sigma[:, a, b] = _seqsum(dd[:, :, a] * sd[:, :, b], 1) * inv_n
        U, _, V = svd3(sigma, F)
        sneg = _det3(U) * _det3(V) < 0
        S = np.ones((H, 3), F)
        S[sneg, 2] = F(-1)
        US = U * S[:, None, :]
        R = np.zeros((H, 3, 3), F)
        for i in range(3):
            for j in range(3):
                R[:, i, j] = (US[:, i, 0] * V[:, j, 0] + US[:, i, 1] * V[:, j, 1]) + US[:, i, 2] * V[:, j, 2]
        t = np.zeros((H, 3), F)
        for i in range(3):
            t[:, i] = dm[:, i] - ((R[:, i, 0] * sm[:, 0] + R[:, i, 1] * sm[:, 1]) + R[:, i, 2] * sm[:, 2])
    return R, t, ~np.isnan(R[:, 0, 0]), sneg


# ------------------------------------------------------------------ the scoring predicate (:259-276)
def inlier_mask(R, t, p1, p2, prm):
    """R (H, 3, 3), t (H, 3); p1, p2 (M, 3) the F1 / F2 points -> (H, M) bool."""
    with np.errstate(all="ignore"):
        x, y, z = p2[None, :, 0], p2[None, :, 1], p2[None, :, 2]
        d = []
        for i in range(3):
            e = ((R[:, i, 0, None] * x + R[:, i, 1, None] * y) + R[:, i, 2, None] * z) + t[:, i, None]
            d.append(e - p1[None, :, i])
        nrm = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        thr = np.full(len(p1), prm["thr"], np.float64)
        if prm["error_version"] == ADAPTIVE_ERROR:
            thr = thr * p1[:, 2].astype(np.float64)
        return nrm.astype(np.float64) < thr[None, :]


def gate(z1, z2):
    """True where the match is removed (:78-81): strict comparisons, a NaN z is kept."""
    with np.errstate(invalid="ignore"):
        return (z1 < F(0.1)) | (z1 > F(6.0)) | (z2 < F(0.1)) | (z2 > F(6.0))


def is_identity(T):
    """Eigen's isIdentity(1e-5f) (:55)."""
    prec = F(1e-5)
    with np.errstate(invalid="ignore"):
        for j in range(4):
            for i in range(4):
                a = F(T[i, j])
                if i == j:
                    if not (np.abs(a - F(1)) <= np.minimum(np.abs(a), F(1)) * prec):
                        return False
                elif not (np.abs(a) <= F(1) * prec):
                    return False
    return True


def inv4(A0):
    """The defined cv::Mat::inv(): f32 Gaussian elimination with partial pivoting on [A | I] (unpinned)."""
    A = np.array(A0, F).reshape(4, 4).copy()
    B = np.eye(4, dtype=F)
    X = np.zeros((4, 4), F)
    for k in range(4):
        piv = k
        for i in range(k + 1, 4):
            if abs(A[i, k]) > abs(A[piv, k]):
                piv = i
        if not abs(A[piv, k]) > 0:
            return np.zeros((4, 4), F)
        if piv != k:
            A[[k, piv]] = A[[piv, k]]
            B[[k, piv]] = B[[piv, k]]
        for i in range(k + 1, 4):
            f = A[i, k] / A[k, k]
            for j in range(k + 1, 4):
                A[i, j] = A[i, j] - f * A[k, j]
            for j in range(4):
                B[i, j] = B[i, j] - f * B[k, j]
    for j in range(4):
        for i in range(3, -1, -1):
            v = B[i, j]
            for k in range(i + 1, 4):
                v = v - A[i, k] * X[k, j]
            X[i, j] = v / A[i, i]
    return X


def pose(T12, Tcw1):
    """inv(T12) * Tcw1 (:53): the product accumulates each dot product in double and rounds once."""
    A, B = inv4(T12).astype(np.float64), np.asarray(Tcw1, F).reshape(4, 4).astype(np.float64)
    out = np.zeros((4, 4), F)
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s += float(A[i, k]) * float(B[k, j])
            out[i, j] = F(s)
    return out


# ------------------------------------------------------------------ the whole call
def solve(oracle, xyz1, xyz2, matches, prm, rng, flags2):
    """Ransac::compute.  matches: structured (queryIdx, trainIdx, ...); rng: oracle.Rng, advanced in place; flags2:
    F2's mvbOutlier, updated in place.  Returns a dict: T (4, 4) f32, inliers (positions in `matches`), ok, iterations,
    best_count, gated, accepts [(iteration, count, new bound)], hyp_pos, hyp_count, hyp_sneg (per evaluated
    hypothesis), best_list (gated positions of the best model's inliers)."""
    xyz1 = np.asarray(xyz1, F).reshape(-1, 3)
    xyz2 = np.asarray(xyz2, F).reshape(-1, 3)
    q, tr = np.asarray(matches["queryIdx"]), np.asarray(matches["trainIdx"])
    flags2[tr] = 1                                   # setOutlier inside the remove_if predicate: every match
    a1, a2 = xyz1[q], xyz2[tr]
    keep = np.nonzero(~gate(a1[:, 2], a2[:, 2]))[0]
    p1, p2 = a1[keep], a2[keep]
    M = len(keep)
    out = dict(T=np.eye(4, dtype=F), inliers=np.zeros(0, np.int64), ok=False, iterations=0, best_count=0, gated=M,
               accepts=[], hyp_pos=[], hyp_count=[], hyp_sneg=[], best_list=np.zeros(0, np.int64))
    if M < prm["min_matches"]:
        return out
    n = prm["used_pairs"]
    tab = bound_table(M, prm["min_inlier_ratio"])
    i, bound, best, best_mask = 0, ITERS0, 0, None
    chunk = 4
    while i < bound:
        # draw a chunk ahead (the generator is rewound to the last hypothesis the loop used)
        states, samples = [], []
        for _ in range(chunk):
            pos, _calls = sample(oracle, rng, M, n)
            samples.append(pos)
            states.append(copy_rng(oracle, rng))
        idx = np.array(samples)
        R, t, valid, sneg = umeyama(p1[idx], p2[idx])
        masks = inlier_mask(R, t, p1, p2, prm)
        counts = np.where(valid, masks.sum(1), -1)
        used = 0
        for h in range(chunk):
            if not i < bound:
                break
            out["hyp_pos"].append(samples[h])
            out["hyp_count"].append(int(counts[h]))
            out["hyp_sneg"].append(bool(sneg[h]))
            if valid[h] and ratio(int(counts[h]), M) > ratio(best, M):   # strictly greater: a tie keeps the earlier
                best, best_mask = int(counts[h]), masks[h].copy()
                bound = min(iters(prm["min_inlier_ratio"]), iters(ratio(best, M)))
                assert bound == tab[best]
                out["accepts"].append((i, best, bound))
            i += 1
            used = h + 1
        C.memmove(C.byref(rng), C.byref(states[used - 1]), C.sizeof(rng))
        chunk = min(256, chunk * 4)
    out["iterations"], out["best_count"] = i, best
    blist = np.nonzero(best_mask)[0] if best_mask is not None else np.zeros(0, np.int64)
    out["best_list"] = blist
    T = np.eye(4, dtype=F)
    fin = blist
    if len(blist):
        R, t, valid, _ = umeyama(p1[blist][None], p2[blist][None])
        if valid[0]:                                  # its failure is ignored: the model is then the identity
            T[:3, :3], T[:3, 3] = R[0], t[0]
        fin = blist[inlier_mask(T[None, :3, :3], T[None, :3, 3], p1[blist], p2[blist], prm)[0]]
    if ratio(best, M) < prm["min_inlier_ratio"]:
        T = np.eye(4, dtype=F)
        fin = np.zeros(0, np.int64)
    out["T"] = T
    out["inliers"] = keep[fin]
    flags2[tr[out["inliers"]]] = 0
    out["ok"] = not is_identity(T)
    return out
