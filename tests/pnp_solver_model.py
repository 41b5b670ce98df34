"""TEST INFRASTRUCTURE ONLY: numpy f64 restatement of DESIGN.md "Motion-only BA definition"
(PnPSolver::compute, Solver/PnPSolver.cpp:31-150), the operator behind rgbd_pnp_solver*.

Every per-edge operation is an elementwise numpy f64 operation in the order the definition gives (numpy never
contracts a multiply and an add), every sum over edges is the definition's: lane l of 256 adds its edges
l, l + 256, ... in sequence to 0.0, then the natural-order binary tree over the 256 lanes.  The serial part
(Cholesky, exponential, quaternion algebra, the LM schedule) is Python float arithmetic, which is IEEE f64.

The quirks of the reference are switches, on by default; a test turns one off to show that an input depends
on it:
  restart      every round starts again from Tcw_in (off: from the previous round's estimate)
  stale        an active edge is classified on the error of the last evaluation (off: on the final estimate)
  keep_kernel  False: the Huber kernel is removed after round robust_rounds - 1 (True: never)
  nu_reset     False: nu carries over between rounds (True: reset to 2 at every round's iteration 0)
"""
import math

import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
LANES = 256
MAX_TRIALS = 10


def sincos_poly(x):
    """gn6_dev.h's sincos_poly: quadrant reduction by pi/2 in two parts, then the Taylor polynomials (Horner)."""
    PIO2_1, PIO2_1T = 1.57079632673412561417e+00, 6.07710050650619224932e-11
    INV_PIO2 = 6.36619772367581382433e-01
    kd = math.floor(x * INV_PIO2 + 0.5)
    k = int(kd)
    kd = float(kd)
    r = (x - kd * PIO2_1) - kd * PIO2_1T
    r2 = r * r
    s = -1.0 / 121645100408832000.0
    for c in (1.0 / 355687428096000.0, -1.0 / 1307674368000.0, 1.0 / 6227020800.0, -1.0 / 39916800.0, 1.0 / 362880.0,
              -1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0, 1.0):
        s = s * r2 + c
    sr = s * r
    c = -1.0 / 6402373705728000.0
    for a in (1.0 / 20922789888000.0, -1.0 / 87178291200.0, 1.0 / 479001600.0, -1.0 / 3628800.0, 1.0 / 40320.0,
              -1.0 / 720.0, 1.0 / 24.0, -0.5, 1.0):
        c = c * r2 + a
    return ((sr, c), (c, -sr), (-sr, -c), (-c, sr))[k & 3]


def quat_from_R(m):
    """Eigen's Quaterniond(Matrix3d) (the algorithm oracle/posegraph_ref.py's quat_from_R restates); m[r][c]."""
    t = (m[0][0] + m[1][1]) + m[2][2]
    if t > 0:
        s = math.sqrt(t + 1.0)
        w = 0.5 * s
        s = 0.5 / s
        return [(m[2][1] - m[1][2]) * s, (m[0][2] - m[2][0]) * s, (m[1][0] - m[0][1]) * s, w]
    i = 0
    if m[1][1] > m[0][0]:
        i = 1
    if m[2][2] > m[i][i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    s = _sqrt(((m[i][i] - m[j][j]) - m[k][k]) + 1.0)
    q = [0.0] * 4
    q[i] = 0.5 * s
    s = 0.5 / s
    q[3] = (m[k][j] - m[j][k]) * s
    q[j] = (m[j][i] + m[i][j]) * s
    q[k] = (m[k][i] + m[i][k]) * s
    return q


def _sqrt(x):
    return math.sqrt(x) if x >= 0 else float("nan")


def normalized(q):
    """SE3Quat::normalizeRotation: the sign first (w >= 0), then every component divided by the norm."""
    x, y, z, w = q
    if w < 0:
        x, y, z, w = -x, -y, -z, -w
    n = _sqrt(((x * x + y * y) + z * z) + w * w)
    return [x / n, y / n, z / n, w / n]


def R_of(q):
    """Eigen's Quaterniond::toRotationMatrix."""
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, 1.0 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def to_se3quat(T):
    """Converter::toSE3Quat: the float pose widened element by element, Quaterniond(R), normalised."""
    T = np.asarray(T, np.float32).reshape(4, 4)
    R = [[float(T[r, c]) for c in range(3)] for r in range(3)]
    return normalized(quat_from_R(R)), [float(T[r, 3]) for r in range(3)]


def to_pose(est):
    """to_homogeneous_matrix() cast to float, last row 0 0 0 1."""
    q, t = est
    T = np.zeros((4, 4), np.float32)
    T[:3, :3] = np.array(R_of(q), np.float64).astype(np.float32)
    T[:3, 3] = np.array(t, np.float64).astype(np.float32)
    T[3, 3] = 1.0
    return T


def se3_exp_times(d, est):
    """exp(d) * est with g2o's SE3Quat::exp; d = (omega, upsilon)."""
    q, t = est
    wx, wy, wz = d[0], d[1], d[2]
    th2 = (wx * wx + wy * wy) + wz * wz
    th = _sqrt(th2)
    Om = [[0.0, -wz, wy], [wz, 0.0, -wx], [-wy, wx, 0.0]]
    xy, xz, yz = wx * wy, wx * wz, wy * wz
    Om2 = [[-(wy * wy + wz * wz), xy, xz], [xy, -(wx * wx + wz * wz), yz], [xz, yz, -(wx * wx + wy * wy)]]
    if th < 1e-5:
        a, b, c = 1.0, 0.5, 1.0 / 6.0
    else:
        sn, cs = sincos_poly(th)
        a = sn / th
        b = (1.0 - cs) / th2
        c = (th - sn) / (th2 * th)
    R = [[0.0] * 3 for _ in range(3)]
    V = [[0.0] * 3 for _ in range(3)]
    for r in range(3):
        for k in range(3):
            e = 1.0 if r == k else 0.0
            R[r][k] = (e + a * Om[r][k]) + b * Om2[r][k]
            V[r][k] = (e + b * Om[r][k]) + c * Om2[r][k]
    tn = [((R[r][0] * t[0] + R[r][1] * t[1]) + R[r][2] * t[2]) + ((V[r][0] * d[3] + V[r][1] * d[4]) + V[r][2] * d[5])
          for r in range(3)]
    ax, ay, az, aw = normalized(quat_from_R(R))
    bx, by, bz, bw = q
    qn = [((aw * bx + ax * bw) + ay * bz) - az * by,
          ((aw * by + ay * bw) + az * bx) - ax * bz,
          ((aw * bz + az * bw) + ax * by) - ay * bx,
          ((aw * bw - ax * bx) - ay * by) - az * bz]
    return normalized(qn), tn


def lane_tree_sum(v, active):
    """Lane l adds v[l], v[l + 256], ... of the active edges to 0.0 in sequence; then the natural binary tree."""
    M = v.shape[-1]
    rows = (M + LANES - 1) // LANES
    pad = np.zeros(v.shape[:-1] + (rows * LANES,))
    with np.errstate(all="ignore"):
        pad[..., :M] = np.where(active, v, 0.0)   # a skipped edge adds nothing: x + 0.0 == x for the x a lane can hold
        acc = np.zeros(v.shape[:-1] + (LANES,))
        for j in range(rows):
            acc = acc + pad[..., j * LANES:(j + 1) * LANES]
        n = LANES
        while n > 1:
            acc = acc[..., 0:n:2] + acc[..., 1:n:2]
            n //= 2
    return acc[..., 0]


class Problem:
    def __init__(self, Xw, obs, K4, chi2_threshold):
        self.X = np.asarray(Xw, np.float32).reshape(-1, 3).astype(np.float64)
        self.o = np.asarray(obs, np.float32).reshape(-1, 2).astype(np.float64)
        self.fx, self.fy, self.cx, self.cy = [float(np.float32(v)) for v in K4]
        self.delta = math.sqrt(chi2_threshold)
        self.delta2 = self.delta * self.delta

    def errors(self, est):
        """Per edge at the estimate: p, err, raw chi2."""
        q, t = est
        R = R_of(q)
        X = self.X
        with np.errstate(all="ignore"):
            p = [((R[r][0] * X[:, 0] + R[r][1] * X[:, 1]) + R[r][2] * X[:, 2]) + t[r] for r in range(3)]
            ex = self.o[:, 0] - ((p[0] / p[2]) * self.fx + self.cx)
            ey = self.o[:, 1] - ((p[1] / p[2]) * self.fy + self.cy)
            chi2 = ex * ex + ey * ey
        return p, ex, ey, chi2

    def evaluate(self, est, active, robust):
        """The 28 sums of one evaluation: the 21 upper entries of H (row-major), the 6 of sum w J^T err, sum rho."""
        (x, y, z), ex, ey, chi2 = self.errors(est)
        fx, fy = self.fx, self.fy
        with np.errstate(all="ignore"):
            iz = 1.0 / z
            iz2 = iz * iz
            zero = np.zeros_like(x)
            J0 = [((x * y) * iz2) * fx, -((1.0 + (x * x) * iz2) * fx), (y * iz) * fx, -(iz * fx), zero, (x * iz2) * fx]
            J1 = [(1.0 + (y * y) * iz2) * fy, -(((x * y) * iz2) * fy), -((x * iz) * fy), zero, -(iz * fy), (y * iz2) * fy]
            if robust:
                s = np.sqrt(chi2)
                inl = chi2 <= self.delta2
                rho = np.where(inl, chi2, (2.0 * s) * self.delta - self.delta2)
                w = np.where(inl, 1.0, self.delta / s)
            else:
                rho, w = chi2, np.ones_like(chi2)
            terms = []
            for a in range(6):
                for b in range(a, 6):
                    terms.append(w * (J0[a] * J0[b] + J1[a] * J1[b]))
            for a in range(6):
                terms.append(w * (J0[a] * ex + J1[a] * ey))
            terms.append(rho)
        return [float(v) for v in lane_tree_sum(np.stack(terms), active)]


def chol_solve(S, lam):
    """(H + lam I) d = b by unpivoted Cholesky; None when a pivot is not > 0.  b = -(sum w J^T err)."""
    A = [[0.0] * 6 for _ in range(6)]
    k = 0
    for a in range(6):
        for b in range(a, 6):
            A[a][b] = A[b][a] = S[k]
            k += 1
    rhs = [-S[21 + a] for a in range(6)]
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = A[j][j] + lam
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not s > 0:
            return None
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    yv = [0.0] * 6
    for i in range(6):
        s = rhs[i]
        for k in range(i):
            s = s - L[i][k] * yv[k]
        yv[i] = s / L[i][i]
    d = [0.0] * 6
    for i in range(5, -1, -1):
        s = yv[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * d[k]
        d[i] = s / L[i][i]
    return d


def solve(Xw, obs, K4, Tcw_in, rounds=4, iterations=10, chi2_threshold=5.991, robust_rounds=3, min_edges=10,
          restart=True, stale=True, keep_kernel=False, nu_reset=False, trace=None):
    """dict(ok, pose (4, 4) f32, mask (M,) u8 [1 = outlier], n_inliers, rounds_run, rounds = per-round records:
    est (7,) f64 [qx qy qz qw tx ty tz], iters, trials, lam, nu, chi2 (M,), level (M,), last_is_trial [the last
    evaluation of the round was a rejected trial], n_active, end [what ended the round: trials, rho_zero, lambda,
    iterations or none], chi [the round's last accepted robust chi]).  trace: a list that receives one
    (round, iteration, trial, rho_hat, lambda and nu before the decision, solved) per trial."""
    pr = Problem(Xw, obs, K4, chi2_threshold)
    M = len(pr.X)
    if M < 3:
        return dict(ok=False, M=M)
    est_in = to_se3quat(Tcw_in)
    level = np.zeros(M, np.uint8)
    lam, nu = 0.0, 2.0
    est = est_in
    recs = []
    for rnd in range(rounds):
        robust = keep_kernel or rnd < robust_rounds
        active = level == 0
        if restart or rnd == 0:
            est = est_in
        last = est
        iters = trials = 0
        end = "none"
        if active.any():
            for it in range(iterations):
                S = pr.evaluate(est, active, robust)
                last = est
                chi = S[27]
                if it == 0:
                    m = 0.0
                    for a in (0, 6, 11, 15, 18, 20):
                        if abs(S[a]) > m:
                            m = abs(S[a])
                    lam = 1e-5 * m
                    if nu_reset:
                        nu = 2.0
                b = [-S[21 + a] for a in range(6)]
                ntr = 0
                while True:
                    d = chol_solve(S, lam)
                    if d is None:
                        chi_new, scale, trial = DBL_MAX, 1e-3, None
                    else:
                        trial = se3_exp_times(d, est)
                        chi_new = pr.evaluate(trial, active, robust)[27]
                        last = trial
                        scale = 0.0
                        for a in range(6):
                            scale = scale + d[a] * (lam * d[a] + b[a])
                        scale = scale + 1e-3
                    with np.errstate(all="ignore"):
                        rho = float((np.float64(chi) - np.float64(chi_new)) / np.float64(scale))
                    ntr += 1
                    if trace is not None:
                        trace.append((rnd, it, ntr, rho, lam, nu, d is not None))
                    if rho > 0 and math.isfinite(chi_new):
                        tmp = 2.0 * rho - 1.0
                        alpha = 1.0 - (tmp * tmp) * tmp
                        if 2.0 / 3.0 < alpha:
                            alpha = 2.0 / 3.0
                        if not 1.0 / 3.0 < alpha:
                            alpha = 1.0 / 3.0
                        lam = lam * alpha
                        nu = 2.0
                        chi = chi_new
                        if trial is not None:
                            est = trial
                    else:
                        with np.errstate(all="ignore"):
                            lam = float(np.float64(lam) * np.float64(nu))
                            nu = float(np.float64(nu) * 2.0)
                    if not (rho < 0 and ntr < MAX_TRIALS):
                        break
                trials += ntr
                iters += 1
                if ntr == MAX_TRIALS or rho == 0 or not math.isfinite(lam):
                    end = "trials" if ntr == MAX_TRIALS else ("rho_zero" if rho == 0 else "lambda")
                    break
            else:
                end = "iterations"
        final = est
        chi_fin = pr.errors(final)[3]
        chi_act = pr.errors(last)[3] if stale else chi_fin
        chi2 = np.where(active, chi_act, chi_fin)
        with np.errstate(all="ignore"):
            level = (chi2 > chi2_threshold).astype(np.uint8)
        recs.append(dict(est=np.array(list(final[0]) + list(final[1])), iters=iters, trials=trials, lam=lam, nu=nu,
                         chi2=chi2.copy(), level=level.copy(), last_is_trial=last is not final, end=end, chi=chi if active.any() else None,
                         n_active=int(active.sum())))
        if M < min_edges:
            break
    return dict(ok=True, M=M, pose=to_pose(est), mask=level.copy(), n_inliers=int((level == 0).sum()),
                rounds_run=len(recs), rounds=recs)
