"""CPU: the numpy model of the Umeyama RANSAC (tests/umeyama_ransac_model.py, DESIGN.md "Umeyama RANSAC definition").

First, from the model alone, that every input of tests/umeyama_ransac_cases.py is in the regime it is named for.
Then the model's pieces against independent checks: iters() at known ratios, the sampler against a set over
orc_random_int, Umeyama against an f64 numpy.linalg.svd Kabsch fit, the f32 SVD restatement against the f64 oracle
orc_svd3, and tests/umeyama_loop_check.cpp (csrc/umeyama_dev.h compiled as host code) against the model bit for bit.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import umeyama_ransac_cases as Cs
import umeyama_ransac_model as UM
from conftest import ROOT

F = np.float32
EPS = float(np.finfo(F).eps)


def m(oracle, name):
    return Cs.model(oracle, name)


# ------------------------------------------------------------------ the regimes
def test_clean(oracle):
    r = m(oracle, "clean")
    assert r["accepts"] == [(0, 10, 0)] and r["iterations"] == 1 and r["ok"] and len(r["inliers"]) == 10


def test_half_outliers(oracle):
    r = m(oracle, "half_outliers")
    assert r["best_count"] == 32 and r["accepts"][-1][2] == UM.iters(0.5) == 29 and r["iterations"] == 29
    assert r["accepts"][-1][2] < UM.ITERS0


def test_grow(oracle):
    r = m(oracle, "grow")
    first = r["accepts"][0]
    assert first[2] > UM.ITERS0                      # the first acceptance raises the bound above 487
    assert r["best_count"] == 8 and r["iterations"] == UM.iters(0.125) == 2000 > 3 * 256   # several rounds
    assert r["ok"] and len(r["inliers"]) == 8


def test_below_ratio(oracle):
    r, c = m(oracle, "below_ratio"), Cs.case("below_ratio")
    assert r["iterations"] == UM.iters(0.1) == 3910 and 0 < r["best_count"] <= 6
    assert not r["ok"] and len(r["inliers"]) == 0 and np.array_equal(r["T"], np.eye(4, dtype=F))
    assert np.all(r["flags2"][c["matches"]["trainIdx"]] == 1)


def test_refit_shrinks(oracle):
    r = m(oracle, "refit_shrinks")
    assert 0 < len(r["inliers"]) < len(r["best_list"]) == r["best_count"]
    assert len(Cs.case("refit_shrinks")["matches"]) == 257


def test_reflection(oracle):
    r = m(oracle, "reflection")
    cnt, sn = np.array(r["hyp_count"]), np.array(r["hyp_sneg"])
    assert np.any(sn & (cnt >= 0)) and np.any(~sn & (cnt >= 0))


def test_tie_keeps_first(oracle):
    r = m(oracle, "tie_keeps_first")
    bi = r["accepts"][-1][0]
    later = [i for i, c in enumerate(r["hyp_count"]) if i > bi and c == r["best_count"]]
    assert later                                       # a later hypothesis ties the best count and is not accepted
    assert all(a[1] < r["best_count"] for a in r["accepts"][:-1])


def test_static_pair(oracle):
    r, c = m(oracle, "static_pair"), Cs.case("static_pair")
    assert not r["ok"] and len(r["inliers"]) == 64
    assert np.max(np.abs(r["T"] - np.eye(4, dtype=F))) <= 1e-5
    assert np.all(r["flags2"][c["matches"]["trainIdx"]] == 0)


def test_adaptive(oracle):
    r, c = m(oracle, "adaptive"), Cs.case("adaptive")
    assert c["prm"]["error_version"] == UM.ADAPTIVE_ERROR
    q, t = c["matches"]["queryIdx"], c["matches"]["trainIdx"]
    p1, p2 = c["xyz1"][q], c["xyz2"][t]
    T = r["T"]
    ad = UM.inlier_mask(T[None, :3, :3], T[None, :3, 3], p1, p2, c["prm"])[0]
    eu = UM.inlier_mask(T[None, :3, :3], T[None, :3, 3], p1, p2, dict(c["prm"], error_version=UM.EUCLIDEAN_ERROR))[0]
    assert np.any(ad != eu) and r["ok"]


def test_depth_gate(oracle):
    r, c = m(oracle, "depth_gate"), Cs.case("depth_gate")
    assert r["gated"] == 14 and {0, 1} <= set(r["inliers"].tolist()) and not {2, 3} & set(r["inliers"].tolist())
    assert c["xyz1"][0, 2] == F(0.1) and c["xyz1"][1, 2] == F(6.0) and c["xyz1"][2, 2] < F(0.1) and c["xyz1"][3, 2] > F(6.0)
    assert np.all(r["flags2"][[2, 3]] == 1) and np.all(r["flags2"][[0, 1]] == 0)


def test_nan_z(oracle):
    r = m(oracle, "nan_z")
    assert r["gated"] == 12                            # the NaN z is kept
    with_nan = [i for i, p in enumerate(r["hyp_pos"]) if 4 in p]
    assert with_nan and all(r["hyp_count"][i] == -1 for i in with_nan)
    assert all(c >= 0 for i, c in enumerate(r["hyp_count"]) if i not in with_nan)
    # a failed hypothesis consumes its draws: the generator ends where a replay of every sample ends
    g = oracle.rng(Cs.case("nan_z")["seed"])
    for p in r["hyp_pos"]:
        assert UM.sample(oracle, g, 12, 3)[0] == p
    assert bytes(g) == r["rng"] and 4 not in r["inliers"]


def test_too_few(oracle):
    r, c = m(oracle, "too_few"), Cs.case("too_few")
    assert r["gated"] == 8 < c["prm"]["min_matches"] and r["iterations"] == 0 and not r["ok"] and len(r["inliers"]) == 0
    assert r["rng"] == bytes(oracle.rng(c["seed"]))
    assert np.all(r["flags2"][c["matches"]["trainIdx"]] == 1)


def test_min_size(oracle):
    r = m(oracle, "min_size")
    assert r["gated"] == 3 and sorted(r["hyp_pos"][0]) == [0, 1, 2] and r["iterations"] == 1 and len(r["inliers"]) == 3


def test_duplicate_rows(oracle):
    r, c = m(oracle, "duplicate_rows"), Cs.case("duplicate_rows")
    assert c["matches"][5] == c["matches"][6]
    assert (5 in r["inliers"]) == (6 in r["inliers"]) and r["ok"]


def test_pairs8(oracle):
    r = m(oracle, "pairs8")
    assert all(len(p) == 8 and len(set(p)) == 8 for p in r["hyp_pos"]) and r["ok"]
    assert r["accepts"][-1][2] < r["accepts"][-1][0]   # the new bound is below the running index


def test_saturate(oracle):
    r = m(oracle, "saturate")
    it, c, b = r["accepts"][0]
    q = np.log(1 - 0.98) / np.log(1 - UM.ratio(c, 2304) ** 3)
    assert q >= 2.0 ** 31 and UM.iters(UM.ratio(c, 2304)) == UM.INT_MAX and b == UM.iters(0.1)
    assert r["gated"] == 2304 and r["ok"]


def test_cap(oracle):
    r = m(oracle, "cap")
    assert r["gated"] == 4096 and r["ok"] and len(r["inliers"]) == 2048


def test_chained(oracle):
    rs = Cs.chain_model(oracle)
    assert len(rs) == 3 and len({r["rng"] for r in rs}) == 3
    assert [r["rng"] for r in rs] != [m(oracle, n)["rng"] for n in Cs.CHAIN]


def test_every_case_has_a_regime_test():
    for n in Cs.NAMES + ["chained"]:
        assert "test_" + n in globals(), n


# ------------------------------------------------------------------ the pieces
def test_iters_known_values():
    assert [UM.iters(r) for r in (0.20, 0.15, 0.6, 0.9, 1.0)] == [487, 1157, 16, 2, 0]
    assert UM.iters(0.05) == 31294
    for M in (3, 64, 257, 2304, 4096):   # the ratios are strictly increasing in the count
        r = [UM.ratio(c, M) for c in range(M + 1)]
        assert all(a < b for a, b in zip(r, r[1:]))


def test_sampler_against_a_set(oracle):
    f = oracle.lib().orc_random_int
    for M, n in ((3, 3), (10, 3), (64, 8), (257, 5)):
        a, b = oracle.rng(7), oracle.rng(7)
        for _ in range(200):
            pos, calls = UM.sample(oracle, a, M, n)
            seen, order, k = set(), [], 0
            while len(seen) < n:
                i = f(C.byref(b), 0, M - 1)
                k += 1
                if i not in seen:
                    seen.add(i)
                    order.append(i)
            assert pos == order and calls == k and bytes(a) == bytes(b)


def kabsch64(dst, src):
    dm, sm = dst.mean(0), src.mean(0)
    U, _, Vt = np.linalg.svd((dst - dm).T @ (src - sm) / len(dst))
    S = np.diag([1, 1, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ S @ Vt
    return R, dm - R @ sm


def test_umeyama_against_f64_kabsch():
    """Well-conditioned samples (8 to 40 points spread over a 3 m box, 1 cm noise).  Bound: 32 ulp of f32 on R's
    entries (|R| <= 1) = 32 * 2^-24 = 1.9e-6, the issue's starting point; worst seen here 5.75e-7 (9.6 ulp) on R, 1.63e-6 on t
    (t = mean - R mean with |mean| up to 3 m: bound 32 ulp of 4 = 1.5e-5)."""
    g = np.random.default_rng(0)
    worst_R = worst_t = 0.0
    for n in (8, 16, 40):
        src = np.stack([g.uniform(-1.5, 1.5, (50, n)), g.uniform(-1.5, 1.5, (50, n)), g.uniform(0.8, 4.0, (50, n))], 2)
        dst = src @ Cs.R_TRUE.T + Cs.T_TRUE + 0.01 * g.standard_normal(src.shape)
        src32, dst32 = src.astype(F), dst.astype(F)
        R, t, valid, _ = UM.umeyama(dst32, src32)
        assert valid.all()
        for h in range(50):
            R64, t64 = kabsch64(dst32[h].astype(np.float64), src32[h].astype(np.float64))
            worst_R = max(worst_R, float(np.max(np.abs(R[h] - R64))))
            worst_t = max(worst_t, float(np.max(np.abs(t[h] - t64))))
    print("umeyama vs f64 Kabsch: worst |dR| %.3g, worst |dt| %.3g" % (worst_R, worst_t))
    assert worst_R <= 32 * 2.0 ** -24 and worst_t <= 32 * 2.0 ** -22


def test_svd32_against_oracle_svd3(oracle):
    """The f32 sweeps against the f64 oracle on the same matrices: the reconstruction U S V^T of both equals the
    matrix, and the singular values agree, to 16 ulp of f32 relative to the largest singular value; U and V are
    orthogonal to the same bound.  16 ulp: a sweep applies 3 two-sided rotations, each a handful of roundings per
    entry, and the sweeps run 4 to 5 times before they converge, so a few ulp per sweep accumulate.  Worst seen
    here: 7.06 ulp on S, 8.97 ulp on the reconstruction, 7.55 ulp on orthogonality."""
    g = np.random.default_rng(1)
    A = g.standard_normal((200, 3, 3)).astype(F)
    U, S, V = UM.svd3(A, F)
    worst_s = worst_r = worst_o = 0.0
    for h in range(200):
        U6, S6, V6 = np.zeros(9), np.zeros(3), np.zeros(9)
        oracle.lib().orc_svd3(np.ascontiguousarray(A[h].astype(np.float64).reshape(9)), U6, S6, V6)
        s0 = S6[0]
        worst_s = max(worst_s, float(np.max(np.abs(S[h] - S6))) / s0)
        rec = (U[h].astype(np.float64) * S[h].astype(np.float64)) @ V[h].astype(np.float64).T
        worst_r = max(worst_r, float(np.max(np.abs(rec - A[h]))) / s0)
        worst_o = max(worst_o, float(np.max(np.abs(U[h].astype(np.float64).T @ U[h] - np.eye(3)))),
                      float(np.max(np.abs(V[h].astype(np.float64).T @ V[h] - np.eye(3)))))
        assert S[h][0] >= S[h][1] >= S[h][2] >= 0
    print("svd f32 vs f64 oracle: S %.2f ulp, reconstruction %.2f ulp, orthogonality %.2f ulp"
          % (worst_s / EPS, worst_r / EPS, worst_o / EPS))
    assert worst_s <= 16 * EPS and worst_r <= 16 * EPS and worst_o <= 16 * EPS
    # the same restatement in f64 is the oracle's, bit for bit
    U64, S64, V64 = UM.svd3(A[:20].astype(np.float64), np.float64)
    for h in range(20):
        U6, S6, V6 = np.zeros(9), np.zeros(3), np.zeros(9)
        oracle.lib().orc_svd3(np.ascontiguousarray(A[h].astype(np.float64).reshape(9)), U6, S6, V6)
        assert np.array_equal(S64[h], S6) and np.array_equal(np.abs(U64[h].reshape(9)), np.abs(U6))


def test_pose_inverse():
    T = np.eye(4, dtype=F)
    T[:3, :3] = Cs.R_TRUE.astype(F)
    T[:3, 3] = Cs.T_TRUE.astype(F)
    X = UM.inv4(T)
    assert np.max(np.abs(X.astype(np.float64) @ T - np.eye(4))) < 8 * EPS
    assert np.array_equal(UM.inv4(np.zeros((4, 4), F)), np.zeros((4, 4), F))


# ------------------------------------------------------------------ csrc/umeyama_dev.h as host code
def build_check(out_dir, extra=()):
    exe = os.path.join(str(out_dir), "umeyama_loop_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-fno-fast-math", *extra, "-I",
           os.path.join(ROOT, "rgbd-slam_amd", "csrc"), os.path.join(ROOT, "tests", "umeyama_loop_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("umeyama_loop"))


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return r.stdout.splitlines()


def test_host_iters_match_model(check_exe):
    rs = [0.05, 0.1, 0.15, 0.2, 0.6, 0.9, 1.0] + [UM.ratio(c, M) for M in (64, 257, 2304, 4096) for c in range(0, M + 1, 7)]
    got = [int(x) for x in run(check_exe, "iters", *[repr(float(r)) for r in rs])]
    assert got == [UM.iters(r) for r in rs]


def test_host_svd_matches_model(check_exe, tmp_path):
    g = np.random.default_rng(2)
    A = g.standard_normal((300, 3, 3)).astype(F)
    A[0] = 0
    A[1] = np.eye(3, dtype=F)
    A[2, 2] = 0                     # rank 2
    A[3] = A[3] * F(1e-30)
    A[4, 1, 1] = np.nan
    path = tmp_path / "svd.txt"
    path.write_text("\n".join(" ".join("%08x" % w for w in a.reshape(9).view(np.uint32)) for a in A) + "\n")
    lines = run(check_exe, "svd", str(path))
    U, _, V = UM.svd3(A, F)
    assert len(lines) == 300
    for h, l in enumerate(lines):
        w = np.array([int(x, 16) for x in l.split()], np.uint32).view(F)
        want = np.concatenate([U[h].reshape(9), V[h].reshape(9)])
        assert np.array_equal(np.isnan(w), np.isnan(want)), h
        ok = ~np.isnan(want)
        assert np.array_equal(w[ok].view(np.uint32), want[ok].view(np.uint32)), (h, w, want)


def write_problem(path, c):
    q, t = c["matches"]["queryIdx"], c["matches"]["trainIdx"]
    pts = np.concatenate([c["xyz1"][q], c["xyz2"][t]], 1).astype(F)
    p = c["prm"]
    d = lambda x: "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]
    import oracle_lib
    rng = oracle_lib.rng(c["seed"])
    words = np.frombuffer(bytes(rng), np.int32)
    with open(path, "w") as f:
        f.write("prm %d %d %d %s %s\n" % (p["error_version"], p["used_pairs"], p["min_matches"], d(p["thr"]), d(p["min_inlier_ratio"])))
        f.write("rng " + " ".join(str(int(w)) for w in words) + "\n")
        f.write("pts %d\n" % len(pts))
        for r in pts:
            f.write(" ".join("%08x" % w for w in r.view(np.uint32)) + "\n")


@pytest.mark.parametrize("name", Cs.NAMES)
def test_host_loop_matches_model(oracle, check_exe, tmp_path, name):
    """The whole call on csrc/umeyama_dev.h's rules, one hypothesis at a time, against the model: T's 16 words, the
    inlier list, ok, the iterations, the generator, every hypothesis's sample, count and S branch, every acceptance."""
    c, want = Cs.case(name), m(oracle, name)
    path = tmp_path / "p.txt"
    write_problem(path, c)
    lines = run(check_exe, "solve", str(path))
    hyp = [[int(x) for x in l.split()[1:]] for l in lines if l.startswith("hyp ")]
    acc = [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("accept ")]
    T = np.array([int(x, 16) for x in next(l for l in lines if l.startswith("T ")).split()[1:]], np.uint32)
    res = [int(x) for x in next(l for l in lines if l.startswith("result ")).split()[1:]]
    inl = [int(x) for x in next(l for l in lines if l.startswith("inliers")).split()[1:]]
    rng = np.array([int(x) for x in next(l for l in lines if l.startswith("rng")).split()[1:]], np.int32).tobytes()
    assert [h[0] for h in hyp] == list(range(want["iterations"]))
    assert [h[1] for h in hyp] == want["hyp_count"]
    assert [bool(h[2]) for h in hyp] == want["hyp_sneg"]
    assert [h[3:] for h in hyp] == want["hyp_pos"]
    assert acc == want["accepts"]
    assert np.array_equal(T, want["T"].reshape(16).view(np.uint32))
    assert res == [int(want["ok"]), want["iterations"], want["best_count"], want["gated"], len(want["accepts"])]
    assert inl == want["inliers"].tolist()
    assert rng == want["rng"]
