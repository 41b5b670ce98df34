"""CPU: every input of tests/pnp_solver_cases.py is in the regime it is named for, shown from the model
(tests/pnp_solver_model.py, DESIGN.md "Motion-only BA definition") alone -- so the GPU comparison against the
model on the same inputs cannot pass by accident.  Where a case is named for a quirk of the reference, the model
with that quirk switched off gives a different mask or pose."""
import math

import numpy as np
import pytest

import pnp_solver_cases as Cs
import pnp_solver_model as BA


def pose_bits(r):
    return r["pose"].view(np.uint32)


def differs(a, b):
    return not np.array_equal(a["mask"], b["mask"]) or not np.array_equal(pose_bits(a), pose_bits(b))


def terr(T, c):
    return float(np.linalg.norm(np.asarray(T, np.float64)[:3, 3] - c["T_true"][:3, 3]))


def round_trip(T):
    return BA.to_pose(BA.to_se3quat(T))


def test_sincos_poly_is_sin_cos():
    for x in (1e-5, 0.01, 0.7, 1.5, 2.0, 3.1, 4.0, 6.0):
        s, c = BA.sincos_poly(x)
        assert abs(s - math.sin(x)) < 1e-15 and abs(c - math.cos(x)) < 1e-15


def test_lane_tree_sum_order():
    """Lane-strided partial sums, then the natural binary tree: not numpy's pairwise sum and not a running sum."""
    rng = np.random.default_rng(0)
    v = rng.normal(0, 1, 700) * 10.0 ** rng.integers(-8, 8, 700)
    act = rng.random(700) < 0.8
    lanes = [0.0] * 256
    for i in range(700):
        if act[i]:
            lanes[i % 256] = lanes[i % 256] + float(v[i])
    while len(lanes) > 1:
        lanes = [lanes[i] + lanes[i + 1] for i in range(0, len(lanes), 2)]
    assert float(BA.lane_tree_sum(v, act)) == lanes[0]


def test_jacobian_is_the_derivative_of_the_error():
    """The analytic Jacobian of the definition against central differences of err under exp(d) * est."""
    c = Cs.case("m10")
    pr = BA.Problem(c["Xw"], c["obs"], c["K4"], 5.991)
    est = BA.to_se3quat(c["Tcw_in"])
    one = np.zeros(len(pr.X), bool)
    for e in range(3):
        one[:] = False
        one[e] = True
        S = pr.evaluate(est, one, False)   # one edge: b_a = J0a ex + J1a ey, H_aa = J0a^2 + J1a^2
        _, ex, ey, _ = pr.errors(est)
        for a in range(6):
            d = [0.0] * 6
            d[a] = 1e-6
            _, exp_, eyp, _ = pr.errors(BA.se3_exp_times(d, est))
            d[a] = -1e-6
            _, exm, eym, _ = pr.errors(BA.se3_exp_times(d, est))
            j0, j1 = (exp_[e] - exm[e]) / 2e-6, (eyp[e] - eym[e]) / 2e-6
            assert abs(S[21 + a] - (j0 * ex[e] + j1 * ey[e])) <= 1e-4 * (1.0 + abs(S[21 + a]))
            k = (0, 6, 11, 15, 18, 20)[a]
            assert abs(S[k] - (j0 * j0 + j1 * j1)) <= 1e-4 * (1.0 + abs(S[k]))


def test_clean_300():
    """Every edge ends an inlier and the translation error shrinks >= 100x against the guess.  Measured with the
    model: 5.1e-2 m -> 1.2e-8 m, a ratio of 4.1e6 (the floor is the f32 rounding of the pixels and of the output
    pose)."""
    c, r = Cs.case("clean_300"), Cs.model("clean_300")
    assert r["ok"] and r["rounds_run"] == 4 and r["n_inliers"] == 300 and not r["mask"].any()
    ratio = terr(c["Tcw_in"], c) / terr(r["pose"], c)
    print("clean_300: translation error %.3g -> %.3g, ratio %.3g" % (terr(c["Tcw_in"], c), terr(r["pose"], c), ratio))
    assert ratio >= 100.0


def test_outliers_30pct():
    c, r = Cs.case("outliers_30pct"), Cs.model("outliers_30pct")
    assert c["planted"].sum() == 90 and np.array_equal(r["mask"], c["planted"]) and r["n_inliers"] == 210
    d = c["obs"][c["planted"] == 1].astype(np.float64) - Cs.project(c["T_true"], c["Xw"])[c["planted"] == 1]
    assert (np.hypot(d[:, 0], d[:, 1]) >= 20.0 - 1e-3).all()


@pytest.mark.parametrize("name,switch", [("restart", dict(restart=False)), ("stale_error", dict(stale=False)),
                                         ("kernel_removed", dict(keep_kernel=True))])
def test_quirk_changes_the_result(name, switch):
    assert differs(Cs.model(name), Cs.model(name, **switch))


def test_restart_round0_is_pulled_away():
    c, r = Cs.case("restart"), Cs.model("restart")
    # the outliers are all active in round 0 and hold the estimate away from the guess and from the planted pose
    assert r["rounds"][0]["n_active"] == 120 and r["rounds"][1]["n_active"] < 120
    e0 = r["rounds"][0]["est"][4:]
    assert np.linalg.norm(e0 - c["Tcw_in"][:3, 3]) > 1e-3 and np.linalg.norm(e0 - c["T_true"][:3, 3]) > 1e-4
    # with the quirk every later round starts from the guess again: rounds 1 and 2 (same edges) repeat each other
    assert np.array_equal(r["rounds"][1]["level"], r["rounds"][0]["level"])
    assert np.array_equal(r["rounds"][1]["est"], r["rounds"][2]["est"])
    off = Cs.model("restart", restart=False)
    assert not np.array_equal(off["rounds"][1]["est"], off["rounds"][2]["est"])


def test_stale_error_flips_one_classification():
    c, r = Cs.case("stale_error"), Cs.model("stale_error")
    r0 = r["rounds"][0]
    assert r0["end"] == "trials" and r0["last_is_trial"]
    off = Cs.model("stale_error", stale=False)["rounds"][0]
    assert np.array_equal(r0["est"], off["est"])   # the same optimisation ...
    flipped = np.nonzero(r0["level"] != off["level"])[0]
    assert c["edge"] in flipped                    # ... and the chosen active edge classified the other way


def test_kernel_removed_only_changes_round_3():
    r, off = Cs.model("kernel_removed"), Cs.model("kernel_removed", keep_kernel=True)
    for k in range(3):
        assert np.array_equal(r["rounds"][k]["est"], off["rounds"][k]["est"])
    assert not np.array_equal(r["rounds"][3]["est"], off["rounds"][3]["est"])


def test_m9_m10_rounds():
    assert Cs.model("m9")["rounds_run"] == 1 and Cs.model("m10")["rounds_run"] == 4
    assert len(Cs.case("m9")["Xw"]) == 9 and len(Cs.case("m10")["Xw"]) == 10


def test_m2_m3_ok():
    assert not Cs.model("m2")["ok"]
    r = Cs.model("m3")
    assert r["ok"] and r["rounds_run"] == 1


def test_all_outliers_after_round0():
    c, r = Cs.case("all_outliers_after_round0"), Cs.model("all_outliers_after_round0")
    assert len(c["Xw"]) >= 10 and r["rounds_run"] == 4
    assert r["rounds"][0]["n_active"] == 12 and r["rounds"][0]["level"].all()
    for k in (1, 2, 3):   # no active edge: nothing optimised, the estimate is the guess, the edges reclassified
        assert r["rounds"][k]["n_active"] == 0 and r["rounds"][k]["iters"] == 0 and r["rounds"][k]["trials"] == 0
        assert r["rounds"][k]["level"].all()
    assert r["n_inliers"] == 0 and np.array_equal(pose_bits(r), round_trip(c["Tcw_in"]).view(np.uint32))


def test_nan_edge():
    c, r = Cs.case("nan_edge"), Cs.model("nan_edge")
    r0 = r["rounds"][0]
    assert math.isnan(r0["chi"]) and r0["iters"] == 10 and r0["trials"] == 10   # ten iterations of one rejection
    assert math.isnan(r0["chi2"][0]) and r["mask"][0] == 0                      # NaN > 5.991 is false: an inlier
    assert np.isfinite(r0["chi2"][1:]).all()
    assert np.array_equal(pose_bits(r), round_trip(c["Tcw_in"]).view(np.uint32))


def test_ten_trials():
    r0 = Cs.model("ten_trials")["rounds"][0]
    assert r0["end"] == "trials"
    tr = []
    c = Cs.case("ten_trials")
    BA.solve(c["Xw"], c["obs"], c["K4"], c["Tcw_in"], trace=tr, **c["prm"])
    last = [t for t in tr if t[0] == 0][-10:]
    assert [t[2] for t in last] == list(range(1, 11)) and all(t[3] < 0 for t in last)


def test_rho_zero():
    c, r = Cs.case("rho_zero"), Cs.model("rho_zero")
    r0 = r["rounds"][0]
    assert len(c["Xw"]) == 3 and r0["end"] == "rho_zero" and r0["iters"] == 1 and r0["trials"] == 1 and r0["chi"] == 0.0
    assert np.array_equal(r["pose"], np.eye(4, dtype=np.float32))


def test_nonorthonormal_guess():
    c, r = Cs.case("nonorthonormal_guess"), Cs.model("nonorthonormal_guess")
    R = c["Tcw_in"][:3, :3].astype(np.float64)
    dev = np.abs(R @ R.T - np.eye(3)).max()
    assert 1e-8 < dev < 1e-6
    # the quaternion round trip, not the matrix, is the starting estimate
    assert not np.array_equal(round_trip(c["Tcw_in"]), c["Tcw_in"])
    assert r["n_inliers"] == 60 and terr(r["pose"], c) < 1e-6


@pytest.mark.parametrize("name,M", [("m255", 255), ("m256", 256), ("m257", 257), ("m4096", 4096)])
def test_sizes(name, M):
    c, r = Cs.case(name), Cs.model(name)
    assert len(c["Xw"]) == M and r["rounds_run"] == 4 and np.array_equal(r["mask"], c["planted"])


def test_nu_carry():
    """nu is the solver object's and is not reset between rounds: at an optimum every round is one rejected
    trial, so round k ends with lambda = lambda_0 * 2^(k+1) and nu = 2^(k+2); with a reset every round would end
    alike."""
    r, off = Cs.model("nu_carry"), Cs.model("nu_carry", nu_reset=True)
    lam0 = r["rounds"][0]["lam"] / 2.0
    assert [x["nu"] for x in r["rounds"]] == [4.0, 8.0, 16.0, 32.0]
    assert [x["lam"] for x in r["rounds"]] == [lam0 * 2.0, lam0 * 4.0, lam0 * 8.0, lam0 * 16.0]
    assert [x["nu"] for x in off["rounds"]] == [4.0] * 4 and [x["lam"] for x in off["rounds"]] == [lam0 * 2.0] * 4


def test_every_case_is_covered():
    assert set(Cs.NAMES) == {"clean_300", "outliers_30pct", "restart", "stale_error", "kernel_removed", "m9", "m10", "m2",
                             "m3", "all_outliers_after_round0", "nan_edge", "ten_trials", "rho_zero",
                             "nonorthonormal_guess", "m255", "m256", "m257", "m4096", "nu_carry"}
