"""GPU: the Umeyama RANSAC (rgbd_ransac_umeyama and its batch / frames / debug / C++ surfaces) against the numpy
restatement of tests/umeyama_ransac_model.py on the inputs of tests/umeyama_ransac_cases.py.  Every comparison is bit
for bit: T's 16 words, the inlier list, ok, flags2, the generator's state, iterations_run and, through the debug
hook, every evaluated hypothesis's sample, count and S branch and every acceptance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import umeyama_ransac_cases as Cs
import umeyama_ransac_model as UM
from conftest import ROOT, synth_seq

pytestmark = pytest.mark.gpu


def f32bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(640, 480, max_batch=1, orb=pkg.orb_params(1000), cam=pkg.camera(517.3, 516.5, 318.6, 255.3))
    yield c
    c.close()


def prm_of(pkg, c):
    p = c["prm"]
    return pkg.umeyama_params(p["error_version"], p["used_pairs"], p["min_matches"], p["thr"], p["min_inlier_ratio"])


def assert_equals_model(got, want, c, what, debug=False):
    assert got["iterations"] == want["iterations"], (what, got["iterations"], want["iterations"])
    if debug:   # first, so that a mismatch is named at the hypothesis it starts at
        assert got["hyp_pos"].tolist() == want["hyp_pos"], what
        cnt = got["hyp_count"].tolist()
        bad = [i for i, (a, b) in enumerate(zip(cnt, want["hyp_count"])) if a != b]
        assert not bad, (what, "first differing hypothesis", bad[0], cnt[bad[0]], want["hyp_count"][bad[0]])
        assert [bool(x) for x in got["hyp_sneg"]] == want["hyp_sneg"], what
        assert [tuple(a) for a in got["accepts"].tolist()] == want["accepts"], what
        assert got["best_count"] == want["best_count"], what
    assert np.array_equal(f32bits(got["T"]), f32bits(want["T"])), (what, got["T"], want["T"])
    assert got["ok"] == want["ok"], what
    assert got["n_inliers"] == len(want["inliers"]), what
    assert np.array_equal(got["inliers"], c["matches"][want["inliers"]]), what
    assert np.array_equal(got["flags2"][:len(want["flags2"])], want["flags2"]), what
    assert bytes(got["rng"]) == want["rng"], what


@pytest.mark.parametrize("name", Cs.NAMES)
def test_case_equals_model(pkg, oracle, ctx, name):
    c, want = Cs.case(name), Cs.model(oracle, name)
    got = ctx.ransac_umeyama(c["xyz1"], c["xyz2"], c["matches"], prm_of(pkg, c), pkg.rng(c["seed"]), debug=True)
    assert_equals_model(got, want, c, name, debug=True)
    plain = ctx.ransac_umeyama(c["xyz1"], c["xyz2"], c["matches"], prm_of(pkg, c), pkg.rng(c["seed"]))
    assert_equals_model(plain, want, c, name)


def test_flags_start_set(pkg, oracle, ctx):
    """flags2 is in / out: flags of unmatched keypoints stay, matched ones are overwritten"""
    c = Cs.case("half_outliers")
    xyz2 = np.concatenate([c["xyz2"], np.ones((3, 3), np.float32)])
    f0 = np.ones(len(xyz2), np.uint8)
    want = Cs.run_model(oracle, dict(c, xyz2=xyz2), flags2=f0.copy())
    got = ctx.ransac_umeyama(c["xyz1"], xyz2, c["matches"], prm_of(pkg, c), pkg.rng(c["seed"]), flags2=f0.copy())
    assert np.array_equal(got["flags2"], want["flags2"]) and np.all(got["flags2"][-3:] == 1)
    assert 0 < int(got["flags2"].sum()) < len(xyz2)


def test_chained(pkg, oracle, ctx):
    """three calls on one generator equal the model's chain, state for state"""
    rng = pkg.rng(4242)
    for name, want in zip(Cs.CHAIN, Cs.chain_model(oracle)):
        c = Cs.case(name)
        got = ctx.ransac_umeyama(c["xyz1"], c["xyz2"], c["matches"], prm_of(pkg, c), rng)
        assert_equals_model(got, want, c, ("chained", name))


def test_batch_equals_single_calls(pkg, oracle, ctx):
    names = ["too_few", "clean", "grow", "refit_shrinks", "nan_z"]
    prm = prm_of(pkg, Cs.case("clean"))
    assert ctx.ransac_umeyama_batch([], prm, []) == []
    ctx.set_timing(True)
    ctx.reset_timing()
    rngs = [pkg.rng(Cs.case(n)["seed"]) for n in names]
    got = ctx.ransac_umeyama_batch([(Cs.case(n)["xyz1"], Cs.case(n)["xyz2"], Cs.case(n)["matches"], None) for n in names], prm, rngs)
    t = ctx.timings()
    ctx.set_timing(False)
    assert t["k_umeyama"][1] == 1 and "k_umeyama_gather" not in t, t
    for n, g in zip(names, got):
        c = Cs.case(n)
        one = ctx.ransac_umeyama(c["xyz1"], c["xyz2"], c["matches"], prm, pkg.rng(c["seed"]))
        for k in ("ok", "n_inliers", "iterations"):
            assert g[k] == one[k], (n, k)
        assert np.array_equal(f32bits(g["T"]), f32bits(one["T"])) and np.array_equal(g["inliers"], one["inliers"]), n
        assert np.array_equal(g["flags2"], one["flags2"][:len(g["flags2"])]) and bytes(g["rng"]) == bytes(one["rng"]), n
        assert_equals_model(g, Cs.model(oracle, n), c, ("batch", n))


def test_limits(pkg, ctx):
    c = Cs.over_cap()
    ok = Cs.case("clean")
    ctx.set_timing(True)
    ctx.reset_timing()
    with pytest.raises(pkg.RgbdError, match=r"status 4"):
        ctx.ransac_umeyama(c["xyz1"], c["xyz2"], c["matches"], prm_of(pkg, c), pkg.rng(1))
    for bad in (dict(error_version=UM.MAHALANOBIS_ERROR), dict(error_version=UM.REPROJECTION_ERROR),
                dict(error_version=UM.EUCLIDEAN_AND_REPROJECTION_ERROR), dict(error_version=5), dict(used_pairs=2),
                dict(used_pairs=9), dict(used_pairs=5, min_matches=4), dict(min_inlier_ratio=0.049),
                dict(min_inlier_ratio=1.01), dict(min_inlier_ratio=float("nan"))):
        with pytest.raises(pkg.RgbdError, match=r"status 4"):
            ctx.ransac_umeyama(ok["xyz1"], ok["xyz2"], ok["matches"], pkg.umeyama_params(**bad), pkg.rng(1))
    m = ok["matches"].copy()
    m["trainIdx"][3] = len(ok["xyz2"])
    with pytest.raises(pkg.RgbdError, match=r"status 1"):
        ctx.ransac_umeyama(ok["xyz1"], ok["xyz2"], m, prm_of(pkg, ok), pkg.rng(1))
    assert "k_umeyama" not in ctx.timings(), ctx.timings()   # nothing launched
    ctx.set_timing(False)


def test_pose(pkg):
    g = np.random.default_rng(3)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = Cs.R_TRUE.astype(np.float32)
    T[:3, 3] = Cs.T_TRUE.astype(np.float32)
    Tcw1 = np.eye(4, dtype=np.float32)
    Tcw1[:3, :3] = Cs.rodrigues(g.uniform(-0.3, 0.3, 3)).astype(np.float32)
    Tcw1[:3, 3] = g.uniform(-1, 1, 3).astype(np.float32)
    got = pkg.Context.ransac_umeyama_pose(T, Tcw1)
    assert np.array_equal(f32bits(got), f32bits(UM.pose(T, Tcw1)))
    assert np.allclose(T.astype(np.float64) @ got, Tcw1, atol=1e-6)


# ---------------------------------------------------------------- real frames
def test_frames_equal_single_calls(pkg):
    import torch
    bgr, depth, gt, cam = synth_seq(3, seed=3, preset="fr1")
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"],
                   cam["factor"])
    ctx = pkg.Context(640, 480, max_batch=3, orb=pkg.orb_params(1000), cam=c)
    d_bgr = torch.from_numpy(np.ascontiguousarray(bgr[:3])).cuda()
    d_dep = torch.from_numpy(np.ascontiguousarray(depth[:3]).view(np.int16)).cuda()
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 3)
    fr = [ctx.batch_frame(b) for b in range(3)]
    qf, tf = [0, -1, 1], [1, 0, 2]
    matches = []
    for a, b in zip(qf, tf):
        a = max(a, 0)
        matches.append(ctx.match(fr[a]["desc"], fr[b]["desc"], np.zeros(len(fr[a]["kps"]), np.uint8), fr[a]["xyz"][:, 2],
                                 fr[b]["xyz"][:, 2], 0.9))
    prm = pkg.umeyama_params()
    rngs = [pkg.rng(11 + p) for p in range(3)]
    ctx.set_timing(True)
    ctx.reset_timing()
    got = ctx.ransac_umeyama_frames(qf, tf, matches, prm, rngs)
    t = ctx.timings()
    ctx.set_timing(False)
    assert t["k_umeyama"][1] == 1 and t["k_umeyama_gather"][1] == 1, t
    assert not got[1]["ok"] and got[1]["iterations"] == 0 and bytes(got[1]["rng"]) == bytes(pkg.rng(12))
    for p in (0, 2):
        a, b = qf[p], tf[p]
        assert len(matches[p]) > 50
        one = ctx.ransac_umeyama(fr[a]["xyz"], fr[b]["xyz"], matches[p], prm, pkg.rng(11 + p))
        assert one["ok"] and one["n_inliers"] > 30, (p, one["n_inliers"])
        for k in ("ok", "n_inliers", "iterations"):
            assert got[p][k] == one[k], (p, k)
        assert np.array_equal(f32bits(got[p]["T"]), f32bits(one["T"])) and np.array_equal(got[p]["inliers"], one["inliers"])
        assert np.array_equal(got[p]["flags2"][:len(one["flags2"])], one["flags2"]) and bytes(got[p]["rng"]) == bytes(one["rng"])
        # the estimate is the planted motion: T12 = Tcw1 * inv(Tcw2)
        want = gt[a].astype(np.float64) @ np.linalg.inv(gt[b].astype(np.float64))
        assert np.max(np.abs(one["T"][:3, 3] - want[:3, 3])) < 0.02, (p, one["T"], want)
    with pytest.raises(pkg.RgbdError, match=r"status 4"):
        ctx.ransac_umeyama_frames([0], [3], matches[:1], prm, [pkg.rng(1)])
    ctx.close()


# ---------------------------------------------------------------- C++ surface
def test_cpp_ransac_example(pkg, oracle, tmp_path):
    exe = os.path.join(ROOT, "rgbd-slam_amd", "build", "ransac_example")
    assert os.path.exists(exe), "build() must compile examples/ransac_example.cpp"
    bgr, depth, gt, cam = synth_seq(4, seed=3, preset="fr1")
    raw = tmp_path / "pair.raw"
    with open(raw, "wb") as f:
        for i in range(2):
            f.write(np.ascontiguousarray(bgr[i]).tobytes())
            f.write(np.ascontiguousarray(depth[i]).tobytes())
    args = [exe, str(raw)] + ["%r" % float(cam[k]) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "factor")]
    out = subprocess.run(args + ["2024", "0", "0.03"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    n = int(lines[0].split()[1])
    rows = np.array([[float(v) for v in l.split()] for l in lines[1:1 + n]])
    ok, ni, it = [int(v) for v in lines[1 + n].split()[1:]]
    hexpose = lambda l: np.array([int(v, 16) for v in l.split()[1:]], np.uint32).view(np.float32).reshape(4, 4)
    T, pose = hexpose(lines[2 + n]), hexpose(lines[3 + n])
    inl = np.array([[float(v) for v in l.split()] for l in lines[4 + n:4 + n + ni]])
    flagged = int(lines[4 + n + ni].split()[1])
    # the model on the same frames and matches
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"],
                   cam["factor"])
    ctx = pkg.Context(640, 480, max_batch=1, orb=pkg.orb_params(1000), cam=c)
    fr = [ctx.frame(bgr[i], depth[i]) for i in range(2)]
    ctx.close()
    m = np.zeros(n, Cs.DMATCH)
    m["queryIdx"], m["trainIdx"], m["imgIdx"], m["distance"] = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    flags2 = np.zeros(len(fr[1]["xyz"]), np.uint8)
    want = UM.solve(oracle, fr[0]["xyz"], fr[1]["xyz"], m, UM.params(), oracle.rng(2024), flags2)
    assert n > 50 and want["ok"] and ok == 1
    assert it == want["iterations"] and ni == len(want["inliers"])
    assert np.array_equal(f32bits(T), f32bits(want["T"]))
    assert np.array_equal(inl, rows[want["inliers"]])
    assert flagged == int(flags2[m["trainIdx"]].sum())
    assert np.array_equal(f32bits(pose), f32bits(UM.pose(want["T"], np.eye(4, dtype=np.float32))))
