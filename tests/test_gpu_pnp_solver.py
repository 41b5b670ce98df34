"""GPU: the motion-only bundle adjustment (rgbd_pnp_solver and its batch / frames / debug / C++ surfaces) against
the numpy restatement of tests/pnp_solver_model.py on the inputs of tests/pnp_solver_cases.py.  Every comparison
is bit for bit: the pose as u32 bits, masks, counts, and through the debug hook the f64 bits of each round's
estimate, lambda, nu and chi2.  (A NaN is compared as a NaN: the sign and payload of a NaN an operation produces
are not part of IEEE 754's arithmetic, and 0 / 0 differs between the two machines.)"""
import os
import subprocess

import numpy as np
import pytest

import chain_model
import pnp_solver_cases as Cs
import pnp_solver_model as BA
from conftest import ROOT, synth_seq

pytestmark = pytest.mark.gpu

SINGLE = {}   # name -> debug_pnp_solver's result under the case's own parameters, shared by the tests


def f64bits(a):
    a = np.ascontiguousarray(a, np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = 0x7FF8000000000000
    return b


def f32bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(640, 480, max_batch=1, orb=pkg.orb_params(1000), cam=pkg.camera(517.3, 516.5, 318.6, 255.3))
    yield c
    c.close()


def _prm(pkg, c):
    return pkg.pnp_solver_params(**c["prm"]) if c["prm"] else None


def _debug(pkg, ctx, name):
    if name not in SINGLE:
        c = Cs.case(name)
        SINGLE[name] = ctx.debug_pnp_solver(c["Xw"], c["obs"], c["K4"], c["Tcw_in"], _prm(pkg, c))
    return SINGLE[name]


def assert_equals_model(got, want, what, debug=True):
    assert got["ok"] == want["ok"], what
    if not want["ok"]:
        assert got["pose"] is None and got["mask"] is None and got["n_inliers"] is None, what
        return
    assert np.array_equal(f32bits(got["pose"]), f32bits(want["pose"])), (what, got["pose"], want["pose"])
    assert np.array_equal(got["mask"], want["mask"]), what
    assert got["n_inliers"] == want["n_inliers"], what
    if not debug:
        return
    assert got["rounds_run"] == want["rounds_run"], what
    for k, rec in enumerate(want["rounds"]):
        w = (what, "round", k)
        assert got["iters"][k] == rec["iters"] and got["trials"][k] == rec["trials"], (w, got["iters"], got["trials"])
        assert np.array_equal(f64bits(got["est"][k]), f64bits(rec["est"])), (w, got["est"][k], rec["est"])
        assert np.array_equal(f64bits(got["lam"][k:k + 1]), f64bits([rec["lam"]])), (w, got["lam"][k], rec["lam"])
        assert np.array_equal(f64bits(got["nu"][k:k + 1]), f64bits([rec["nu"]])), (w, got["nu"][k], rec["nu"])
        assert np.array_equal(f64bits(got["chi2"][k]), f64bits(rec["chi2"])), w
        assert np.array_equal(got["level"][k], rec["level"]), w
    for k in range(want["rounds_run"], len(got["iters"])):   # rounds not run: zeros
        assert got["iters"][k] == 0 and not got["est"][k].any() and not got["level"][k].any(), (what, k)


# ---------------------------------------------------------------- every case: debug hook and single entry
@pytest.mark.parametrize("name", Cs.NAMES)
def test_case_equals_model(pkg, ctx, name):
    c, want = Cs.case(name), Cs.model(name)
    got = _debug(pkg, ctx, name)
    assert_equals_model(got, want, name)
    one = ctx.pnp_solver(c["Xw"], c["obs"], c["K4"], c["Tcw_in"], _prm(pkg, c))
    assert_equals_model(one, want, name, debug=False)


def test_m2_writes_nothing(pkg, ctx):
    """ok = 0 leaves every other output as it was."""
    import ctypes as C
    c = Cs.case("m2")
    pose = np.full(16, 7.0, np.float32)
    mask = np.full(2, 9, np.uint8)
    ni, ok = C.c_int32(-5), C.c_int32(1)
    Xw, obs = np.ascontiguousarray(c["Xw"]), np.ascontiguousarray(c["obs"])
    K4, T = np.ascontiguousarray(c["K4"]), np.ascontiguousarray(c["Tcw_in"])
    st = pkg.lib().rgbd_pnp_solver(ctx._h, Xw.ctypes.data, obs.ctypes.data, 2, K4.ctypes.data, T.ctypes.data, None,
                                   pose.ctypes.data, mask.ctypes.data, C.byref(ni), C.byref(ok))
    assert st == 0 and ok.value == 0 and ni.value == -5 and (pose == 7.0).all() and (mask == 9).all()


# ---------------------------------------------------------------- batch
def test_batch_equals_single_calls(pkg, ctx):
    """All inputs that share the fr1 camera as one launch under the default parameters (mixed sizes, the ok = 0 one
    included; a batch has one K4 and one parameter set, so the two exact-optimum inputs with their own camera stay
    out and the inputs with parameters of their own run under the defaults here, in the batch and alone)."""
    probs = [(Cs.case(n)["Xw"], Cs.case(n)["obs"], Cs.case(n)["Tcw_in"]) for n in Cs.NAMES if Cs.case(n)["K4"] is Cs.K4]
    names = [n for n in Cs.NAMES if Cs.case(n)["K4"] is Cs.K4]
    assert "m2" in names and "m4096" in names and len(names) >= 16
    ctx.set_timing(True)
    ctx.reset_timing()
    got = ctx.pnp_solver_batch(probs, Cs.K4)
    t = ctx.timings()
    ctx.set_timing(False)
    assert t["k_pnpba"][1] == 1 and "k_pnpba_gather" not in t, t
    for n, g, p in zip(names, got, probs):
        one = ctx.pnp_solver(p[0], p[1], Cs.K4, p[2])
        assert g["ok"] == one["ok"], n
        if one["ok"]:
            assert np.array_equal(f32bits(g["pose"]), f32bits(one["pose"])) and np.array_equal(g["mask"], one["mask"]), n
            assert g["n_inliers"] == one["n_inliers"], n
        if not Cs.case(n)["prm"]:
            assert_equals_model(g, Cs.model(n), n, debug=False)


# ---------------------------------------------------------------- real frames
def _frames_ctx(pkg, preset):
    import torch
    seed, nf = {"fr1": (3, 1000), "fr2": (7, 2000)}[preset]
    bgr, depth, gt, cam = synth_seq(3, seed=seed, preset=preset)
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"],
                   cam["factor"])
    ctx = pkg.Context(640, 480, max_batch=3, orb=pkg.orb_params(nf), cam=c)
    d_bgr = torch.from_numpy(np.ascontiguousarray(bgr[:3])).cuda()
    d_dep = torch.from_numpy(np.ascontiguousarray(depth[:3]).view(np.int16)).cuda()
    ctx.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 3)
    return ctx, [np.asarray(g, np.float32) for g in gt[:3]], cam


@pytest.mark.parametrize("preset", ["fr1", "fr2"])
def test_real_frames(pkg, preset):
    ctx, gt, cam = _frames_ctx(pkg, preset)
    fr = [ctx.batch_frame(b) for b in range(3)]
    K4 = np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], np.float32)
    qf, tf = [0, -1, 0], [1, 0, 2]
    matches = ctx.projection_match_batch(qf, tf, np.stack(gt), 5.0)
    # the guesses: the train frames' poses 3 cm and 1 degree off; the query frame keeps its pose
    off = Cs.pose(np.deg2rad(1.0) * np.array([0.6, -0.64, 0.48]), [0.018, -0.019, 0.014])
    poses = np.stack([gt[0], (off @ gt[1].astype(np.float64)).astype(np.float32),
                      (np.linalg.inv(off) @ gt[2].astype(np.float64)).astype(np.float32)])
    for as_written in (False, True):
        ctx.set_timing(True)
        ctx.reset_timing()
        got = ctx.pnp_solver_frames(qf, tf, poses, matches, as_written)
        t = ctx.timings()
        ctx.set_timing(False)
        assert t["k_pnpba"][1] == 1 and t["k_pnpba_gather"][1] == 1, t
        assert not got[1]["ok"]   # the skipped pair
        for p in (0, 2):
            m = matches[p]
            assert len(m) > 150, (preset, p, len(m))
            a, b = qf[p], tf[p]
            if as_written:
                Xw = np.stack([chain_model.unproject_world(poses[b], fr[b]["xyz"][j]) for j in m["trainIdx"]])
            else:
                Xw = np.stack([chain_model.unproject_world(poses[a], fr[a]["xyz"][i]) for i in m["queryIdx"]])
            ku = fr[b]["kps_un"][m["trainIdx"]]
            obs = np.stack([ku["x"], ku["y"]], 1).astype(np.float32)
            one = ctx.pnp_solver(Xw, obs, K4, poses[b])
            want = BA.solve(Xw, obs, K4, poses[b])
            what = (preset, as_written, p)
            assert_equals_model(one, want, what, debug=False)
            assert_equals_model(got[p], want, what, debug=False)
            if not as_written:   # the refinement moves the perturbed pose back towards the ground truth
                e0 = np.linalg.norm(poses[b][:3, 3].astype(np.float64) - gt[b][:3, 3])
                e1 = np.linalg.norm(got[p]["pose"][:3, 3].astype(np.float64) - gt[b][:3, 3])
                print(what, "translation error %.3g -> %.3g, inliers %d of %d" % (e0, e1, got[p]["n_inliers"], len(m)))
                assert e1 < 0.5 * e0, what
    ctx.close()


# ---------------------------------------------------------------- limits and degenerate calls
def test_limits_and_degenerate_calls(pkg, ctx):
    c = Cs.case("m4096")
    Xw, obs = np.concatenate([c["Xw"], c["Xw"][:1]]), np.concatenate([c["obs"], c["obs"][:1]])
    ctx.set_timing(True)
    ctx.reset_timing()
    with pytest.raises(pkg.RgbdError, match=r"status 4"):
        ctx.pnp_solver(Xw, obs, c["K4"], c["Tcw_in"])
    with pytest.raises(pkg.RgbdError, match=r"status 4"):
        ctx.pnp_solver_batch([(Xw[:5], obs[:5], c["Tcw_in"]), (Xw, obs, c["Tcw_in"])], c["K4"])
    assert ctx.pnp_solver_batch([], c["K4"]) == []
    small = ctx.pnp_solver_batch([(Xw[:2], obs[:2], c["Tcw_in"])], c["K4"])
    assert len(small) == 1 and not small[0]["ok"]
    assert "k_pnpba" not in ctx.timings(), ctx.timings()   # nothing launched by any of the four
    ctx.set_timing(False)
    for bad in (dict(rounds=0), dict(rounds=17), dict(iterations=0), dict(chi2_threshold=0.0),
                dict(chi2_threshold=float("nan"))):
        with pytest.raises(pkg.RgbdError, match=r"status 1"):
            ctx.pnp_solver(Xw[:20], obs[:20], c["K4"], c["Tcw_in"], pkg.pnp_solver_params(**bad))


def test_null_params_equal_explicit_defaults(pkg, ctx):
    c = Cs.case("m257")
    a = ctx.debug_pnp_solver(c["Xw"], c["obs"], c["K4"], c["Tcw_in"], None)
    b = ctx.debug_pnp_solver(c["Xw"], c["obs"], c["K4"], c["Tcw_in"], pkg.pnp_solver_params())
    d = pkg.pnp_solver_params()
    assert (d.rounds, d.iterations, d.chi2_threshold, d.robust_rounds, d.min_edges) == (4, 10, 5.991, 3, 10)
    for k in ("est", "lam", "nu", "chi2"):
        assert np.array_equal(f64bits(a[k]), f64bits(b[k])), k
    assert np.array_equal(f32bits(a["pose"]), f32bits(b["pose"])) and np.array_equal(a["mask"], b["mask"])


def test_context_reuse_after_a_larger_call(pkg, ctx):
    big = Cs.case("m4096")
    first = ctx.pnp_solver(big["Xw"], big["obs"], big["K4"], big["Tcw_in"])
    for name in ("m9", "clean_300"):
        c = Cs.case(name)
        assert_equals_model(ctx.pnp_solver(c["Xw"], c["obs"], c["K4"], c["Tcw_in"]), Cs.model(name), name, debug=False)
    again = ctx.pnp_solver(big["Xw"], big["obs"], big["K4"], big["Tcw_in"])
    assert np.array_equal(f32bits(first["pose"]), f32bits(again["pose"])) and np.array_equal(first["mask"], again["mask"])


# ---------------------------------------------------------------- C++ surface
@pytest.mark.parametrize("as_written", [0, 1])
def test_cpp_pnp_solver_example(pkg, tmp_path, as_written):
    exe = os.path.join(ROOT, "rgbd-slam_amd", "build", "pnp_solver_example")
    assert os.path.exists(exe), "build() must compile examples/pnp_solver_example.cpp"
    bgr, depth, gt, cam = synth_seq(4, seed=3, preset="fr1")
    raw = tmp_path / "pair.raw"
    with open(raw, "wb") as f:
        for i in range(2):
            f.write(np.ascontiguousarray(bgr[i]).tobytes())
            f.write(np.ascontiguousarray(depth[i]).tobytes())
    args = [exe, str(raw)] + ["%r" % float(cam[k]) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "factor")]
    out = subprocess.run(args + ["5.0", str(as_written)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[0].split()[0] == "1"   # RansacSE3 tracked the pair
    hexpose = lambda l: np.array([int(v, 16) for v in l.split()[1:]], np.uint32).view(np.float32).reshape(4, 4)
    guess = hexpose(lines[1])
    n = int(lines[2].split()[1])
    rows = np.array([[float(v) for v in l.split()] for l in lines[3:3 + n]])
    assert lines[3 + n].split() == ["solver", "1"]
    pose = hexpose(lines[4 + n])
    ni = int(lines[5 + n].split()[1])
    inl = np.array([[float(v) for v in l.split()] for l in lines[6 + n:6 + n + ni]])
    flagged = int(lines[6 + n + ni].split()[1])
    # the Python path on the same frames and matches
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"],
                   cam["factor"])
    ctx = pkg.Context(640, 480, max_batch=1, orb=pkg.orb_params(1000), cam=c)
    fr = [ctx.frame(bgr[i], depth[i]) for i in range(2)]
    qi, ti = rows[:, 0].astype(int), rows[:, 1].astype(int)
    if as_written:
        Xw = np.stack([chain_model.unproject_world(guess, fr[1]["xyz"][j]) for j in ti])
    else:
        Xw = np.stack([chain_model.unproject_world(np.eye(4, dtype=np.float32), fr[0]["xyz"][i]) for i in qi])
    ku = fr[1]["kps_un"][ti]
    K4 = np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], np.float32)
    want = ctx.pnp_solver(Xw, np.stack([ku["x"], ku["y"]], 1), K4, guess)
    ctx.close()
    assert n > 150 and want["ok"]
    assert np.array_equal(f32bits(pose), f32bits(want["pose"]))
    keep = np.nonzero(want["mask"] == 0)[0]
    keep = keep[np.argsort(ti[keep], kind="stable")]   # ascending trainIdx, not match order
    assert ni == len(keep) == want["n_inliers"] and flagged == n - ni
    assert np.array_equal(inl, rows[keep])
    assert not np.array_equal(keep, np.sort(keep)), "the matches are in query order: the two orders must differ here"
