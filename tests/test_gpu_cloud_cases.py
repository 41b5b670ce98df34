"""cloud.hip in its edge regimes (tests/cloud_cases.py; each regime is asserted on the CPU by
test_cloud_cases.py) against the oracle, every point bit-identical: the u16 and f32 depth entries, the batch
entry, workspace regrowth, and the error returns."""
import ctypes as C

import numpy as np
import pytest

import cloud_cases as cc

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = 0, 1, 3, 4


def _cam(pkg, cam):
    return pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"],
                      cam["k3"], cam["factor"])


def _ctx128(pkg, B=1):
    return pkg.Context(cc.W, cc.H, max_batch=B, orb=pkg.orb_params(1000, 1.2, 1), cam=_cam(pkg, cc.CAM))


@pytest.fixture(scope="module")
def ctx(pkg):
    c = _ctx128(pkg, 3)
    yield c
    c.close()


def _same(got, want, what=""):
    assert got.dtype == want.dtype
    assert len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.view(np.uint8).reshape(-1, 16) != want.view(np.uint8).reshape(-1, 16))
        i = int(bad[0]) // 16
        raise AssertionError(f"{what}: point {i} of {len(want)} differs: {got[i]} vs {want[i]}")


_WANT = {}


def _want(oracle, key, bgr, depth, kw):
    """The oracle's cloud of an input that is not a named case, computed once per module."""
    if key not in _WANT:
        _WANT[key] = cc.stages(oracle, bgr, depth, cc.CAM, kw)["out"]
    return _WANT[key]


def _frames3():
    """Three frames with about 60 % invalid pixels (keeps the oracle's SOR at stride 1 short)."""
    bgr = np.stack([cc.random_bgr(30 + i) for i in range(3)])
    depth = np.stack([cc.random_depth(40 + i, zeros=0.6) for i in range(3)])
    return bgr, depth


@pytest.mark.parametrize("name", cc.NAMES)
def test_case_bit_exact(pkg, oracle, ctx, name):
    bgr, depth, _, kw = cc.case(name)
    want = cc.case_stages(oracle, name)["out"]
    prm = pkg.cloud_params(**kw)
    got = ctx.keyframe_cloud(bgr, depth, prm)   # an error status raises
    _same(got, want, name + " (u16 depth)")
    got32 = ctx.keyframe_cloud_f32(bgr, cc.depth_f32(depth), prm)
    _same(got32, want, name + " (f32 depth)")
    if name.startswith("empty"):
        assert len(got) == 0 and len(got32) == 0


def test_f32_specials(pkg, oracle, ctx):
    """Non-finite and non-positive pixels of Frame::mImDepth are skipped like a zero depth."""
    bgr = cc.random_bgr(50)
    depth = cc.random_depth(51)
    kw = dict(cc.DEFAULTS, stride=2)
    dimg = cc.depth_f32(depth)
    specials = [np.nan, np.inf, -1.0, -0.0, 0.0, 1e-40]
    assert 0 < np.float32(1e-40) < np.finfo(np.float32).tiny   # a positive subnormal
    rs = np.random.default_rng(52)
    at = rs.choice((cc.H // 2) * (cc.W // 2), size=10 * len(specials), replace=False)
    zeroed = depth.copy()
    for i, s in enumerate(at):
        r, c = 2 * (int(s) // (cc.W // 2)), 2 * (int(s) % (cc.W // 2))
        dimg[r, c] = specials[i % len(specials)]
        zeroed[r, c] = 0
    dimg[1::2, :] = np.nan   # off the sample grid: never read
    dimg[:, 1::2] = -np.inf
    assert np.all(depth > 0) and int(np.sum(zeroed == 0)) == len(at)   # every special replaces a valid pixel
    want = _want(oracle, "specials", bgr, zeroed, kw)
    got = ctx.keyframe_cloud_f32(bgr, dimg, pkg.cloud_params(**kw))
    _same(got, want, "f32 specials")
    _same(ctx.keyframe_cloud(bgr, zeroed, pkg.cloud_params(**kw)), want, "u16 zeroed")


def test_batch_repeated_index_and_empty_list(pkg, oracle, ctx):
    import torch
    bgr, depth = _frames3()
    kw = dict(cc.DEFAULTS, stride=2)
    prm = pkg.cloud_params(**kw)
    d_bgr = torch.from_numpy(bgr).cuda()
    d_dep = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda()
    torch.cuda.synchronize()
    frames = [2, 2, 0]
    got = ctx.keyframe_cloud_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 3, frames, prm, W=cc.W, H=cc.H)
    assert len(got) == 3
    for k, f in enumerate(frames):
        want = _want(oracle, ("f3s2", f), bgr[f], depth[f], kw)
        assert len(want) > 100
        _same(got[k], want, f"batch slot {k} (frame {f})")
    assert ctx.keyframe_cloud_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 3, [], prm, W=cc.W, H=cc.H) == []
    for bad in ([3], [0, -1], [1, 2, 3]):
        with pytest.raises(pkg.RgbdError, match=r"outside the batch \(status 1\)"):
            ctx.keyframe_cloud_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 3, bad, prm, W=cc.W, H=cc.H)


def test_workspace_regrowth(pkg, oracle):
    """ws_get on one context: a small capacity, a larger one, more keyframes, the small capacity again."""
    import torch
    bgr, depth = _frames3()
    k6, k1 = dict(cc.DEFAULTS, stride=6), dict(cc.DEFAULTS, stride=1)
    want6 = _want(oracle, ("f3s6", 0), bgr[0], depth[0], k6)
    want1 = [_want(oracle, ("f3s1", f), bgr[f], depth[f], k1) for f in range(3)]
    assert 10 < len(want6) < 484 and all(len(w) > 484 for w in want1)
    c = _ctx128(pkg, 3)
    try:
        _same(c.keyframe_cloud(bgr[0], depth[0], pkg.cloud_params(**k6)), want6, "stride 6")
        _same(c.keyframe_cloud(bgr[0], depth[0], pkg.cloud_params(**k1)), want1[0], "stride 1")
        d_bgr = torch.from_numpy(bgr).cuda()
        d_dep = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda()
        torch.cuda.synchronize()
        got = c.keyframe_cloud_batch(d_bgr.data_ptr(), d_dep.data_ptr(), 3, [0, 1, 2], pkg.cloud_params(**k1),
                                     W=cc.W, H=cc.H)
        for f in range(3):
            _same(got[f], want1[f], f"stride-1 batch, frame {f}")
        _same(c.keyframe_cloud(bgr[0], depth[0], pkg.cloud_params(**k6)), want6, "stride 6 again")
    finally:
        c.close()


def _raw_cloud(pkg, c, bgr, depth, prm, cap):
    out = np.zeros(max(cap, 1), pkg.POINT_DTYPE)
    n = C.c_int32(-7)
    st = pkg.lib().rgbd_keyframe_cloud(c._h, pkg._ptr(bgr), pkg._ptr(depth), C.byref(prm), pkg._ptr(out), cap,
                                       C.byref(n))
    return st, n.value, out


def test_errors(pkg, oracle, ctx):
    bgr, depth, _, kw = cc.case("k1")
    want = cc.case_stages(oracle, "k1")["out"]
    ctx.set_timing(True)
    ctx.reset_timing()
    try:
        for bad in (dict(sor_k=0), dict(sor_k=64), dict(sor_k=-1), dict(leaf=0.0), dict(leaf=-0.04),
                    dict(leaf=float("nan")), dict(stride=0), dict(stride=-2)):
            st, _, _ = _raw_cloud(pkg, ctx, bgr, depth, pkg.cloud_params(**dict(kw, **bad)), 16384)
            assert st == ERR_ARG, bad
            assert b"cloud params" in pkg.lib().rgbd_last_error(ctx._h)
        assert "k_cloud" not in ctx.timings()   # nothing was launched
        # an output one point too small: the status says so and the count is still the true one
        st, n, out = _raw_cloud(pkg, ctx, bgr, depth, pkg.cloud_params(**kw), len(want) - 1)
        assert st == ERR_CAPACITY and n == len(want)
        assert out.tobytes() == want[:len(want) - 1].tobytes()
        st, n, out = _raw_cloud(pkg, ctx, bgr, depth, pkg.cloud_params(**kw), len(want))
        assert st == OK and n == len(want) and out.tobytes() == want.tobytes()
        assert ctx.timings()["k_cloud"][1] == 2
    finally:
        ctx.set_timing(False)
        ctx.reset_timing()


def test_too_many_samples(pkg, oracle):
    """Stride 4 at 640 x 480 is 19200 samples, above the 16384 that the 14-bit point index of the sort key holds."""
    c = pkg.Context(640, 480, max_batch=1)
    try:
        bgr = np.random.default_rng(60).integers(0, 256, size=(480, 640, 3), dtype=np.uint8)
        depth = np.full((480, 640), 5000, np.uint16)
        c.set_timing(True)
        st, _, _ = _raw_cloud(pkg, c, bgr, depth, pkg.cloud_params(stride=4), 19200)
        assert st == ERR_UNSUPPORTED
        assert b"16384" in pkg.lib().rgbd_last_error(c._h)
        assert "k_cloud" not in c.timings()   # nothing was launched
        with pytest.raises(pkg.RgbdError, match=r"16384 samples.*\(status 4\)"):
            c.keyframe_cloud_f32(bgr, depth.astype(np.float32), pkg.cloud_params(stride=4))
        # stride 5 is 128 x 96 = 12288 samples: the same context takes it
        cam = dict(cc.CAM, fx=535.4, fy=539.2, cx=320.1, cy=247.6)   # Context's default camera
        want = cc.stages(oracle, bgr, depth, cam, dict(cc.DEFAULTS, stride=5))["out"]
        assert len(want) > 100
        _same(c.keyframe_cloud(bgr, depth, pkg.cloud_params(stride=5)), want, "stride 5 after the refusal")
    finally:
        c.close()
