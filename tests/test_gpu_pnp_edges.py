"""GPU parity: PnPRansac on gfx950 (rgbd_pnp_ransac_batch) in its edge regimes (tests/pnp_edge_cases.py), bit for bit
against the oracle restatement (oracle/orc_pnp.cpp): point counts on the kernels' strides, inliers placed across the
mask passes' waves, iteration counts and best iterations on every hand-over between the device chunks and the host
continuation under the three chunk schedules a context can be steered into, degenerate and non-finite input, every
operator argument.  ok, the inlier count, the iteration count and the mask always; the f64 bits of R and t when ok;
identity, zero and an empty mask when not."""
import ctypes as C

import numpy as np
import pytest

import pnp_edge_cases as E
from pnp_cases import K_TUM

pytestmark = pytest.mark.gpu

_WANT = {}


def _want(oracle, name):
    """The oracle's answer for a named case, computed once."""
    if name not in _WANT:
        p3, p2, prm = E.tiny(int(name[5:])) if name.startswith("tiny_") else E.case(name)
        _WANT[name] = (p3, p2, prm, E.expected(oracle, p3, p2, prm))
    return _WANT[name]


def _check(res, want, what=""):
    ok, R, t, mask, ni, it = want
    assert res["ok"] == ok, what
    assert res["n_inliers"] == ni, what
    assert res["iters"] == it, what
    assert np.array_equal(res["mask"], mask), what
    if ok:
        assert np.array_equal(res["R"].view(np.uint64), R.view(np.uint64)), (what, res["R"] - R)
        assert np.array_equal(res["t"].view(np.uint64), t.view(np.uint64)), (what, res["t"] - t)
    else:
        assert ni == 0 and not mask.any()
        assert np.array_equal(res["R"].view(np.uint64), np.eye(3).view(np.uint64)), what
        assert np.array_equal(res["t"].view(np.uint64), np.zeros(3).view(np.uint64)), what


def _bytes(res):
    return [(r["ok"], r["n_inliers"], r["iters"], r["mask"].tobytes(), r["R"].tobytes(), r["t"].tobytes()) for r in res]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(640, 480, max_batch=1)
    yield c
    c.close()


def _context_in(pkg, schedule):
    """A fresh context steered into `schedule` the way production gets there: by a preceding solve."""
    c = pkg.Context(640, 480, max_batch=1)
    assert c.debug_pnp_chunks() == (8, 16)
    batch = E.prime(schedule)
    if batch:
        c.pnp_ransac_batch(batch, K_TUM, pkg.pnp_params(min_matches=0))
    assert c.debug_pnp_chunks() == schedule
    return c


# ------------------------------------------------------------------ every case alone
@pytest.mark.parametrize("name", E.NAMES)
def test_case_matches_oracle(pkg, oracle, ctx, name):
    p3, p2, prm, want = _want(oracle, name)
    _check(ctx.pnp_ransac(p3, p2, K_TUM, pkg.pnp_params(**prm)), want, name)


def test_all_sizes_in_one_batch(pkg, oracle, ctx):
    probs = [_want(oracle, n) for n in E.SIZE_NAMES]
    res = ctx.pnp_ransac_batch([(p3, p2) for p3, p2, _, _ in probs], K_TUM, pkg.pnp_params(min_matches=0))
    for name, (_, _, _, want), r in zip(E.SIZE_NAMES, probs, res):
        _check(r, want, name)


# ------------------------------------------------------------------ the chunk schedules
@pytest.mark.parametrize("schedule", list(E.SCHEDULES), ids=lambda s: "%d_%d" % s)
def test_schedule_boundaries_match_oracle(pkg, oracle, schedule):
    """One batch on a context in `schedule`: a problem whose loop ends on each hand-over between chunks and one
    past it, problems whose best model is a chunk's last or the next one's first, an empty, a 4-point and a 5-point
    problem between them and a 4096-point problem.  The host continuation ran (a third k_pnp_hyp launch) exactly
    when a problem's iteration count exceeds the two device chunks."""
    names = E.schedule_names(schedule)
    for at, tiny in ((3, "tiny_0"), (7, "tiny_4"), (11, "tiny_5")):
        names.insert(at, tiny)
    names.append("size_4096")
    assert all(_want(oracle, n)[2] == E.DEFAULTS for n in names)
    c = _context_in(pkg, schedule)
    c.set_timing(True)
    c.reset_timing()
    res = c.pnp_ransac_batch([_want(oracle, n)[:2] for n in names], K_TUM, pkg.pnp_params(min_matches=0))
    launches = c.timings()["k_pnp_hyp"][1]
    c.close()
    for n, r in zip(names, res):
        _check(r, _want(oracle, n)[3], n)
    assert max(_want(oracle, n)[3][5] for n in names) > sum(schedule)   # some problem needs the host
    assert launches > 2


@pytest.mark.parametrize("name", E.FORCED_NAMES)
def test_forced_iteration_counts_on_a_fresh_context(pkg, oracle, name):
    """No model is ever accepted, so exactly the iteration cap runs: 8 ends with the first chunk of (8, 16), 24
    with the second, 25 takes one host round of a single hypothesis."""
    p3, p2, prm, want = _want(oracle, name)
    c = _context_in(pkg, (8, 16))
    c.set_timing(True)
    c.reset_timing()
    r = c.pnp_ransac(p3, p2, K_TUM, pkg.pnp_params(**prm))
    launches = c.timings()["k_pnp_hyp"][1]
    c.close()
    _check(r, want, name)
    assert (launches > 2) == (want[5] > 24) and launches == (3 if want[5] > 24 else 2)


@pytest.mark.parametrize("schedule", list(E.SCHEDULES), ids=lambda s: "%d_%d" % s)
def test_host_continuation_runs_only_past_the_device_chunks(pkg, oracle, schedule):
    """No problem of the batch runs past K0 + K1 iterations: two k_pnp_hyp launches, no host round."""
    k0, k1 = schedule
    names = [n for n in E.ITER_NAMES + E.BEST_NAMES if _want(oracle, n)[3][5] <= k0 + k1]
    assert any(_want(oracle, n)[3][5] == k0 + k1 for n in names) and any(_want(oracle, n)[3][5] > k0 for n in names)
    c = _context_in(pkg, schedule)
    c.set_timing(True)
    c.reset_timing()
    res = c.pnp_ransac_batch([_want(oracle, n)[:2] for n in names], K_TUM, pkg.pnp_params(min_matches=0))
    assert c.timings()["k_pnp_hyp"][1] == 2
    c.close()
    for n, r in zip(names, res):
        _check(r, _want(oracle, n)[3], n)


def test_results_do_not_depend_on_the_schedule(pkg, oracle):
    """The same 12 problems (under each schedule one ends in the second device chunk and one in the host
    continuation) on contexts in the three schedules and one by one: the same bytes, the oracle's."""
    probs = [_want(oracle, n)[:2] for n in E.INDEPENDENCE]
    prm = pkg.pnp_params(min_matches=0)
    got = {}
    for schedule in E.SCHEDULES:
        c = _context_in(pkg, schedule)
        got[schedule] = c.pnp_ransac_batch(probs, K_TUM, prm)
        c.close()
    c = pkg.Context(640, 480, max_batch=1)
    alone = [c.pnp_ransac(p3, p2, K_TUM, prm) for p3, p2 in probs]
    c.close()
    for n, r in zip(E.INDEPENDENCE, alone):
        _check(r, _want(oracle, n)[3], n)
    for schedule in E.SCHEDULES:
        assert _bytes(got[schedule]) == _bytes(alone), schedule


@pytest.mark.parametrize("P", [1, 2, 3, 5, 7])
@pytest.mark.parametrize("schedule", list(E.SCHEDULES), ids=lambda s: "%d_%d" % s)
def test_wave_tail_groups(pkg, oracle, schedule, P):
    """P x K0 hypotheses that do not fill their last wave of five ((4, 4), P = 1: one wave of four)."""
    names = E.WAVE_TAIL[:P]
    c = _context_in(pkg, schedule)
    res = c.pnp_ransac_batch([_want(oracle, n)[:2] for n in names], K_TUM, pkg.pnp_params(min_matches=0))
    c.close()
    for n, r in zip(names, res):
        _check(r, _want(oracle, n)[3], n)


# ------------------------------------------------------------------ limits
def _raw_batch(pkg, c, counts, npts, prm):
    """rgbd_pnp_ransac_batch on sentinel-filled outputs: (status, the outputs, their copies from before)."""
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    counts = np.array(counts, np.int32)
    p3, p2 = np.ones((max(npts, 1), 3), np.float32), np.ones((max(npts, 1), 2), np.float32)
    P = len(counts)
    outs = [np.full((max(P, 1), 9), 7.0), np.full((max(P, 1), 3), 7.0), np.full(max(npts, 1), 9, np.uint8),
            np.full(max(P, 1), -5, np.int32), np.full(max(P, 1), -5, np.int32), np.full(max(P, 1), -5, np.int32)]
    before = [a.copy() for a in outs]
    K4 = np.ascontiguousarray(K_TUM, np.float32)
    st = pkg.lib().rgbd_pnp_ransac_batch(c._h, P, ptr(counts), ptr(p3), ptr(p2), ptr(K4), C.byref(prm),
                                         *[ptr(a) for a in outs])
    return st, outs, before


def test_limits(pkg, oracle, ctx):
    prm = pkg.pnp_params(min_matches=0)
    ctx.set_timing(True)
    try:
        for counts in ([4097], [30, 4097]):
            ctx.reset_timing()
            st, outs, before = _raw_batch(pkg, ctx, counts, sum(counts), prm)
            assert st == 4 and "4096" in pkg.lib().rgbd_last_error(ctx._h).decode()
            assert all(np.array_equal(a, b) for a, b in zip(outs, before))
            assert not [k for k in ctx.timings() if k.startswith("k_pnp_")]
        st, outs, before = _raw_batch(pkg, ctx, [30, -1], 30, prm)
        assert st == 1 and all(np.array_equal(a, b) for a, b in zip(outs, before))
        st, outs, before = _raw_batch(pkg, ctx, [], 0, prm)   # no problem at all
        assert st == 0 and all(np.array_equal(a, b) for a, b in zip(outs, before))
        assert ctx.pnp_ransac_batch([], K_TUM, prm) == []
    finally:
        ctx.set_timing(False)
    p3, p2, _, want = _want(oracle, "size_4096")   # the context serves the next call
    _check(ctx.pnp_ransac(p3, p2, K_TUM, prm), want)
    with pytest.raises(pkg.RgbdError, match="4096"):
        ctx.pnp_ransac(np.zeros((4097, 3), np.float32), np.zeros((4097, 2), np.float32), K_TUM, prm)
