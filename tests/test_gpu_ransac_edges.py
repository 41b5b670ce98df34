"""GPU parity: RansacSE3::compute on gfx950 in the edge regimes of tests/ransac_se3_cases.py
(tests/test_ransac_se3_cases.py asserts on the CPU that each case reaches its regime) vs the oracle
(oracle/orc_solver.cpp), by tests/test_gpu_ransac.py's _compare: ok, the transform's and rmse's f32 bits, the inlier
list, the RNG state afterwards, the sticky covariance and the F2 flags, all exact.  One context for the module, so the
workspace grows and is reused across the calls.  The refusals (more than 2304 matches, sample_size > 8, a match
index out of range) have no counterpart in the oracle: they are held to the contract of csrc/solver.cpp."""
import ctypes as C
import functools

import numpy as np
import pytest

import ransac_se3_cases as E
from test_gpu_ransac import _compare, _ransac_raw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(640, 480, max_batch=1)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def case(name):
    return E.case(name)


def compare_case(pkg, oracle, ctx, name, iterations=None):
    xyz1, xyz2, m, prm, seed, sticky, update_f2 = case(name)
    if iterations is not None:
        prm = (iterations,) + prm[1:]
    return _compare(pkg, oracle, ctx, xyz1, xyz2, m, seed, sticky_cov=sticky, prm_args=prm,
                    update_f2=update_f2 != 0, flags2=update_f2 is not None)


def small_problem():
    P = E.frustum(40, np.random.default_rng(40))
    return E.matched(P, E.moved(P), np.random.default_rng(41))


def test_workspace_grows_and_is_reused(pkg, oracle, ctx):
    """40 matches, then 2304 with 1000 iterations (past the workspace's first 1024 matches and 256 hypotheses), then
    the 40 again over the large call's leftovers."""
    xyz1, xyz2, m = small_problem()
    first = _compare(pkg, oracle, ctx, xyz1, xyz2, m, 3)
    assert first[0] and first[2] == 40
    ok, _, n = compare_case(pkg, oracle, ctx, "contam_2304", iterations=1000)
    assert ok and n >= 10
    again = _compare(pkg, oracle, ctx, xyz1, xyz2, m, 3)
    assert again[0] and again[2] == 40 and np.array_equal(first[1], again[1])


@pytest.mark.parametrize("name", E.NAMES)
def test_ransac_edge_case_matches_oracle(pkg, oracle, ctx, name):
    compare_case(pkg, oracle, ctx, name)


def refused_call(pkg, ctx, xyz1, xyz2, m, prm):
    """A call that must be refused: (status, whether anything it was handed changed, k_ransac_hyp launched)."""
    rng, st = pkg.Rng(), pkg.Sticky()
    pkg.lib().rgbd_rng_seed(C.byref(rng), 7)
    st.cov, st.set = 2.5e-4, 1
    flags = np.full(len(xyz2), 3, np.uint8)
    T, inl = np.full(16, 7.0, np.float32), np.zeros(len(m), pkg.DMATCH_DTYPE)
    inl["queryIdx"] = -5
    n_in, ok, rm = C.c_int32(-1), C.c_int32(-1), C.c_float(-2.0)
    before = [bytes(rng), bytes(st), flags.tobytes(), T.tobytes(), inl.tobytes(), xyz1.tobytes(), xyz2.tobytes(), m.tobytes()]
    ctx.set_timing(True)
    ctx.reset_timing()
    status = _ransac_raw(pkg, ctx, xyz1, xyz2, m, prm, rng, st, 1, flags, T, inl, n_in, rm, ok)
    launched = "k_ransac_hyp" in ctx.timings()
    ctx.set_timing(False)
    after = [bytes(rng), bytes(st), flags.tobytes(), T.tobytes(), inl.tobytes(), xyz1.tobytes(), xyz2.tobytes(), m.tobytes()]
    untouched = before == after and (n_in.value, ok.value, rm.value) == (-1, -1, -2.0)
    return status, untouched, launched


def test_too_many_matches_refused(pkg, oracle, ctx):
    P = E.frustum(2305, np.random.default_rng(2305))
    xyz1, xyz2, m = E.matched(P, E.moved(P), np.random.default_rng(2306))
    assert refused_call(pkg, ctx, xyz1, xyz2, m, pkg.ransac_params()) == (4, True, False)   # RGBD_ERR_UNSUPPORTED
    assert "2304" in pkg.lib().rgbd_last_error(ctx._h).decode()
    ok, _, n = _compare(pkg, oracle, ctx, xyz1, xyz2, m[:2304], 7)   # the context goes on working, at the capacity
    assert ok and n == 2304


def test_sample_size_nine_refused(pkg, oracle, ctx):
    xyz1, xyz2, m = small_problem()
    assert refused_call(pkg, ctx, xyz1, xyz2, m, pkg.ransac_params(200, 10, 3.0, 9)) == (4, True, False)
    assert "sample_size" in pkg.lib().rgbd_last_error(ctx._h).decode()
    assert _compare(pkg, oracle, ctx, xyz1, xyz2, m, 7, prm_args=(200, 10, 3.0, 8))[0]


def test_timing_sees_an_ordinary_call(pkg, oracle, ctx):
    """The refusal tests' probe: a call that runs does list k_ransac_hyp."""
    xyz1, xyz2, m = small_problem()
    ctx.set_timing(True)
    ctx.reset_timing()
    _compare(pkg, oracle, ctx, xyz1, xyz2, m, 7)
    launched = "k_ransac_hyp" in ctx.timings()
    ctx.set_timing(False)
    assert launched


@pytest.mark.parametrize("field,value", [("trainIdx", 40), ("trainIdx", -1), ("queryIdx", 40), ("queryIdx", -1)])
def test_match_index_out_of_range(pkg, oracle, ctx, field, value):
    xyz1, xyz2, m = small_problem()
    m = m.copy()
    m[field][17] = value
    assert refused_call(pkg, ctx, xyz1, xyz2, m, pkg.ransac_params()) == (1, True, False)   # RGBD_ERR_ARG
    m[field][17] = 0   # in range again (a many-to-one match): the context goes on working
    _compare(pkg, oracle, ctx, xyz1, xyz2, m, 7)
