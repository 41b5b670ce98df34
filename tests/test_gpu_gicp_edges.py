"""GPU parity: GICP on gfx950 in the edge regimes of tests/gicp_edge_cases.py (tests/test_gicp_edge_cases.py
asserts on the CPU that each case reaches its regime) vs the oracle (oracle/orc_gicp.cpp).  Bit-exact: the final
transformation (f32 bits), the convergence flag, the iterations, and through rgbd_debug_gicp_cov the covariance
of every point of either cloud (f64 bits), also of the points no correspondence ever uses."""
import ctypes as C
import functools

import numpy as np
import pytest

import gicp_edge_cases as E

pytestmark = pytest.mark.gpu

EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(640, 480, max_batch=1)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def case(name):
    return E.case(name)


@functools.lru_cache(maxsize=None)
def want(name):
    import oracle_lib
    _, P, Q, guess, prm = case(name)
    return oracle_lib.gicp(P, Q, guess, E.make_params(oracle_lib, prm))


def assert_align_matches(pkg, ctx, name, ref=None):
    _, P, Q, guess, prm = case(name)
    conv, Tg, it = ctx.gicp(P, Q, guess, E.make_params(pkg, prm))
    oconv, To, oit, _ = ref or want(name)
    assert (conv, it) == (oconv, oit)
    assert np.array_equal(Tg.view(np.uint32), To.view(np.uint32)), np.abs(Tg - To).max()


@pytest.mark.parametrize("name", E.NAMES)
def test_gicp_edge_case_matches_oracle(pkg, oracle, ctx, name):
    assert_align_matches(pkg, ctx, name)


@pytest.mark.parametrize("name", E.NAMES)
def test_gicp_covariances_match_oracle(pkg, oracle, ctx, name):
    _, P, Q, _, prm = case(name)
    k, eps = prm["k_correspondences"], prm["gicp_epsilon"]
    for pts in (P, Q):
        ok, Co = oracle.gicp_covariances(pts, k, eps)
        if not ok:   # PCL refuses fewer points than neighbours
            with pytest.raises(pkg.RgbdError, match="status 4"):
                ctx.debug_gicp_cov(pts, k, eps)
            continue
        Cg = ctx.debug_gicp_cov(pts, k, eps)
        bad = np.nonzero((Cg.view(np.uint64) != Co.view(np.uint64)).any(axis=(1, 2)))[0]
        assert len(bad) == 0, (bad[:8], np.abs(Cg - Co).max())


def test_gicp_compute_on_edges(pkg, oracle, ctx):
    problems = [case(n)[1:] for n in ("four_eq", "four_below", "all_identical")]
    _, P, Q, guess, prm = case("size_63")
    problems.append((P[:19], Q[:19], guess, prm))   # Gicp::compute's own 20-pair rule
    for P, Q, guess, prm in problems:
        ok, Tg = ctx.gicp_compute(P, Q, guess, E.make_params(pkg, prm))
        ook, To = oracle.gicp_compute(P, Q, guess, E.make_params(oracle, prm))
        assert ok == ook
        assert np.array_equal(Tg.view(np.uint32), To.view(np.uint32))


def test_workspace_reuse(pkg, oracle):
    """A small problem over a large one's leftovers (keys, LDS-staged points, covariances, M_i scratch of the
    2043-point problem) gives what it gives on a fresh context."""
    def results(c, name):
        _, P, Q, guess, prm = case(name)
        conv, T, it = c.gicp(P, Q, guess, E.make_params(pkg, prm))
        cov = c.debug_gicp_cov(Q, prm["k_correspondences"], prm["gicp_epsilon"])
        return conv, it, T.tobytes(), cov.tobytes()

    fresh = {}
    for name in ("rounds_nc32", "size_63", "M1_k1"):
        c = pkg.Context(640, 480, max_batch=1)
        fresh[name] = results(c, name)
        c.close()
    c = pkg.Context(640, 480, max_batch=1)
    for name in ("rounds_nc32", "size_63", "M1_k1", "size_63"):
        assert results(c, name) == fresh[name], name
    c.close()
    assert fresh["size_63"][0] and not fresh["M1_k1"][0]


def test_error_returns(pkg, ctx):
    lib, h = pkg.lib(), ctx._h
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    big = np.zeros((2049, 3), np.float32)
    guess, T = EYE.copy(), np.full(16, 7.0, np.float32)
    cv, it = C.c_int32(-1), C.c_int32(-1)

    def gicp(src, tgt, M, g, prm, Tp, cvp):
        return lib.rgbd_gicp(h, src, tgt, M, g, C.byref(prm), Tp, cvp, C.byref(it))

    prm = pkg.gicp_params()
    assert gicp(ptr(big), ptr(big), 2049, ptr(guess), prm, ptr(T), C.byref(cv)) == 4      # RGBD_ERR_UNSUPPORTED
    for k in (0, 33):
        bad = pkg.gicp_params()
        bad.k_correspondences = k
        assert gicp(ptr(big), ptr(big), 100, ptr(guess), bad, ptr(T), C.byref(cv)) == 4
    assert gicp(ptr(big), ptr(big), -1, ptr(guess), prm, ptr(T), C.byref(cv)) == 1         # RGBD_ERR_ARG
    assert gicp(ptr(big), ptr(big), 100, None, prm, ptr(T), C.byref(cv)) == 1
    assert gicp(ptr(big), ptr(big), 100, ptr(guess), prm, None, C.byref(cv)) == 1
    assert gicp(ptr(big), ptr(big), 100, ptr(guess), prm, ptr(T), None) == 1
    assert gicp(None, ptr(big), 100, ptr(guess), prm, ptr(T), C.byref(cv)) == 1
    assert gicp(None, None, 0, ptr(guess), prm, ptr(T), C.byref(cv)) == 0                   # empty clouds: RGBD_OK
    assert cv.value == 0 and it.value == 0 and np.array_equal(T.reshape(4, 4), EYE)

    cov = np.zeros((2049, 9))
    dbg = lib.rgbd_debug_gicp_cov
    assert dbg(h, ptr(big), 2049, 20, 1e-3, ptr(cov)) == 4
    assert dbg(h, ptr(big), 100, 0, 1e-3, ptr(cov)) == 4 and dbg(h, ptr(big), 100, 33, 1e-3, ptr(cov)) == 4
    assert dbg(h, ptr(big), 19, 20, 1e-3, ptr(cov)) == 4
    assert dbg(h, None, 100, 20, 1e-3, ptr(cov)) == 1 and dbg(h, ptr(big), 100, 20, 1e-3, None) == 1
    assert dbg(h, ptr(big), -1, 20, 1e-3, ptr(cov)) == 1
    assert not cov.any()   # nothing written by a refused call
