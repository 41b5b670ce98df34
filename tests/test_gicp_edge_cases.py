"""CPU: every case of tests/gicp_edge_cases.py reaches the regime of csrc/gicp.hip it is named after, asserted
from the oracle (oracle/orc_gicp.cpp) and the path model (tests/gicp_path_model.py) alone, so that the device
parity of tests/test_gpu_gicp_edges.py pins those regimes; the oracle's covariances against the independent
numpy formulation; the grid's 27-cell argument against brute force in float32."""
import functools

import numpy as np
import pytest

import gicp_edge_cases as E
import gicp_path_model as Mo
from gicp_cases import np_covariances

F = np.float32
EYE = np.eye(4, dtype=F)


@functools.lru_cache(maxsize=None)
def case(name):
    return E.case(name)


@functools.lru_cache(maxsize=None)
def _run(name):
    import oracle_lib
    _, P, Q, guess, prm = case(name)
    return oracle_lib.gicp(P, Q, guess, E.make_params(oracle_lib, prm))


@pytest.fixture
def run(oracle):
    return _run


def cov(oracle, pts, prm):
    ok, C = oracle.gicp_covariances(pts, prm["k_correspondences"], prm["gicp_epsilon"])
    assert ok
    return C


def test_names_unique_and_sizes_supported():
    assert len(set(E.NAMES)) == len(E.NAMES)
    for name in E.NAMES:
        _, P, Q, guess, prm = case(name)
        assert P.shape == Q.shape and P.dtype == Q.dtype == guess.dtype == F and 1 <= len(P) <= 2048
        assert np.isfinite(P).all() and np.isfinite(Q).all() and 1 <= prm["k_correspondences"] <= 32


@pytest.mark.parametrize("name", E.NAMES)
def test_oracle_well_posed(run, name):
    conv, T, it, nc = run(name)
    assert np.isfinite(T).all() and 0 <= it <= case(name)[4]["max_iterations"]
    if not conv:
        assert np.array_equal(T, EYE)


@pytest.mark.parametrize("nc", list(E.ROUNDS_L))
def test_rounds_cases_take_both_knn_paths(nc):
    _, P, Q, _, prm = case("rounds_nc%d" % nc)
    assert E.ROUNDS_L[nc] < prm["k_correspondences"]   # t is a far key: the whole cluster survives
    for pts in (P, Q):
        got_nc, n_rounds, n_threshold, max_total = Mo.knn_paths(pts, prm["k_correspondences"])
        assert got_nc == nc and n_rounds >= 64 and n_threshold >= 64 and max_total > 64


@pytest.mark.parametrize("total", [64, 65])
def test_total_cases_sit_on_the_path_switch(total):
    _, P, Q, _, prm = case("total_%d" % total)
    for pts in (P, Q):
        t = Mo.knn_totals(pts, prm["k_correspondences"])
        assert t.max() == total and int((t == total).sum()) == total - 1   # the cluster's points
        assert int((t > 64).sum()) == (0 if total == 64 else 64)


@pytest.mark.parametrize("n", list(E.SIZE_NC))
def test_size_cases(run, n):
    _, P, Q, _, prm = case("size_%d" % n)
    assert len(P) == n
    assert Mo.knn_paths(P, 20)[0] == Mo.knn_paths(Q, 20)[0] == E.SIZE_NC[n]
    assert run("size_%d" % n)[0]


def test_dup_pairs_have_zero_distance_neighbours():
    _, P, Q, _, _ = case("dup_pairs")
    for pts in (P, Q):
        d = Mo.dist2f(pts[:, None, :], pts[None, :, :])
        np.fill_diagonal(d, 1.0)
        assert (d.min(axis=1) == 0).all()


def test_dup_block25_is_the_zero_matrix_svd(oracle):
    _, P, Q, _, prm = case("dup_block25")
    for pts in (P, Q):
        assert (pts[40:65] == pts[40]).all()
        C = cov(oracle, pts, prm)[40:65]
        assert np.array_equal(C, np.broadcast_to(np.diag([1.0, 1.0, prm["gicp_epsilon"]]), C.shape))


def test_all_identical(run):
    conv, T, _, nc = run("all_identical")
    assert conv and np.isfinite(T).all() and nc == 30


@pytest.mark.parametrize("name", ["exact_plane", "exact_plane_moved", "exact_line"])
def test_exact_plane_and_line_covariances(oracle, name):
    _, P, Q, _, prm = case(name)
    assert (P[:, 2] == F(2.0)).all() and (name != "exact_line" or (P[:, 1] == F(0.25)).all())
    eps = prm["gicp_epsilon"]
    for pts in (P, Q):
        C = cov(oracle, pts, prm)
        assert np.abs(C - C.transpose(0, 2, 1)).max() <= 1e-9
        w, V = np.linalg.eigh((C + C.transpose(0, 2, 1)) / 2)
        assert np.abs(w - np.array([eps, 1.0, 1.0])).max() <= 1e-9
        if pts is P and name != "exact_line":   # the regularised direction is the plane's normal
            assert np.abs(np.abs(V[:, :, 0]) - np.array([0.0, 0.0, 1.0])).max() <= 1e-9


def test_lattice_cases_tie(run):
    _, P, Q, guess, prm = case("lattice_half")
    assert Mo.nn_ties(P, Q, guess) >= 200
    assert Mo.grid_stats(P, Q, guess, prm["max_corr_dist"]) == (True, 320, 0)
    _, P, Q, guess, prm = case("lattice_half_gridoff")
    assert Mo.nn_ties(P, Q, guess) >= 200
    assert Mo.grid_stats(P, Q, guess, prm["max_corr_dist"]) == (False, 0, 320)
    assert run("lattice_half")[0] and run("lattice_half_gridoff")[0]


def test_full_scan_cases(run):
    _, P, Q, guess, prm = case("small_maxcorr")
    assert not Mo.grid_stats(P, Q, guess, prm["max_corr_dist"])[0] and run("small_maxcorr")[3] >= 4
    _, P, Q, guess, prm = case("query_far_mixed")
    assert Mo.grid_stats(P, Q, guess, prm["max_corr_dist"]) == (True, 298, 2)
    _, P, Q, guess, prm = case("guess_far")
    assert Mo.grid_stats(P, Q, guess, prm["max_corr_dist"]) == (True, 0, 300)
    conv, _, it, _ = run("guess_far")
    assert not conv and it == 0
    _, P, Q, guess, prm = case("maxcorr_zero")
    assert np.isinf(Mo.grid_hinv(0.0)) and not Mo.grid_stats(P, Q, guess, 0.0)[0]
    assert not run("maxcorr_zero")[0]


def test_grid_rim(run):
    hinv = Mo.grid_hinv(0.07)
    _, P, Q, guess, prm = case("grid_rim")
    c, v = Mo.grid_cells(Q[300:], hinv)
    assert [c[0, 0], c[1, 1], c[2, 2]] == [-511.0, 509.0, 510.0] and v.all()   # the range's first and last cells
    cq, vq = Mo.grid_cells(Mo.queries(P, guess)[300:], hinv)
    assert np.array_equal(cq, c) and vq.all()
    assert Mo.grid_stats(P, Q, guess, 0.07) == (True, 303, 0)
    j, _, has = Mo.corr0(P, Q, guess, 0.07)
    assert has[300:].all() and list(j[300:]) == [300, 301, 302]   # found through cells 0 and 1023 of the key
    _, P, Q, guess, prm = case("grid_rim_out")
    c, v = Mo.grid_cells(Q[300:], hinv)
    assert c[3, 0] == 511.0 and not v[3, 0] and v[:3].all()
    assert Mo.grid_stats(P, Q, guess, 0.07) == (False, 0, 304)
    assert run("grid_rim")[0] and run("grid_rim_out")[0]


def test_edge_ring_sits_on_max_corr(oracle):
    _, P, Q, guess, prm = case("edge_ring")
    mc = prm["max_corr_dist"]
    j, bd, has = Mo.corr0(P, Q, guess, mc)
    d = np.sqrt(bd.astype(np.float64))
    assert int((has & (d >= 0.97 * mc)).sum()) >= 10
    assert int((~has & (d < 1.03 * mc)).sum()) >= 10   # and as many just beyond it
    one = dict(prm, max_iterations=1)
    assert oracle.gicp(P, Q, guess, E.make_params(oracle, one))[3] == int(has.sum())   # the model's rule is the oracle's
    # cells smaller than max_corr lose some of these correspondences; the 1.01 cells lose none
    thr = mc * mc
    for margin, lost in ((Mo.CELL_MARGIN, False), (0.9, True)):
        grid = Mo.Grid(Q, mc, margin)
        got = np.array([Mo.device_corr(q, grid, thr) for q in Mo.queries(P, guess)])
        assert (got != np.where(has, j, -1)).any() == lost


def test_four_correspondence_boundary(run):
    for name in ("four_eq", "four_below"):
        _, P, Q, guess, prm = case(name)
        assert prm["max_corr_dist"] ** 2 == 2.0 ** -8
        _, bd, has = Mo.corr0(P, Q, guess, prm["max_corr_dist"])
        assert int(has.sum()) == (3 if name == "four_eq" else 4)
        assert (np.float64(bd[16]) == 2.0 ** -8) == (name == "four_eq")   # the pair that decides
    conv, _, it, nc = run("four_eq")
    assert not conv and it == 0 and nc == 3
    conv, _, it, nc = run("four_below")
    assert conv and it >= 1 and nc == 4


def test_late_abort(run):
    conv, _, it, nc = run("late_abort")
    assert not conv and it >= 1 and nc < 4
    _, P, Q, guess, prm = case("late_abort")
    assert int(Mo.corr0(P, Q, guess, prm["max_corr_dist"])[2].sum()) == 5


def test_k_cases(run, oracle):
    for name, (M, k) in E.K_CASES.items():
        _, P, Q, guess, prm = case(name)
        assert len(P) == M and prm["k_correspondences"] == k
        conv, T, it, _ = run(name)
        if name == "k32_M31":
            assert not conv and it == 0 and np.array_equal(T, EYE)
            assert not oracle.gicp_covariances(P, k)[0]
        else:
            assert np.isfinite(cov(oracle, P, prm)).all() and np.isfinite(cov(oracle, Q, prm)).all()
    assert all(run(n)[0] for n in ("k1", "k2", "k3", "k5", "k32", "k32_M32"))
    assert not run("M1_k1")[0]   # one pair: fewer than four correspondences


def test_parameter_cases(run):
    conv, _, it, _ = run("mi1")
    assert conv and it == 1
    conv, _, it, _ = run("mi3_gn1")
    assert conv and it == 3          # stops on the iteration limit, not on delta
    conv, _, it, _ = run("mi50_gn8")
    assert conv and 1 < it < 50
    conv, T, it, nc = run("gn0")
    assert conv and it == 1 and nc >= 4 and np.array_equal(T, EYE)   # no step: delta 0
    conv, _, it, _ = run("loose_eps")
    assert conv and 1 < it < 50      # stops on delta
    conv, T, it, _ = run("big_rot_guess")
    want = E.big_rot_truth()
    assert conv and np.abs(T[:3, :3] - want[:3, :3]).max() < 5e-3 and np.abs(T[:3, 3] - want[:3, 3]).max() < 5e-3


# cases whose every neighbourhood has a simple smallest covariance eigenvalue (np_covariances is defined there);
# of the rounds_nc cases the points outside the 2 mm cluster, whose eigenvalue gaps are too small for 1e-9
NON_DEGENERATE = (["size_%d" % n for n in E.SIZE_NC] + ["small_maxcorr", "query_far_mixed", "grid_rim", "guess_far",
                  "edge_ring", "k3", "k5", "k32", "k32_M32", "mi1", "big_rot_guess"] +
                  ["rounds_nc%d" % nc for nc in E.ROUNDS_L])


@pytest.mark.parametrize("name", NON_DEGENERATE)
def test_covariances_match_independent(oracle, name):
    _, P, Q, _, prm = case(name)
    k, eps = prm["k_correspondences"], prm["gicp_epsilon"]
    idx = None
    if name.startswith("rounds_nc"):
        nc = int(name[len("rounds_nc"):])
        idx = np.setdiff1d(np.arange(len(P)), E.rounds_cluster(len(P), E.ROUNDS_L[nc]))[::7]
    for pts in (P, Q):
        C = cov(oracle, pts, prm)
        np.testing.assert_allclose(C if idx is None else C[idx], np_covariances(pts, k, eps, idx), atol=1e-9)


@pytest.mark.parametrize("name", [n for n in E.NAMES if n != "k32_M31"])
def test_model_grid_equals_scan_on_every_case(name):
    """The model's device decision (27 cells or full scan) against the oracle's scan at outer iteration 0."""
    _, P, Q, guess, prm = case(name)
    mc = prm["max_corr_dist"]
    j, _, has = Mo.corr0(P, Q, guess, mc)
    grid = Mo.Grid(Q, mc)
    got = np.array([Mo.device_corr(q, grid, mc * mc) for q in Mo.queries(P, guess)])
    assert np.array_equal(got, np.where(has, j, -1))


@pytest.mark.parametrize("mc", [0.01, 0.07, 0.08, 0.3])
def test_grid_argument_against_brute_force(mc):
    """Targets on cell edges +- {0, 1e-6, 1e-3}, queries 0.98 - 1.0001 max_corr from one of them (half of them
    along an axis): the 27 cells of 1.01 max_corr hold every correspondence and the (d, j) minimum among them is
    the scan's.  Cells of 0.9 max_corr do lose some, so the construction does probe the margin."""
    rs = np.random.default_rng(int(mc * 1000))
    h = 1.01 * mc
    nt, nq = 200, 4000
    # on every second edge, so that a query's own target (about max_corr away) is nearer than the next site's
    tgt = (2 * rs.integers(-3, 4, size=(nt, 3)) * h + rs.choice([0, 1e-6, -1e-6, 1e-3, -1e-3], size=(nt, 3))).astype(F)
    d = rs.normal(size=(nq, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    axis = np.zeros((nq // 2, 3))
    axis[np.arange(nq // 2), rs.integers(0, 3, nq // 2)] = rs.choice([-1.0, 1.0], nq // 2)
    d[:nq // 2] = axis
    q = (tgt[rs.integers(0, nt, nq)].astype(np.float64) + d * (rs.uniform(0.98, 1.0001, size=(nq, 1)) * mc)).astype(F)
    thr = np.float64(mc) * np.float64(mc)
    want = []
    for x in q:
        best, bd = Mo.full_nn(x, tgt)
        want.append(best if np.float64(bd) < thr else -1)
    want = np.array(want)
    assert (want >= 0).sum() >= nq // 4 and (want < 0).sum() >= 10
    grid = Mo.Grid(tgt, mc)
    assert grid.ok
    got = np.array([Mo.device_corr(x, grid, thr) for x in q])
    assert int((got != want).sum()) == 0
    small = Mo.Grid(tgt, mc, 0.9)
    assert int((np.array([Mo.device_corr(x, small, thr) for x in q]) != want).sum()) > 0
