"""The PnPRansac edge cases (tests/pnp_edge_cases.py) reach their regimes: asserted from the oracle alone, so a change
of a generator cannot quietly move a case off the edge that tests/test_gpu_pnp_edges.py runs it for."""
import numpy as np
import pytest

import pnp_edge_cases as E
from pnp_cases import K_TUM

# (ok, iterations) of the degenerate, non-finite and parameter cases
PINNED = {"collinear": (False, 500), "coplanar": (False, 500), "two_distinct": (False, 500), "behind": (False, 500),
          "all_outlier": (False, 500), "coplanar_jitter": (True, 1), "collinear_5": (False, 0), "coplanar_5": (False, 0),
          "nan_px_5": (False, 0), "inf_5": (False, 0), "reproj_0": (False, 500),
          # the rest as measured when the cases were written
          "every_twice": (True, 2), "behind_fit5": (True, 500), "zero_7th": (True, 10), "scale_1e4": (True, 39),
          "scale_1e-4": (True, 39), "reproj_1e6": (True, 1), "conf_0": (True, 1), "conf_1": (True, 500),
          "iters_0": (True, 1), "iters_1": (True, 1), "iters_2": (True, 2), "iters_3000": (False, 3000),
          "minm_count": (True, 18), "minm_count1": (False, 0), "forced_8": (False, 8), "forced_24": (False, 24),
          "forced_25": (False, 25)}


@pytest.fixture(scope="module")
def results(oracle):
    """Every case solved once by the oracle: name -> (ok, R, t, mask, n_inliers, iterations)."""
    out = {}
    for name in E.NAMES:
        p3, p2, prm = E.case(name)
        out[name] = E.expected(oracle, p3, p2, prm)
    return out


def _getsubset_over_stream(oracle, count, k):
    """getSubset restated over the oracle's cv::RNG((uint64)-1) uniform(0, count) stream: a repeated index is
    drawn again."""
    L = oracle._pnp_sigs()
    buf = np.zeros(40 * k + 64, np.int32)   # at 6 points a subset takes about 15 draws
    L.orc_cvrng_uniform_stream((1 << 64) - 1, count, len(buf), buf)
    out, j = [], 0
    for _ in range(k):
        cur = []
        while len(cur) < 5:
            v = int(buf[j])
            j += 1
            if v not in cur:
                cur.append(v)
        out.append(cur)
    return out


@pytest.mark.parametrize("count", [6, 40, 256, 600])
def test_subset_stream_is_the_oracles(oracle, count):
    assert E.subsets(count, 600) == _getsubset_over_stream(oracle, count, 600)


def test_names_are_unique_and_buildable():
    assert len(set(E.NAMES)) == len(E.NAMES)
    for name in E.NAMES:
        p3, p2, prm = E.case(name)
        assert p3.dtype == np.float32 and p2.dtype == np.float32 and p3.shape == (len(p2), 3) and p2.shape[1:] == (2,)
        assert set(prm) == set(E.DEFAULTS)


def test_sizes_solve(results):
    for n, name in zip(E.SIZES, E.SIZE_NAMES):
        assert len(E.case(name)[0]) == n
        assert results[name][0], name
    assert not results["size_5"][5]   # five points: one EPnP, no loop


def test_every_ok_result_is_finite(results):
    for name, (ok, R, t, mask, ni, it) in results.items():
        if ok:
            assert np.isfinite(R).all() and np.isfinite(t).all(), name
            assert ni == mask.sum() >= 5, name
        else:
            assert ni == 0 and not mask.any() and np.array_equal(R, np.eye(3)) and not t.any(), name


def test_pinned_outcomes(results):
    for name, want in PINNED.items():
        assert (results[name][0], results[name][5]) == want, name
    assert set(PINNED) >= set(E.DEGENERATE + E.PARAMS + E.FORCED_NAMES)   # (the other non-finite cases: below)


def test_placements_put_the_inliers_where_they_say(results):
    for name in E.PLACE_NAMES:
        _, kind, n = name.split("_")
        want = np.zeros(int(n), bool)
        want[E.placement_inliers(kind, int(n))] = True
        ok, _, _, mask, ni, _ = results[name]
        assert ok and np.array_equal(mask, want), name
    assert set(E.placement_inliers("edges", 600)) >= {63, 64, 255, 256} and len(E.placement_inliers("edges", 600)) == 8
    assert set(E.placement_inliers("edges", 256)) >= {63, 64, 255}
    for n in E.PLACE_SIZES:
        w = E.placement_inliers("wave", n)
        assert len(w) == 64 and w[0] % 64 == 0


def test_schedule_boundaries_are_the_handovers():
    for sch, ks in E.SCHEDULES.items():
        assert ks == sorted(k for h in E.handovers(sch) for k in (h, h + 1))
        assert set(ks) <= set(E.ITER_TABLE) and set(ks) <= set(E.BEST_TABLE)


def test_iteration_table(results):
    for k, name in zip(E.ITER_TABLE, E.ITER_NAMES):
        ok, *_, it = results[name]
        assert ok and it == k, name


def test_best_iteration_table(oracle, results):
    for (b, (_, _, _, iters)), name in zip(E.BEST_TABLE.items(), E.BEST_NAMES):
        ok, _, _, mask, ni, it = results[name]
        assert ok and it == iters > b, name
        p3, p2, prm = E.case(name)
        # the smallest iteration cap that already gives the final mask and count is b
        r = oracle.pnp_ransac(p3, p2, K_TUM, b)
        assert r[0] and r[4] == ni and np.array_equal(r[3], mask), name
        r = oracle.pnp_ransac(p3, p2, K_TUM, b - 1)
        assert not (r[0] and r[4] == ni and np.array_equal(r[3], mask)), name


def test_poisoned_index_is_in_the_first_subset_and_the_run_survives(results):
    assert E.NF_IN in E.subsets(E.NF_N, 1)[0]
    for name in ("nan_px_in", "inf_px_in", "nan_obj_in"):
        p3, p2, _ = E.case(name)
        assert not (np.isfinite(p3[E.NF_IN]).all() and np.isfinite(p2[E.NF_IN]).all())
        assert np.isfinite(np.delete(p3, E.NF_IN, 0)).all() and np.isfinite(np.delete(p2, E.NF_IN, 0)).all()
        ok, _, _, mask, _, it = results[name]
        assert ok and it > 1 and not mask[E.NF_IN], name


def test_unsampled_poisoned_index_is_in_no_subset(results):
    for name, j in E.NF_OUT.items():
        p3, p2, _ = E.case(name)
        assert not (np.isfinite(p3[j]).all() and np.isfinite(p2[j]).all())
        ok, _, _, mask, _, it = results[name]
        assert ok and not mask[j], name
        assert all(j not in s for s in E.subsets(E.NF_N, it)), name


def test_priming_batches_steer_the_schedule(oracle):
    for sch in E.SCHEDULES:
        batch = E.prime(sch)
        if not batch:
            continue
        iters = [oracle.pnp_ransac(p3, p2, K_TUM)[5] for p3, p2 in batch]
        if sch == (4, 4):
            assert len(batch) == 10 and max(iters) <= 3
        assert E.adapted_chunks(iters) == sch


def test_independence_batch_reaches_every_stage_under_every_schedule(results):
    assert len(E.INDEPENDENCE) == 12
    its = [results[n][5] for n in E.INDEPENDENCE]
    for k0, k1 in E.SCHEDULES:
        assert any(k0 < it <= k0 + k1 for it in its), (k0, k1)
        assert any(it > k0 + k1 for it in its), (k0, k1)
