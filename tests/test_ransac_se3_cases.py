"""CPU: every case of tests/ransac_se3_cases.py reaches the regime of csrc/ransac.hip / csrc/solver.cpp it is named
after, asserted from the oracle (oracle/orc_solver.cpp), the restated sampler and numpy alone, so that the device
parity of tests/test_gpu_ransac_edges.py pins those regimes.  hypotheses_consumed tells how many loop iterations a
call ran and which sorted positions each sampled; the oracle's T and rmse are finite in every case, so comparing
their bits on the device is meaningful."""
import functools
import types

import numpy as np
import pytest

import ransac_se3_cases as E

F = np.float32
EYE = np.eye(4, dtype=F)


@functools.lru_cache(maxsize=None)
def case(name):
    return E.case(name)


@functools.lru_cache(maxsize=None)
def _run(name):
    import oracle_lib as O
    xyz1, xyz2, m, prm, seed, sticky, update_f2 = case(name)
    rng, st = O.rng(seed), O.Sticky()
    if sticky is not None:
        st.cov, st.set = sticky, 1
    flags = None if update_f2 is None else np.zeros(len(xyz2), np.uint8)
    ok, T, inl, rmse = O.ransac_se3(xyz1, xyz2, m, O.ransac_params(*prm), rng, st, flags, update_f2=bool(update_f2))
    order = E.sorted_order(m)
    return types.SimpleNamespace(
        ok=ok, T=T, inl=inl, rmse=rmse, sticky=st, flags=flags, order=order, M=len(m), prm=prm, xyz1=xyz1, xyz2=xyz2, m=m,
        src=xyz1[m["queryIdx"][order]], tgt=xyz2[m["trainIdx"][order]],   # the points in sorted order: what ids index
        cons=E.hypotheses_consumed(seed, len(m), prm[3], rng, limit=max(prm[0], 0)))


@pytest.fixture
def run(oracle):
    return _run


def positions(r, match_ids):
    """Sorted positions (the sampler's ids) of the given matches."""
    return set(np.nonzero(np.isin(r.order, match_ids))[0].tolist())


def cross_cov(r, ids):
    """The weighted cross-covariance of PCL's TransformationFromCorrespondences over the sorted positions ids, f64."""
    p, q = r.src[ids].astype(np.float64), r.tgt[ids].astype(np.float64)
    w = 1.0 / (p[:, 2] * q[:, 2])
    w = w / w.sum()
    dp, dq = p - w @ p, q - w @ q
    return (dq * w[:, None]).T @ dp


def inlier_matches(r):
    """The returned inliers as indices into the case's matches (their order is the sorted order)."""
    keys = {(int(a), int(b), float(d)): i for i, (a, b, d) in enumerate(zip(r.m["queryIdx"], r.m["trainIdx"], r.m["distance"]))}
    return [keys[(int(a), int(b), float(d))] for a, b, d in zip(r.inl["queryIdx"], r.inl["trainIdx"], r.inl["distance"])]


# ------------------------------------------------------------------ one regime check per case name
def check_size(r, name):
    M = int(name.split("_")[1])
    assert r.M == M and r.ok and len(r.cons) == 1
    if name.endswith("_noisy"):
        assert 0.5 * M < len(r.inl) < M
    else:
        assert len(r.inl) == M   # the refinement fits all M points: the fit pipeline meets the block boundary


def check_contam(r, name):
    assert r.M == int(name.split("_")[1]) and r.ok and len(r.cons) > 24   # the host's second chunk runs
    assert 10 <= len(r.inl) < 0.5 * r.M


def zw_state(r):
    bad = positions(r, E.zw_bad_matches())
    with np.errstate(all="ignore"):
        w = F(1.0) / (r.src[:, 2] * r.tgt[:, 2])
    zero = np.isnan(r.src[:, 2]) | np.isnan(r.tgt[:, 2]) | (w == 0)   # skipped by the fit, or added with weight 0
    assert set(np.nonzero(zero)[0].tolist()) == bad and len(bad) == 100 and 0 not in bad
    assert int(np.isnan(r.src[:, 2]).sum()) == 40 and int(np.isposinf(r.src[:, 2]).sum()) == 30
    assert int(np.isposinf(r.tgt[:, 2]).sum()) == 30
    return bad


def check_zw(r, name):
    bad = zw_state(r)
    assert r.prm[3] == int(name[len("zw_ss"):]) and r.ok and len(r.inl) == 100
    # every consumed sample holds a zero-weight id, so the winning hypothesis's first fit ran on a compacted set
    assert len(r.cons) == E.ZW_ITERS and all(len(s) == r.prm[3] and bad & set(s) for s in r.cons)


def check_zw_keep(r, name):
    bad = zw_state(r)
    keep = int(name[len("zw_keep"):])
    assert len(r.cons) >= 1 and len(set(r.cons[0]) - bad) == keep and len(r.cons[0]) == 4
    if keep == 2:   # two points: a covariance of rank one on the compacted set
        assert np.linalg.matrix_rank(cross_cov(r, sorted(set(r.cons[0]) - bad))) == 1


def check_all_identical(r, name):
    assert (r.src == r.src[0]).all() and (r.tgt == r.tgt[0]).all()
    assert not cross_cov(r, r.cons[0]).any() and r.ok and len(r.inl) == r.M   # the zero matrix: svd3's scale == 0


def check_rank(r, name):
    rank = {"exact_line": 1, "exact_plane": 2}[name]
    assert np.linalg.matrix_rank(cross_cov(r, r.cons[0])) == rank
    assert np.linalg.matrix_rank(cross_cov(r, np.arange(r.M))) == rank   # the refinement's fit as well
    assert r.ok and len(r.inl) == r.M


def check_mirror(r, name):
    assert np.array_equal(r.tgt, r.src * np.array([-1, 1, 1], F))
    assert np.linalg.det(cross_cov(r, r.cons[0])) < 0          # det(U) det(V) < 0: the reflection branch runs
    assert np.linalg.det(r.T[:3, :3].astype(np.float64)) > 0   # and returns a rotation
    if name == "mirror_slab":
        assert np.abs(r.src[:, 0]).max() <= F(0.004) and r.ok and len(r.inl) == 200
    else:
        assert r.prm[1] == 4


def check_identity(r, name):
    static = positions(r, E.identity_static(np.random.default_rng(77)))
    assert len(static) == E.IDENT_STATIC and len(r.cons) == r.prm[0]
    assert (r.src[sorted(static)] == r.tgt[sorted(static)]).all()
    if name == "ident_refused":   # evaluated and refused: the rule is count > min_inlier_th
        assert r.prm[1] == E.IDENT_STATIC == len(_run("ident_it1").inl)
        assert np.array_equal(r.xyz2, _run("ident_it1").xyz2) and np.array_equal(r.m, _run("ident_it1").m)
        assert not r.ok and r.rmse == 1e6 and len(r.inl) == 0
    else:
        assert r.ok and np.array_equal(r.T, EYE) and r.rmse >= 1e6 and len(r.inl) == E.IDENT_STATIC
        assert positions(r, inlier_matches(r)) == static


def check_iters(r, name):
    it = int(name[len("iters_"):])
    assert r.prm[0] == it and len(r.cons) == max(it, 0)   # from 23 on: no early end
    if it <= 0:
        assert not r.ok and r.rmse == 1e6 and r.sticky.set == 1   # the identity is still evaluated
    assert r.ok == (it == 1 or it >= 25)   # hypothesis 24, the first of the second chunk, is the first accepted
    if it == 1000:
        assert len(r.cons) > 256           # past the workspace's first capacity


def check_ss(r, name):
    ss = int(name[3:])
    assert r.prm[3] == ss
    if ss == 0:
        assert r.cons == [] and not r.ok   # 200 iterations, no draw: the RNG stays where it was
    else:
        assert r.ok and len(r.cons) >= 1 and all(len(s) == ss for s in r.cons)


def check_m_lt_ss(r, name):
    assert r.prm[1] <= r.M < r.prm[3] and r.cons == [] and not r.ok and r.rmse == 1e6 and r.sticky.set == 1


def check_maxd(r, name):
    assert r.prm[2] == float(name[5:])
    n = {k: len(_run(k).inl) for k in ("maxd_0.5", "minth_3", "maxd_10")}   # minth_3: the same cloud at 3.0
    assert 10 <= n["maxd_0.5"] < n["minth_3"] <= n["maxd_10"] and r.ok


def check_minth(r, name):
    if name == "minth_3":
        assert r.prm[1] == 3 and r.ok
    else:
        assert r.prm[1] == r.M and not r.ok and len(_run("minth_3").inl) < r.M and len(r.cons) == r.prm[0]


def check_target_z0(r, name):
    bad = positions(r, E.odd_ids(name))
    assert len(bad) == 30 and (r.tgt[sorted(bad), 2] == 0).all() and (r.tgt[sorted(bad), 0] != 0).all()
    with np.errstate(all="ignore"):
        assert np.isinf(F(1.0) / (r.src[sorted(bad), 2] * r.tgt[sorted(bad), 2])).all()   # infinite weights
    assert sum(1 for s in r.cons if bad & set(s)) >= 10   # hypotheses with a NaN transform
    assert r.ok and not (positions(r, inlier_matches(r)) & bad)


def check_neg_z(r, name):
    bad = positions(r, E.odd_ids(name))
    assert len(bad) == 10 and (r.src[sorted(bad), 2] < 0).all() and (r.tgt > 0)[:, 2].all()
    assert len(r.cons) > 1 and bad & set(r.cons[0]) and r.ok


def check_src_z0_all(r, name):
    assert (r.src[:, 2] == 0).all() and not r.ok and r.sticky.set == 0 and r.sticky.cov == 0.0
    assert len(r.cons) == r.prm[0]


def check_first20_invalid(r, name):
    skipped = (r.src[:, 2] == 0) | (r.tgt[:, 0] == 0) | np.isnan(r.src[:, 2]) | np.isnan(r.tgt[:, 2])
    assert skipped[:20].all() and not skipped[20:].any()
    assert int((r.src[:20, 2] == 0).sum()) == 7 and int((r.tgt[:20, 0] == 0).sum()) == 7 and int(np.isnan(r.src[:20, 2]).sum()) == 6
    sd = 0.01 * float(r.src[20, 2]) * float(r.src[20, 2])
    assert r.sticky.set == 1 and r.sticky.cov == sd * sd and r.ok


def check_sticky(r, name):
    assert r.sticky.set == 1 and r.sticky.cov == E.STICKY_PRESETS[name] and r.ok
    assert len({_run(k).rmse for k in E.STICKY_PRESETS}) == 3   # the preset is what the distances use


def check_dup(r, name):
    assert r.M == 240 and np.array_equal(r.m[0::2], r.m[1::2]) and r.ok
    assert len(r.inl) % 2 == 0 and np.array_equal(r.inl[0::2], r.inl[1::2])


def check_many_to_one(r, name):
    assert len(np.unique(r.m["trainIdx"])) == 10 and len(np.unique(r.m["queryIdx"])) == 120
    assert r.ok and len(r.inl) > 10 and len(np.unique(r.inl["trainIdx"])) <= 10


def check_equal_dist(r, name):
    assert len(np.unique(r.m["distance"])) == 1 and sorted(r.order.tolist()) == list(range(r.M))
    assert not np.array_equal(r.order, np.arange(r.M)) and r.ok   # std::sort's own order of the ties


def check_f2(r, name):
    on = _run("minth_3")   # the same cloud with the flags updated
    assert np.array_equal(r.m, on.m) and r.ok and on.ok
    assert 0 < int(on.flags.sum()) == r.M - len(on.inl)
    if name == "f2_off":
        assert case(name)[6] == 0 and r.flags is not None and not r.flags.any()
    else:
        assert case(name)[6] is None and r.flags is None
    assert np.array_equal(r.T, on.T) and np.array_equal(r.inl, on.inl)


CHECKS = {}
for _n in E.NAMES:
    for _prefix, _fn in (("size_", check_size), ("contam_", check_contam), ("zw_ss", check_zw), ("zw_keep", check_zw_keep),
                         ("all_identical", check_all_identical), ("exact_", check_rank), ("mirror_", check_mirror),
                         ("ident_", check_identity), ("iters_", check_iters), ("ss_", check_ss), ("m_lt_ss", check_m_lt_ss),
                         ("maxd_", check_maxd), ("minth_", check_minth), ("target_z0", check_target_z0),
                         ("neg_z", check_neg_z), ("src_z0_all", check_src_z0_all),
                         ("first20_invalid", check_first20_invalid), ("sticky_", check_sticky), ("dup_matches", check_dup),
                         ("many_to_one", check_many_to_one), ("equal_dist", check_equal_dist), ("f2_off", check_f2),
                         ("flags_none", check_f2)):
        if _n.startswith(_prefix):
            CHECKS[_n] = _fn


def test_every_name_has_a_regime_check():
    assert len(set(E.NAMES)) == len(E.NAMES) and set(CHECKS) == set(E.NAMES)


@pytest.mark.parametrize("name", E.NAMES)
def test_case_reaches_its_regime(run, name):
    r = run(name)
    xyz1, xyz2, m, prm, seed, sticky, update_f2 = case(name)
    assert xyz1.dtype == xyz2.dtype == F and 1 <= len(m) <= 2304 and prm[3] <= 8
    assert 0 <= m["queryIdx"].min() and m["queryIdx"].max() < len(xyz1)
    assert 0 <= m["trainIdx"].min() and m["trainIdx"].max() < len(xyz2)
    if name != "equal_dist":   # the sort is unambiguous (duplicated matches are equal as a whole)
        assert len(np.unique(m["distance"])) == len(np.unique(m))
    assert np.isfinite(r.T).all() and np.isfinite(r.rmse)   # so that comparing bits is meaningful
    assert r.ok == (len(r.inl) >= prm[1])
    if not r.ok:
        assert np.array_equal(r.T, EYE) or len(r.inl) > 0
    CHECKS[name](r, name)


def test_hypotheses_consumed_follows_the_loop(run):
    """An early accept ends the loop after one hypothesis; without one the loop runs `iterations` samples, each of
    sample_size distinct ascending ids below M."""
    assert len(run("size_64").cons) == 1 and len(run("contam_257").cons) > 24
    for name in ("iters_300", "contam_2304", "zw_ss8"):
        r = run(name)
        assert all(s == sorted(set(s)) and len(s) == r.prm[3] and 0 <= s[0] and s[-1] < r.M for s in r.cons)
