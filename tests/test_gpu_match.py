"""GPU parity: Hamming knn-2 and Matcher::match filters vs the CPU oracle (bit-exact)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.Context(640, 480, max_batch=1)


def test_knn2_random_descriptors(ctx, oracle):
    rs = np.random.default_rng(1)
    for nq, nt in [(1, 2), (5, 3), (300, 257), (1000, 1000), (2004, 1777)]:
        dq = rs.integers(0, 256, size=(nq, 32), dtype=np.uint8)
        dt = rs.integers(0, 256, size=(nt, 32), dtype=np.uint8)
        assert np.array_equal(ctx.knn2(dq, dt), oracle.knn2(dq, dt)), (nq, nt)


def test_knn2_ties_lowest_index_first(ctx, oracle):
    """Duplicated train rows produce distance ties; batchDistance keeps the lower index first."""
    rs = np.random.default_rng(2)
    base = rs.integers(0, 256, size=(40, 32), dtype=np.uint8)
    dt = np.concatenate([base, base, base[::-1]])
    dq = base.copy()
    dq[:, 0] ^= 1
    got, want = ctx.knn2(dq, dt), oracle.knn2(dq, dt)
    assert np.array_equal(got, want)
    assert np.all(got[:, 0] == got[:, 2])      # every query has a tied pair


def test_knn2_single_train_row(ctx, oracle):
    rs = np.random.default_rng(3)
    dq = rs.integers(0, 256, size=(7, 32), dtype=np.uint8)
    dt = rs.integers(0, 256, size=(1, 32), dtype=np.uint8)
    got = ctx.knn2(dq, dt)
    assert np.array_equal(got, oracle.knn2(dq, dt))
    assert np.all(got[:, 3] == -1)


def test_match_filters(ctx, oracle, seq_fr1):
    bgr, depth, _, cam = seq_fr1
    p = oracle.orb_params(1000)
    oc = oracle.camera(cam)
    f0 = oracle.frame(bgr[0], depth[0], p, oc)
    f1 = oracle.frame(bgr[1], depth[1], p, oc)
    rs = np.random.default_rng(4)
    outl = (rs.random(len(f0["kps"])) < 0.2).astype(np.uint8)
    for ratio, discard in [(0.9, True), (0.6, True), (0.9, False)]:
        got = ctx.match(f0["desc"], f1["desc"], outl, f0["xyz"][:, 2], f1["xyz"][:, 2], ratio, discard)
        want = oracle.match(f0["desc"], f1["desc"], outl, f0["xyz"][:, 2], f1["xyz"][:, 2], ratio, discard)
        assert len(want) > 50
        assert np.array_equal(got, want), (ratio, discard)


def test_match_empty_inputs(ctx):
    z = np.zeros(0, np.float32)
    d = np.zeros((0, 32), np.uint8)
    assert len(ctx.match(d, d, np.zeros(0, np.uint8), z, z)) == 0


# ---- the ends of the key arithmetic, tile and workgroup boundaries, placed ties, the 16-bit train index
INT_MAX = 2 ** 31 - 1


def _rand(rs, n):
    return rs.integers(0, 256, size=(n, 32), dtype=np.uint8)


def _pools():
    """512 queries and 97 trains, random with all-zero and all-one rows mixed in (distances 0 and 256 occur)."""
    rs = np.random.default_rng(5)
    dq, dt = _rand(rs, 512), _rand(rs, 97)
    dq[[0, 40, 254, 256, 511]] = 0
    dq[[1, 41, 255, 300]] = 255
    dt[[0, 30, 32, 63, 96]] = 0
    dt[[1, 31, 64, 95]] = 255
    return dq, dt


def test_knn2_extreme_rows(ctx, oracle):
    dq, dt = _pools()
    got = ctx.knn2(dq, dt)
    assert np.array_equal(got, oracle.knn2(dq, dt))
    assert got[0].tolist() == [0, 0, 0, 30] and got[1].tolist() == [0, 1, 0, 31]   # |t| = q.t = 0, and both 256
    zero, one = np.zeros((3, 32), np.uint8), np.full((5, 32), 255, np.uint8)
    for q, t in [(zero, one), (one, zero)]:   # every distance is 256
        got = ctx.knn2(q, t)
        assert np.array_equal(got, oracle.knn2(q, t))
        assert np.all(got == [256, 0, 256, 1])
    for q, t in [(zero, zero), (one, one)]:   # every distance is 0
        got = ctx.knn2(q, t)
        assert np.array_equal(got, oracle.knn2(q, t))
        assert np.all(got == [0, 0, 0, 1])


@pytest.mark.parametrize("nt", [31, 32, 33, 64, 96, 97])
def test_knn2_tile_and_workgroup_boundaries(ctx, oracle, nt):
    """The 32-row train tile and the 256-query workgroup, at their multiples and one off them."""
    dq, dt = _pools()
    for nq in [255, 256, 257, 512]:
        assert np.array_equal(ctx.knn2(dq[:nq], dt[:nt]), oracle.knn2(dq[:nq], dt[:nt])), (nq, nt)


def test_knn2_and_match_one_side_empty(ctx, oracle):
    dq, dt = _pools()
    none = np.zeros((0, 32), np.uint8)
    got = ctx.knn2(dq[:257], none)
    assert got.shape == (257, 4)
    assert np.array_equal(got, oracle.knn2(dq[:257], none))
    assert np.all(got == [INT_MAX, -1, INT_MAX, -1])
    assert ctx.knn2(none, dt).shape == (0, 4)
    z = np.ones(97, np.float32)
    assert len(ctx.match(dq[:97], none, np.zeros(97, np.uint8), z, z[:0])) == 0
    assert len(ctx.match(none, dt, np.zeros(0, np.uint8), z[:0], z)) == 0
    assert len(oracle.match(dq[:97], none, np.zeros(97, np.uint8), z, z[:0])) == 0


def _planted(ctx, oracle, rows, qi, nq=257, nt=100, seed=6):
    """Exact copies of one train row (query qi with three bits flipped) at `rows`; the whole result equals the
    oracle's, and the planted query's row comes back."""
    rs = np.random.default_rng(seed)
    dq, dt = _rand(rs, nq), _rand(rs, nt)
    row = dq[qi].copy()
    row[[2, 17, 31]] ^= np.array([1, 16, 128], np.uint8)
    dt[list(rows)] = row
    got = ctx.knn2(dq, dt)
    assert np.array_equal(got, oracle.knn2(dq, dt)), (rows, qi)
    return got[qi].tolist()


def test_knn2_placed_ties(ctx, oracle):
    """Register j of the accumulator holds train row (j & 3) + 8 (j >> 2) + 4 h of its tile: rows r and r + 4 sit in
    the two lane halves, r and r + 1 in one register group, r and r + 8 in neighbouring groups, 31 and 32 and
    r and r + 32 in neighbouring tiles.  The lower index comes first."""
    pairs = [(31, 32)]
    for r in (0, 1, 3, 4, 7, 8, 12, 27, 35, 59):
        pairs += [(r, r + 4), (r, r + 1), (r, r + 8), (r, r + 32)]
    qis = [0, 31, 32, 63, 64, 255, 256]   # first / last lane of a query tile, of a wave, of a workgroup
    for n, (a, b) in enumerate(pairs):
        assert _planted(ctx, oracle, (a, b), qis[n % len(qis)]) == [3, a, 3, b], (a, b)


def test_knn2_three_way_ties(ctx, oracle):
    for n, rows in enumerate([(5, 6, 7), (2, 6, 10), (3, 7, 39), (30, 31, 32), (0, 32, 64), (31, 63, 95),
                              (60, 64, 99)]):
        assert _planted(ctx, oracle, rows, [0, 33, 256][n % 3]) == [3, rows[0], 3, rows[1]], rows


def test_knn2_train_index_limit(pkg, ctx, oracle):
    """The rank key holds the train index in 16 bits: 65536 rows are exact, 65537 are refused."""
    rs = np.random.default_rng(8)
    dq, dt = _rand(rs, 33), _rand(rs, 65537)
    dt[65535] = dq[5]
    dt[[3, 65534]] = dq[6]
    got = ctx.knn2(dq, dt[:65536])
    assert np.array_equal(got, oracle.knn2(dq, dt[:65536]))
    assert got[5, :2].tolist() == [0, 65535] and got[6].tolist() == [0, 3, 0, 65534]
    # one row more: row 65536 would carry the key of (distance + 1, index 0)
    dt[65536] = dq[7]
    ctx.set_timing(True)
    ctx.reset_timing()
    try:
        out = np.full((33, 4), -5, np.int32)
        st = pkg.lib().rgbd_knn2(ctx._h, pkg._ptr(dq), 33, pkg._ptr(dt), 65537, pkg._ptr(out))
        assert st == 4   # RGBD_ERR_UNSUPPORTED
        assert b"65536" in pkg.lib().rgbd_last_error(ctx._h)
        assert np.all(out == -5)
        with pytest.raises(pkg.RgbdError, match=r"65536 train rows.*\(status 4\)"):
            ctx.knn2(dq, dt)
        z = np.ones(65537, np.float32)
        with pytest.raises(pkg.RgbdError, match=r"65536 train rows.*\(status 4\)"):
            ctx.match(dq, dt, np.zeros(33, np.uint8), z[:33], z)
        assert "k_knn2" not in ctx.timings()   # refused before any launch
    finally:
        ctx.set_timing(False)
        ctx.reset_timing()
    # the context still serves the next call
    assert np.array_equal(ctx.knn2(dq, dt[:97]), oracle.knn2(dq, dt[:97]))
