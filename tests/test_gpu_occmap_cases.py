"""GPU: the coloured occupancy map (rgbd_occmap_*) against the Python restatement of tests/occmap_model.py on the inputs of
tests/occmap_cases.py.  Every comparison is through `leaves`, bit for bit: keys, log-odds floats and colours, after
every scan of a case."""
import ctypes as C

import numpy as np
import pytest

import occmap_cases as OC
import occmap_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(640, 480, max_batch=1, orb=pkg.orb_params(1000), cam=pkg.camera(517.3, 516.5, 318.6, 255.3))
    yield c
    c.close()


def assert_equal(got, model, what):
    keys, lo, rgb = got.leaves()
    wk, wl, wc = model.leaves()
    assert len(got) == len(model) == len(keys), what
    assert np.array_equal(keys, wk), what
    assert np.array_equal(lo.view(np.uint32), wl.view(np.uint32)), what
    assert np.array_equal(rgb, wc), what


@pytest.mark.parametrize("name", sorted(OC.CASES))
def test_case_equals_model(pkg, ctx, name):
    cap, scans = OC.CASES[name]
    m, ref = pkg.OccupancyMap(ctx, pkg.occmap_params(capacity=cap)), M.Map(M.Params(capacity=cap))
    try:
        for i, (p, T, o, mr) in enumerate(scans):
            assert ref.insert(p, T, o, mr)
            m.insert(p, T, o, mr)
            assert_equal(m, ref, (name, i))
        # clear, then the same scans as one batch: the same leaves
        m.clear()
        assert len(m) == 0 and len(m.leaves()[0]) == 0
        if len({s[3] for s in scans}) == 1:     # a batch has one maxrange
            assert m.insert_batch([s[0] for s in scans], [s[1] for s in scans], [s[2] for s in scans], scans[0][3]) == len(scans)
        else:
            for p, T, o, mr in scans:
                m.insert(p, T, o, mr)
        assert_equal(m, ref, (name, "again"))
    finally:
        m.close()


def test_overflow_leaves_the_map_as_it_was(pkg, ctx):
    cap, scans = OC.OVERFLOW
    m, ref = pkg.OccupancyMap(ctx, pkg.occmap_params(capacity=cap)), M.Map(M.Params(capacity=cap))
    try:
        m.insert(*scans[0])
        assert ref.insert(*scans[0])
        before = [a.tobytes() for a in m.leaves()]
        assert not ref.insert(*scans[1])
        with pytest.raises(pkg.RgbdError, match=r"status 3"):
            m.insert(*scans[1])
        assert [a.tobytes() for a in m.leaves()] == before and len(m) == len(ref)
        assert_equal(m, ref, "after the scan that did not fit")
        m.insert(*scans[2])                       # the table still works, and the slots claimed by the failed scan are free
        assert ref.insert(*scans[2])
        assert_equal(m, ref, "a scan that fits after one that did not")
        # the batch stops at the first scan that does not fit
        m.clear()
        applied = m.insert_batch([s[0] for s in scans], [s[1] for s in scans], [s[2] for s in scans])
        ref2 = M.Map(M.Params(capacity=cap))
        assert ref2.insert(*scans[0])
        assert applied == 1
        assert_equal(m, ref2, "batch")
    finally:
        m.close()


def test_unsupported_arguments(pkg, ctx):
    lib, U = pkg.lib(), 4
    h = C.c_void_p()

    def create(**kw):
        prm = pkg.occmap_params(**kw)
        return lib.rgbd_occmap_create(ctx._h, C.byref(prm), C.byref(h))
    assert lib.rgbd_occmap_create(None, C.byref(pkg.occmap_params()), C.byref(h)) == U
    assert lib.rgbd_occmap_create(ctx._h, None, C.byref(h)) == U
    assert lib.rgbd_occmap_create(ctx._h, C.byref(pkg.occmap_params()), None) == U
    for kw in (dict(resolution=0.0), dict(resolution=-0.08), dict(resolution=float("nan")), dict(resolution=float("inf")),
               dict(prob_hit=1.0), dict(prob_miss=0.0), dict(clamp_min=-0.1), dict(clamp_max=1.5), dict(prob_hit=float("nan")),
               dict(clamp_min=0.999, clamp_max=0.001), dict(capacity=32), dict(capacity=0), dict(capacity=-64),
               dict(capacity=100), dict(capacity=1 << 31), dict(capacity=1 << 40)):
        assert create(**kw) == U, kw
        assert not h.value
    m = pkg.OccupancyMap(ctx, pkg.occmap_params(capacity=64))
    try:
        p = OC.pts([OC.E_X])
        T, o = OC.I34, OC.O
        ptr = pkg._ptr
        assert lib.rgbd_occmap_insert(None, ptr(p), 1, ptr(T), ptr(o), -1.0) == U
        assert lib.rgbd_occmap_insert(m._h, None, 1, ptr(T), ptr(o), -1.0) == U
        assert lib.rgbd_occmap_insert(m._h, ptr(p), 1, None, ptr(o), -1.0) == U
        assert lib.rgbd_occmap_insert(m._h, ptr(p), 1, ptr(T), None, -1.0) == U
        big = OC.pts([OC.E_X] * 16385)
        assert lib.rgbd_occmap_insert(m._h, ptr(big), 16385, ptr(T), ptr(o), -1.0) == U
        bad = T.copy()
        bad[1, 2] = np.nan
        assert lib.rgbd_occmap_insert(m._h, ptr(p), 1, ptr(bad), ptr(o), -1.0) == U
        assert lib.rgbd_occmap_insert(m._h, ptr(p), 1, ptr(T), ptr(np.array((0, np.inf, 0), np.float32)), -1.0) == U
        assert lib.rgbd_occmap_insert(m._h, ptr(p), 1, ptr(T), ptr(o), float("nan")) == U
        n = C.c_int32(0)
        cnt = np.array([1], np.int32)
        assert lib.rgbd_occmap_insert_batch(m._h, ptr(p), None, 1, 1, ptr(T), ptr(o), -1.0, C.byref(n)) == U
        assert lib.rgbd_occmap_insert_batch(m._h, ptr(p), ptr(cnt), 1, 1, ptr(T), ptr(o), -1.0, None) == U
        n64 = C.c_int64(0)
        assert lib.rgbd_occmap_leaves(m._h, C.c_float(-np.inf), None, None, None, 4, C.byref(n64)) == U
        assert lib.rgbd_occmap_leaves(None, C.c_float(-np.inf), None, None, None, 0, C.byref(n64)) == U
        assert lib.rgbd_occmap_size(m._h, None) == U and lib.rgbd_occmap_clear(None) == U
        assert lib.rgbd_occmap_sensor_pose(None, ptr(T), ptr(o)) == U
        Tn = np.eye(4, dtype=np.float32)
        Tn[0, 3] = np.inf
        assert lib.rgbd_occmap_sensor_pose(ptr(Tn), ptr(T.copy()), ptr(o.copy())) == U
        assert len(m) == 0 and len(m.leaves()[0]) == 0     # nothing above touched the map
        m.insert(OC.pts([OC.E_X] * 16384), T, o)           # the cap itself is supported
        assert len(m) == 6
        assert lib.rgbd_occmap_leaves(m._h, C.c_float(-np.inf), None, None, None, 0, C.byref(n64)) == 3 and n64.value == 6
        assert len(m.leaves(min_prob=0.5)[0]) == 1 and len(m.leaves(min_prob=0.95)[0]) == 0
    finally:
        m.close()
