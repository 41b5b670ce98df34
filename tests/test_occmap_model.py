"""CPU: pins tests/occmap_model.py, the Python restatement of DESIGN.md "Occupancy map definition" that the GPU tests
compare with: known-answer rays, the structure of random rays, the log-odds constants and their saturation."""
import numpy as np
import pytest

import occmap_model as M

F = np.float32
O = (0.04, 0.04, 0.04)
K = 32768

RAYS = [
    ((0.44, 0.04, 0.04), [(K + i, K, K) for i in range(5)]),
    ((0.20, 0.20, 0.20), [(K, K, K), (K, K, K + 1), (K, K + 1, K + 1), (K + 1, K + 1, K + 1), (K + 1, K + 1, K + 2),
                          (K + 1, K + 2, K + 2)]),
    ((-0.12, 0.04, 0.20), [(K, K, K), (K - 1, K, K), (K - 1, K, K + 1), (K - 2, K, K + 1)]),
]


@pytest.mark.parametrize("e,want", RAYS)
def test_ray_known_answers(e, want):
    assert M.ray_keys(np.array(O, F), np.array(e, F)) == want


def test_ray_end_cell_is_not_in_the_ray():
    cells = M.ray_keys(np.array(O, F), np.array((0.44, 0.04, 0.04), F))
    assert (K + 5, K, K) == M.key3(np.array((0.44, 0.04, 0.04), F), 1.0 / 0.08) and (K + 5, K, K) not in cells


def test_ray_degenerate_ends():
    o = np.array(O, F)
    assert M.ray_keys(o, np.array((0.05, 0.07, 0.01), F)) == []           # one voxel
    assert M.ray_keys(o, np.array((3000.0, 0.0, 0.0), F)) is None         # beyond +-2621.44 m
    assert M.ray_keys(np.array((0.0, -2700.0, 0.0), F), o) is None
    assert M.key(F(2621.4), 12.5) == 65535 and M.key(F(2621.5), 12.5) is None
    assert M.key(F(-2621.4), 12.5) == 0 and M.key(F(-2621.5), 12.5) is None


def test_ray_structure_over_random_rays():
    rng = np.random.default_rng(5)
    rf = 1.0 / 0.08
    for _ in range(300):
        o = rng.uniform(-3, 3, 3).astype(F)
        e = (o + rng.normal(0, rng.choice([0.05, 0.5, 3.0]), 3)).astype(F)
        if rng.random() < 0.3:
            e[rng.integers(3)] = o[rng.integers(3)]
        cells = M.ray_keys(o, e)
        ko, ke = M.key3(o, rf), M.key3(e, rf)
        if ko == ke:
            assert cells == []
            continue
        assert cells[0] == ko and ke not in cells and len(set(cells)) == len(cells)
        a = np.array(cells)
        d = np.diff(a, axis=0)
        assert (np.abs(d).sum(1) == 1).all()                      # one step in one axis
        for ax in range(3):
            assert (d[:, ax] >= 0).all() or (d[:, ax] <= 0).all()   # monotone
        assert np.abs(a[-1] - np.array(ke)).sum() <= 3            # ends beside the end voxel


def test_logodds_constants_and_saturation():
    g = M.Params()
    assert [float(v) for v in (g.l_hit, g.l_miss, g.l_min, g.l_max)] == \
        [float(F(x)) for x in (2.1972246, -0.4054651, -6.906755, 6.906755)]
    assert all(v.dtype == np.float32 for v in (g.l_hit, g.l_miss, g.l_min, g.l_max))
    m = M.Map(g)
    p = np.zeros(1, [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("pad", "u1")])
    p["x"], p["y"], p["z"], p["r"] = 0.44, 0.04, 0.04, 9
    T = np.eye(4, dtype=F)[:3]
    hit, free = [], []
    for _ in range(20):
        assert m.insert(p, T, np.array(O, F))
        assert len(m) == 6
        hit.append(m.vox[(K + 5, K, K)][0])
        free.append(m.vox[(K, K, K)][0])
    assert hit[2] < g.l_max and hit[3] == g.l_max and hit[-1] == g.l_max          # the 4th hit saturates
    assert free[16] > g.l_min and free[17] == g.l_min and free[-1] == g.l_min     # the 18th miss saturates
    assert all(v.dtype == np.float32 for v in hit + free)


def test_sensor_pose_is_a_rotation_for_every_shepperd_branch():
    import math
    for ax, ang in (((0, 0, 1), 0.3), ((1, 0, 0), 3.0), ((0, 1, 0), 3.0), ((0, 0, 1), 3.0)):
        a = np.array(ax, float)
        Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        R = np.eye(3) + math.sin(ang) * Kx + (1 - math.cos(ang)) * Kx @ Kx
        T = np.eye(4, dtype=F)
        T[:3, :3] = R.T
        T[:3, 3] = (0.1, -0.2, 0.3)
        Twc, o = M.sensor_pose(T)
        assert np.abs(Twc[:, :3].astype(float) - R).max() < 1e-6
        assert np.abs(o.astype(float) + R @ np.array((0.1, -0.2, 0.3))).max() < 1e-6
