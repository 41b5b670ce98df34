"""CPU: the inputs of tests/occmap_cases.py hit the rules they are named for, on the Python model alone, so a case that
drifts is caught without a device."""
import numpy as np

import occmap_cases as OC
import occmap_model as M


def test_cases_exercise_their_rules():
    """The cases hit what they are named for (model only, so a case that drifts is caught without a device)."""
    def run(name):
        cap, scans = OC.CASES[name]
        r = M.Map(M.Params(capacity=cap))
        for s in scans:
            assert r.insert(*s)
        return r
    g = M.Params()
    K = 32768
    for name in OC.CASES:       # every case fits its table
        run(name)
    assert len(run("same_voxel")) == 1
    r = run("end_on_other_ray")
    assert r.vox[(K + 5, K, K)][0] == g.l_hit and run("end_on_other_ray_swapped").leaves()[1].tolist() == r.leaves()[1].tolist()
    a, b = run("forty_in_one_voxel"), run("forty_in_one_voxel_reversed")
    assert len(a) == len(b) == 6 and a.vox[(K + 5, K, K)][0] == g.l_hit and a.vox[(K + 5, K, K)][1:] != b.vox[(K + 5, K, K)][1:]
    assert run("white_then_colour").vox[(K + 5, K, K)][1:] == [7, 90, 200]
    assert run("white_voxel_hit_again").vox[(K + 5, K, K)][1:] == [50, 26, 137]
    assert run("saturate_20").vox[(K + 5, K, K)][0] == g.l_max and run("saturate_20").vox[(K, K, K)][0] == g.l_min
    assert run("hit_after_l_min").vox[(K + 5, K, K)][0] == np.float32(g.l_min + g.l_hit)
    r = run("maxrange_far")
    occ = [k for k, v in r.vox.items() if v[0] > 0]
    assert occ == [(K + 25, K, K)] and r.vox[occ[0]][1:] == [120, 80, 65] and len(r) > 20
    r = run("maxrange_exact")
    assert sum(v[0] > 0 for v in r.vox.values()) == 1
    assert len(run("bad_points")) == 6 and len(run("far_origin")) == 1
    assert 45 <= len(run("wrap_64")) <= 60
    cap, scans = OC.OVERFLOW
    r = M.Map(M.Params(capacity=cap))
    assert r.insert(*scans[0]) and not r.insert(*scans[1]) and r.insert(*scans[2]) and 25 <= len(r) <= 64
