"""CPU: the extraction geometry (csrc/geometry.cpp), exercised by tests/geometry_check.cpp (own main, geometry.cpp
alone) under the host sanitizers.

a) the bytes of every table at the shapes of the GPU parity tests, and the documented refusals, are those recorded
   from the function before it left api.cpp (tests/geometry_cases.py);
b) what the kernels take on trust holds over a sweep of 1232 configurations, of which at least half must be
   accepted.  The quadtree's LDS rule, dist_node_bytes + 64 + dist_key_bytes(dist_kc) <= RGBD_DIST_LDS_KB KiB, can
   only hold where the node arrays fit that budget (node_cap <= 256 at these cell counts), so the sweep that asserts
   it as it stands runs at 240 features: one level then takes all of them and node_cap is 256.  At 1000 features 1
   and 4 levels give node_cap 1024 / 512, node arrays of 96,336 / 48,208 B on their own and dist_kc = 0 (the keys
   stay in HBM, the launch asks for the larger LDS): a second sweep at 1000 features checks everything else as it
   stands and, for those configurations, dist_kc == 0;
c) level sizes, budgets, scale factors and umax equal the CPU oracle's tables, exactly."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from geometry_cases import CASES, OK, SWEEP_CONFIGS


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    csrc = os.path.join(ROOT, "rgbd-slam_amd", "csrc")
    exe = os.path.join(str(tmp_path_factory.mktemp("geometry")), "geometry_check")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", csrc, os.path.join(ROOT, "tests", "geometry_check.cpp"),
           os.path.join(csrc, "geometry.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def run(exe, *args):
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout.strip().splitlines()


@pytest.fixture(scope="module")
def case_blocks(check_exe):
    """One block of output lines per case of CASES, in order."""
    lines = run(check_exe, "case", *[v for c in CASES for v in c[:5]])
    blocks = []
    for l in lines:
        if l.startswith("CASE "):
            blocks.append([])
        blocks[-1].append(l)
    assert len(blocks) == len(CASES)
    return blocks


def test_geometry_bytes_match_recorded(case_blocks):
    for (W, H, nf, nl, sc, status, msg, cells, segs, digest), block in zip(CASES, case_blocks):
        head, _, got_msg = block[0].partition(" msg ")
        f = head.split()
        assert f[1:6] == [str(W), str(H), str(nf), str(nl), sc], block[0]
        assert int(f[7]) == status and got_msg == msg, block[0]
        if status == OK:
            assert (int(f[9]), int(f[11]), f[13]) == (cells, segs, digest), block[0]


@pytest.mark.parametrize("nfeatures,strict", [(240, 1), (1000, 0)])
def test_geometry_invariants(check_exe, nfeatures, strict):
    last = run(check_exe, "sweep", nfeatures, strict)[-1].split()
    assert last[:4] == ["SWEEP", "nfeatures", str(nfeatures), "configs"], last
    configs, accepted, fails = int(last[4]), int(last[6]), int(last[8])
    assert configs == SWEEP_CONFIGS and fails == 0, last
    assert 2 * accepted >= configs, last


def test_geometry_levels_match_oracle(case_blocks, oracle):
    checked = 0
    for (W, H, nf, nl, sc, status, *_), block in zip(CASES, case_blocks):
        if status != OK:
            continue
        t = oracle.tables(oracle.orb_params(nf, float(sc), nl), W, H)
        lv = [l.split() for l in block if l.startswith("LV ")]
        assert [int(l[1]) for l in lv] == list(range(nl)), block[0]
        assert [int(l[2]) for l in lv] == t["w"].tolist(), block[0]
        assert [int(l[3]) for l in lv] == t["h"].tolist(), block[0]
        assert [int(l[4]) for l in lv] == t["nfeat"].tolist(), block[0]
        assert [int(l[5], 16) for l in lv] == t["scale"].view(np.uint32).tolist(), block[0]
        umax = [l for l in block if l.startswith("UMAX")]
        assert len(umax) == 1 and [int(v) for v in umax[0].split()[1:]] == t["umax"].tolist(), block[0]
        checked += 1
    assert checked == sum(c[5] == OK for c in CASES) >= 10
