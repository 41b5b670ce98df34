"""GPU: the owning buffer types of rgbd-slam_amd/csrc/devmem.h on a device, and what the context does with
them: teardown releases everything, and the output set a context hands out is its own unless the pipelined
API selected the second one."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_devmem import build_check

pytestmark = pytest.mark.gpu


def test_buffers_on_a_device(tmp_path):
    """tests/devmem_check.cpp, mode "ok": alloc(0) gives a 16-byte buffer, reserve(100) then reserve(150) gives
    capacity 200 in a new allocation (of 800 bytes where the first had 400; the address may be the released
    one again) and a third reserve(150) keeps it, a move-assigned buffer holds its
    source's pointer and leaves the source empty, a DevBuf / PinnedBuf pair round-trips a memset, an Event is
    created once and destroyed once."""
    r = subprocess.run([build_check(tmp_path), "ok"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "devmem_check ok: all checks passed" in r.stdout, r.stdout


def test_teardown_releases_everything():
    """Eight create / use / close cycles in a fresh process (tests/devmem_cycles.py: every workspace of a
    640 x 480, max_batch 4 context is used).  Free device memory after cycle 8 against cycle 2: no drift is
    expected; a quarter of one cycle's footprint is allowed for the runtime's own pooling, which is still
    less than any one leaked workspace."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "devmem_cycles.py")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = json.loads(r.stdout.strip().splitlines()[-1])
    drift = m["free2"] - m["free8"]
    print("footprint %d B, free after cycle 2 %d B, after cycle 8 %d B, drift %d B"
          % (m["footprint"], m["free2"], m["free8"], drift))
    assert m["footprint"] > 0
    assert drift <= m["footprint"] // 4, m


def _outputs(pkg, ctx):
    p = [C.c_void_p() for _ in range(5)]
    assert pkg.lib().rgbd_batch_outputs(ctx._h, *[C.byref(q) for q in p]) == 0
    return [q.value for q in p]


def test_output_set_addresses_and_pipelined_read_back(pkg, seq_fr1):
    """rgbd_batch_outputs of a context that only extracted returns the same addresses before and after an
    unrelated GICP call; a context that ran submit / collect steps (its latest submission wrote the second
    output set) reads back, frame by frame, the bits of a context that only extracted the same input."""
    import torch
    bgr, depth, _, cam = seq_fr1
    B = len(bgr)
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"],
                   cam["factor"])
    d_bgr = torch.from_numpy(np.ascontiguousarray(bgr)).cuda()
    d_dep = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda()
    plain = pkg.Context(640, 480, max_batch=B, orb=pkg.orb_params(1000), cam=c)
    piped = pkg.Context(640, 480, max_batch=B, orb=pkg.orb_params(1000), cam=c)
    try:
        plain.extract_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B)
        before = _outputs(pkg, plain)
        assert all(before) and len(set(before)) == 5
        rs = np.random.RandomState(5)
        src = (rs.rand(300, 3) * [2.0, 1.5, 2.0] + [-1.0, -0.75, 1.0]).astype(np.float32)
        plain.gicp(src, src + np.float32([0.01, -0.005, 0.008]), np.eye(4, dtype=np.float32))
        assert _outputs(pkg, plain) == before
        own = _outputs(pkg, piped)
        for _ in range(2):   # the second submission writes output set 1
            piped.pnp_track_submit(d_bgr.data_ptr(), d_dep.data_ptr(), B, 0.9)
        for _ in range(2):
            piped.pnp_track_collect()
        second = _outputs(pkg, piped)
        assert all(second) and not set(second) & set(own)
        for b in range(B):
            want, got = plain.batch_frame(b), piped.batch_frame(b)
            assert len(want["kps"]) > 500
            for k in ("kps", "kps_un", "desc", "xyz"):
                assert want[k].tobytes() == got[k].tobytes(), (b, k)
    finally:
        plain.close()
        piped.close()
