"""GPU: a plain bench.py run times exactly --steps steps, prints the headline alone, and --dump-outputs writes
what its last timed step returned: the same bits the library returns in this process for the same seeded frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, synth_seq

pytestmark = pytest.mark.gpu

B, U = 16, 4   # the smallest shape with the walk back over the rendered frames (0 1 2 3 2 1 0 1 ...)


def test_plain_bench_dumps_last_step_outputs(pkg, tmp_path):
    import torch
    import synth
    import rgbd_slam_amd.dist as D
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                          "--batch", str(B), "--unique", str(U), "--dump-outputs", str(tmp_path / "dump")],
                         capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["unit"] == "frames/s" and line["higher_is_better"]
    assert abs(line["value"] - B * 1e3 / line["ms_per_step"]) <= 0.01 * line["value"]
    # the headline alone: nothing of --full was measured
    assert line["full"] is False
    for k in ("roofline", "cpu_baseline", "flag_chain", "flag_chain_one", "se3_chain_one", "se3_chain_one_cfg3",
              "lowtex", "extract_stage", "kernels_hbm", "ate_rmse_m"):
        assert line[k] is None, k
    assert line["kernels_ms_warmup"] == {}

    got = {n[:-4]: np.load(tmp_path / "dump" / n) for n in sorted(os.listdir(tmp_path / "dump"))}
    assert sorted(got) == ["n_inliers", "n_matches", "poses", "status"]
    assert all(a.dtype == np.float32 for a in got.values())

    # the same frames through the library here (the bench's workload: dist.workload, frames walked back and forth)
    n_global, lo, hi, seed = D.workload("chunks", B, 1, 0)
    assert (n_global, lo, hi) == (B, 0, B)
    ub, ud, _, cam = synth_seq(U, seed=seed, preset="fr1")
    r = np.arange(B) % (2 * U - 2)
    src = np.where(r < U, r, 2 * U - 2 - r)
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"],
                   cam["k3"], cam["factor"])
    ctx = pkg.Context(640, 480, max_batch=B, orb=pkg.orb_params(1000), cam=c)
    d_bgr = torch.from_numpy(ub[src]).cuda()
    d_dep = torch.from_numpy(np.ascontiguousarray(ud[src]).view(np.int16)).cuda()
    pose0 = synth.trajectory(U, seed=seed)[src][0].astype(np.float32)
    poses, status, ninl, nm = ctx.pnp_track_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B, 0.9,
                                                  pkg.pnp_params(500, 3.0, 0.85, 10), pose0)
    ctx.close()
    assert status[1:].mean() > 0.9   # tracked frames: the dump compared below is not a batch of failures
    assert np.array_equal(got["poses"].view(np.uint32), poses.reshape(B, 16).view(np.uint32))
    assert np.array_equal(got["status"], status.astype(np.float32))
    assert np.array_equal(got["n_inliers"], ninl.astype(np.float32))
    assert np.array_equal(got["n_matches"], nm.astype(np.float32))
