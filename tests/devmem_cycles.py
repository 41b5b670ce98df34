"""Child process of tests/test_gpu_devmem.py: create / use / close cycles of one context; prints, as one JSON
line, the free device memory after cycles 2 and 8 and one cycle's footprint (free memory before the create
minus free memory after the use, in cycle 2)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_pkg, synth_seq   # noqa: E402


def main(cycles=8):
    import torch
    pkg = load_pkg()
    B = 4
    bgr, depth, _, cam = synth_seq(B, seed=3, preset="fr1")
    c = pkg.camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"],
                   cam["factor"])
    d_bgr = torch.from_numpy(np.ascontiguousarray(bgr)).cuda()
    d_dep = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda()
    rs = np.random.RandomState(5)
    src = (rs.rand(300, 3) * [2.0, 1.5, 2.0] + [-1.0, -0.75, 1.0]).astype(np.float32)
    tgt = (src + np.float32([0.01, -0.005, 0.008])).astype(np.float32)

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    out = {}
    for cyc in range(1, cycles + 1):
        before = free()
        ctx = pkg.Context(640, 480, max_batch=B, orb=pkg.orb_params(1000), cam=c)
        ctx.pnp_track_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B, 0.9)
        for _ in range(2):
            ctx.pnp_track_submit(d_bgr.data_ptr(), d_dep.data_ptr(), B, 0.9)
        for _ in range(2):
            ctx.pnp_track_collect()
        ctx.track_lanes(d_bgr.data_ptr(), d_dep.data_ptr(), B, 0.9, pkg.ransac_params(), 2, [pkg.rng(1), pkg.rng(2)],
                        [pkg.Sticky(), pkg.Sticky()])
        ctx.gicp(src, tgt, np.eye(4, dtype=np.float32))
        ctx.keyframe_cloud(bgr[0], depth[0])
        used = free()
        ctx.close()
        if cyc == 2:
            out["footprint"] = before - used
            out["free2"] = free()
        if cyc == cycles:
            out["free8"] = free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
