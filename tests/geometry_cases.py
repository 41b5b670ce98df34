"""Expected geometry of tests/test_geometry.py: per case the status, the refusal's message, the table sizes and the
FNV-1a digest (start value 1469598103934665603, prime 1099511628211) over the bytes of cfg, cells, segs, rsx, rsy, qx
and blur_tab, in that order.

The values were recorded from build_geometry() as it stood inside csrc/api.cpp at commit 7d3e857, before it moved
to csrc/geometry.cpp, with the camera fx = fy = 525, cx = W / 2, cy = H / 2, depth_map_factor = 5000 and the ORB
parameters {nfeatures, scale, nlevels, 20, 7}.  They pin the bytes the kernels are handed: a change to them is a
change of the device tables and needs the GPU parity tests, never a re-record from the code under test alone.

The shapes are those of the GPU parity tests (test_gpu_fast_segments, test_gpu_pyramid_shapes, the default
configuration) and the documented refusals."""

OK, UNSUPPORTED = 0, 4

# (W, H, nfeatures, nlevels, scale, status, message, cells, segs, digest)
CASES = [
    (640, 480, 1000, 8, "1.2", OK, "", 815, 215, "514114230602c335"),
    (368, 240, 1000, 8, "1.2", OK, "", 176, 50, "3368ddcce5fb79e0"),
    (512, 384, 1000, 8, "1.2", OK, "", 484, 138, "0514a07c6074ada7"),
    (640, 480, 1000, 3, "1.2", OK, "", 602, 152, "dc778eb0504601c4"),
    (640, 480, 1000, 10, "1.2", OK, "", 827, 219, "92c3cf3f5a23b198"),
    (640, 480, 1000, 6, "1.25", OK, "", 682, 182, "ef13ba2a979f0038"),
    (3200, 240, 1000, 8, "1.2", OK, "", 1748, 444, "2a55799b5558b675"),
    (640, 480, 1000, 1, "1.2", OK, "", 280, 70, "765623df17e631ef"),
    (64, 80, 100, 1, "1.2", OK, "", 1, 1, "bf7334f34a3be34d"),
    (1280, 720, 2000, 8, "1.2", OK, "", 2656, 675, "a262184441f6f9af"),
    (4800, 240, 1000, 8, "1.2", UNSUPPORTED, "pyramid strip does not fit in LDS", None, None, None),
    (376, 240, 1000, 8, "1.2", UNSUPPORTED, "width must be a multiple of 16 and >= 64", None, None, None),
    (640, 480, 1000, 6, "1.5", UNSUPPORTED, "FAST cell ROI larger than 48 px", None, None, None),
]

# the invariant sweep of geometry_check: W in 64..1280 step 16, H in {80, 240, 480, 720}, nlevels in {1, 4, 8, 12}
SWEEP_CONFIGS = 77 * 4 * 4
