"""Seeded keyframe-cloud inputs (test infrastructure), one per edge regime of cloud.hip: empty clouds, one
point, fewer points than neighbours, exact ties at the k-th neighbour distance, a leaf too small for the int
voxel index, the 16384-sample capacity, one long voxel run, the inclusive pass-through limits, sor_k at 1
and 63.  tests/test_cloud_cases.py asserts from the oracle alone that each case reaches its regime.

128 x 128 image, fx = fy = 128, cx = cy = 64, no distortion, factor 5000: depth 5000 is z = 1.0f and the
x / y of such a pixel are exact dyadic fractions."""
import numpy as np

W = H = 128
CAM = dict(fx=128.0, fy=128.0, cx=64.0, cy=64.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, factor=5000.0)
DEFAULTS = dict(stride=6, zmin=0.5, zmax=4.0, leaf=0.04, sor_k=50, sor_std=1.0)   # Tracking::createKeyFrame's

NAMES = ["empty_zero", "empty_range", "one_point", "two_points", "few_points", "plane_ties", "plane_ties_k8",
         "tiny_leaf", "one_voxel", "k63", "k1", "holes", "limits", "std0", "plane_ties_k63"]


def scale():
    """mDepthMapFactor as the camera holds it (f32)."""
    return np.float32(1.0) / np.float32(CAM["factor"])


def depth_f32(depth):
    """Frame::mImDepth: convertTo(CV_32F, 1/factor) of the u16 depth."""
    return depth.astype(np.float32) * scale() + np.float32(0.0)


def random_bgr(seed):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def random_depth(seed, zeros=0.0):
    """Depths strictly inside the default pass-through limits; a fraction `zeros` of the pixels invalid."""
    rs = np.random.default_rng(seed)
    d = rs.integers(2501, 20000, size=(H, W)).astype(np.uint16)
    if zeros > 0:
        d[rs.random((H, W)) < zeros] = 0
    return d


def case(name):
    """(bgr, depth_u16, cam dict, CloudParams keyword arguments) of the named case."""
    bgr = random_bgr(100 + NAMES.index(name))
    d = np.zeros((H, W), np.uint16)
    kw = dict(DEFAULTS)
    if name == "empty_zero":
        kw.update(stride=1)
    elif name == "empty_range":
        d[:] = 1000   # 0.2 m, below zmin
        kw.update(stride=1)
    elif name == "one_point":
        d[37, 91] = 7000
        kw.update(stride=1)
    elif name == "two_points":
        d[5, 9] = 4000
        d[120, 100] = 15000
        kw.update(stride=1)
    elif name == "few_points":
        d[60:63, 70:73] = np.random.default_rng(0).integers(4000, 6001, size=(3, 3))
        kw.update(stride=1, leaf=0.001)
    elif name == "plane_ties":
        d[:] = 5000
        kw.update(stride=1, leaf=1.0 / 32)
    elif name == "plane_ties_k8":
        d[:] = 5000
        kw.update(stride=1, leaf=1.0 / 16, sor_k=8)
    elif name == "plane_ties_k63":
        # k + 1 = 64 fills every lane of the cross-lane sort, and values equal to the 64th smallest are left over
        d[:] = 5000
        kw.update(stride=1, leaf=1.0 / 32, sor_k=63)
    elif name == "tiny_leaf":
        d = random_depth(11)
        kw.update(stride=1, leaf=1e-5)
    elif name == "one_voxel":
        d = random_depth(11)
        kw.update(stride=1, leaf=100.0)
    elif name == "k63":
        d = random_depth(11)
        kw.update(stride=2, sor_k=63)
    elif name == "k1":
        d = random_depth(11)
        kw.update(stride=2, sor_k=1)
    elif name == "holes":
        d = random_depth(12, zeros=0.3)
        kw.update(stride=1)
    elif name == "limits":
        # 2 x 2 pixel blocks, so that the stride-2 samples see all four values
        r, c = np.indices((H, W))
        d = np.array([[2500, 2499], [20000, 20001]], np.uint16)[(r >> 1) & 1, (c >> 1) & 1]
        kw.update(stride=2, zmin=float(np.float32(2500) * scale()), zmax=float(np.float32(20000) * scale()))
    elif name == "std0":
        d = random_depth(13)
        kw.update(stride=2, sor_std=0.0)
    else:
        raise KeyError(name)
    return bgr, np.ascontiguousarray(d), dict(CAM), kw


_STAGES = {}


def stages(oracle, bgr, depth, cam, kw):
    """The oracle's stages for one input: dict(cloud, voxel, out, dist)."""
    pts = oracle.cloud(bgr, depth, cam, res=kw["stride"], zmin=kw["zmin"], zmax=kw["zmax"])
    vox = oracle.voxel(pts, leaf=kw["leaf"])
    out, dist = oracle.sor(vox, k=kw["sor_k"], std_mul=kw["sor_std"])
    return dict(cloud=pts, voxel=vox, out=out, dist=dist[:len(vox)])


def case_stages(oracle, name):
    """stages() of a named case, computed once per process and shared (do not modify)."""
    if name not in _STAGES:
        _STAGES[name] = stages(oracle, *case(name))
    return _STAGES[name]


def sq_dist(points):
    """All pairwise squared distances as FLANN's L2_Simple<float> forms them: ((dx^2 + dy^2) + dz^2) in f32."""
    x, y, z = (points[a].astype(np.float32) for a in "xyz")
    dx, dy, dz = x[:, None] - x[None, :], y[:, None] - y[None, :], z[:, None] - z[None, :]
    return (dx * dx + dy * dy) + dz * dz
