"""CPU: the occupancy map's entry points are declared, bound and exported, its kernels are built for gfx950, and the
host-only parts (argument checks, rgbd_occmap_sensor_pose) work without a device."""
import ctypes as C
import re
import subprocess

import numpy as np

import occmap_model as M

NAMES = ["rgbd_occmap_create", "rgbd_occmap_destroy", "rgbd_occmap_clear", "rgbd_occmap_size", "rgbd_occmap_insert",
         "rgbd_occmap_insert_batch", "rgbd_occmap_leaves", "rgbd_occmap_sensor_pose"]


def test_occmap_symbols_declared_bound_and_exported(pkg):
    lib = pkg.lib()
    header = re.sub(r"/\*.*?\*/", "", open(pkg.HEADER).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (rgbd_\w+)", out))
    for n in NAMES:
        assert n in pkg.exported_symbols() and n in exported and re.search(r"\b%s\s*\(" % n, header), n
        getattr(lib, n)
    blob = open(pkg.LIB_PATH, "rb").read()
    for k in (b"k_occ_mark", b"k_occ_apply", b"k_occ_colour"):
        assert k in blob, k
    assert C.sizeof(pkg.OccmapParams) == 48


def test_occmap_checks_arguments_without_a_device(pkg):
    lib = pkg.lib()
    h = C.c_void_p()
    assert lib.rgbd_occmap_create(None, C.byref(pkg.occmap_params()), C.byref(h)) == 4 and not h.value
    assert lib.rgbd_occmap_insert(None, None, 0, None, None, -1.0) == 4
    assert lib.rgbd_occmap_clear(None) == 4 and lib.rgbd_occmap_size(None, None) == 4
    lib.rgbd_occmap_destroy(None)
    assert [float(pkg.occmap_logodds(p)) for p in (0.9, 0.4, 0.001, 0.999)] == \
        [float(np.float32(v)) for v in (2.1972246, -0.4054651, -6.906755, 6.906755)]


def test_sensor_pose_equals_model_on_the_host(pkg):
    from rgbd_slam_amd import occmap
    rng = np.random.default_rng(9)
    poses = []
    for _ in range(40):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = R
        T[:3, 3] = rng.normal(size=3)
        poses.append(T)
    branches = set()
    for T in poses:
        got, want = occmap.sensor_pose(T), M.sensor_pose(T)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        Rwc = T[:3, :3].T
        branches.add(-1 if np.trace(Rwc) > 0 else int(np.argmax(np.diag(Rwc))))
    assert branches == {-1, 0, 1, 2}
    bad = np.eye(4, dtype=np.float32)
    bad[2, 1] = np.nan
    try:
        occmap.sensor_pose(bad)
        assert False, "a pose that is not finite must be refused"
    except pkg.RgbdError:
        pass
