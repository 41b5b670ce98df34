"""The occupancy map's upkeep over OccupancyMap (rgbd_occmap_*), as the reference's map drawer drives its octomap:

  sensor_pose    <- Frame::updateSensor (Core/Frame.cpp:551-608): the f32 [R' | Ow] that takes a keyframe's cloud to
                    the world on the device, and the scan's origin Ow
  MapBuilder     <- MapDrawer::drawOctomap (Drawer/MapDrawer.cpp:48-71) over OctomapDrawer::insertCloud
                    (Drawer/OctomapDrawer.cpp:38-59): a keyframe id is inserted once; when the big-change index moves
                    (a loop closure corrected the poses) the map is cleared and every keyframe inserted again, in
                    keyframe order with its current pose, as one batch on the device
  render_leaves  <- OctomapDrawer::render's query (:133-156): the leaves with occupancy >= 0.9, their centres and
                    half size (the GL drawing itself is the viewer's, not built)
The definition is DESIGN.md "Occupancy map definition"; parity with liboctomap is unpinned.
"""
from __future__ import annotations

import numpy as np

from . import OccupancyMap, RgbdError, lib, occmap_params, _ptr

TMAX = 32768
RENDER_OCCUPANCY = 0.9   # OctomapDrawer::render's occThresh


def sensor_pose(Tcw):
    """(Twc34 (3, 4) f32, origin (3,) f32) of a keyframe pose Tcw (4x4): rgbd_occmap_sensor_pose."""
    T = np.ascontiguousarray(Tcw, np.float32).reshape(4, 4)
    Twc34, o = np.zeros((3, 4), np.float32), np.zeros(3, np.float32)
    st = lib().rgbd_occmap_sensor_pose(_ptr(T), _ptr(Twc34), _ptr(o))
    if st != 0:
        raise RgbdError(f"occmap_sensor_pose: status {st} (a pose that is not finite)")
    return Twc34, o


class MapBuilder:
    """MapDrawer::drawOctomap's rule over one OccupancyMap."""

    def __init__(self, ctx, prm=None, maxrange: float = -1.0):
        self.map = OccupancyMap(ctx, prm or occmap_params())
        self.maxrange = float(maxrange)
        self.inserted = set()        # OctomapDrawer::msIdxs
        self.last_big_change = 0     # MapDrawer::mLastBigChange

    def close(self):
        self.map.close()

    def update(self, keyframes, big_change_idx: int = 0) -> int:
        """keyframes: (id, cloud, Tcw) in keyframe order, cloud = the keyframe's rgbd_points (None: no valid cloud), Tcw
        its current pose.  Returns the number of scans applied; a table too small raises."""
        if big_change_idx != self.last_big_change:
            self.last_big_change = big_change_idx
            self.map.clear()
            self.inserted.clear()
        todo = [(kid, cloud, Tcw) for kid, cloud, Tcw in keyframes if cloud is not None and kid not in self.inserted]
        if not todo:
            return 0
        poses = [sensor_pose(Tcw) for _, _, Tcw in todo]
        applied = self.map.insert_batch([c for _, c, _ in todo], np.stack([p[0] for p in poses]),
                                        np.stack([p[1] for p in poses]), self.maxrange)
        self.inserted.update(kid for kid, _, _ in todo[:applied])
        if applied < len(todo):
            raise RgbdError(f"occupancy map: keyframe {todo[applied][0]} does not fit a table of "
                            f"{self.map.prm.capacity} voxels ({applied} of {len(todo)} scans applied)")
        return applied


def occmap_sequence(pkg, get_frame, camera: dict, poses, kfs, capacity: int = 1 << 22, maxrange: float = -1.0,
                    device: int = 0, W: int = 640, H: int = 480):
    """The map of a tracked sequence: the clouds of the keyframes `kfs` (Tracking::createKeyFrame's, on the device) under
    their poses poses[k] (Tcw, e.g. the pose graph's corrected ones), inserted in keyframe order.  Returns (keys,
    occupancy probabilities, log-odds, rgb) of every leaf."""
    c = pkg.camera(camera["fx"], camera["fy"], camera["cx"], camera["cy"], camera["k1"], camera["k2"], camera["p1"],
                   camera["p2"], camera["k3"], camera["factor"])
    ctx = pkg.Context(W, H, max_batch=1, cam=c, device=device)
    try:
        b = MapBuilder(ctx, pkg.occmap_params(capacity=capacity), maxrange)
        try:
            frames = []
            for k in kfs:
                bgr, depth = get_frame(k)
                cloud = ctx.keyframe_cloud(bgr, depth)
                frames.append((int(k), cloud if len(cloud) else None, poses[k]))
            b.update(frames)
            keys, lo, rgb = b.map.leaves()
        finally:
            b.close()
    finally:
        ctx.close()
    return keys, 1.0 - 1.0 / (1.0 + np.exp(lo.astype(np.float64))), lo, rgb


def render_leaves(m: OccupancyMap):
    """What OctomapDrawer::render draws: (centres (n, 3) f64, half size, rgb (n, 3) u8, occupancy (n,) f64) of the
    leaves with occupancy >= 0.9; a centre is coord(k) = ((k - 32768) + 0.5) * res."""
    keys, lo, rgb = m.leaves(min_prob=RENDER_OCCUPANCY)
    res = float(m.prm.resolution)
    centres = ((keys.astype(np.float64) - TMAX) + 0.5) * res
    occ = 1.0 - 1.0 / (1.0 + np.exp(lo.astype(np.float64)))
    return centres, res / 2.0, rgb, occ
