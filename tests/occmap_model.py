"""The occupancy map definition (DESIGN.md "Occupancy map definition") in plain Python / numpy: octomap::ColorOcTree as
OctomapDrawer drives it (Drawer/OctomapDrawer.cpp:15-79), leaves at depth 16 only.  A map is a dict from the key triple
to [logodds f32, r, g, b].  Where the definition says f32 the value is an np.float32; f64 values are Python floats."""
import math
import sys

import numpy as np

F = np.float32
TMAX = 32768
DBL_MAX = sys.float_info.max
MAX_POINTS = 16384


def logodds(p):
    """(float)log(p / (1 - p)) with the f64 libm log."""
    return F(math.log(p / (1.0 - p)))


class Params:
    def __init__(self, res=0.08, prob_hit=0.9, prob_miss=0.4, clamp_min=0.001, clamp_max=0.999, capacity=1 << 16):
        self.res = float(res)
        self.rf = 1.0 / self.res
        self.l_hit, self.l_miss = logodds(prob_hit), logodds(prob_miss)
        self.l_min, self.l_max = logodds(clamp_min), logodds(clamp_max)
        self.capacity = int(capacity)


def key(c, rf):
    """One axis: (int)floor(rf * (double)c) + tmax, None when outside [0, 65536)."""
    f = math.floor(rf * float(c))
    if not (-TMAX <= f < TMAX):
        return None
    return int(f) + TMAX


def key3(p, rf):
    k = (key(p[0], rf), key(p[1], rf), key(p[2], rf))
    return None if None in k else k


def coord(k, res):
    return (float(k - TMAX) + 0.5) * res


def _sign(x):
    return int(x > 0) - int(x < 0)


def ray_keys(o, e, res=0.08):
    """computeRayKeys(o, e), o and e f32 triples: the list of key triples, key(o) first, key(e) never; None when a key
    is invalid (the ray yields nothing), [] when both ends share a voxel."""
    o, e = np.asarray(o, F), np.asarray(e, F)
    rf = 1.0 / res
    ko, ke = key3(o, rf), key3(e, rf)
    if ko is None or ke is None:
        return None
    if ko == ke:
        return []
    cells = [ko]
    with np.errstate(all="ignore"):
        d = e - o
        nsq = F(F(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        length = F(math.sqrt(float(nsq)))
        d = d / length
    step, tmax, tdelta = [0, 0, 0], [DBL_MAX] * 3, [DBL_MAX] * 3
    cur = list(ko)
    for i in range(3):
        step[i] = _sign(d[i])
        if step[i] != 0:
            border = coord(cur[i], res) + float(F(step[i] * res * 0.5))
            di = float(d[i])
            tmax[i] = (border - float(o[i])) / di
            tdelta[i] = res / abs(di)
    flen = float(length)
    while True:
        if tmax[0] < tmax[1]:
            dim = 0 if tmax[0] < tmax[2] else 2
        else:
            dim = 1 if tmax[1] < tmax[2] else 2
        cur[dim] += step[dim]
        tmax[dim] += tdelta[dim]
        if not (0 <= cur[dim] < 2 * TMAX):   # a walk that leaves the key range ends (never reached between valid ends)
            break
        if tuple(cur) == ke:
            break
        if min(min(tmax[0], tmax[1]), tmax[2]) > flen:
            break
        cells.append(tuple(cur))
    return cells


def transform(Twc34, xyz):
    """x' = ((R'00*x + R'01*y) + R'02*z) + Ow_x in f32, row by row."""
    T = np.asarray(Twc34, F).reshape(3, 4)
    p = np.asarray(xyz, F).reshape(-1, 3)
    out = np.empty_like(p)
    with np.errstate(all="ignore"):
        for r in range(3):
            out[:, r] = ((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3]
    return out


class Map:
    def __init__(self, prm=None):
        self.prm = prm or Params()
        self.vox = {}

    def clear(self):
        self.vox = {}

    def __len__(self):
        return len(self.vox)

    def scan_sets(self, world, origin, maxrange):
        """The free and occupied key sets of one scan (world: finite f32 points)."""
        g = self.prm
        free, occ = set(), set()
        o = np.asarray(origin, F)
        for p in world:
            with np.errstate(all="ignore"):
                d = p - o
                nsq = F(F(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            norm = math.sqrt(float(nsq))
            if maxrange < 0 or norm <= maxrange:
                free.update(ray_keys(o, p, g.res) or ())
                k = key3(p, g.rf)
                if k is not None:
                    occ.add(k)
            else:
                with np.errstate(all="ignore"):
                    e = o + (d / F(norm)) * F(maxrange)
                free.update(ray_keys(o, e, g.res) or ())
                k = key3(e, g.rf)
                if k is not None:
                    free.add(k)
        return free - occ, occ

    def insert(self, pts, Twc34, origin, maxrange=-1.0):
        """One scan of rgbd_points (camera frame, BGR bytes).  False, and the map untouched, when the scan's voxels do
        not fit the capacity."""
        g = self.prm
        assert len(pts) <= MAX_POINTS
        cam = np.stack([pts["x"], pts["y"], pts["z"]], 1).astype(F).reshape(-1, 3)
        world = transform(Twc34, cam)
        ok = np.isfinite(cam).all(1) & np.isfinite(world).all(1)
        world = world[ok]
        rgb = np.stack([pts["r"], pts["g"], pts["b"]], 1).reshape(-1, 3)[ok]
        free, occ = self.scan_sets(world, origin, float(maxrange))
        new = [k for k in free | occ if k not in self.vox]
        if len(self.vox) + len(new) > g.capacity:
            return False
        for ks, l in ((free, g.l_miss), (occ, g.l_hit)):
            for k in ks:
                leaf = self.vox.setdefault(k, [F(0.0), 255, 255, 255])
                v = F(leaf[0] + l)
                leaf[0] = min(max(v, g.l_min), g.l_max)
        for p, c in zip(world, rgb):
            k = key3(p, g.rf)
            leaf = self.vox.get(k) if k is not None else None
            if leaf is None:
                continue
            if tuple(leaf[1:]) != (255, 255, 255):
                leaf[1:] = [(int(leaf[1 + j]) + int(c[j])) // 2 for j in range(3)]
            else:
                leaf[1:] = [int(c[0]), int(c[1]), int(c[2])]
        return True

    def leaves(self, min_logodds=-math.inf):
        """(keys (n, 3) u16, logodds (n,) f32, rgb (n, 3) u8), ascending by (kx << 32) | (ky << 16) | kz."""
        ks = sorted(k for k, leaf in self.vox.items() if leaf[0] >= min_logodds)
        keys = np.array(ks, np.uint16).reshape(-1, 3)
        lo = np.array([self.vox[k][0] for k in ks], F)
        rgb = np.array([self.vox[k][1:] for k in ks], np.uint8).reshape(-1, 3)
        return keys, lo, rgb


def sensor_pose(Tcw):
    """Frame::updateSensor's pose (Core/Frame.cpp:551-608): Twc34 = [R' | Ow] (3x4 f32) and the origin Ow, R' the f32
    rotation of Eigen::Quaternionf(Rwc)."""
    T = np.asarray(Tcw, F).reshape(4, 4)
    Rwc = T[:3, :3].T.copy()
    Ow = np.zeros(3, F)
    for r in range(3):
        s = 0.0
        for k in range(3):
            s += float(T[k, r]) * float(T[k, 3])
        Ow[r] = F(-s)
    m = Rwc
    one, half = F(1.0), F(0.5)
    with np.errstate(all="ignore"):
        t = F(F(m[0, 0] + m[1, 1]) + m[2, 2])
        q = [F(0)] * 3
        if t > 0:
            t = F(np.sqrt(F(t + one)))
            w = F(half * t)
            t = F(half / t)
            q[0] = F(F(m[2, 1] - m[1, 2]) * t)
            q[1] = F(F(m[0, 2] - m[2, 0]) * t)
            q[2] = F(F(m[1, 0] - m[0, 1]) * t)
        else:
            i = 0
            if m[1, 1] > m[0, 0]:
                i = 1
            if m[2, 2] > m[i, i]:
                i = 2
            j, k = (i + 1) % 3, (i + 2) % 3
            t = F(np.sqrt(F(F(F(m[i, i] - m[j, j]) - m[k, k]) + one)))
            q[i] = F(half * t)
            t = F(half / t)
            w = F(F(m[k, j] - m[j, k]) * t)
            q[j] = F(F(m[j, i] + m[i, j]) * t)
            q[k] = F(F(m[k, i] + m[i, k]) * t)
        x, y, z = q
        two = F(2.0)
        tx, ty, tz = F(two * x), F(two * y), F(two * z)
        twx, twy, twz = F(tx * w), F(ty * w), F(tz * w)
        txx, txy, txz = F(tx * x), F(ty * x), F(tz * x)
        tyy, tyz, tzz = F(ty * y), F(tz * y), F(tz * z)
        R = np.array([[one - F(tyy + tzz), F(txy - twz), F(txz + twy)],
                      [F(txy + twz), one - F(txx + tzz), F(tyz - twx)],
                      [F(txz - twy), F(tyz + twx), one - F(txx + tyy)]], F)
    Twc34 = np.concatenate([R, Ow.reshape(3, 1)], 1).astype(F)
    return Twc34, Ow.copy()
