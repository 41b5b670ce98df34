// occmap_host.cpp -- C ABI of the coloured occupancy map (occmap.hip): the device table and its upkeep, one scan and a
// batch of scans, the sorted leaf query and Frame::updateSensor's pose.  Every limit is checked before any copy or
// launch (DESIGN.md "Occupancy map definition").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "context.h"
#include "occmap_dev.h"

using namespace rgbd;

struct rgbd_occmap {
    rgbd_ctx* c = nullptr;
    OccCfg g{};
    uint32_t cap = 0;
    uint32_t seq = 0;    // the last scan's sequence number; stamps hold 2 * seq + occupied
    int32_t size = 0;    // voxels, as of the last insert
    DevBuf<unsigned long long> key, pkey;
    DevBuf<float> val;
    DevBuf<uint32_t> rgb, stamp, born;
    DevBuf<int32_t> touched;
    DevBuf<OccHdr> hdr;
    DevBuf<OccScan> scans;
    DevBuf<OccPose> poses;
    DevBuf<rgbd_point> pts;

    OccTable view() const { return OccTable{key, val, rgb, stamp, born, touched, cap - 1}; }
};

namespace {

rgbd_status unsupported(rgbd_ctx* c, const char* why) { return c ? fail(c, RGBD_ERR_UNSUPPORTED, why) : RGBD_ERR_UNSUPPORTED; }

bool prob_ok(double p) { return std::isfinite(p) && p > 0.0 && p < 1.0; }
float logodds(double p) { return (float)std::log(p / (1.0 - p)); }

bool all_finite(const float* v, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// an empty table; stamps and births restart with the sequence
rgbd_status table_reset(rgbd_occmap* m)
{
    rgbd_ctx* c = m->c;
    const hipStream_t st = c->stream;
    const size_t n = m->cap;
    rgbd_status s = check_hip(c, hipMemsetAsync(m->key, 0xFF, n * 8, st), "occmap keys clear");
    if (!s) s = check_hip(c, hipMemsetAsync(m->stamp, 0, n * 4, st), "occmap stamps clear");
    if (!s) s = check_hip(c, hipMemsetAsync(m->born, 0, n * 4, st), "occmap births clear");
    if (!s) s = check_hip(c, hipMemsetAsync(m->hdr, 0, sizeof(OccHdr), st), "occmap header clear");
    if (!s) s = check_hip(c, hipStreamSynchronize(st), "sync");
    if (s) return s;
    m->seq = 0;
    m->size = 0;
    return RGBD_OK;
}

}  // namespace

extern "C" {

rgbd_status rgbd_occmap_create(rgbd_ctx* c, const rgbd_occmap_params* prm, rgbd_occmap** out)
{
    if (out) *out = nullptr;
    if (!c || !prm || !out) return unsupported(c, "occmap: null argument");
    if (!std::isfinite(prm->resolution) || !(prm->resolution > 0.0)) return unsupported(c, "occmap: resolution not finite and > 0");
    if (!prob_ok(prm->prob_hit) || !prob_ok(prm->prob_miss) || !prob_ok(prm->clamp_min) || !prob_ok(prm->clamp_max))
        return unsupported(c, "occmap: a probability outside (0, 1)");
    if (!(prm->clamp_min < prm->clamp_max)) return unsupported(c, "occmap: clamping bounds out of order");
    const int64_t cap = prm->capacity;
    if (cap < 64 || cap > ((int64_t)1 << 30) || (cap & (cap - 1)) != 0)
        return unsupported(c, "occmap: capacity not a power of two in [64, 2^30]");
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    rgbd_occmap* m = new rgbd_occmap();
    m->c = c;
    m->cap = (uint32_t)cap;
    m->g = OccCfg{prm->resolution, 1.0 / prm->resolution, logodds(prm->prob_hit), logodds(prm->prob_miss), logodds(prm->clamp_min),
                  logodds(prm->clamp_max)};
    const size_t n = (size_t)cap;
    s = check_hip(c, m->key.alloc(n), "occmap keys");
    if (!s) s = check_hip(c, m->val.alloc(n), "occmap log-odds");
    if (!s) s = check_hip(c, m->rgb.alloc(n), "occmap colours");
    if (!s) s = check_hip(c, m->stamp.alloc(n), "occmap stamps");
    if (!s) s = check_hip(c, m->born.alloc(n), "occmap births");
    if (!s) s = check_hip(c, m->touched.alloc(n), "occmap touched list");
    if (!s) s = check_hip(c, m->hdr.alloc(1), "occmap header");
    if (!s) s = check_hip(c, m->pkey.alloc(kOccMaxPoints), "occmap point keys");
    if (!s) s = table_reset(m);
    if (s) {
        delete m;
        return s;
    }
    *out = m;
    return RGBD_OK;
}

void rgbd_occmap_destroy(rgbd_occmap* m)
{
    if (!m) return;
    (void)hipSetDevice(m->c->device);
    (void)hipStreamSynchronize(m->c->stream);
    delete m;
}

rgbd_status rgbd_occmap_clear(rgbd_occmap* m)
{
    if (!m) return RGBD_ERR_UNSUPPORTED;
    rgbd_status s = check_hip(m->c, hipSetDevice(m->c->device), "hipSetDevice");
    if (s) return s;
    return table_reset(m);
}

rgbd_status rgbd_occmap_size(rgbd_occmap* m, int64_t* n)
{
    if (!m || !n) return RGBD_ERR_UNSUPPORTED;
    *n = m->size;   // every insert ends with the header read back
    return RGBD_OK;
}

rgbd_status rgbd_occmap_insert_batch(rgbd_occmap* m, const rgbd_point* pts, const int32_t* counts, int32_t cap, int32_t nscan,
                                     const float* Twc34s, const float* origins, double maxrange, int32_t* applied)
{
    if (!m) return RGBD_ERR_UNSUPPORTED;
    rgbd_ctx* c = m->c;
    if (applied) *applied = 0;
    if (!applied || nscan < 0 || cap < 0) return unsupported(c, "occmap insert: null or negative argument");
    if (nscan > 0 && (!counts || !Twc34s || !origins)) return unsupported(c, "occmap insert: null argument");
    if (std::isnan(maxrange)) return unsupported(c, "occmap insert: maxrange is NaN");
    size_t total = 0;
    for (int k = 0; k < nscan; k++) {
        if (counts[k] > kOccMaxPoints) return unsupported(c, "occmap insert: more than 16384 points in a scan");
        if (counts[k] < 0 || counts[k] > cap) return fail(c, RGBD_ERR_ARG, "occmap insert: a count outside [0, cap]");
        total += (size_t)counts[k];
    }
    if (total > 0 && !pts) return unsupported(c, "occmap insert: null points");
    if (!all_finite(Twc34s, (size_t)nscan * 12) || !all_finite(origins, (size_t)nscan * 3))
        return unsupported(c, "occmap insert: a pose that is not finite");
    if (nscan == 0) return RGBD_OK;
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    if (m->seq > 0x7FFF0000u - (uint32_t)nscan) {   // stamps are 2 * seq + 1 in 32 bits: start over, nothing is pending
        const hipStream_t st0 = c->stream;
        s = check_hip(c, hipMemsetAsync(m->stamp, 0, (size_t)m->cap * 4, st0), "occmap stamps clear");
        if (!s) s = check_hip(c, hipMemsetAsync(m->born, 0, (size_t)m->cap * 4, st0), "occmap births clear");
        if (s) return s;
        m->seq = 0;
    }
    s = check_hip(c, m->pts.reserve(std::max<size_t>(total, 1)), "occmap points");
    if (!s) s = check_hip(c, m->poses.reserve((size_t)nscan), "occmap poses");
    if (!s) s = check_hip(c, m->scans.reserve((size_t)nscan), "occmap scan words");
    if (s) return s;
    std::vector<OccPose> hp(nscan);
    for (int k = 0; k < nscan; k++) {
        std::memcpy(hp[k].T, Twc34s + 12 * (size_t)k, 48);
        std::memcpy(hp[k].o, origins + 3 * (size_t)k, 12);
        hp[k].pad = 0.f;
    }
    const hipStream_t st = c->stream;
    const OccHdr h0{0, 0, m->size, 0};
    s = check_hip(c, hipMemcpyAsync(m->hdr, &h0, sizeof(OccHdr), hipMemcpyHostToDevice, st), "occmap header up");
    if (!s) s = check_hip(c, hipMemcpyAsync(m->poses, hp.data(), (size_t)nscan * sizeof(OccPose), hipMemcpyHostToDevice, st), "occmap poses up");
    if (!s) s = check_hip(c, hipMemsetAsync(m->scans, 0, (size_t)nscan * sizeof(OccScan), st), "occmap scan words clear");
    size_t off = 0;
    for (int k = 0; k < nscan && !s; k++) {
        if (counts[k])
            s = check_hip(c, hipMemcpyAsync(m->pts + off, pts + (size_t)k * cap, (size_t)counts[k] * sizeof(rgbd_point),
                                            hipMemcpyHostToDevice, st), "occmap points up");
        off += (size_t)counts[k];
    }
    if (s) return s;
    const OccTable t = m->view();
    off = 0;
    for (int k = 0; k < nscan; k++) {
        const uint32_t seq = ++m->seq;
        const rgbd_point* p = m->pts + off;
        const int n = counts[k];
        int tk = timer_begin(c, "k_occ_mark");
        RGBD_TRY(c, launch_occ_mark(t, m->g, p, n, m->poses + k, maxrange, seq, m->hdr, m->scans + k, m->pkey, st), "occ_mark");
        timer_end(c, tk);
        tk = timer_begin(c, "k_occ_apply");
        RGBD_TRY(c, launch_occ_apply(t, m->g, seq, m->hdr, m->scans + k, st), "occ_apply");
        timer_end(c, tk);
        tk = timer_begin(c, "k_occ_colour");
        RGBD_TRY(c, launch_occ_colour(t, p, m->pkey, n, m->hdr, m->scans + k, st), "occ_colour");
        timer_end(c, tk);
        off += (size_t)n;
    }
    OccHdr h{};
    s = check_hip(c, hipMemcpyAsync(&h, m->hdr, sizeof(OccHdr), hipMemcpyDeviceToHost, st), "occmap header");
    if (!s) s = check_hip(c, hipStreamSynchronize(st), "sync");
    if (s) return s;
    m->size = h.size;
    *applied = h.applied;
    if (h.applied < nscan) return fail(c, RGBD_ERR_CAPACITY, "occmap insert: a scan's voxels do not fit the table");
    return RGBD_OK;
}

rgbd_status rgbd_occmap_insert(rgbd_occmap* m, const rgbd_point* pts, int32_t n, const float* Twc34, const float* origin,
                               double maxrange)
{
    if (!m) return RGBD_ERR_UNSUPPORTED;
    if (n < 0) return fail(m->c, RGBD_ERR_ARG, "occmap insert: negative point count");
    if (n > kOccMaxPoints) return unsupported(m->c, "occmap insert: more than 16384 points in a scan");
    int32_t applied = 0;
    return rgbd_occmap_insert_batch(m, pts, &n, n, 1, Twc34, origin, maxrange, &applied);
}

rgbd_status rgbd_occmap_leaves(rgbd_occmap* m, float min_logodds, uint16_t* keys, float* logodds_out, uint8_t* rgb, int64_t cap,
                               int64_t* n)
{
    if (!m) return RGBD_ERR_UNSUPPORTED;
    rgbd_ctx* c = m->c;
    if (!n || cap < 0 || (cap > 0 && (!keys || !logodds_out || !rgb))) return unsupported(c, "occmap leaves: null argument");
    if (std::isnan(min_logodds)) return unsupported(c, "occmap leaves: threshold is NaN");
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    const size_t N = m->cap;
    std::vector<unsigned long long> hk(N);
    std::vector<float> hv(N);
    std::vector<uint32_t> hc(N);
    const hipStream_t st = c->stream;
    s = check_hip(c, hipMemcpyAsync(hk.data(), m->key, N * 8, hipMemcpyDeviceToHost, st), "occmap keys");
    if (!s) s = check_hip(c, hipMemcpyAsync(hv.data(), m->val, N * 4, hipMemcpyDeviceToHost, st), "occmap log-odds");
    if (!s) s = check_hip(c, hipMemcpyAsync(hc.data(), m->rgb, N * 4, hipMemcpyDeviceToHost, st), "occmap colours");
    if (!s) s = check_hip(c, hipStreamSynchronize(st), "sync");
    if (s) return s;
    std::vector<uint32_t> idx;
    for (size_t i = 0; i < N; i++)
        if (hk[i] != kOccEmpty && hv[i] >= min_logodds) idx.push_back((uint32_t)i);
    std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return hk[a] < hk[b]; });
    *n = (int64_t)idx.size();
    if ((int64_t)idx.size() > cap) return fail(c, RGBD_ERR_CAPACITY, "occmap leaves: output capacity below the leaf count");
    for (size_t i = 0; i < idx.size(); i++) {
        const unsigned long long k = hk[idx[i]];
        keys[3 * i] = (uint16_t)(k >> 32);
        keys[3 * i + 1] = (uint16_t)(k >> 16);
        keys[3 * i + 2] = (uint16_t)k;
        logodds_out[i] = hv[idx[i]];
        const uint32_t col = hc[idx[i]];
        rgb[3 * i] = (uint8_t)col;
        rgb[3 * i + 1] = (uint8_t)(col >> 8);
        rgb[3 * i + 2] = (uint8_t)(col >> 16);
    }
    return RGBD_OK;
}

rgbd_status rgbd_occmap_sensor_pose(const float* Tcw, float* Twc34, float* origin)
{
    if (!Tcw || !Twc34 || !origin) return RGBD_ERR_UNSUPPORTED;
    if (!all_finite(Tcw, 16)) return RGBD_ERR_UNSUPPORTED;
    float m[3][3], Ow[3];
    for (int r = 0; r < 3; r++) {
        double s = 0.0;
        for (int k = 0; k < 3; k++) {
            m[r][k] = Tcw[4 * k + r];   // Rwc = Rcw^T
            s += (double)Tcw[4 * k + r] * (double)Tcw[4 * k + 3];
        }
        Ow[r] = (float)-s;
    }
    // Eigen::Quaternionf(Rwc): Shepperd's method on the trace or the largest diagonal entry
    float q[3], w;
    float t = (m[0][0] + m[1][1]) + m[2][2];
    if (t > 0.0f) {
        t = std::sqrt(t + 1.0f);
        w = 0.5f * t;
        t = 0.5f / t;
        q[0] = (m[2][1] - m[1][2]) * t;
        q[1] = (m[0][2] - m[2][0]) * t;
        q[2] = (m[1][0] - m[0][1]) * t;
    } else {
        int i = 0;
        if (m[1][1] > m[0][0]) i = 1;
        if (m[2][2] > m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        t = std::sqrt(((m[i][i] - m[j][j]) - m[k][k]) + 1.0f);
        q[i] = 0.5f * t;
        t = 0.5f / t;
        w = (m[k][j] - m[j][k]) * t;
        q[j] = (m[j][i] + m[i][j]) * t;
        q[k] = (m[k][i] + m[i][k]) * t;
    }
    // toRotationMatrix
    const float x = q[0], y = q[1], z = q[2];
    const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
    const float twx = tx * w, twy = ty * w, twz = tz * w;
    const float txx = tx * x, txy = ty * x, txz = tz * x;
    const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const float R[9] = {1.0f - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0f - (txx + tzz), tyz - twx,
                        txz - twy, tyz + twx, 1.0f - (txx + tyy)};
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) Twc34[4 * r + k] = R[3 * r + k];
        Twc34[4 * r + 3] = Ow[r];
        origin[r] = Ow[r];
    }
    return RGBD_OK;
}

}  // extern "C"
