// svo_host.cpp -- host side of the SVO + BRIEF front end (svo.hip): Extractor(SVO, BRIEF, NORMAL), the
// reference's default (main.cpp:31), behind the same extraction entry points as the ORBextractor.
//   Extractor::createDetector SVO   Features/Extractor.cpp:162-165  -> svo_configure (SvoCfg, tile table)
//   Extractor::detectAndCompute     Features/Extractor.cpp:50-61    -> SvoWS::run (one launch chain)
//   Frame::undistortKeyPoints + uprojectCamera (Core/Frame.cpp:91-117, 251-281) -> k_undistort
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "brief_front.h"
#include "launch.h"

namespace rgbd {

struct SvoWS : FrontEnd {
    BriefFront bf;             // its cfg is the SVO configuration, its d_pyr the SVO pyramid
    std::vector<SvoTile> tiles;
    DevBuf<SvoTile> d_tiles;
    DevBuf<unsigned long long> d_cells;
    DevBuf<uint2> d_cand;
    DevBuf<int> d_ncand;
    DevBuf<float> d_rt_resp;   // rgbd_svo_retain_best staging
    DevBuf<int> d_rt_order;

    rgbd_status alloc(rgbd_ctx* c) override;
    rgbd_status run(rgbd_ctx* c, const uint8_t* d_bgr, const uint16_t* d_depth, int B, bool from_gray,
                    const ExtractHook* after_fast) override;
    BriefFront* brief() override { return &bf; }
};

namespace {

SvoWS* ws(rgbd_ctx* c) { return dynamic_cast<SvoWS*>(c->front.get()); }   // null: not an SVO context

}  // namespace

rgbd_status svo_configure(rgbd_ctx* c, const rgbd_svo_params& p)
{
    if (p.nlevels < 1 || p.nlevels > kSvoMaxLevels)
        return fail(c, RGBD_ERR_UNSUPPORTED, "SVO: nlevels must be 1..8");
    if (p.cell_size < 1 || p.threshold < 0 || p.threshold > 254 || p.nfeatures < 0 || p.max_keypoints < 0)
        return fail(c, RGBD_ERR_ARG, "SVO: cell_size >= 1, 0 <= threshold <= 254, nfeatures >= 0, max_keypoints >= 0");
    if (c->W < 1 || c->H < 1 || c->W > 2047 || c->H > 2047)
        return fail(c, RGBD_ERR_UNSUPPORTED, "SVO: image sides 1..2047");
    SvoWS* w = new SvoWS();
    c->front.reset(w);
    SvoCfg& g = w->bf.cfg;
    g.W = c->W;
    g.H = c->H;
    g.nlevels = p.nlevels;
    g.cell = p.cell_size;
    g.barrier = p.threshold;
    g.gcols = (int)std::ceil((double)c->W / p.cell_size);   // SVOextractor::detect :93-94
    g.grows = (int)std::ceil((double)c->H / p.cell_size);
    g.ncells = g.gcols * g.grows;
    if (g.ncells > kSvoSelThreads * kSvoSelMaxE)
        return fail(c, RGBD_ERR_UNSUPPORTED, "SVO: more than 12288 grid cells (raise cell_size)");
    int off = 0;
    for (int l = 0; l < p.nlevels; l++) {
        g.lw[l] = l ? g.lw[l - 1] / 2 : c->W;
        g.lh[l] = l ? g.lh[l - 1] / 2 : c->H;
        if (l + 1 < p.nlevels && (g.lw[l] & 1))   // halfSample's row walk (:24-35) assumes even widths
            return fail(c, RGBD_ERR_UNSUPPORTED, "SVO: odd level width above the last level");
        g.loff[l] = off;
        off += g.lw[l] * g.lh[l];
    }
    g.frame_bytes = (off + 63) & ~63;
    g.nfeatures = p.nfeatures;
    // retainBest keeps nfeatures + every tie of the boundary response (more fail loudly, RGBD_ERR_CAPACITY)
    g.kp_cap = std::min(g.ncells, p.max_keypoints > 0 ? p.max_keypoints : p.nfeatures + 64);
    g.border = kBriefBorder;
    for (int l = 0; l < p.nlevels; l++) {   // FAST-10 tiles of 64 x 32 over the detector's domain
        if (g.lw[l] < 7 || g.lh[l] < 7) continue;
        for (int y = 0; y < g.lh[l]; y += 32)
            for (int x = 0; x < g.lw[l]; x += 64) w->tiles.push_back(SvoTile{(int16_t)l, (int16_t)x, (int16_t)y, 0});
    }
    c->cfg.kp_cap = g.kp_cap;   // the output arrays (kps, desc, xyz, knn) are sized by it
    return RGBD_OK;
}

rgbd_status SvoWS::alloc(rgbd_ctx* c)
{
    const SvoCfg& g = bf.cfg;
    const size_t B = (size_t)c->maxB;
    rgbd_status s = check_hip(c, d_tiles.alloc(tiles.size()), "svo tiles");
    if (!s) s = bf.alloc(c, "svo", "pyramid");
    if (!s) s = check_hip(c, d_cells.alloc(B * g.ncells), "svo cells");
    if (!s) s = check_hip(c, d_cand.alloc(B * g.ncells), "svo candidates");
    if (!s) s = check_hip(c, d_ncand.alloc(B), "svo candidate counts");
    if (s) return s;
    if (!tiles.empty())
        s = check_hip(c, hipMemcpy(d_tiles, tiles.data(), tiles.size() * sizeof(SvoTile), hipMemcpyHostToDevice), "svo tiles up");
    if (!s) s = check_hip(c, hipMemset(d_cells, 0, B * g.ncells * 8), "svo cells zero");
    if (!s) s = check_hip(c, hipMemset(d_ncand, 0, B * 4), "svo ncand zero");
    if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
    return s;
}

rgbd_status SvoWS::run(rgbd_ctx* c, const uint8_t* d_bgr, const uint16_t* d_depth, int B, bool from_gray,
                       const ExtractHook* after_fast)
{
    const SvoCfg& g = bf.cfg;
    const hipStream_t st = c->stream;
    rgbd_status s = bf.run_pyramid(c, d_bgr, B, from_gray);
    if (s) return s;
    int tk = timer_begin(c, "k_svo_detect");
    RGBD_TRY(c, launch_svo_detect(bf.d_pyr, d_tiles, (int)tiles.size(), g, d_cells, B, st), "svo_detect");
    timer_end(c, tk);
    // e.g. the deferred PnPRansac solves of earlier pipelined steps (pnp_host.cpp)
    if ((s = call_hook(after_fast, 1)) || (s = call_hook(after_fast, 2))) return s;
    tk = timer_begin(c, "k_svo_select");
    RGBD_TRY(c, launch_svo_select(d_cells, g, d_cand, d_ncand, c->out.count, c->out.kps, c->d_err, B, st), "svo_select");
    timer_end(c, tk);
#ifdef RGBD_PNP_PROFILE
    svo_prof_dump(st);
#endif
    return bf.run_describe(c, d_depth, B);
}

}  // namespace rgbd

using namespace rgbd;

extern "C" {

rgbd_status rgbd_svo_debug_level(rgbd_ctx* c, int32_t b, int32_t level, uint8_t* out)
{
    SvoWS* w = c ? ws(c) : nullptr;
    if (!w || !out || b < 0 || b >= c->last_B) return RGBD_ERR_ARG;
    const SvoCfg& g = w->bf.cfg;
    if (level < 0 || level >= g.nlevels) return RGBD_ERR_ARG;
    rgbd_status s = check_hip(c, hipMemcpyAsync(out, w->bf.d_pyr + (size_t)b * g.frame_bytes + g.loff[level],
                                                (size_t)g.lw[level] * g.lh[level], hipMemcpyDeviceToHost, c->stream),
                              "read level");
    return s ? s : check_hip(c, hipStreamSynchronize(c->stream), "sync");
}

rgbd_status rgbd_svo_debug_grid(rgbd_ctx* c, int32_t b, int32_t* xyl, float* resp, int32_t cap, int32_t* n)
{
    SvoWS* w = c ? ws(c) : nullptr;
    if (!w || !n || b < 0 || b >= c->last_B) return RGBD_ERR_ARG;
    const SvoCfg& g = w->bf.cfg;
    int cnt = 0;
    rgbd_status s = check_hip(c, hipMemcpyAsync(&cnt, w->d_ncand + b, 4, hipMemcpyDeviceToHost, c->stream), "read ncand");
    if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
    if (s) return s;
    *n = cnt;
    if (cnt > cap) return fail(c, RGBD_ERR_CAPACITY, "output capacity smaller than the grid keypoint count");
    std::vector<uint2> v((size_t)cnt);
    if (cnt) {
        s = check_hip(c, hipMemcpyAsync(v.data(), w->d_cand + (size_t)b * g.ncells, (size_t)cnt * 8, hipMemcpyDeviceToHost,
                                        c->stream), "read candidates");
        if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
        if (s) return s;
    }
    for (int i = 0; i < cnt; i++) {
        const uint32_t ord = ~v[i].y;
        const int L = (int)(ord >> 22);
        if (xyl) {
            xyl[3 * i] = (int)(ord & 2047u) << L;
            xyl[3 * i + 1] = (int)((ord >> 11) & 2047u) << L;
            xyl[3 * i + 2] = L;
        }
        if (resp) std::memcpy(resp + i, &v[i].x, 4);
    }
    return RGBD_OK;
}

rgbd_status rgbd_svo_retain_best(rgbd_ctx* c, const float* resp, int32_t n, int32_t n_points, int32_t depth_limit,
                                 int32_t* order, int32_t* m)
{
    if (!c || !order || !m || n < 0 || (n > 0 && !resp)) return RGBD_ERR_ARG;
    SvoWS* w = ws(c);
    if (!w) return fail(c, RGBD_ERR_ARG, "not an SVO context (rgbd_create_svo)");
    if (n > kSvoSelThreads * kSvoSelMaxE) return fail(c, RGBD_ERR_UNSUPPORTED, "retainBest: n <= 12288");
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    if (!w->d_rt_order) {   // the one allocated last
        s = check_hip(c, w->d_rt_resp.alloc((size_t)kSvoSelThreads * kSvoSelMaxE), "retain resp");
        if (!s) s = check_hip(c, w->d_rt_order.alloc((size_t)kSvoSelThreads * kSvoSelMaxE + 1), "retain order");
        if (s) return s;
    }
    if (n == 0) { *m = 0; return RGBD_OK; }
    s = check_hip(c, hipMemcpyAsync(w->d_rt_resp, resp, (size_t)n * 4, hipMemcpyHostToDevice, c->stream), "retain up");
    if (s) return s;
    int* d_m = w->d_rt_order + kSvoSelThreads * kSvoSelMaxE;
    RGBD_TRY(c, launch_svo_retain_test(w->d_rt_resp, n, n_points < 0 ? n : n_points, depth_limit, w->d_rt_order, d_m, c->stream), "svo_retain_test");
    int mm = 0;
    s = check_hip(c, hipMemcpyAsync(&mm, d_m, 4, hipMemcpyDeviceToHost, c->stream), "retain m");
    if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
    if (s) return s;
    *m = mm;
    s = check_hip(c, hipMemcpyAsync(order, w->d_rt_order, (size_t)mm * 4, hipMemcpyDeviceToHost, c->stream), "retain order");
    return s ? s : check_hip(c, hipStreamSynchronize(c->stream), "sync");
}

}  // extern "C"
