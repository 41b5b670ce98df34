// fast_host.cpp -- host side of the plain FAST front end (fast.hip): Extractor(FAST, BRIEF, NORMAL) and
// Extractor(FAST, ORB, NORMAL), behind the same extraction entry points as the ORBextractor and the other front ends.
//   Extractor::createDetector FAST  Features/Extractor.cpp:168-171  -> fast_configure (FastCfg)
//   Extractor::detectAndCompute     Features/Extractor.cpp:50-61    -> FastWS::run (one launch chain)
//   Frame::undistortKeyPoints + uprojectCamera (Core/Frame.cpp:91-117, 251-281) -> k_undistort
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "brief_front.h"
#include "fast_dev.h"
#include "launch.h"

namespace rgbd {

struct FastWS : FrontEnd {
    FastCfg cfg{};
    bool orb = false;             // the ORB descriptor: gray and blur are level 0 of the context's ORB pyramid
    AdpCfg score{};               // what k_adp_score reads: W (the gray rows' stride), H
    BriefFront bf;                // BRIEF: one level, gray + box sums
    DevBuf<uint8_t> d_smap;       // [B][H][sstride]
    DevBuf<int> d_rowc;           // [B][H]
    DevBuf<uint32_t> d_cand;      // [B][cand_cap]
    DevBuf<int> d_ncand;          // [B]
    DevBuf<float> d_R;            // [B][cand_cap]
    DevBuf<uint16_t> d_I, d_posL, d_posR;
    FastBufs bufs{};
    DevBuf<float> d_rt_R;         // rgbd_fast_retain_best staging: kFastMaxCandCap each
    DevBuf<uint16_t> d_rt_I, d_rt_posL, d_rt_posR;
    DevBuf<int> d_rt_order;       // + 1: the kept count

    rgbd_status alloc(rgbd_ctx* c) override;
    rgbd_status run(rgbd_ctx* c, const uint8_t* d_bgr, const uint16_t* d_depth, int B, bool from_gray,
                    const ExtractHook* after_fast) override;
    BriefFront* brief() override { return orb ? nullptr : &bf; }
};

namespace {

FastWS* ws(rgbd_ctx* c) { return dynamic_cast<FastWS*>(c->front.get()); }   // null: not a FAST context

rgbd_status not_fast(rgbd_ctx* c) { return fail(c, RGBD_ERR_ARG, "not a FAST context (rgbd_create_fast)"); }

}  // namespace

rgbd_status fast_configure(rgbd_ctx* c, const rgbd_fast_params& p)
{
    // every refusal before anything is allocated
    if (p.nfeatures < 1 || p.nfeatures > kFastMaxFeatures) return fail(c, RGBD_ERR_UNSUPPORTED, "FAST: nfeatures must be 1..12288");
    if (p.threshold < 1 || p.threshold > 255) return fail(c, RGBD_ERR_UNSUPPORTED, "FAST: threshold must be 1..255");
    if (p.descriptor != RGBD_FAST_BRIEF && p.descriptor != RGBD_FAST_ORB) return fail(c, RGBD_ERR_UNSUPPORTED, "FAST: descriptor must be RGBD_FAST_BRIEF or RGBD_FAST_ORB");
    if (p.cand_cap < 0 || p.cand_cap > kFastMaxCandCap) return fail(c, RGBD_ERR_UNSUPPORTED, "FAST: cand_cap must be 1..65536 (0: 32768)");
    const int cap = p.cand_cap > 0 ? p.cand_cap : kFastDefaultCandCap;
    if (p.max_keypoints < 0 || p.max_keypoints > kFastMaxCandCap || (p.max_keypoints != 0 && p.max_keypoints < p.nfeatures))
        return fail(c, RGBD_ERR_UNSUPPORTED, "FAST: max_keypoints must be nfeatures..65536 (0: nfeatures + nfeatures / 4)");
    if (c->W < 1 || c->H < 1 || c->W > 2047 || c->H > 2047) return fail(c, RGBD_ERR_UNSUPPORTED, "FAST: image sides 1..2047");
    FastCfg g{};
    g.W = c->W;
    g.H = c->H;
    g.thr = p.threshold;
    g.nfeatures = p.nfeatures;
    g.cand_cap = cap;
    g.kp_cap = p.max_keypoints > 0 ? p.max_keypoints : p.nfeatures + p.nfeatures / 4;
    const bool orb = p.descriptor == RGBD_FAST_ORB;
    g.border = orb ? kFastOrbBorder : kBriefBorder;
    g.sstride = g.W;   // BRIEF; the ORB pyramid's level-0 stride once its geometry is accepted (FastWS::alloc)
    FastWS* w = new FastWS();
    c->front.reset(w);
    w->orb = orb;
    w->cfg = g;
    if (!orb) w->bf.one_level(c->W, c->H, g.kp_cap);
    c->cfg.kp_cap = g.kp_cap;   // the output arrays (kps, desc, xyz, knn) are sized by it
    return RGBD_OK;
}

rgbd_status FastWS::alloc(rgbd_ctx* c)
{
    if (orb) cfg.sstride = c->cfg.lv[0].stride;
    const FastCfg& g = cfg;
    score.W = g.sstride;
    score.H = g.H;
    const size_t B = (size_t)c->maxB, lists = B * g.cand_cap;
    rgbd_status s = orb ? RGBD_OK : bf.alloc(c, "FAST", "gray");
    if (!s) s = check_hip(c, d_smap.alloc(B * g.sstride * g.H), "FAST score map");
    if (!s) s = check_hip(c, d_rowc.alloc(B * g.H), "FAST row counts");
    if (!s) s = check_hip(c, d_cand.alloc(lists), "FAST corners");
    if (!s) s = check_hip(c, d_ncand.alloc(B), "FAST corner counts");
    if (!s) s = check_hip(c, d_R.alloc(lists), "FAST selection responses");
    if (!s) s = check_hip(c, d_I.alloc(lists), "FAST selection payloads");
    if (!s) s = check_hip(c, d_posL.alloc(lists), "FAST left stoppers");
    if (!s) s = check_hip(c, d_posR.alloc(lists), "FAST right stoppers");
    if (!s) s = check_hip(c, hipMemset(d_ncand, 0, B * sizeof(int)), "memset FAST counts");
    if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
    if (s) return s;
    bufs = FastBufs{d_smap, d_rowc, d_cand, d_ncand, d_R, d_I, d_posL, d_posR};
    return RGBD_OK;
}

rgbd_status FastWS::run(rgbd_ctx* c, const uint8_t* d_bgr, const uint16_t* d_depth, int B, bool from_gray,
                        const ExtractHook* after_fast)
{
    const hipStream_t st = c->stream;
    const ExtractCfg& C = c->cfg;
    rgbd_status s = orb ? run_orb_pyramid(c, d_bgr, B, from_gray) : bf.run_pyramid(c, d_bgr, B, from_gray);
    if (s) return s;
    const uint8_t* gray = orb ? c->d_pyr + C.lv[0].off : bf.d_pyr;
    int tk = timer_begin(c, "k_adp_score");
    RGBD_TRY(c, launch_adp_score(gray, orb ? (size_t)C.frame_pyr_bytes : (size_t)bf.cfg.frame_bytes, d_smap, score, B, st), "adp_score");
    timer_end(c, tk);
    tk = timer_begin(c, "k_fast_rows");
    RGBD_TRY(c, launch_fast_rows(cfg, bufs, c->d_err, B, st), "fast_rows");
    timer_end(c, tk);
    // e.g. the deferred PnPRansac solves of earlier pipelined steps (pnp_host.cpp)
    if ((s = call_hook(after_fast, 1)) || (s = call_hook(after_fast, 2))) return s;
    tk = timer_begin(c, "k_fast_select");
    RGBD_TRY(c, launch_fast_select(cfg, bufs, c->out.count, c->out.kps, c->d_err, B, st), "fast_select");
    timer_end(c, tk);
    if (!orb) return bf.run_describe(c, d_depth, B);
    // the k_fast grid's blur blocks alone (no FAST segments), as the cv::ORB front end launches them: blurred level 0
    tk = timer_begin(c, "k_fast(blur)");
    RGBD_TRY(c, launch_fast(c->d_pyr, c->d_cells, c->d_segs, 0, c->d_cfg, c->d_cellc, c->d_slots, B, st, c->d_blur,
                            C.blur_t0[kMaxLevels] + C.blur_e0[kMaxLevels], c->d_blur_tab, C.blur_m0[kMaxLevels]), "fast (blur blocks)");
    timer_end(c, tk);
    tk = timer_begin(c, "k_fast_orb_describe");
    RGBD_TRY(c, launch_fast_orb_describe(c->d_blur + C.lv[0].off, (size_t)C.frame_pyr_bytes, C.lv[0].stride, cfg, c->out.count, c->out.kps,
                                         c->out.desc, B, st), "fast_orb_describe");
    timer_end(c, tk);
    tk = timer_begin(c, "k_undistort");
    RGBD_TRY(c, launch_undistort(d_depth, c->out.count, c->d_cfg, cfg.kp_cap, c->out.kps, c->out.kun, c->out.xyz, B, st), "undistort");
    timer_end(c, tk);
    c->last_B = B;
    return RGBD_OK;
}

}  // namespace rgbd

using namespace rgbd;

extern "C" {

rgbd_status rgbd_fast_debug_corners(rgbd_ctx* c, int32_t b, int32_t* n_candidates, int32_t* xys, int32_t cap, int32_t* n)
{
    if (!c || !n_candidates) return RGBD_ERR_ARG;
    FastWS* w = ws(c);
    if (!w) return not_fast(c);
    if (b < 0 || b >= c->last_B || cap < 0) return fail(c, RGBD_ERR_ARG, "FAST: frame index outside the last batch, or a negative capacity");
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    int nc = 0;
    s = check_hip(c, hipMemcpyAsync(&nc, w->d_ncand + b, 4, hipMemcpyDeviceToHost, c->stream), "read FAST count");
    if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
    if (s) return s;
    *n_candidates = nc;
    const int m = std::min(nc, w->cfg.cand_cap);
    if (n) *n = m;
    if (!xys || m == 0) return RGBD_OK;
    if (m > cap) return fail(c, RGBD_ERR_CAPACITY, "output capacity smaller than the frame's corner list");
    std::vector<uint32_t> v((size_t)m);
    s = check_hip(c, hipMemcpyAsync(v.data(), w->d_cand + (size_t)b * w->cfg.cand_cap, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream),
                  "read FAST corners");
    if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
    if (s) return s;
    for (int i = 0; i < m; i++) {
        xys[3 * i] = adp_x(v[i]);
        xys[3 * i + 1] = adp_y(v[i]);
        xys[3 * i + 2] = adp_s(v[i]);
    }
    return RGBD_OK;
}

rgbd_status rgbd_fast_retain_best(rgbd_ctx* c, const float* resp, int32_t n, int32_t n_points, int32_t depth_limit, int32_t* order,
                                  int32_t* m)
{
    if (!c || !order || !m || n < 0 || (n > 0 && !resp)) return RGBD_ERR_ARG;
    FastWS* w = ws(c);
    if (!w) return not_fast(c);
    if (n > kFastMaxCandCap) return fail(c, RGBD_ERR_UNSUPPORTED, "retainBest: n <= 65536");
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    if (!w->d_rt_order) {   // the one allocated last
        s = check_hip(c, w->d_rt_R.alloc((size_t)kFastMaxCandCap), "retain resp");
        if (!s) s = check_hip(c, w->d_rt_I.alloc((size_t)kFastMaxCandCap), "retain payloads");
        if (!s) s = check_hip(c, w->d_rt_posL.alloc((size_t)kFastMaxCandCap), "retain left stoppers");
        if (!s) s = check_hip(c, w->d_rt_posR.alloc((size_t)kFastMaxCandCap), "retain right stoppers");
        if (!s) s = check_hip(c, w->d_rt_order.alloc((size_t)kFastMaxCandCap + 1), "retain order");
        if (s) return s;
    }
    if (n == 0) { *m = 0; return RGBD_OK; }
    s = check_hip(c, hipMemcpyAsync(w->d_rt_R, resp, (size_t)n * 4, hipMemcpyHostToDevice, c->stream), "retain up");
    if (s) return s;
    int* d_m = w->d_rt_order + kFastMaxCandCap;
    const FastBufs tb{nullptr, nullptr, nullptr, nullptr, w->d_rt_R, w->d_rt_I, w->d_rt_posL, w->d_rt_posR};
    RGBD_TRY(c, launch_fast_retain_test(tb, n, n_points < 0 ? n : n_points, depth_limit, w->d_rt_order, d_m, c->stream), "fast_retain_test");
    int mm = 0;
    s = check_hip(c, hipMemcpyAsync(&mm, d_m, 4, hipMemcpyDeviceToHost, c->stream), "retain m");
    if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
    if (s) return s;
    *m = mm;
    if (mm == 0) return RGBD_OK;
    s = check_hip(c, hipMemcpyAsync(order, w->d_rt_order, (size_t)mm * 4, hipMemcpyDeviceToHost, c->stream), "retain order");
    return s ? s : check_hip(c, hipStreamSynchronize(c->stream), "sync");
}

}  // extern "C"
