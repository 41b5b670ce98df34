// cvorb_host.cpp -- host side of the OpenCV ORB front end (cvorb.hip): Extractor(ORB, ORB, NORMAL), behind the same
// extraction entry points as the ORBextractor, the SVO, the adaptive and the GFTT front ends.
//   Extractor::create(ORB)        Features/Extractor.cpp:163-166, 216-218  -> cvorb_configure (CvorbCfg)
//   Extractor::detectAndCompute   Features/Extractor.cpp:50-61             -> CvorbWS::run (one launch chain)
//   Frame::undistortKeyPoints + uprojectCamera (Core/Frame.cpp:91-117, 251-281) -> k_undistort
// The pyramid and the blurred pyramid are the ORB geometry's (geometry.cpp): k_pyramid / k_pyr_tail and the blur
// blocks of the k_fast grid, launched without FAST segments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "context.h"
#include "cvorb_dev.h"
#include "launch.h"

namespace rgbd {

struct CvorbWS : FrontEnd {
    CvorbCfg cfg{};
    DevBuf<uint8_t> d_score;       // [B][frame_pyr_bytes]
    DevBuf<uint32_t> d_cand, d_s1, d_s2;   // [B][L][cand_cap]
    DevBuf<float> d_h1, d_h2;      // [B][L][cand_cap]
    DevBuf<int> d_n;               // nfast, n1, n2: [3][B][L], then nstrip [B][L][kCvListStrips]
    DevBuf<uint32_t> d_fsel;       // [B][kp_cap]
    CvorbBufs bufs{};

    rgbd_status alloc(rgbd_ctx* c) override;
    rgbd_status run(rgbd_ctx* c, const uint8_t* d_bgr, const uint16_t* d_depth, int B, bool from_gray,
                    const ExtractHook* after_fast) override;
};

namespace {

CvorbWS* ws(rgbd_ctx* c) { return dynamic_cast<CvorbWS*>(c->front.get()); }   // null: not a cv::ORB context

rgbd_status not_cvorb(rgbd_ctx* c) { return fail(c, RGBD_ERR_ARG, "not a cv::ORB context (rgbd_create_cvorb)"); }

int cv_round_f(float v) { return (int)std::nearbyint(v); }   // cvRound: to nearest, halves to even (the default mode)

}  // namespace

rgbd_status cvorb_check_params(rgbd_ctx* c, const rgbd_cvorb_params& p)
{
    if (p.nfeatures < 1 || p.nfeatures > kCvorbMaxFeatures) return fail(c, RGBD_ERR_UNSUPPORTED, "cv::ORB: nfeatures must be 1..8192");
    if (p.fast_threshold < 1 || p.fast_threshold > 255) return fail(c, RGBD_ERR_UNSUPPORTED, "cv::ORB: fast_threshold must be 1..255");
    if (p.edge_threshold < 22 || p.edge_threshold > 255)
        return fail(c, RGBD_ERR_UNSUPPORTED, "cv::ORB: edge_threshold must be 22..255 (22: the descriptor's reach)");
    if (p.cand_cap < 0 || p.cand_cap > kCvorbMaxCandCap) return fail(c, RGBD_ERR_UNSUPPORTED, "cv::ORB: cand_cap must be 1..12288 (0: 8192)");
    if (p.max_keypoints != 0 && p.max_keypoints < p.nfeatures)
        return fail(c, RGBD_ERR_UNSUPPORTED, "cv::ORB: max_keypoints below nfeatures (0: nfeatures + nfeatures / 4)");
    return RGBD_OK;
}

rgbd_status cvorb_configure(rgbd_ctx* c, const rgbd_cvorb_params& p)
{
    const ExtractCfg& C = c->cfg;   // the ORB geometry of (width, height, scale_factor, nlevels), accepted
    CvorbCfg g{};
    g.W = c->W;
    g.H = c->H;
    g.nlevels = C.nlevels;
    g.frame_pyr_bytes = C.frame_pyr_bytes;
    g.nfeatures = p.nfeatures;
    g.edge = p.edge_threshold;
    g.thr = p.fast_threshold;
    g.cand_cap = p.cand_cap > 0 ? p.cand_cap : kCvorbDefaultCandCap;
    g.kp_cap = p.max_keypoints > 0 ? p.max_keypoints : p.nfeatures + p.nfeatures / 4;
    g.frame_cap = (int)std::min<long>(kCvorbFrameCap, (long)g.nlevels * g.cand_cap);
    const float sc = 1.f / (4 * 7 * 255.f);
    g.ssq = sc * sc * sc * sc;
    // cv::ORB's tables: layerScale in f64 powers of the float scale factor, sizes by cvRound of the f32 quotient
    const double sf = (double)p.scale_factor;
    for (int l = 0; l < g.nlevels; l++) {
        g.scale[l] = (float)std::pow(sf, (double)l);
        g.size[l] = 31.0f * g.scale[l];
        const LevelCfg& L = C.lv[l];
        if (cv_round_f((float)c->W / g.scale[l]) != L.w || cv_round_f((float)c->H / g.scale[l]) != L.h)
            return fail(c, RGBD_ERR_UNSUPPORTED, "cv::ORB: a level's size differs from the ORB pyramid's for this shape and scale");
        g.lw[l] = L.w;
        g.lh[l] = L.h;
        g.lstride[l] = L.stride;
        g.loff[l] = L.off;
    }
    if (c->W > 2047 || c->H > 2047) return fail(c, RGBD_ERR_UNSUPPORTED, "cv::ORB: image sides of at most 2047 px");
    // the budgets (orb.cpp: ORB_Impl::detectAndCompute)
    const float factor = (float)(1.0 / sf);
    float nd = p.nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)g.nlevels));
    int sum = 0;
    for (int l = 0; l < g.nlevels - 1; l++) {
        g.N[l] = cv_round_f(nd);
        sum += g.N[l];
        nd *= factor;
    }
    g.N[g.nlevels - 1] = std::max(p.nfeatures - sum, 0);
    for (int v = 0; v < 16; v++) g.umax[v] = C.umax[v];
    CvorbWS* w = new CvorbWS();
    c->front.reset(w);
    w->cfg = g;
    c->cfg.kp_cap = g.kp_cap;   // the output arrays (kps, desc, xyz, knn) are sized by it
    return RGBD_OK;
}

rgbd_status CvorbWS::alloc(rgbd_ctx* c)
{
    const CvorbCfg& g = cfg;
    const size_t B = (size_t)c->maxB, BL = B * g.nlevels, lists = BL * g.cand_cap;
    rgbd_status s = check_hip(c, d_score.alloc(B * g.frame_pyr_bytes + 64), "cv::ORB score maps");
    if (!s) s = check_hip(c, d_cand.alloc(lists), "cv::ORB corners");
    if (!s) s = check_hip(c, d_s1.alloc(lists), "cv::ORB first selection");
    if (!s) s = check_hip(c, d_h1.alloc(lists), "cv::ORB Harris responses");
    if (!s) s = check_hip(c, d_s2.alloc(lists), "cv::ORB second selection");
    if (!s) s = check_hip(c, d_h2.alloc(lists), "cv::ORB kept responses");
    if (!s) s = check_hip(c, d_n.alloc((3 + kCvListStrips) * BL), "cv::ORB counts");
    if (!s) s = check_hip(c, d_fsel.alloc(B * g.kp_cap), "cv::ORB keypoint positions");
    if (!s) s = check_hip(c, hipMemset(d_score, 0, B * g.frame_pyr_bytes + 64), "memset score maps");
    if (!s) s = check_hip(c, hipMemset(d_n, 0, (3 + kCvListStrips) * BL * sizeof(int)), "memset cv::ORB counts");
    if (s) return s;
    bufs = CvorbBufs{d_score, d_cand, d_n, d_n + 3 * BL, d_s1, d_h1, d_n + BL, d_s2, d_h2, d_n + 2 * BL, d_fsel};
    return RGBD_OK;
}

rgbd_status CvorbWS::run(rgbd_ctx* c, const uint8_t* d_bgr, const uint16_t* d_depth, int B, bool from_gray,
                         const ExtractHook* after_fast)
{
    const CvorbCfg& g = cfg;
    const ExtractCfg& C = c->cfg;
    const hipStream_t st = c->stream;
    rgbd_status hs = run_orb_pyramid(c, d_bgr, B, from_gray);
    if (hs) return hs;
    if ((hs = call_hook(after_fast, 0))) return hs;
    // the k_fast grid's blur blocks alone (no FAST segments): the blurred pyramid
    int tk = timer_begin(c, "k_fast(blur)");
    RGBD_TRY(c, launch_fast(c->d_pyr, c->d_cells, c->d_segs, 0, c->d_cfg, c->d_cellc, c->d_slots, B, st, c->d_blur,
                            C.blur_t0[kMaxLevels] + C.blur_e0[kMaxLevels], c->d_blur_tab, C.blur_m0[kMaxLevels]), "fast (blur blocks)");
    timer_end(c, tk);
    tk = timer_begin(c, "k_cvorb_score");
    RGBD_TRY(c, launch_cvorb_score(c->d_pyr, g, bufs, B, st), "cvorb_score");
    timer_end(c, tk);
    tk = timer_begin(c, "k_cvorb_list");
    RGBD_TRY(c, launch_cvorb_list(g, bufs, c->d_err, B, st), "cvorb_list");
    timer_end(c, tk);
    if ((hs = call_hook(after_fast, 1))) return hs;   // e.g. the deferred PnPRansac solves of earlier pipelined steps (pnp_host.cpp)
    tk = timer_begin(c, "k_cvorb_select");
    RGBD_TRY(c, launch_cvorb_select(c->d_pyr, g, bufs, B, st), "cvorb_select");
    timer_end(c, tk);
    tk = timer_begin(c, "k_cvorb_frame");
    RGBD_TRY(c, launch_cvorb_frame(g, bufs, c->out.count, c->out.kps, c->d_err, B, st), "cvorb_frame");
    timer_end(c, tk);
    if ((hs = call_hook(after_fast, 2))) return hs;
    tk = timer_begin(c, "k_cvorb_describe");
    RGBD_TRY(c, launch_cvorb_describe(c->d_pyr, c->d_blur, g, bufs, c->out.count, c->out.kps, c->out.desc, B, st), "cvorb_describe");
    timer_end(c, tk);
    tk = timer_begin(c, "k_undistort");
    RGBD_TRY(c, launch_undistort(d_depth, c->out.count, c->d_cfg, g.kp_cap, c->out.kps, c->out.kun, c->out.xyz, B, st), "undistort");
    timer_end(c, tk);
    c->last_B = B;
    return RGBD_OK;
}

}  // namespace rgbd

using namespace rgbd;

extern "C" {

rgbd_status rgbd_cvorb_debug_level(rgbd_ctx* c, int32_t b, int32_t level, int32_t stage, int32_t* xys, float* harris, int32_t cap,
                                   int32_t* n)
{
    if (!c || !n) return RGBD_ERR_ARG;
    CvorbWS* w = ws(c);
    if (!w) return not_cvorb(c);
    const CvorbCfg& g = w->cfg;
    if (b < 0 || b >= c->last_B) return fail(c, RGBD_ERR_ARG, "cv::ORB: frame index outside the last batch");
    if (level < 0 || level >= g.nlevels || stage < 0 || stage > 3 || cap < 0)
        return fail(c, RGBD_ERR_ARG, "cv::ORB: level, stage (0..3) or capacity out of range");
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    const size_t cl = (size_t)b * g.nlevels + level;
    const int* cnt = stage == 0 ? w->bufs.nfast : stage == 3 ? w->bufs.n2 : w->bufs.n1;
    int m = 0;
    s = check_hip(c, hipMemcpyAsync(&m, cnt + cl, 4, hipMemcpyDeviceToHost, c->stream), "read cv::ORB count");
    if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
    if (s) return s;
    *n = m;
    if (stage == 0 || m == 0 || (!xys && !harris)) return RGBD_OK;
    if (m > cap) return fail(c, RGBD_ERR_CAPACITY, "output capacity smaller than the level's list");
    const uint32_t* keys = stage == 3 ? w->bufs.s2 : w->bufs.s1;
    const float* resp = stage == 3 ? w->bufs.h2 : w->bufs.h1;
    if (xys && stage != 2) {
        std::vector<uint32_t> k((size_t)m);
        s = check_hip(c, hipMemcpyAsync(k.data(), keys + cl * g.cand_cap, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream), "read cv::ORB list");
        if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
        if (s) return s;
        for (int i = 0; i < m; i++) {
            xys[3 * i] = key_x(k[i]);
            xys[3 * i + 1] = key_y(k[i]);
            xys[3 * i + 2] = key_s(k[i]);
        }
    }
    if (harris && stage != 1) {
        s = check_hip(c, hipMemcpyAsync(harris, resp + cl * g.cand_cap, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream), "read cv::ORB responses");
        if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
    }
    return s;
}

}  // extern "C"
