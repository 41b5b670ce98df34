// brief_front.cpp -- the shared head and tail of the SVO, adaptive, GFTT and FAST + BRIEF extractions (brief_front.h).
#include "brief_front.h"

#include <cstring>
#include <string>

#include "launch.h"

namespace rgbd {

namespace {

const int8_t kDefaultBrief[256 * 4] = {
#include "brief_pattern.inc"
};

rgbd_status upload_pattern(rgbd_ctx* c, BriefFront* w)
{
    uint32_t packed[256];
    for (int t = 0; t < 256; t++) {
        const uint8_t* q = reinterpret_cast<const uint8_t*>(w->pattern + 4 * t);
        packed[t] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
    }
    return check_hip(c, hipMemcpyAsync(w->d_pat, packed, sizeof(packed), hipMemcpyHostToDevice, c->stream), "brief pattern");
}

BriefFront* brief_of(rgbd_ctx* c) { return c->front ? c->front->brief() : nullptr; }

rgbd_status no_brief(rgbd_ctx* c)
{
    return fail(c, RGBD_ERR_ARG, "not an SVO, adaptive, GFTT or FAST + BRIEF context (rgbd_create_svo, rgbd_create_adaptive, rgbd_create_gftt, rgbd_create_fast)");
}

}  // namespace

BriefFront::BriefFront() { std::memcpy(pattern, kDefaultBrief, sizeof(kDefaultBrief)); }

void BriefFront::one_level(int W, int H, int kp_cap)
{
    cfg.W = W;
    cfg.H = H;
    cfg.nlevels = 1;
    cfg.lw[0] = W;
    cfg.lh[0] = H;
    cfg.loff[0] = 0;
    cfg.frame_bytes = (W * H + 63) & ~63;
    cfg.kp_cap = kp_cap;
    cfg.border = kBriefBorder;
}

rgbd_status BriefFront::alloc(rgbd_ctx* c, const char* who, const char* gray_what)
{
    const size_t B = (size_t)c->maxB;
    const std::string p = std::string(who) + " ";
    rgbd_status s = check_hip(c, d_pyr.alloc(B * cfg.frame_bytes + 64), (p + gray_what).c_str());
    if (!s) s = check_hip(c, d_box.alloc(B * cfg.W * cfg.H), (p + "box").c_str());
    if (!s) s = check_hip(c, d_pat.alloc(256), (p + "pattern").c_str());
    if (!s) s = upload_pattern(c, this);
    return s;
}

rgbd_status BriefFront::set_pattern(rgbd_ctx* c, const int8_t* pairs)
{
    std::memcpy(pattern, pairs, 1024);
    const rgbd_status s = upload_pattern(c, this);
    return s ? s : check_hip(c, hipStreamSynchronize(c->stream), "sync");
}

void BriefFront::get_pattern(int8_t* pairs) const { std::memcpy(pairs, pattern, 1024); }

rgbd_status BriefFront::run_pyramid(rgbd_ctx* c, const uint8_t* d_bgr, int B, bool from_gray)
{
    const int tk = timer_begin(c, "k_svo_pyramid");
    RGBD_TRY(c, launch_svo_pyramid(from_gray ? nullptr : d_bgr, d_pyr, d_box, cfg, B, c->stream), "svo_pyramid");
    timer_end(c, tk);
    return RGBD_OK;
}

rgbd_status BriefFront::run_describe(rgbd_ctx* c, const uint16_t* d_depth, int B)
{
    const hipStream_t st = c->stream;
    int tk = timer_begin(c, "k_svo_brief");
    RGBD_TRY(c, launch_svo_brief(d_box, c->out.count, c->out.kps, d_pat, cfg, c->out.desc, B, st), "svo_brief");
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

rgbd_status rgbd_svo_set_brief_pattern(rgbd_ctx* c, const int8_t* pairs)
{
    if (!c || !pairs) return RGBD_ERR_ARG;
    BriefFront* bf = brief_of(c);
    if (!bf) return no_brief(c);
    for (int i = 0; i < 1024; i++)
        if (pairs[i] < -24 || pairs[i] > 24) return fail(c, RGBD_ERR_ARG, "BRIEF offsets must lie in [-24, 24]");
    const rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    return s ? s : bf->set_pattern(c, pairs);
}

rgbd_status rgbd_svo_get_brief_pattern(rgbd_ctx* c, int8_t* pairs)
{
    if (!c || !pairs) return RGBD_ERR_ARG;
    BriefFront* bf = brief_of(c);
    if (!bf) return no_brief(c);
    bf->get_pattern(pairs);
    return RGBD_OK;
}

}  // extern "C"
