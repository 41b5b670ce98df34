// brief_front.h -- what the SVO, adaptive, GFTT and FAST + BRIEF front ends share around their detectors: k_svo_pyramid (gray,
// halfSample levels, 9x9 box sums) as the head of an extraction, k_svo_brief + k_undistort as its tail, and the
// BRIEF-32 test table behind rgbd_svo_set / get_brief_pattern.
#pragma once
#include "context.h"
#include "svo_dev.h"

namespace rgbd {

constexpr int kBriefBorder = 48 / 2 + 9 / 2;   // BriefDescriptorExtractorImpl PATCH_SIZE, KERNEL_SIZE

struct BriefFront {
    SvoCfg cfg{};               // what k_svo_pyramid and k_svo_brief take
    DevBuf<uint8_t> d_pyr;      // [B][frame_bytes]; level 0 of frame 0 is the gray upload target
    DevBuf<uint16_t> d_box;     // [B][H][W]
    DevBuf<uint32_t> d_pat;
    int8_t pattern[256 * 4];    // host copy, the default table (brief_pattern.inc) until set_pattern

    BriefFront();
    void one_level(int W, int H, int kp_cap);   // cfg of the detectors that work on the gray image alone
    // the buffers and the table's upload (not synchronised); errors read "<who> <gray_what>", "<who> box", ...
    rgbd_status alloc(rgbd_ctx* c, const char* who, const char* gray_what);
    rgbd_status set_pattern(rgbd_ctx* c, const int8_t* pairs);   // synchronised: the caller's array may go away
    void get_pattern(int8_t* pairs) const;
    rgbd_status run_pyramid(rgbd_ctx* c, const uint8_t* d_bgr, int B, bool from_gray);
    // descriptors and undistortion of the keypoints in c->out (read at the call: pipelined steps swap output sets)
    rgbd_status run_describe(rgbd_ctx* c, const uint16_t* d_depth, int B);
};

}  // namespace rgbd
