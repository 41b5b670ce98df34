// orb_pattern_dev.h -- cv::ORB's bit_pattern_31_ (orb_pattern.inc) packed for the steered-BRIEF kernels: one dword per
// test.  Each translation unit that includes it defines its own __constant__ copy (k_cvorb_describe, k_fast_orb_describe).
#pragma once
#include <cstdint>

namespace rgbd {

namespace {
constexpr int kCvPatternRaw[256 * 4] = {
#include "orb_pattern.inc"
};
// bit_pattern_31_ with each test packed into one dword (x0, y0, x1, y1 as int8)
struct CvPattern { uint32_t v[256]; };
constexpr CvPattern make_cv_pattern()
{
    CvPattern p{};
    for (int t = 0; t < 256; t++) {
        uint32_t w = 0;
        for (int i = 0; i < 4; i++) w |= (uint32_t)(uint8_t)(int8_t)kCvPatternRaw[4 * t + i] << (8 * i);
        p.v[t] = w;
    }
    return p;
}
}  // namespace

}  // namespace rgbd
