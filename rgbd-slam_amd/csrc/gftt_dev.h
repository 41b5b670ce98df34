// gftt_dev.h -- the Shi-Tomasi GFTT + BRIEF extractor (the reference's Extractor(GFTT, BRIEF, NORMAL),
// Features/Extractor.cpp:178-181): per-launch configuration and launchers (gftt.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rgbd_internal.h"

namespace rgbd {

constexpr int kGfttMaxCorners = 12288;          // nfeatures bound: the accepted list lives in LDS (4 B per corner)
constexpr int kGfttDefaultCandCap = 32768;      // about 1.6x a uniform-noise 640 x 480 frame (about 20,300 candidates)
constexpr int kGfttMaxCandCap = 1 << 20;        // cand_cap bound (8 B per candidate and frame)
constexpr int kGfttMaxChunk = 4096;             // ranks per selection pass: the sorted chunk lives in LDS
constexpr int kGfttSelThreads = 1024;           // k_gftt_select: one workgroup per frame
constexpr int kGfttErrFlag = 8;                 // the frame's bit in rgbd_ctx::d_err: more candidates than cand_cap

struct GfttCfg {
    int32_t W, H;
    int32_t nfeatures;        // maxCorners
    int32_t cand_cap;         // stored candidates per frame
    int32_t chunk;            // ranks per selection pass
    int32_t dist_lim;         // ceil(min_distance^2): integer d2 < min_distance^2 (f64) <=> d2 < dist_lim; 0: no spacing test
    int32_t border;           // BRIEF runByImageBorder: 28
    int32_t kp_cap;           // = nfeatures
    double quality_level;
};

// a candidate's rank key: the eigenvalue's bits (positive floats order as unsigned) above its raster index
// y * W + x, so descending keys are step 8's order and keys are unique
RGBD_HD inline uint64_t gftt_key(uint32_t val_bits, uint32_t raster) { return ((uint64_t)val_bits << 32) | raster; }

// the default chunk for a corner budget: the greedy consumes about 1.1 ranks per accepted corner on real
// frames (profiles/gftt), so the power of two at or above 1.25x the budget usually ends in one pass
RGBD_HD inline int gftt_default_chunk(int max_corners)
{
    int c = 256;
    while (c < kGfttMaxChunk && c < max_corners + max_corners / 4) c *= 2;
    return c;
}

// per batch of B frames:
//   maxkey [B] u32          order-preserving image of the frame's largest e (0: below every float)
//   keys   [B][cand_cap]    candidates' rank keys, in arrival order
//   ncand  [B]              candidates found (may exceed cand_cap: then the frame's flag is raised)
//   corners[B][nfeatures]   accepted corners' keys in acceptance order (before the border filter)
//   ncorner[B], ranks[B]    accepted corners; ranks the greedy consumed
hipError_t launch_gftt_max(const uint8_t* gray, size_t frame_bytes, const GfttCfg& g, uint32_t* maxkey, int B, hipStream_t st);
hipError_t launch_gftt_cand(const uint8_t* gray, size_t frame_bytes, const GfttCfg& g, const uint32_t* maxkey, uint64_t* keys,
                            int* ncand, int* err, int B, hipStream_t st);
hipError_t launch_gftt_eig(const uint8_t* gray, const GfttCfg& g, float* out, hipStream_t st);   // one frame's raw map
// rank + spacing (+ border filter and keypoints when kps != nullptr); ncand == nullptr: every frame has n_fixed keys
hipError_t launch_gftt_select(const uint64_t* keys, const int* ncand, int n_fixed, const GfttCfg& g, uint64_t* corners,
                              int* ncorner, int* ranks, int* counts, float* kps, int B, hipStream_t st);
RGBD_HD inline float gftt_decode_max(uint32_t k)
{
    const uint32_t b = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
    union { uint32_t u; float f; } v;
    v.u = b;
    return v.f;
}

}  // namespace rgbd
