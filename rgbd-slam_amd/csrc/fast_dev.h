// fast_dev.h -- the plain FAST extractor (the reference's Extractor(FAST, BRIEF | ORB, NORMAL), Features/Extractor.cpp:
// 50-61, 168-171, 216-218, 224-226): per-launch configuration and launchers (fast.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "adaptive_dev.h"

namespace rgbd {

constexpr int kFastMaxFeatures = 12288;       // nfeatures bound
constexpr int kFastDefaultCandCap = 32768;    // stored corners per frame (a uniform-noise 640 x 480 frame has 31,337)
constexpr int kFastMaxCandCap = 65536;        // cand_cap bound: the selection's payload is 16 bits wide
constexpr int kFastLdsTier = 12288;           // live ranges up to this many elements are selected in LDS (10 B each)
constexpr int kFastThreads = 1024;            // k_fast_select: one workgroup per frame
constexpr int kFastRowThreads = 256;          // k_fast_rows: one workgroup per image row
constexpr int kFastErrCand = 64;              // rgbd_ctx::d_err bits: more corners than cand_cap stores,
constexpr int kFastErrKeep = 128;             // more keypoints kept by retainBest than max_keypoints
constexpr int kFastOrbBorder = 31;            // cv::ORB::create()'s edgeThreshold: compute()'s runByImageBorder

struct FastCfg {
    int32_t W, H;
    int32_t thr;          // cv::FAST's threshold (1..255)
    int32_t nfeatures;    // retainBest(nfeatures), Features/Extractor.cpp:56-57
    int32_t cand_cap;     // stored corners per frame
    int32_t kp_cap;       // max_keypoints
    int32_t border;       // the descriptor's runByImageBorder: 28 (BRIEF), 31 (ORB)
    int32_t sstride;      // row stride of the gray image and of the score map: W (BRIEF), the ORB pyramid's level-0 stride (ORB)
};

// per batch of B frames, C = cand_cap:
//   smap  [B][H][sstride] u8   k_adp_score's threshold-free score S = max(M, 1) - 1 (columns from W - 3 on are not read)
//   rowc  [B][H]          strict 3x3 maxima with S >= thr of every row
//   cand  [B][C] u32      those maxima in raster order as adp_pack(x, y, S); ncand [B] counts past C
//   R [B][C] f32, I / posL / posR [B][C] u16   k_fast_select's scratch while the live range exceeds kFastLdsTier
struct FastBufs {
    uint8_t* smap;
    int* rowc;
    uint32_t* cand;
    int* ncand;
    float* R;
    uint16_t* I;
    uint16_t* posL;
    uint16_t* posR;
};

hipError_t launch_fast_rows(const FastCfg& g, const FastBufs& w, int* err, int B, hipStream_t st);
hipError_t launch_fast_select(const FastCfg& g, const FastBufs& w, int* counts, float* kps, int* err, int B, hipStream_t st);
// the ORB descriptor of the keypoints in kps (integer positions, the stored angle): level 0 of the blurred ORB pyramid
hipError_t launch_fast_orb_describe(const uint8_t* blur, size_t frame_bytes, int stride, const FastCfg& g, const int* counts,
                                    const float* kps, uint8_t* desc, int B, hipStream_t st);
// k_fast_select's retainBest(nkeep) on n responses already in w.R (n <= kFastMaxCandCap): order[0..*m)
hipError_t launch_fast_retain_test(const FastBufs& w, int n, int nkeep, int depth_limit, int* order, int* m, hipStream_t st);

}  // namespace rgbd
