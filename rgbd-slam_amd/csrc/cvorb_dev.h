// cvorb_dev.h -- the OpenCV ORB extractor (the reference's Extractor(ORB, ORB, NORMAL), Features/Extractor.cpp:
// 163-166, 216-218): per-launch configuration and launchers (cvorb.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rgbd_internal.h"

namespace rgbd {

constexpr int kCvorbMaxFeatures = 8192;         // nfeatures bound
constexpr int kCvorbDefaultCandCap = 8192;      // stored FAST corners per (frame, level)
constexpr int kCvorbMaxCandCap = 12288;         // cand_cap bound: the selection's list lives in LDS (10 B per corner)
constexpr int kCvorbFrameCap = 12288;           // keypoints of all levels the frame-level selection takes (same LDS bound)
constexpr int kCvorbThreads = 1024;             // k_cvorb_select / k_cvorb_frame: one workgroup each
constexpr int kCvListStrips = 8;                // k_cvorb_list: row strips per level, one workgroup each
constexpr int kCvorbErrCand = 16;               // rgbd_ctx::d_err bits: a level has more FAST corners than cand_cap,
constexpr int kCvorbErrKeep = 32;               // the frame keeps more keypoints than max_keypoints
constexpr int kCvorbDescBorder = 31;            // cv::ORB::create()'s edgeThreshold (the descriptor side)

struct CvorbCfg {
    int32_t W, H, nlevels;
    int32_t frame_pyr_bytes;      // the ORB geometry's pyramid layout (rgbd_internal.h), also the score maps'
    int32_t nfeatures;
    int32_t edge;                 // edge_threshold
    int32_t thr;                  // fast_threshold
    int32_t cand_cap;
    int32_t kp_cap;               // max_keypoints
    int32_t frame_cap;            // min(kCvorbFrameCap, nlevels * cand_cap)
    float ssq;                    // (1 / (4 * 7 * 255))^4, f32 products left to right
    int32_t lw[kMaxLevels], lh[kMaxLevels], lstride[kMaxLevels], loff[kMaxLevels];
    int32_t N[kMaxLevels];        // cv::ORB's per-level budgets
    float scale[kMaxLevels];      // layerScale[l] = (float)pow((double)scale_factor, (double)l)
    float size[kMaxLevels];       // 31 * layerScale[l]
    int32_t umax[16];             // IC_Angle's half-widths
};

// a stored corner: level x | y << 11 | FAST score << 22 (pack_key); a final keypoint's position for k_cvorb_describe:
// level x | y << 11 | level << 22
//
// per batch of B frames, L = nlevels, C = cand_cap:
//   score [B][frame_pyr_bytes] u8   FAST-9 score S of every level pixel where S >= fast_threshold, else 0
//   cand  [B][L][C] u32, nfast [B][L]   the level's corners inside the border in raster order; nfast counts past C
//   nstrip [B][L][kCvListStrips]        the corners of each row strip of the level (k_cvorb_list's counting pass)
//   s1    [B][L][C] u32, h1 [B][L][C] f32, n1 [B][L]   after retainBest(2 N) on the score, with the Harris responses
//   s2    [B][L][C] u32, h2 [B][L][C] f32, n2 [B][L]   after retainBest(N) on the Harris response
//   fsel  [B][kp_cap] u32          the final keypoints' level positions, in output order
struct CvorbBufs {
    uint8_t* score;
    uint32_t* cand;
    int* nfast;
    int* nstrip;
    uint32_t* s1;
    float* h1;
    int* n1;
    uint32_t* s2;
    float* h2;
    int* n2;
    uint32_t* fsel;
};

hipError_t launch_cvorb_score(const uint8_t* pyr, const CvorbCfg& g, const CvorbBufs& w, int B, hipStream_t st);
hipError_t launch_cvorb_list(const CvorbCfg& g, const CvorbBufs& w, int* err, int B, hipStream_t st);
hipError_t launch_cvorb_select(const uint8_t* pyr, const CvorbCfg& g, const CvorbBufs& w, int B, hipStream_t st);
hipError_t launch_cvorb_frame(const CvorbCfg& g, const CvorbBufs& w, int* counts, float* kps, int* err, int B, hipStream_t st);
hipError_t launch_cvorb_describe(const uint8_t* pyr, const uint8_t* blur, const CvorbCfg& g, const CvorbBufs& w, const int* counts,
                                 float* kps, uint8_t* desc, int B, hipStream_t st);

}  // namespace rgbd
