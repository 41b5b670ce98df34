// adaptive_dev.h -- the adaptive FAST + BRIEF extractor (the reference's Extractor(FAST, BRIEF, ADAPTIVE),
// Features/Extractor.cpp:82-109): per-launch configuration and launchers (adaptive.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rgbd_internal.h"

namespace rgbd {

constexpr int kAdpMaxGrid = 8;            // grid_rows, grid_cols <= 8
constexpr int kAdpMaxCells = kAdpMaxGrid * kAdpMaxGrid;
constexpr int kAdpSelMax = 12288;         // introselect's LDS bound (R, I, posL, posR: 10 B per element)
constexpr int kAdpThreads = 1024;         // k_adp_cells / k_adp_select / k_adp_frame: one workgroup per cell or frame
constexpr int kAdpDefaultCellCap = 8192;  // DESIGN.md, "Adaptive FAST + BRIEF definition": about 3x a rich cell at threshold 2

struct AdpCfg {
    int32_t W, H;
    int32_t rows, cols, ncells, edge;     // VideoGridAdaptedFeatureDetector(.., gridRows, gridCols, edgeThreshold)
    int32_t iterations;                   // VideoDynamicAdaptedFeatureDetector's mEscapeIters
    int32_t grid_min, grid_max;           // its mMinFeatures / mMaxFeatures (per cell)
    int32_t max_per_cell;                 // keepStrongest(maxPerCell)
    int32_t nfeatures;                    // retainBest(nfeatures), Features/Extractor.cpp:56-57
    int32_t kp_cap;                       // ncells * max_per_cell: what a frame can hold before retainBest
    int32_t cell_cap;                     // stored maxima per (frame, cell)
    int32_t tmin;                         // max(1, (int)min_thresh): the weakest score a list keeps
    int32_t border;                       // BRIEF runByImageBorder: 28
    int32_t pad;
    double min_thresh, max_thresh, increase, decrease;   // DetectorAdjuster
};

// cell (i, j)'s ROI (VideoGridAdaptedFeatureDetector.cpp:62-69): rows [y0, y1), columns [x0, x1)
RGBD_HD inline void adp_roi(const AdpCfg& g, int cell, int& x0, int& y0, int& x1, int& y1)
{
    const int i = cell / g.cols, j = cell - i * g.cols;
    y0 = (i * g.H) / g.rows - g.edge;
    if (y0 < 0) y0 = 0;
    y1 = ((i + 1) * g.H) / g.rows + g.edge;
    if (y1 > g.H) y1 = g.H;
    x0 = (j * g.W) / g.cols - g.edge;
    if (x0 < 0) x0 = 0;
    x1 = ((j + 1) * g.W) / g.cols + g.edge;
    if (x1 > g.W) x1 = g.W;
}

// a stored corner: y (12 bits) | x (12 bits) | score (8 bits)
RGBD_HD inline uint32_t adp_pack(int x, int y, int s) { return ((uint32_t)y << 20) | ((uint32_t)x << 8) | (uint32_t)s; }
RGBD_HD inline int adp_x(uint32_t k) { return (int)((k >> 8) & 4095u); }
RGBD_HD inline int adp_y(uint32_t k) { return (int)(k >> 20); }
RGBD_HD inline int adp_s(uint32_t k) { return (int)(k & 255u); }

// per batch of B frames (c = b * ncells + cell):
//   smap  [B][H][W] u8       the threshold-free FAST-9 score S = max(M, 1) - 1 (0 where the ring leaves the image)
//   list  [c][cell_cap] u32  the ROI's strict 3x3 maxima with S >= tmin in raster order (ROI coordinates)
//   nlist [c]                how many of them were stored (<= cell_cap)
//   nge   [c][256]           nge[t] = strict maxima with S >= t (all of them, stored or not)
//   before [c] f64, used [c], tries [c]   the threshold chain's record;  state [ncells] f64
//   sel   [c][max_per_cell] u32, nsel [c]   keepStrongest's survivors in libstdc++'s order (image coordinates)
hipError_t launch_adp_score(const uint8_t* gray, size_t frame_bytes, uint8_t* smap, const AdpCfg& g, int B, hipStream_t st);
hipError_t launch_adp_cells(const uint8_t* smap, const AdpCfg& g, uint32_t* list, int* nlist, int* nge, int B, hipStream_t st);
hipError_t launch_adp_chain(const int* nge, const AdpCfg& g, double* state, double* before, int* used, int* tries, int B,
                            hipStream_t st);
hipError_t launch_adp_select(const uint32_t* list, const int* nlist, const int* nge, const int* used, const AdpCfg& g,
                             uint32_t* sel, int* nsel, int* err, int B, hipStream_t st);
hipError_t launch_adp_frame(const uint32_t* sel, const int* nsel, const AdpCfg& g, int* counts, float* kps, int B,
                            hipStream_t st);
// the device std::nth_element(begin, begin + nth, end) of k_adp_select on a given response array (parity tests)
hipError_t launch_adp_keep_test(const float* resp, int n, int nth, int depth_limit, int* order, hipStream_t st);

}  // namespace rgbd
