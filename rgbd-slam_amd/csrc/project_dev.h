// project_dev.h -- argument blocks of the projection-guided matcher (project.hip), shared with its host side
// (project_host.cpp).  Operator: DESIGN.md "Projection match definition" (Matcher::projectionMatch,
// Features/Matcher.cpp:35-104 over Frame::getFeaturesInArea, Core/Frame.cpp:179-241).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rgbd_hip.h"

namespace rgbd {

constexpr int kProjCols = 64, kProjRows = 48;          // FRAME_GRID_COLS / FRAME_GRID_ROWS
constexpr int kProjCells = kProjCols * kProjRows;
constexpr int kProjKeys = 16;                          // rank keys kept per query (the rest is found again by a rescan)
constexpr int kProjMaxTrain = 65536;                   // the rank key holds the train's sorted position in 16 bits
constexpr int kProjThHigh = 100;                       // Matcher::TH_HIGH, inclusive
constexpr uint32_t kProjEmpty = 0xFFFFFFFFu;           // no key
constexpr int kProjUnresolved = -2, kProjNoMatch = -1; // per-query result until it holds the matched key

// status of a query (rgbd_debug_projection)
enum { kProjSearched = 0, kProjOutlier = 1, kProjNoDepth = 2, kProjBehind = 3, kProjOutside = 4, kProjNoCells = 5 };

struct ProjCfg {
    float fx, fy, cx, cy;
    float min_x, max_x, min_y, max_y;
    float winv, hinv;   // mfGridElementWidthInv / HeightInv: 64.f / (max_x - min_x), 48.f / (max_y - min_y)
    float th;
};

// frames as rows of `cap` keypoints: the last extraction's outputs, or the two staged host frames
struct ProjFrames {
    const int* counts;        // [frames]
    const float* kun;         // [frames][cap][7] (rgbd_keypoint; x, y read)
    const float* xyz;         // [frames][cap][3]
    const uint8_t* desc;      // [frames][cap][32]
    const uint8_t* outlier;   // [frames][cap] or null
    const float* poses;       // [frames][16] Tcw row-major
    const int* qf;            // [pairs] query frame (< 0: pair skipped)
    const int* tf;            // [pairs] train frame
    int cap;
};

// per-pair work arrays: rows of qcap queries / tcap trains
struct ProjWork {
    int qcap, tcap;
    // k_proj_grid: the train keypoints inside the grid in visiting order (cell column, cell row, index)
    int* cell_off;       // [pairs][kProjCells + 1]
    float4* s_rec;       // [pairs][tcap] x, y, the bits of (original index | (z > 0) << 16), 0
    uint4* s_desc;       // [pairs][tcap][2]
    // k_proj_search
    float2* uv;          // [pairs][qcap]
    uint32_t* win;       // [pairs][qcap] c0 | c1 << 8 | r0 << 16 | r1 << 24
    int* status;         // [pairs][qcap]
    uint32_t* keys;      // [pairs][qcap][kProjKeys] ascending (distance << 16 | sorted position), kProjEmpty-padded
    uint8_t* more;       // [pairs][qcap] candidates beyond the kept keys exist
    int* head;           // [pairs][qcap] first key not yet known taken
    int* res;            // [pairs][qcap] kProjUnresolved / kProjNoMatch / the matched key
    // k_proj_assign
    uint32_t* minq;      // [pairs][tcap] lowest unresolved query that lists the train (global form; k_proj_grid's
                         // scratch for the sorted positions before that)
    uint8_t* taken;      // [pairs][tcap]
    rgbd_dmatch* out;    // [pairs][qcap]
    int* out_count;      // [pairs]
    // rgbd_debug_projection (one pair): candidates before the z and taken filters
    int* cand;           // [qcap][ccap] original train indices, visiting order
    int* ccount;         // [qcap] (may exceed ccap)
    int ccap;
};

}  // namespace rgbd
