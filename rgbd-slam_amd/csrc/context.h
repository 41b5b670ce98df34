// context.h -- the rgbd_ctx behind the C ABI (host runtime, not exported).
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/rgbd_hip.h"
#include "devmem.h"
#include "rgbd_internal.h"

namespace rgbd {
struct RansacWS; struct PnpWS; struct PnpPipe; struct GicpWS; struct LaneWS; struct CloudWS; struct ProjWS; struct BaWS; struct UmWS; struct BowWS; struct BriefFront;
// the per-batch extraction outputs a step's knn-2 / gather read, as the kernels see them
struct OutSet {
    int* count = nullptr;
    float* kps = nullptr;
    float* kun = nullptr;
    uint8_t* desc = nullptr;
    float* xyz = nullptr;
    int4* knn = nullptr;
};
struct OutBufs {   // one owned set
    DevBuf<int> count;
    DevBuf<float> kps, kun;
    DevBuf<uint8_t> desc;
    DevBuf<float> xyz;
    DevBuf<int4> knn;
    OutSet view() const { return OutSet{count, kps, kun, desc, xyz, knn}; }
};
// called by an extraction at its launch points (launch-stream order): 0 before FAST, 1 after FAST,
// 2 after the quadtree (the pipelined PnP solves use point 1; SVO extractions call points 1 and 2)
using ExtractHook = std::function<rgbd_status(int at)>;
inline rgbd_status call_hook(const ExtractHook* hook, int at) { return hook ? (*hook)(at) : RGBD_OK; }
// an extractor other than the ORBextractor, in rgbd_ctx::front.  Its debug and state entry points are free functions
// of the file that defines it, which downcasts the slot to its own type.
struct FrontEnd {
    virtual ~FrontEnd() = default;
    virtual rgbd_status alloc(rgbd_ctx* c) = 0;   // after the context's own allocations
    virtual rgbd_status run(rgbd_ctx* c, const uint8_t* d_bgr, const uint16_t* d_depth, int B, bool from_gray,
                            const ExtractHook* after_fast) = 0;   // one launch chain, ends with last_B set
    virtual BriefFront* brief() { return nullptr; }   // the SVO pyramid + BRIEF plumbing, where the extractor uses it
};
}  // namespace rgbd

struct rgbd_ctx {
    int device = 0;
    int W = 0, H = 0, maxB = 0;
    rgbd_camera cam{};
    rgbd::ExtractCfg cfg{};              // host copy of the geometry (geometry.cpp); its tables live on the device only
    int n_segs = 0;                      // k_fast segments per frame (d_segs)
    std::string err;

    hipStream_t stream = nullptr;        // launch stream (own or external)
    hipStream_t own_stream = nullptr;
    hipStream_t match_stream = nullptr;  // pipelined API: knn-2 + gather of a step beside the next extraction
    hipStream_t solve_stream = nullptr;  // high-priority stream of the pipelined PnPRansac solves: the
                                         // latency-bound solve of step i runs beside step i+1's extraction
    bool serial = false;                 // RGBD_SERIAL=1: match / solve streams are the launch stream
                                         // (kernels never overlap: attributable PMC counters)

    // device workspace
    rgbd::DevBuf<rgbd::ExtractCfg> d_cfg;
    rgbd::DevBuf<rgbd::Cell> d_cells;
    rgbd::DevBuf<rgbd::FastSeg> d_segs;
    rgbd::DevBuf<rgbd::ResizeX> d_rsx;
    rgbd::DevBuf<rgbd::ResizeY> d_rsy;
    rgbd::DevBuf<rgbd::QuadX> d_qx;
    rgbd::DevBuf<uint8_t> d_blur_tab;          // operand tables of the level blur on the matrix cores (blur_tab.h)
    rgbd::DevBuf<uint8_t> d_pyr;
    rgbd::DevBuf<uint8_t> d_blur;              // blurred pyramid, same layout as d_pyr
    rgbd::DevBuf<int> d_cellc;
    rgbd::DevBuf<uint32_t> d_slots;
    rgbd::DevBuf<uint32_t> d_keys;
    rgbd::DevBuf<uint16_t> d_node;
    rgbd::DevBuf<int> d_selc;
    rgbd::DevBuf<uint32_t> d_sel;
    rgbd::DevBuf<uint8_t> d_dist_path;         // k_distribute: the path of every (frame, level) tree (rgbd_debug_dist_path)
    rgbd::OutBufs own_out;               // the context's own output set; knn: [maxB][kp_cap]
    rgbd::OutSet out{};                  // the set the kernels read and write: own_out unless a pipelined
                                         // submission selected the second one (pnp_host.cpp)
    rgbd::DevBuf<int> d_err;
    rgbd::DevBuf<uint8_t> d_in_bgr;            // single-frame staging (host-buffer entry points)
    rgbd::DevBuf<uint16_t> d_in_depth;
    rgbd::DevBuf<int> d_pairs;                 // qf[maxB], tf[maxB]
    // host-array knn staging
    rgbd::DevBuf<uint8_t> d_mdesc;
    rgbd::DevBuf<int> d_mcount;
    rgbd::DevBuf<int4> d_mknn;
    int last_B = 0;
    rgbd::Event extract_done;            // recorded after every extraction on the stream it ran on
    hipStream_t extract_stream = nullptr;

    // workspaces, each owned and freed by the file that defines it (*_free below)
    rgbd::RansacWS* ransac = nullptr;    // solver.cpp
    rgbd::PnpWS* pnp = nullptr;          // PnPRansac (pnp_host.cpp)
    rgbd::PnpPipe* pnp_pipe = nullptr;   // the PnPRansac workspaces of the submit / collect tracking API
    int pnp_chunk = 0, pnp_chunk2 = 0;   // PnPRansac device chunks, adapted per solve (pnp_host.cpp)
    rgbd::GicpWS* gicp = nullptr;        // gicp_host.cpp
    rgbd::LaneWS* lanes = nullptr;       // device-resident RansacSE3 tracking chain (lanes_host.cpp)
    rgbd::CloudWS* cloud = nullptr;      // keyframe cloud (cloud_host.cpp)
    std::unique_ptr<rgbd::FrontEnd> front;   // the extractor; null: the ORBextractor
    rgbd::ProjWS* proj = nullptr;        // projection-guided matching (project_host.cpp)
    rgbd::BaWS* pnpba = nullptr;         // motion-only bundle adjustment, PnPSolver (pnpba_host.cpp)
    rgbd::UmWS* umeyama = nullptr;       // Umeyama RANSAC, Ransac (umeyama_host.cpp)
    rgbd::BowWS* bow = nullptr;          // vocabulary, BoW transform and loop database (bow_host.cpp)
    bool bounds_set = false;             // rgbd_image_bounds: computed on first use
    rgbd_bounds bounds{};
    rgbd_gicp_params track_gicp{10, 20, 0.07, 1e-9, 2e-3, 1e-3, 4, 1};

    // timing
    bool timing = false;
    std::string timing_only;             // non-empty: only launches of this kernel are timed
    struct TEntry { std::string name; double ms = 0; long launches = 0; };
    std::vector<TEntry> tentries;
    struct Pending { int idx; hipEvent_t a, b; hipStream_t st; bool ended; };   // ended: b was recorded
    std::vector<Pending> pending;
    std::vector<hipEvent_t> event_pool;
};

namespace rgbd {
rgbd_status extract_batch(rgbd_ctx* c, const void* d_bgr, const void* d_depth, int B, const ExtractHook* after_fast);
// records the elapsed time of the launches between begin and end under `name`
int timer_begin(rgbd_ctx* c, const char* name, hipStream_t st = nullptr);   // nullptr: the context stream
void timer_end(rgbd_ctx* c, int tok);
void timer_flush(rgbd_ctx* c);
rgbd_status fail(rgbd_ctx* c, rgbd_status code, const std::string& msg);
// what a frame's extraction flag (rgbd_ctx::d_err, nonzero) says, for RGBD_ERR_CAPACITY: one wording on every path
inline const char* extract_flag_message(int flag)
{
    if (flag & 128) return "FAST: keypoints kept by retainBest exceed max_keypoints (retainBest keeps ties)";
    if (flag & 64) return "FAST: the frame has more corners than cand_cap stores";
    if (flag & 32) return "cv::ORB: the frame keeps more keypoints than max_keypoints (retainBest keeps ties)";
    if (flag & 16) return "cv::ORB: a level has more FAST corners than cand_cap stores";
    if (flag & 8) return "gftt: the frame has more candidates than cand_cap stores";
    if (flag & 4) return "adaptive: a cell has more corners at its threshold than cell_cap stores";
    if (flag & 2) return "SVO: keypoints kept by retainBest exceed rgbd_max_keypoints";
    return "quadtree node capacity exceeded";
}
rgbd_status check_hip(rgbd_ctx* c, hipError_t e, const char* what);
// cv::Mat(CV_32F) * cv::Mat on 4x4 row-major matrices: OpenCV's gemm for 32F accumulates each dot product in
// double in k order (GEMMSingleMul<float,double>) and rounds once
inline void matmul4(const float* A, const float* B, float* C)
{
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0.0;
            for (int k = 0; k < 4; k++) s += (double)A[4 * i + k] * (double)B[4 * k + j];
            C[4 * i + j] = (float)s;
        }
}
// c->stream waits for the last extraction when that ran on another stream (api.cpp)
rgbd_status order_after_extraction(rgbd_ctx* c);
// a launcher's status (dispatch.h: geometry, LDS opt-in and launch checked) as the entry point's result
#define RGBD_TRY(c, call, what)                                                            \
    do {                                                                                   \
        const rgbd_status rgbd_try_s_ = check_hip((c), (call), "launch of k_" what);        \
        if (rgbd_try_s_) return rgbd_try_s_;                                               \
    } while (0)
void ransac_free(rgbd_ctx* c);   // solver.cpp
void pnp_free(rgbd_ctx* c);      // pnp_host.cpp
void gicp_free(rgbd_ctx* c);     // gicp_host.cpp
void cloud_free(rgbd_ctx* c);    // cloud_host.cpp
void proj_free(rgbd_ctx* c);     // project_host.cpp
void pnpba_free(rgbd_ctx* c);    // pnpba_host.cpp
void umeyama_free(rgbd_ctx* c);  // umeyama_host.cpp
void bow_free(rgbd_ctx* c);      // bow_host.cpp
// k_pyramid and k_pyr_tail, or k_gray for a one-level pyramid, into c->d_pyr (api.cpp)
rgbd_status run_orb_pyramid(rgbd_ctx* c, const uint8_t* d_bgr, int B, bool from_gray);
// the extractors' configure steps: each validates, sets c->front and cfg.kp_cap (which sizes the output arrays)
rgbd_status svo_configure(rgbd_ctx* c, const rgbd_svo_params& p);             // svo_host.cpp
rgbd_status adaptive_configure(rgbd_ctx* c, const rgbd_adaptive_params& p);   // adaptive_host.cpp
rgbd_status gftt_configure(rgbd_ctx* c, const rgbd_gftt_params& p);           // gftt_host.cpp
rgbd_status fast_configure(rgbd_ctx* c, const rgbd_fast_params& p);           // fast_host.cpp
rgbd_status cvorb_check_params(rgbd_ctx* c, const rgbd_cvorb_params& p);      // cvorb_host.cpp: the parameter refusals, before the geometry's
rgbd_status cvorb_configure(rgbd_ctx* c, const rgbd_cvorb_params& p);         // on an accepted geometry
}  // namespace rgbd
