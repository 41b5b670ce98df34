// adaptive_host.cpp -- host side of the adaptive FAST + BRIEF front end (adaptive.hip): Extractor(FAST, BRIEF,
// ADAPTIVE), behind the same extraction entry points as the ORBextractor and the SVO front end.
//   Extractor::createAdaptiveDetector Features/Extractor.cpp:82-109  -> adaptive_configure (AdpCfg, derived counts)
//   Extractor::detectAndCompute       Features/Extractor.cpp:50-61   -> AdpWS::run (one launch chain)
//   Frame::undistortKeyPoints + uprojectCamera (Core/Frame.cpp:91-117, 251-281) -> k_undistort
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "adaptive_dev.h"
#include "brief_front.h"
#include "launch.h"

namespace rgbd {

struct AdpWS : FrontEnd {
    AdpCfg cfg{};
    BriefFront bf;                // one level: gray + box sums
    DevBuf<uint8_t> d_smap;       // [B][H][W]
    DevBuf<uint32_t> d_list;      // [B][ncells][cell_cap]
    DevBuf<int> d_nlist;          // [B][ncells]
    DevBuf<int> d_nge;            // [B][ncells][256]
    DevBuf<double> d_state;       // [ncells]
    DevBuf<double> d_before;      // [B][ncells]
    DevBuf<int> d_used, d_tries;  // [B][ncells]
    DevBuf<uint32_t> d_sel;       // [B][ncells][max_per_cell]
    DevBuf<int> d_nsel;           // [B][ncells]
    DevBuf<float> d_kt_resp;      // rgbd_adaptive_keep_strongest staging
    DevBuf<int> d_kt_order;
    double init_thresh = 20.0;

    rgbd_status alloc(rgbd_ctx* c) override;
    rgbd_status run(rgbd_ctx* c, const uint8_t* d_bgr, const uint16_t* d_depth, int B, bool from_gray,
                    const ExtractHook* after_fast) override;
    BriefFront* brief() override { return &bf; }
};

namespace {

AdpWS* ws(rgbd_ctx* c) { return dynamic_cast<AdpWS*>(c->front.get()); }   // null: not an adaptive context

rgbd_status not_adaptive(rgbd_ctx* c) { return fail(c, RGBD_ERR_ARG, "not an adaptive context (rgbd_create_adaptive)"); }

}  // namespace

rgbd_status adaptive_configure(rgbd_ctx* c, const rgbd_adaptive_params& p)
{
    // every refusal before anything is allocated
    if (!(p.min_thresh >= 1.0) || !(p.min_thresh <= p.init_thresh) || !(p.init_thresh <= p.max_thresh) || !(p.max_thresh <= 1e9))
        return fail(c, RGBD_ERR_UNSUPPORTED, "adaptive: 1 <= min_thresh <= init_thresh <= max_thresh <= 1e9 (the score map serves thresholds >= 1)");
    if (!(p.decrease > 0.0 && p.decrease < 1.0 && p.increase > 1.0))
        return fail(c, RGBD_ERR_UNSUPPORTED, "adaptive: 0 < decrease < 1 < increase");
    if (p.iterations < 1 || p.iterations > 32) return fail(c, RGBD_ERR_UNSUPPORTED, "adaptive: iterations must be 1..32");
    if (p.grid_rows < 1 || p.grid_rows > kAdpMaxGrid || p.grid_cols < 1 || p.grid_cols > kAdpMaxGrid)
        return fail(c, RGBD_ERR_UNSUPPORTED, "adaptive: a grid of 1..8 by 1..8 cells");
    if (p.edge_threshold < 0) return fail(c, RGBD_ERR_UNSUPPORTED, "adaptive: edge_threshold >= 0");
    if (p.nfeatures < 0 || p.min_features < 0) return fail(c, RGBD_ERR_UNSUPPORTED, "adaptive: nfeatures >= 0, min_features >= 0");
    if (c->W < 1 || c->H < 1 || c->W > 2047 || c->H > 2047) return fail(c, RGBD_ERR_UNSUPPORTED, "adaptive: image sides 1..2047");
    const int cap = p.cell_cap > 0 ? p.cell_cap : kAdpDefaultCellCap;
    if (p.cell_cap < 0 || cap > kAdpSelMax) return fail(c, RGBD_ERR_UNSUPPORTED, "adaptive: cell_cap must be 1..12288 (0: 8192)");
    AdpCfg g{};
    g.W = c->W;
    g.H = c->H;
    g.rows = p.grid_rows;
    g.cols = p.grid_cols;
    g.ncells = g.rows * g.cols;
    g.edge = p.edge_threshold;
    g.iterations = p.iterations;
    // Extractor::createAdaptiveDetector (:97-105): int maxFeatures = minFeatures * 1.7; round(x / float(cells))
    const int max_features = (int)((double)p.min_features * 1.7);
    if (max_features > kAdpSelMax) return fail(c, RGBD_ERR_UNSUPPORTED, "adaptive: (int)(min_features * 1.7) <= 12288");
    g.grid_min = (int)std::round((float)p.min_features / (float)g.ncells);
    g.grid_max = (int)std::round((float)max_features / (float)g.ncells);
    g.max_per_cell = max_features / g.ncells;
    if (g.max_per_cell < 1) return fail(c, RGBD_ERR_UNSUPPORTED, "adaptive: maxPerCell = (int)(min_features * 1.7) / cells must be >= 1");
    for (int k = 0; k < g.ncells; k++) {
        int x0, y0, x1, y1;
        adp_roi(g, k, x0, y0, x1, y1);
        if (x1 - x0 < 7 || y1 - y0 < 7) return fail(c, RGBD_ERR_UNSUPPORTED, "adaptive: every cell ROI must be at least 7 x 7");
    }
    g.nfeatures = p.nfeatures;
    g.kp_cap = g.ncells * g.max_per_cell;
    g.cell_cap = cap;
    g.tmin = std::max(1, (int)p.min_thresh);
    g.border = kBriefBorder;
    g.min_thresh = p.min_thresh;
    g.max_thresh = p.max_thresh;
    g.increase = p.increase;
    g.decrease = p.decrease;
    AdpWS* w = new AdpWS();
    c->front.reset(w);
    w->cfg = g;
    w->init_thresh = p.init_thresh;
    w->bf.one_level(c->W, c->H, g.kp_cap);
    c->cfg.kp_cap = g.kp_cap;   // the output arrays (kps, desc, xyz, knn) are sized by it
    return RGBD_OK;
}

rgbd_status AdpWS::alloc(rgbd_ctx* c)
{
    const AdpCfg& g = cfg;
    const size_t B = (size_t)c->maxB, nc = (size_t)g.ncells;
    rgbd_status s = bf.alloc(c, "adaptive", "gray");
    if (!s) s = check_hip(c, d_smap.alloc(B * g.W * g.H), "adaptive score map");
    if (!s) s = check_hip(c, d_list.alloc(B * nc * g.cell_cap), "adaptive cell lists");
    if (!s) s = check_hip(c, d_nlist.alloc(B * nc), "adaptive list counts");
    if (!s) s = check_hip(c, d_nge.alloc(B * nc * 256), "adaptive suffix counts");
    if (!s) s = check_hip(c, d_state.alloc(nc), "adaptive thresholds");
    if (!s) s = check_hip(c, d_before.alloc(B * nc), "adaptive thresholds before");
    if (!s) s = check_hip(c, d_used.alloc(B * nc), "adaptive thresholds used");
    if (!s) s = check_hip(c, d_tries.alloc(B * nc), "adaptive tries");
    if (!s) s = check_hip(c, d_sel.alloc(B * nc * g.max_per_cell), "adaptive cell survivors");
    if (!s) s = check_hip(c, d_nsel.alloc(B * nc), "adaptive survivor counts");
    if (s) return s;
    std::vector<double> init(nc, init_thresh);
    s = check_hip(c, hipMemcpy(d_state, init.data(), nc * 8, hipMemcpyHostToDevice), "adaptive thresholds up");
    if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
    return s;
}

rgbd_status AdpWS::run(rgbd_ctx* c, const uint8_t* d_bgr, const uint16_t* d_depth, int B, bool from_gray,
                       const ExtractHook* after_fast)
{
    const AdpCfg& g = cfg;
    const hipStream_t st = c->stream;
    rgbd_status s = bf.run_pyramid(c, d_bgr, B, from_gray);
    if (s) return s;
    int tk = timer_begin(c, "k_adp_score");
    RGBD_TRY(c, launch_adp_score(bf.d_pyr, (size_t)bf.cfg.frame_bytes, d_smap, g, B, st), "adp_score");
    timer_end(c, tk);
    tk = timer_begin(c, "k_adp_cells");
    RGBD_TRY(c, launch_adp_cells(d_smap, g, d_list, d_nlist, d_nge, B, st), "adp_cells");
    timer_end(c, tk);
    // e.g. the deferred PnPRansac solves of earlier pipelined steps (pnp_host.cpp)
    if ((s = call_hook(after_fast, 1)) || (s = call_hook(after_fast, 2))) return s;
    tk = timer_begin(c, "k_adp_chain");
    RGBD_TRY(c, launch_adp_chain(d_nge, g, d_state, d_before, d_used, d_tries, B, st), "adp_chain");
    timer_end(c, tk);
    tk = timer_begin(c, "k_adp_select");
    RGBD_TRY(c, launch_adp_select(d_list, d_nlist, d_nge, d_used, g, d_sel, d_nsel, c->d_err, B, st), "adp_select");
    timer_end(c, tk);
    tk = timer_begin(c, "k_adp_frame");
    RGBD_TRY(c, launch_adp_frame(d_sel, d_nsel, g, c->out.count, c->out.kps, B, st), "adp_frame");
    timer_end(c, tk);
    return bf.run_describe(c, d_depth, B);
}

}  // namespace rgbd

using namespace rgbd;

extern "C" {

rgbd_status rgbd_adaptive_get_thresholds(rgbd_ctx* c, double* thresh)
{
    if (!c || !thresh) return RGBD_ERR_ARG;
    if (!ws(c)) return not_adaptive(c);
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (!s) s = check_hip(c, hipMemcpyAsync(thresh, ws(c)->d_state, (size_t)ws(c)->cfg.ncells * 8, hipMemcpyDeviceToHost, c->stream),
                          "read thresholds");
    return s ? s : check_hip(c, hipStreamSynchronize(c->stream), "sync");
}

rgbd_status rgbd_adaptive_set_thresholds(rgbd_ctx* c, const double* thresh)
{
    if (!c || !thresh) return RGBD_ERR_ARG;
    if (!ws(c)) return not_adaptive(c);
    const AdpCfg& g = ws(c)->cfg;
    for (int k = 0; k < g.ncells; k++)
        if (!(thresh[k] >= g.min_thresh && thresh[k] <= g.max_thresh))
            return fail(c, RGBD_ERR_ARG, "adaptive: thresholds must lie in [min_thresh, max_thresh]");
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (!s) s = check_hip(c, hipMemcpyAsync(ws(c)->d_state, thresh, (size_t)g.ncells * 8, hipMemcpyHostToDevice, c->stream),
                          "write thresholds");
    return s ? s : check_hip(c, hipStreamSynchronize(c->stream), "sync");   // the caller's array may go away
}

rgbd_status rgbd_adaptive_rewind(rgbd_ctx* c, int32_t k)
{
    if (!c) return RGBD_ERR_ARG;
    if (!ws(c)) return not_adaptive(c);
    if (k < 1 || k > c->last_B) return fail(c, RGBD_ERR_ARG, "adaptive: rewind by 1 .. the last batch's frames");
    AdpWS* w = ws(c);
    const size_t nc = (size_t)w->cfg.ncells;
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_state, w->d_before + (size_t)(c->last_B - k) * nc, nc * 8, hipMemcpyDeviceToDevice,
                                            c->stream), "rewind thresholds");
    return s;
}

rgbd_status rgbd_adaptive_debug_cell(rgbd_ctx* c, int32_t b, int32_t cell, uint64_t* thresh_before_bits, int32_t* thresh_used,
                                     int32_t* tries, int32_t* xys, int32_t cap, int32_t* n)
{
    if (!c || !ws(c) || b < 0 || b >= c->last_B) return RGBD_ERR_ARG;
    AdpWS* w = ws(c);
    const AdpCfg& g = w->cfg;
    if (cell < 0 || cell >= g.ncells || cap < 0) return RGBD_ERR_ARG;
    const size_t ci = (size_t)b * g.ncells + cell;
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    double before = 0;
    int used = 0, ntry = 0, ns = 0;
    s = check_hip(c, hipMemcpyAsync(&before, w->d_before + ci, 8, hipMemcpyDeviceToHost, c->stream), "read before");
    if (!s) s = check_hip(c, hipMemcpyAsync(&used, w->d_used + ci, 4, hipMemcpyDeviceToHost, c->stream), "read used");
    if (!s) s = check_hip(c, hipMemcpyAsync(&ntry, w->d_tries + ci, 4, hipMemcpyDeviceToHost, c->stream), "read tries");
    if (!s) s = check_hip(c, hipMemcpyAsync(&ns, w->d_nlist + ci, 4, hipMemcpyDeviceToHost, c->stream), "read list count");
    if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
    if (s) return s;
    if (thresh_before_bits) std::memcpy(thresh_before_bits, &before, 8);
    if (thresh_used) *thresh_used = used;
    if (tries) *tries = ntry;
    std::vector<uint32_t> v((size_t)std::max(ns, 1));
    if (ns) {
        s = check_hip(c, hipMemcpyAsync(v.data(), w->d_list + ci * g.cell_cap, (size_t)ns * 4, hipMemcpyDeviceToHost, c->stream),
                      "read cell list");
        if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
        if (s) return s;
    }
    int k = 0;
    for (int i = 0; i < ns; i++) {
        if (adp_s(v[i]) < used) continue;
        if (xys && k < cap) {
            xys[3 * k] = adp_x(v[i]);
            xys[3 * k + 1] = adp_y(v[i]);
            xys[3 * k + 2] = adp_s(v[i]);
        }
        k++;
    }
    if (n) *n = k;
    return xys && k > cap ? fail(c, RGBD_ERR_CAPACITY, "output capacity smaller than the cell's corner count") : RGBD_OK;
}

rgbd_status rgbd_adaptive_keep_strongest(rgbd_ctx* c, const float* resp, int32_t n, int32_t N, int32_t depth_limit,
                                         int32_t* order)
{
    if (!c || !order || n < 0 || N < 0 || (n > 0 && !resp)) return RGBD_ERR_ARG;
    if (!ws(c)) return not_adaptive(c);
    if (n > kAdpSelMax) return fail(c, RGBD_ERR_UNSUPPORTED, "keepStrongest: n <= 12288");
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    AdpWS* w = ws(c);
    if (!w->d_kt_order) {   // the one allocated last
        s = check_hip(c, w->d_kt_resp.alloc((size_t)kAdpSelMax), "keep resp");
        if (!s) s = check_hip(c, w->d_kt_order.alloc((size_t)kAdpSelMax), "keep order");
        if (s) return s;
    }
    const int keep = std::min(n, N);
    if (keep == 0) return RGBD_OK;
    s = check_hip(c, hipMemcpyAsync(w->d_kt_resp, resp, (size_t)n * 4, hipMemcpyHostToDevice, c->stream), "keep up");
    if (s) return s;
    RGBD_TRY(c, launch_adp_keep_test(w->d_kt_resp, n, N, depth_limit, w->d_kt_order, c->stream), "adp_keep_test");
    s = check_hip(c, hipMemcpyAsync(order, w->d_kt_order, (size_t)keep * 4, hipMemcpyDeviceToHost, c->stream), "keep order");
    return s ? s : check_hip(c, hipStreamSynchronize(c->stream), "sync");
}

}  // extern "C"
