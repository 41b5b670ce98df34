// api.cpp -- C ABI (include/rgbd_hip.h): context, extraction and matching entry points.  The geometry a context
// uploads once at creation is derived by geometry.cpp.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include <algorithm>
#include <string>
#include <vector>

#include "brief_front.h"
#include "geometry.h"
#include "launch.h"

using namespace rgbd;

namespace rgbd {

rgbd_status fail(rgbd_ctx* c, rgbd_status code, const std::string& msg)
{
    if (c) c->err = msg;
    return code;
}

rgbd_status check_hip(rgbd_ctx* c, hipError_t e, const char* what)
{
    if (e == hipSuccess) return RGBD_OK;
    return fail(c, RGBD_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

rgbd_status order_after_extraction(rgbd_ctx* c)
{
    if (!c->extract_done || c->extract_stream == c->stream) return RGBD_OK;
    const rgbd_status s = check_hip(c, hipStreamWaitEvent(c->stream, c->extract_done, 0), "wait for extraction");
    if (!s) c->extract_stream = c->stream;   // ordered: later calls on this stream need no second wait
    return s;
}

static hipEvent_t ev_get(rgbd_ctx* c)
{
    if (!c->event_pool.empty()) {
        hipEvent_t e = c->event_pool.back();
        c->event_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}

int timer_begin(rgbd_ctx* c, const char* name, hipStream_t st)
{
    if (!c->timing) return -1;
    if (!c->timing_only.empty() && c->timing_only != name) return -1;
    int idx = -1;
    for (size_t i = 0; i < c->tentries.size(); i++)
        if (c->tentries[i].name == name) idx = (int)i;
    if (idx < 0) {
        c->tentries.push_back(rgbd_ctx::TEntry{name, 0.0, 0});
        idx = (int)c->tentries.size() - 1;
    }
    rgbd_ctx::Pending p{idx, ev_get(c), ev_get(c), st ? st : c->stream, false};
    (void)hipEventRecord(p.a, p.st);
    c->pending.push_back(p);
    return (int)c->pending.size() - 1;
}

void timer_end(rgbd_ctx* c, int tok)
{
    if (tok < 0) return;
    (void)hipEventRecord(c->pending[tok].b, c->pending[tok].st);
    c->pending[tok].ended = true;
}

void timer_flush(rgbd_ctx* c)
{
    for (auto& p : c->pending) {
        // a launch whose entry point returned early (RGBD_TRY) never recorded its end: not a timed launch
        float ms = 0;
        if (p.ended && hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            c->tentries[p.idx].ms += ms;
            c->tentries[p.idx].launches++;
        }
        c->event_pool.push_back(p.a);
        c->event_pool.push_back(p.b);
    }
    c->pending.clear();
}

rgbd_status run_orb_pyramid(rgbd_ctx* c, const uint8_t* d_bgr, int B, bool from_gray)
{
    const ExtractCfg& C = c->cfg;
    const hipStream_t st = c->stream;
    int tk;
    if (C.nlevels > 1) {   // k_pyramid converts BGR -> gray (level 0) itself unless given a gray level 0
        tk = timer_begin(c, "k_pyramid");
        RGBD_TRY(c, launch_pyramid(c->d_pyr, from_gray ? nullptr : d_bgr, c->d_rsy, c->d_qx, c->d_cfg, C.pyr_lds + C.pyr_rsy_lds, B, st), "pyramid");
        timer_end(c, tk);
        if (C.pyr_top < C.nlevels) {   // the small levels after the strips
            tk = timer_begin(c, "k_pyr_tail");
            RGBD_TRY(c, launch_pyr_tail(c->d_pyr, c->d_rsy, c->d_qx, c->d_cfg, B, st), "pyramid tail");
            timer_end(c, tk);
        }
    } else if (!from_gray) {
        tk = timer_begin(c, "k_gray");
        RGBD_TRY(c, launch_gray(d_bgr, c->d_pyr, C.W, C.H, C.frame_pyr_bytes, B, st), "gray");
        timer_end(c, tk);
    }
    return RGBD_OK;
}

}  // namespace rgbd

namespace {

// a later call that reads the extraction's outputs on another stream waits on this event
// (order_after_extraction: rgbd_set_stream, and rgbd_track_lanes on the extracted frames)
static rgbd_status mark_extracted(rgbd_ctx* c)
{
    rgbd_status s = check_hip(c, c->extract_done.ensure(), "extract event");
    if (s) return s;
    if ((s = check_hip(c, hipEventRecord(c->extract_done, c->stream), "extract event record"))) return s;
    c->extract_stream = c->stream;
    return RGBD_OK;
}

rgbd_status run_extract(rgbd_ctx* c, const uint8_t* d_bgr, const uint16_t* d_depth, int B, bool from_gray,
                        const rgbd::ExtractHook* after_fast = nullptr)
{
    // per-frame capacity flags (k_distribute and the front ends' kernels: extract_flag_message), cleared for every extraction
    rgbd_status s0 = check_hip(c, hipMemsetAsync(c->d_err, 0, sizeof(int) * (size_t)B, c->stream), "clear err");
    if (s0) return s0;
    if (c->front) {
        if ((s0 = c->front->run(c, d_bgr, d_depth, B, from_gray, after_fast))) return s0;
        return mark_extracted(c);
    }
    ExtractCfg& C = c->cfg;
    hipStream_t st = c->stream;
    rgbd_status hs = run_orb_pyramid(c, d_bgr, B, from_gray);
    if (hs) return hs;
    if ((hs = call_hook(after_fast, 0))) return hs;
    // every level is blurred by each frame's leading blocks of the k_fast grid (blur_tile_walk's tile waves,
    // then blur_thread for the levels below the tile path's floor and for 1-level pyramids), so blur and FAST
    // waves share the CUs inside one launch
    int tk = timer_begin(c, "k_fast");
#ifdef RGBD_PNP_PROFILE
    // profiling build: RGBD_PROF_FAST_SPLIT=1 dispatches the grid's blur blocks and its FAST segments as two
    // k_fast launches (blur-only grid first), so per-dispatch counters give the blur's share of the launch
    if (getenv("RGBD_PROF_FAST_SPLIT")) {
        RGBD_TRY(c, launch_fast(c->d_pyr, c->d_cells, c->d_segs, 0, c->d_cfg, c->d_cellc, c->d_slots, B, st, c->d_blur,
                    C.blur_t0[kMaxLevels] + C.blur_e0[kMaxLevels], c->d_blur_tab, C.blur_m0[kMaxLevels]), "fast (blur blocks)");
        RGBD_TRY(c, launch_fast(c->d_pyr, c->d_cells, c->d_segs, c->n_segs, c->d_cfg, c->d_cellc, c->d_slots, B, st,
                    c->d_blur, 0), "fast (segments)");
    } else
#endif
    RGBD_TRY(c, launch_fast(c->d_pyr, c->d_cells, c->d_segs, c->n_segs, c->d_cfg, c->d_cellc, c->d_slots, B, st, c->d_blur,
                C.blur_t0[kMaxLevels] + C.blur_e0[kMaxLevels], c->d_blur_tab, C.blur_m0[kMaxLevels]), "fast");
    timer_end(c, tk);
    // e.g. the deferred PnPRansac solves of earlier pipelined steps (pnp_host.cpp)
    if ((hs = call_hook(after_fast, 1))) return hs;
    tk = timer_begin(c, "k_distribute");
    RGBD_TRY(c, launch_distribute(c->d_cellc, c->d_slots, c->d_cfg, C.node_cap, C.scan_cap, 0, C.nlevels, C.dist_kc, c->d_keys,
                      c->d_node, c->d_selc, c->d_sel, c->d_err, c->d_dist_path, B, st), "distribute");
    timer_end(c, tk);
    if ((hs = call_hook(after_fast, 2))) return hs;
#ifdef RGBD_PNP_PROFILE
    pyr_prof_dump(st);
    fprintf(stderr, "[pyr_lds] %d bytes per workgroup (odd levels at %d)\n", C.pyr_lds, C.pyr_lds_b);
    fast_prof_dump(st, c->n_segs);
    dist_prof_dump(st);
#endif
    tk = timer_begin(c, "k_describe");
    RGBD_TRY(c, launch_describe(c->d_pyr, c->d_blur, c->d_selc, sel_count_elems(c->maxB, C.nlevels), C.nlevels, c->d_sel, c->d_cfg,
                                C.kp_cap, c->out.count, c->out.kps, c->out.desc, B, st), "describe");
    timer_end(c, tk);
    tk = timer_begin(c, "k_undistort");
    RGBD_TRY(c, launch_undistort(d_depth, c->out.count, c->d_cfg, C.kp_cap, c->out.kps, c->out.kun, c->out.xyz, B, st), "undistort");
    timer_end(c, tk);
    c->last_B = B;
#ifdef RGBD_PNP_PROFILE
    desc_prof_dump(st);
#endif
    return mark_extracted(c);
}

rgbd_status read_frame(rgbd_ctx* c, int b, rgbd_keypoint* kps, rgbd_keypoint* kun, uint8_t* desc, float* xyz,
                       int cap, int* n)
{
    const int K = c->cfg.kp_cap;
    int cnt = 0;
    rgbd_status s = check_hip(c, hipMemcpyAsync(&cnt, c->out.count + b, sizeof(int), hipMemcpyDeviceToHost, c->stream),
                              "read count");
    if (s) return s;
    int errflag = 0;
    if ((s = check_hip(c, hipMemcpyAsync(&errflag, c->d_err + b, sizeof(int), hipMemcpyDeviceToHost, c->stream), "read err")))
        return s;
    if ((s = check_hip(c, hipStreamSynchronize(c->stream), "sync"))) return s;
    if (errflag) return fail(c, RGBD_ERR_CAPACITY, extract_flag_message(errflag));
    if (n) *n = cnt;
    if (cnt > cap) return fail(c, RGBD_ERR_CAPACITY, "output capacity smaller than keypoint count");
    if (cnt == 0) return RGBD_OK;
    const size_t o = (size_t)b * K;
    if (kps && (s = check_hip(c, hipMemcpyAsync(kps, c->out.kps + o * 7, (size_t)cnt * 28, hipMemcpyDeviceToHost, c->stream), "read kps"))) return s;
    if (kun && (s = check_hip(c, hipMemcpyAsync(kun, c->out.kun + o * 7, (size_t)cnt * 28, hipMemcpyDeviceToHost, c->stream), "read kun"))) return s;
    if (desc && (s = check_hip(c, hipMemcpyAsync(desc, c->out.desc + o * 32, (size_t)cnt * 32, hipMemcpyDeviceToHost, c->stream), "read desc"))) return s;
    if (xyz && (s = check_hip(c, hipMemcpyAsync(xyz, c->out.xyz + o * 3, (size_t)cnt * 12, hipMemcpyDeviceToHost, c->stream), "read xyz"))) return s;
    return check_hip(c, hipStreamSynchronize(c->stream), "sync");
}

// one host table on the device: its buffer (of T, or of bytes), then the upload unless the table is empty
template <typename D, typename T>
rgbd_status upload_table(rgbd_ctx* c, DevBuf<D>& d, const std::vector<T>& v, const char* what, const char* what_upload)
{
    static_assert(sizeof(T) % sizeof(D) == 0, "a table element is whole buffer elements");
    rgbd_status s = check_hip(c, d.alloc(v.size() * (sizeof(T) / sizeof(D))), what);
    if (!s && !v.empty()) s = check_hip(c, hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice), what_upload);
    return s;
}

rgbd_status create_ctx(int device, int width, int height, int max_batch, const rgbd_orb_params* orb,
                       const rgbd_svo_params* svo, const rgbd_adaptive_params* adp, const rgbd_gftt_params* gftt,
                       const rgbd_cvorb_params* cvorb, const rgbd_fast_params* fast, const rgbd_camera* cam, rgbd_ctx** out)
{
    if (!out || !orb || !cam || max_batch < 1) return RGBD_ERR_ARG;
    rgbd_ctx* c = new rgbd_ctx();
    *out = c;   // also when the creation fails: the caller reads rgbd_last_error, then destroys it
    c->device = device;
    c->W = width;
    c->H = height;
    c->maxB = max_batch;
    c->cam = *cam;
    Geometry g;   // the host tables: gone after the upload
    rgbd_status s = build_geometry(width, height, *orb, *cam, g, c->err);
    c->cfg = g.cfg;
    c->n_segs = (int)g.segs.size();
    // the adaptive extractor's own refusals first (they name the parameter), then the ORB geometry's
    if (adp) {
        const rgbd_status sa = adaptive_configure(c, *adp);   // sets cfg.kp_cap before the allocations
        if (sa) return sa;
    }
    if (gftt) {
        const rgbd_status sg = gftt_configure(c, *gftt);   // likewise
        if (sg) return sg;
    }
    if (cvorb) {
        const rgbd_status sc = cvorb_check_params(c, *cvorb);
        if (sc) return sc;
    }
    if (fast) {
        const rgbd_status sf = fast_configure(c, *fast);   // as the adaptive extractor's
        if (sf) return sf;
    }
    if (s) return s;
    if (svo && (s = svo_configure(c, *svo))) return s;   // sets cfg.kp_cap before the allocations
    if (cvorb && (s = cvorb_configure(c, *cvorb))) return s;   // likewise, from the accepted geometry
    if ((s = check_hip(c, hipSetDevice(device), "hipSetDevice"))) return s;
    if ((s = check_hip(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking), "stream"))) return s;
    c->stream = c->own_stream;
    {
        const char* ser = std::getenv("RGBD_SERIAL");
        c->serial = ser && std::atoi(ser) != 0;
    }
    const ExtractCfg& C = c->cfg;
    const size_t B = (size_t)max_batch;
    // k_describe addresses the pyramids with 32-bit byte offsets from the buffer base
    if (B * C.frame_pyr_bytes + 64 > 0xFFFFFFFFull)
        return fail(c, RGBD_ERR_CAPACITY, "max_batch x pyramid bytes exceeds 4 GiB (use more contexts)");
    // k_fast addresses the FAST cell lists with 32-bit byte offsets too
    if (B * C.n_cells * C.cell_cap * 4 > 0xFFFFFFFFull)
        return fail(c, RGBD_ERR_CAPACITY, "max_batch x FAST cell lists exceed 4 GiB (use more contexts)");
    s = check_hip(c, c->d_cfg.alloc(1), "cfg");
    if (!s) s = check_hip(c, hipMemcpy(c->d_cfg, &c->cfg, sizeof(ExtractCfg), hipMemcpyHostToDevice), "upload cfg");
    if (!s) s = upload_table(c, c->d_cells, g.cells, "cells", "upload cells");
    if (!s) s = upload_table(c, c->d_segs, g.segs, "fast segments", "upload segments");
    if (!s) s = upload_table(c, c->d_rsx, g.rsx, "rsx", "upload rsx");
    if (!s) s = upload_table(c, c->d_qx, g.qx, "resize quads", "upload quads");
    if (!s) s = upload_table(c, c->d_rsy, g.rsy, "rsy", "upload rsy");
    if (!s) s = upload_table(c, c->d_blur_tab, g.blur_tab, "blur tables", "upload blur tables");
    if (!s) s = check_hip(c, c->d_pyr.alloc(B * C.frame_pyr_bytes + 64), "pyramid");
    if (!s) s = check_hip(c, c->d_blur.alloc(B * C.frame_pyr_bytes + 64), "blurred pyramid");
    if (!s) s = check_hip(c, c->d_cellc.alloc(B * C.n_cells), "cell counts");
    if (!s) s = check_hip(c, c->d_slots.alloc(B * C.n_cells * C.cell_cap), "cell slots");
    if (!s) s = check_hip(c, c->d_keys.alloc(B * C.keys_per_frame), "keys");
    if (!s) s = check_hip(c, c->d_node.alloc(B * C.keys_per_frame), "node ids");
    // + kMaxLevels of slack: k_describe reads kMaxLevels counts from any frame's row unconditionally
    if (!s) s = check_hip(c, c->d_selc.alloc(sel_count_elems((int)B, C.nlevels)), "sel counts");
    if (!s) s = check_hip(c, c->d_sel.alloc(B * C.sel_per_frame), "sel");
    if (!s) s = check_hip(c, c->d_dist_path.alloc(B * C.nlevels), "quadtree paths");
    if (!s) s = check_hip(c, c->own_out.count.alloc(B), "counts");
    if (!s) s = check_hip(c, c->own_out.kps.alloc(B * C.kp_cap * 7), "kps");
    if (!s) s = check_hip(c, c->own_out.kun.alloc(B * C.kp_cap * 7), "kps_un");
    if (!s) s = check_hip(c, c->own_out.desc.alloc(B * C.kp_cap * 32), "desc");
    if (!s) s = check_hip(c, c->own_out.xyz.alloc(B * C.kp_cap * 3), "xyz");
    if (!s) s = check_hip(c, c->d_err.alloc(B), "err");   // one flag per frame
    if (!s) s = check_hip(c, c->d_in_bgr.alloc((size_t)width * height * 3), "bgr staging");
    if (!s) s = check_hip(c, c->d_in_depth.alloc((size_t)width * height), "depth staging");
    if (!s) s = check_hip(c, c->own_out.knn.alloc(B * C.kp_cap), "knn");
    if (!s) s = check_hip(c, c->d_pairs.alloc(2 * B), "pairs");
    if (s) return s;
    c->out = c->own_out.view();
    s = check_hip(c, hipMemset(c->d_err, 0, sizeof(int) * B), "memset err");
    if (!s) s = check_hip(c, hipMemset(c->d_pyr, 0, B * C.frame_pyr_bytes + 64), "memset pyr");
    if (!s) s = check_hip(c, hipMemset(c->d_blur, 0, B * C.frame_pyr_bytes + 64), "memset blur");
    if (!s && c->front) s = c->front->alloc(c);
    return s;
}

}  // namespace

extern "C" {

rgbd_status rgbd_create(int device, int width, int height, int max_batch, const rgbd_orb_params* orb,
                        const rgbd_camera* cam, rgbd_ctx** out)
{
    return create_ctx(device, width, height, max_batch, orb, nullptr, nullptr, nullptr, nullptr, nullptr, cam, out);
}

rgbd_status rgbd_create_svo(int device, int width, int height, int max_batch, const rgbd_svo_params* svo,
                            const rgbd_camera* cam, rgbd_ctx** out)
{
    if (!svo) return RGBD_ERR_ARG;
    // Extractor::Extractor -> setParameters(1000, 1.2f, 8, 20, 7) (Features/Extractor.cpp:15-22): the ORB
    // fields only shape the scale tables the reference's getters report (the ORB workspace is never run,
    // so its budget is kept small)
    const rgbd_orb_params orb{std::max(1, std::min(svo->nfeatures, 1000)), 1.2f, 8, 20, 7};
    return create_ctx(device, width, height, max_batch, &orb, svo, nullptr, nullptr, nullptr, nullptr, cam, out);
}

rgbd_status rgbd_create_adaptive(int device, int width, int height, int max_batch, const rgbd_adaptive_params* params,
                                 const rgbd_camera* cam, rgbd_ctx** out)
{
    if (!params) return RGBD_ERR_ARG;
    // the ORB workspace is never run: a one-level ORB geometry (every adaptive keypoint has octave 0), so of the
    // ORB shape refusals only level 0's remain (the 8-level geometry refuses e.g. 320 x 256 for its level 7)
    const rgbd_orb_params orb{std::max(1, std::min(params->nfeatures, 1000)), 1.2f, 1, 20, 7};
    return create_ctx(device, width, height, max_batch, &orb, nullptr, params, nullptr, nullptr, nullptr, cam, out);
}

rgbd_status rgbd_create_gftt(int device, int width, int height, int max_batch, const rgbd_gftt_params* params,
                             const rgbd_camera* cam, rgbd_ctx** out)
{
    if (!params) return RGBD_ERR_ARG;
    // as for rgbd_create_adaptive: a one-level ORB geometry that is never run (every GFTT keypoint has octave 0)
    const rgbd_orb_params orb{std::max(1, std::min(params->nfeatures, 1000)), 1.2f, 1, 20, 7};
    return create_ctx(device, width, height, max_batch, &orb, nullptr, nullptr, params, nullptr, nullptr, cam, out);
}

rgbd_status rgbd_create_cvorb(int device, int width, int height, int max_batch, const rgbd_cvorb_params* params,
                              const rgbd_camera* cam, rgbd_ctx** out)
{
    if (!params) return RGBD_ERR_ARG;
    // the ORB geometry of the caller's pyramid: its k_pyramid and blur run; its FAST cells and quadtree never do, so
    // their budget is kept small (as for rgbd_create_svo)
    const rgbd_orb_params orb{std::max(1, std::min(params->nfeatures, 1000)), params->scale_factor, params->nlevels, 20, 7};
    return create_ctx(device, width, height, max_batch, &orb, nullptr, nullptr, nullptr, params, nullptr, cam, out);
}

rgbd_status rgbd_create_fast(int device, int width, int height, int max_batch, const rgbd_fast_params* params,
                             const rgbd_camera* cam, rgbd_ctx** out)
{
    if (!params) return RGBD_ERR_ARG;
    // as for rgbd_create_adaptive: a one-level ORB geometry (every FAST keypoint has octave 0); the ORB descriptor runs its
    // gray level and blur, the BRIEF descriptor nothing of it
    const rgbd_orb_params orb{std::max(1, std::min(params->nfeatures, 1000)), 1.2f, 1, 20, 7};
    return create_ctx(device, width, height, max_batch, &orb, nullptr, nullptr, nullptr, nullptr, params, cam, out);
}

void rgbd_destroy(rgbd_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    if (c->solve_stream) (void)hipStreamSynchronize(c->solve_stream);
    if (c->match_stream) (void)hipStreamSynchronize(c->match_stream);
    rgbd::pnp_free(c);
    rgbd::ransac_free(c);
    rgbd::gicp_free(c);
    rgbd::cloud_free(c);
    rgbd::proj_free(c);
    rgbd::pnpba_free(c);
    rgbd::umeyama_free(c);
    rgbd::bow_free(c);
    c->front.reset();
    for (auto& p : c->pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto e : c->event_pool) (void)hipEventDestroy(e);
    const hipStream_t own = c->own_stream, solve = c->solve_stream, match = c->match_stream;
    delete c;   // the context's buffers and its extraction event go here, before the streams
    for (hipStream_t st : {solve, match})   // serial: aliases of own_stream
        if (st && st != own) (void)hipStreamDestroy(st);
    if (own) (void)hipStreamDestroy(own);
}

const char* rgbd_last_error(const rgbd_ctx* c) { return c ? c->err.c_str() : "null context"; }

int32_t rgbd_max_keypoints(const rgbd_ctx* c) { return c ? c->cfg.kp_cap : 0; }

rgbd_status rgbd_debug_fast_rank16(rgbd_ctx* c, const uint8_t* flags, int32_t rows, uint32_t* slots, uint32_t* counts)
{
    if (!c || rows < 1 || rows > 4096 || !flags || !slots || !counts) return RGBD_ERR_ARG;
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    DevBuf<uint8_t> d_f;
    DevBuf<uint32_t> d_s;
    const size_t n = (size_t)rows * 64;
    s = check_hip(c, d_f.alloc(n), "rank flags");
    if (!s) s = check_hip(c, d_s.alloc(n + 64), "rank slots");
    if (!s) s = check_hip(c, hipMemcpyAsync(d_f, flags, n, hipMemcpyHostToDevice, c->stream), "rank in");
    if (!s) {
        s = check_hip(c, rgbd::launch_debug_rank16(d_f, rows, d_s, d_s + n, c->stream), "launch of k_debug_rank16");
    }
    if (!s) s = check_hip(c, hipMemcpyAsync(slots, d_s, n * 4, hipMemcpyDeviceToHost, c->stream), "rank out");
    if (!s) s = check_hip(c, hipMemcpyAsync(counts, d_s + n, 64 * 4, hipMemcpyDeviceToHost, c->stream), "rank counts");
    if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "rank sync");
    return s;
}

rgbd_status rgbd_set_stream(rgbd_ctx* c, void* stream)
{
    if (!c) return RGBD_ERR_ARG;
    const hipStream_t prev = c->stream;
    c->stream = stream ? (hipStream_t)stream : c->own_stream;
    // every consumer of the last extraction's outputs (rgbd_track_lanes / rgbd_batch_frame / the debug
    // readers, or the caller's own kernels on this stream) is then ordered behind it; if that wait cannot be
    // queued the context keeps its previous stream, so the call can be retried
    const rgbd_status s = order_after_extraction(c);
    if (s) c->stream = prev;
    return s;
}

rgbd_status rgbd_detect_and_compute(rgbd_ctx* c, const uint8_t* gray, int32_t step, rgbd_keypoint* kps,
                                    uint8_t* desc, int32_t cap, int32_t* n)
{
    if (!c) return RGBD_ERR_ARG;
    if (n) *n = 0;
    if (!gray) return RGBD_OK;   // empty image -> no output (:708-709)
    if (step < c->W) return fail(c, RGBD_ERR_ARG, "step < width");
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    // level 0 of frame 0: of the front end's BRIEF pyramid (tight rows) where it has one, else of the ORB pyramid
    BriefFront* bf = c->front ? c->front->brief() : nullptr;
    s = check_hip(c, hipMemcpy2DAsync(bf ? bf->d_pyr : c->d_pyr, bf ? c->W : c->cfg.lv[0].stride, gray, step, c->W, c->H,
                                      hipMemcpyHostToDevice, c->stream), "upload gray");
    if (s) return s;
    if ((s = run_extract(c, nullptr, nullptr, 1, true))) return s;
    return read_frame(c, 0, kps, nullptr, desc, nullptr, cap, n);
}

rgbd_status rgbd_frame(rgbd_ctx* c, const uint8_t* bgr, const uint16_t* depth, rgbd_keypoint* kps,
                       rgbd_keypoint* kun, uint8_t* desc, float* xyz, int32_t cap, int32_t* n)
{
    if (!c || !bgr || !depth) return RGBD_ERR_ARG;
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    const size_t px = (size_t)c->W * c->H;
    if ((s = check_hip(c, hipMemcpyAsync(c->d_in_bgr, bgr, px * 3, hipMemcpyHostToDevice, c->stream), "upload bgr"))) return s;
    if ((s = check_hip(c, hipMemcpyAsync(c->d_in_depth, depth, px * 2, hipMemcpyHostToDevice, c->stream), "upload depth"))) return s;
    if ((s = run_extract(c, c->d_in_bgr, c->d_in_depth, 1, false))) return s;
    return read_frame(c, 0, kps, kun, desc, xyz, cap, n);
}

rgbd_status rgbd_extract_batch(rgbd_ctx* c, const void* d_bgr, const void* d_depth, int32_t B)
{
    if (!c || !d_bgr || B < 1) return RGBD_ERR_ARG;
    if (B > c->maxB) return fail(c, RGBD_ERR_CAPACITY, "batch larger than max_batch");
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    return run_extract(c, (const uint8_t*)d_bgr, (const uint16_t*)d_depth, B, false);
}

rgbd_status rgbd_batch_frame(rgbd_ctx* c, int32_t b, rgbd_keypoint* kps, rgbd_keypoint* kun, uint8_t* desc,
                             float* xyz, int32_t cap, int32_t* n)
{
    if (!c || b < 0 || b >= c->last_B) return RGBD_ERR_ARG;
    return read_frame(c, b, kps, kun, desc, xyz, cap, n);
}

rgbd_status rgbd_batch_outputs(rgbd_ctx* c, void** counts, void** kps, void** kun, void** desc, void** xyz)
{
    if (!c) return RGBD_ERR_ARG;
    if (counts) *counts = c->out.count;
    if (kps) *kps = c->out.kps;
    if (kun) *kun = c->out.kun;
    if (desc) *desc = c->out.desc;
    if (xyz) *xyz = c->out.xyz;
    return RGBD_OK;
}

// one level of frame b of the pyramid or the blurred pyramid, rows packed to the level's width
static rgbd_status read_level(rgbd_ctx* c, DevBuf<uint8_t> rgbd_ctx::*pyr, int32_t b, int32_t level, uint8_t* out, const char* what)
{
    if (!c || !out || b < 0 || b >= c->maxB || level < 0 || level >= c->cfg.nlevels) return RGBD_ERR_ARG;
    const LevelCfg& L = c->cfg.lv[level];
    rgbd_status s = check_hip(c, hipMemcpy2DAsync(out, L.w, c->*pyr + (size_t)b * c->cfg.frame_pyr_bytes + L.off, L.stride,
                                                  L.w, L.h, hipMemcpyDeviceToHost, c->stream), what);
    if (s) return s;
    return check_hip(c, hipStreamSynchronize(c->stream), "sync");
}

rgbd_status rgbd_debug_level(rgbd_ctx* c, int32_t b, int32_t level, uint8_t* out)
{
    return read_level(c, &rgbd_ctx::d_pyr, b, level, out, "read level");
}

rgbd_status rgbd_debug_blurred(rgbd_ctx* c, int32_t b, int32_t level, uint8_t* out)
{
    return read_level(c, &rgbd_ctx::d_blur, b, level, out, "read blurred level");
}

// packed key v as entry k of an (x, y, score) list of cap entries; a null list or an entry past cap is only counted
static void put_xys(int32_t* xys, int cap, int k, uint32_t v)
{
    if (!xys || k >= cap) return;
    xys[3 * k] = key_x(v);
    xys[3 * k + 1] = key_y(v);
    xys[3 * k + 2] = key_s(v);
}

rgbd_status rgbd_debug_candidates(rgbd_ctx* c, int32_t b, int32_t level, int32_t* xys, int32_t cap, int32_t* n)
{
    if (!c || b < 0 || b >= c->maxB || level < 0 || level >= c->cfg.nlevels) return RGBD_ERR_ARG;
    const ExtractCfg& C = c->cfg;
    const LevelCfg& L = C.lv[level];
    std::vector<int> cnt(L.cell_count);
    std::vector<uint32_t> slots((size_t)L.cell_count * C.cell_cap);
    rgbd_status s = check_hip(c, hipMemcpyAsync(cnt.data(), c->d_cellc + (size_t)b * C.n_cells + L.cell_begin,
                                                cnt.size() * 4, hipMemcpyDeviceToHost, c->stream), "read cell counts");
    if (s) return s;
    s = check_hip(c, hipMemcpyAsync(slots.data(), c->d_slots + ((size_t)b * C.n_cells + L.cell_begin) * C.cell_cap,
                                    slots.size() * 4, hipMemcpyDeviceToHost, c->stream), "read cell slots");
    if (s) return s;
    if ((s = check_hip(c, hipStreamSynchronize(c->stream), "sync"))) return s;
    int k = 0;
    for (int i = 0; i < L.cell_count; i++)
        for (int j = 0; j < cnt[i]; j++) put_xys(xys, cap, k++, slots[(size_t)i * C.cell_cap + j]);
    if (n) *n = k;
    return k > cap ? fail(c, RGBD_ERR_CAPACITY, "capacity") : RGBD_OK;
}

rgbd_status rgbd_debug_selected(rgbd_ctx* c, int32_t b, int32_t level, int32_t* xys, int32_t cap, int32_t* n)
{
    if (!c || b < 0 || b >= c->maxB || level < 0 || level >= c->cfg.nlevels) return RGBD_ERR_ARG;
    const ExtractCfg& C = c->cfg;
    const LevelCfg& L = C.lv[level];
    int cnt = 0;
    rgbd_status s = check_hip(c, hipMemcpyAsync(&cnt, c->d_selc + (size_t)b * C.nlevels + level, 4, hipMemcpyDeviceToHost,
                                                c->stream), "read sel count");
    if (s) return s;
    if ((s = check_hip(c, hipStreamSynchronize(c->stream), "sync"))) return s;
    std::vector<uint32_t> v(std::max(cnt, 1));
    s = check_hip(c, hipMemcpy(v.data(), c->d_sel + (size_t)b * C.sel_per_frame + L.sel_off, (size_t)cnt * 4,
                               hipMemcpyDeviceToHost), "read sel");
    if (s) return s;
    for (int i = 0; i < cnt; i++) put_xys(xys, cap, i, v[i]);
    if (n) *n = cnt;
    return cnt > cap ? fail(c, RGBD_ERR_CAPACITY, "capacity") : RGBD_OK;
}

rgbd_status rgbd_debug_dist_path(rgbd_ctx* c, int32_t b, int32_t level, int32_t* path)
{
    if (!c || !path || b < 0 || b >= c->maxB || level < 0 || level >= c->cfg.nlevels) return RGBD_ERR_ARG;
    rgbd_status s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
    if (s) return s;
    uint8_t v = 0;
    s = check_hip(c, hipMemcpy(&v, c->d_dist_path + (size_t)b * c->cfg.nlevels + level, 1, hipMemcpyDeviceToHost),
                  "read quadtree path");
    *path = v;
    return s;
}

// ------------------------------------------------------------------ matching
// staging for query and train sets of `need` rows; *cap: the rows of each half of d_mdesc and of d_mknn that
// both buffers hold, whichever of them a failed call left smaller
static rgbd_status ensure_mcap(rgbd_ctx* c, int need, int* cap)
{
    const size_t rows = (size_t)std::max(need, c->cfg.kp_cap);
    const bool pairs = !c->d_mcount;
    rgbd_status s = check_hip(c, c->d_mdesc.reserve(2 * rows * 32), "match desc");
    if (!s) s = check_hip(c, c->d_mcount.reserve(4), "match counts");
    if (!s) s = check_hip(c, c->d_mknn.reserve(rows), "match knn");
    if (!s && pairs) {
        int pr[2] = {0, 1};
        s = check_hip(c, hipMemcpy(c->d_mcount + 2, pr, 8, hipMemcpyHostToDevice), "pairs");
    }
    if (s && pairs) c->d_mcount.release();   // the pairs are written once, with the allocation
    *cap = (int)std::min(c->d_mdesc.capacity() / 64, c->d_mknn.capacity());
    return s;
}

rgbd_status rgbd_knn2(rgbd_ctx* c, const uint8_t* dq, int32_t nq, const uint8_t* dt, int32_t nt, int32_t* out)
{
    if (!c || nq < 0 || nt < 0 || (nq > 0 && (!dq || !out)) || (nt > 0 && !dt)) return RGBD_ERR_ARG;
    // k_knn2m's rank key holds the train index in its low 16 bits
    if (nt > kKnnMaxTrain) return fail(c, RGBD_ERR_UNSUPPORTED, "knn-2: more than 65536 train rows (16-bit train index in the rank key)");
    if (nq == 0) return RGBD_OK;
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    int cap = 0;
    if ((s = ensure_mcap(c, std::max(nq, nt), &cap))) return s;
    int counts[2] = {nq, nt};
    if ((s = check_hip(c, hipMemcpyAsync(c->d_mcount, counts, 8, hipMemcpyHostToDevice, c->stream), "counts"))) return s;
    if ((s = check_hip(c, hipMemcpyAsync(c->d_mdesc, dq, (size_t)nq * 32, hipMemcpyHostToDevice, c->stream), "dq"))) return s;
    if (nt > 0 && (s = check_hip(c, hipMemcpyAsync(c->d_mdesc + (size_t)cap * 32, dt, (size_t)nt * 32, hipMemcpyHostToDevice, c->stream), "dt")))
        return s;
    const int tk = timer_begin(c, "k_knn2");
    RGBD_TRY(c, launch_knn2(c->d_mdesc, c->d_mcount, c->d_mcount + 2, c->d_mcount + 3, cap, nq, c->d_mknn, 1, c->stream), "knn2");
    timer_end(c, tk);
    if ((s = check_hip(c, hipMemcpyAsync(out, c->d_mknn, (size_t)nq * 16, hipMemcpyDeviceToHost, c->stream), "knn out"))) return s;
    return check_hip(c, hipStreamSynchronize(c->stream), "sync");
}

}  // extern "C"

namespace rgbd {
// Matcher::match filter stage (Features/Matcher.cpp:115-136) over knn-2 rows, query order.
int match_filter(const int32_t* knn, int nq, const uint8_t* outlier_q, const float* z_q, const float* z_t,
                 float nnratio, int discard, rgbd_dmatch* out, int cap)
{
    std::vector<uint8_t> used;
    int m = 0;
    for (int i = 0; i < nq; i++) {
        const int i2b = knn[4 * i + 3];
        if (i2b < 0) continue;   // fewer than 2 train rows: reference UB (matchesKnn[i][1]); skip
        const float d1 = (float)knn[4 * i], d2 = (float)knn[4 * i + 2];
        if (d1 < nnratio * d2) {
            const int i2 = knn[4 * i + 1];
            if ((int)used.size() <= i2) used.resize(i2 + 1, 0);
            if (used[i2]) continue;
            if (discard && outlier_q && outlier_q[i]) continue;
            if (!(z_q[i] > 0) || !(z_t[i2] > 0)) continue;
            used[i2] = 1;
            if (m < cap) {
                out[m].queryIdx = i;
                out[m].trainIdx = i2;
                out[m].imgIdx = 0;
                out[m].distance = d1;
            }
            m++;
        }
    }
    return m;
}
}  // namespace rgbd

extern "C" {

rgbd_status rgbd_match(rgbd_ctx* c, const uint8_t* dq, int32_t nq, const uint8_t* dt, int32_t nt,
                       const uint8_t* outlier_q, const float* z_q, const float* z_t, float nnratio,
                       int32_t discard, rgbd_dmatch* out, int32_t cap, int32_t* m)
{
    if (!c || !m) return RGBD_ERR_ARG;
    *m = 0;
    if (nq <= 0 || nt <= 0) return RGBD_OK;   // knnMatch on an empty set returns no rows
    if (!z_q || !z_t) return fail(c, RGBD_ERR_ARG, "z arrays required");
    std::vector<int32_t> knn((size_t)nq * 4);
    rgbd_status s = rgbd_knn2(c, dq, nq, dt, nt, knn.data());
    if (s) return s;
    const int cnt = match_filter(knn.data(), nq, outlier_q, z_q, z_t, nnratio, discard, out, cap);
    *m = cnt;
    return cnt > cap ? fail(c, RGBD_ERR_CAPACITY, "match capacity") : RGBD_OK;
}

rgbd_status rgbd_set_timing(rgbd_ctx* c, int32_t enable)
{
    if (!c) return RGBD_ERR_ARG;
    c->timing = enable != 0;
    return RGBD_OK;
}

rgbd_status rgbd_set_timing_filter(rgbd_ctx* c, const char* kernel)
{
    if (!c) return RGBD_ERR_ARG;
    c->timing_only = kernel ? kernel : "";
    return RGBD_OK;
}

rgbd_status rgbd_reset_timing(rgbd_ctx* c)
{
    if (!c) return RGBD_ERR_ARG;
    timer_flush(c);
    c->tentries.clear();
    return RGBD_OK;
}

int32_t rgbd_timing_count(const rgbd_ctx* c) { return c ? (int32_t)c->tentries.size() : 0; }

rgbd_status rgbd_timing_entry(rgbd_ctx* c, int32_t idx, const char** name, double* total_ms, int64_t* launches)
{
    if (!c) return RGBD_ERR_ARG;
    timer_flush(c);
    if (idx < 0 || idx >= (int)c->tentries.size()) return RGBD_ERR_ARG;
    if (name) *name = c->tentries[idx].name.c_str();
    if (total_ms) *total_ms = c->tentries[idx].ms;
    if (launches) *launches = c->tentries[idx].launches;
    return RGBD_OK;
}

rgbd_status rgbd_synchronize(rgbd_ctx* c)
{
    if (!c) return RGBD_ERR_ARG;
    rgbd_status s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
    if (!s && c->match_stream) s = check_hip(c, hipStreamSynchronize(c->match_stream), "sync match stream");
    if (!s && c->solve_stream) s = check_hip(c, hipStreamSynchronize(c->solve_stream), "sync solve stream");
    return s;
}

}  // extern "C"

namespace rgbd {
rgbd_status extract_batch(rgbd_ctx* c, const void* d_bgr, const void* d_depth, int B, const ExtractHook* after_fast)
{
    if (!c || !d_bgr || B < 1) return RGBD_ERR_ARG;
    if (B > c->maxB) return fail(c, RGBD_ERR_CAPACITY, "batch larger than max_batch");
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    return run_extract(c, (const uint8_t*)d_bgr, (const uint16_t*)d_depth, B, false, after_fast);
}
}  // namespace rgbd
