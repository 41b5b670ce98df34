// project_host.cpp -- C ABI of the projection-guided matcher (project.hip): Matcher::projectionMatch
// (Features/Matcher.cpp:35-104) and Frame::computeImageBounds (Core/Frame.cpp:283-315).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "context.h"
#include "launch.h"

using namespace rgbd;

namespace rgbd {

struct ProjWS {
    int pairs = 0, qcap = 0, tcap = 0;   // what the per-pair arrays hold
    DevBuf<int> d_cell_off, d_status, d_head, d_res, d_count;
    DevBuf<float2> d_uv;
    DevBuf<float4> d_srec;
    DevBuf<uint32_t> d_win, d_keys, d_minq;
    DevBuf<uint4> d_sdesc;
    DevBuf<uint8_t> d_more, d_taken;
    DevBuf<rgbd_dmatch> d_out;
    // the frames a call reads: pair list, poses, outlier flags; host-buffer entry points stage two frames
    DevBuf<int> d_pairs, d_fcount;
    DevBuf<float> d_poses, d_kun, d_xyz;
    DevBuf<uint8_t> d_outlier, d_desc;
    // rgbd_debug_projection
    DevBuf<int> d_cand, d_ccount;
};

void proj_free(rgbd_ctx* c)
{
    delete c->proj;
    c->proj = nullptr;
}

}  // namespace rgbd

namespace {

rgbd_status ws_get(rgbd_ctx* c, int pairs, int qcap, int tcap, ProjWS** out)
{
    ProjWS* w = c->proj;
    if (!w) c->proj = w = new ProjWS();
    if (w->pairs < pairs || w->qcap < qcap || w->tcap < tcap) {
        const size_t P = (size_t)std::max(pairs, w->pairs), Q = (size_t)std::max(qcap, w->qcap), T = (size_t)std::max(tcap, w->tcap);
        w->pairs = 0;   // no capacity until every array is there
        rgbd_status s = check_hip(c, w->d_cell_off.alloc(P * (kProjCells + 1)), "projection cells");
        if (!s) s = check_hip(c, w->d_srec.alloc(P * T), "projection sorted keypoints");
        if (!s) s = check_hip(c, w->d_sdesc.alloc(P * T * 2), "projection sorted descriptors");
        if (!s) s = check_hip(c, w->d_minq.alloc(P * T), "projection minq");
        if (!s) s = check_hip(c, w->d_taken.alloc(P * T), "projection taken");
        if (!s) s = check_hip(c, w->d_uv.alloc(P * Q), "projection uv");
        if (!s) s = check_hip(c, w->d_win.alloc(P * Q), "projection windows");
        if (!s) s = check_hip(c, w->d_status.alloc(P * Q), "projection status");
        if (!s) s = check_hip(c, w->d_keys.alloc(P * Q * kProjKeys), "projection keys");
        if (!s) s = check_hip(c, w->d_more.alloc(P * Q), "projection flags");
        if (!s) s = check_hip(c, w->d_head.alloc(P * Q), "projection heads");
        if (!s) s = check_hip(c, w->d_res.alloc(P * Q), "projection results");
        if (!s) s = check_hip(c, w->d_out.alloc(P * Q), "projection matches");
        if (!s) s = check_hip(c, w->d_count.alloc(P), "projection counts");
        if (!s) s = check_hip(c, w->d_pairs.alloc(2 * P), "projection pairs");
        if (s) return s;
        w->pairs = (int)P;
        w->qcap = (int)Q;
        w->tcap = (int)T;
    }
    *out = w;
    return RGBD_OK;
}

bool th_ok(float th) { return std::isfinite(th) && th >= 0.0f && th <= 65536.0f; }

rgbd_status make_cfg(rgbd_ctx* c, const rgbd_bounds* bounds, float th, ProjCfg* g)
{
    rgbd_bounds b{};
    if (bounds) b = *bounds;
    else {
        const rgbd_status s = rgbd_image_bounds(c, &b);
        if (s) return s;
    }
    if (!std::isfinite(b.min_x) || !std::isfinite(b.max_x) || !std::isfinite(b.min_y) || !std::isfinite(b.max_y) ||
        !(b.max_x > b.min_x) || !(b.max_y > b.min_y))
        return fail(c, RGBD_ERR_ARG, "projection match: bounds must be finite with max > min");
    g->fx = c->cam.fx; g->fy = c->cam.fy; g->cx = c->cam.cx; g->cy = c->cam.cy;
    g->min_x = b.min_x; g->max_x = b.max_x; g->min_y = b.min_y; g->max_y = b.max_y;
    g->winv = 64.0f / (b.max_x - b.min_x);   // mfGridElementWidthInv (Core/Frame.cpp:62-63)
    g->hinv = 48.0f / (b.max_y - b.min_y);
    g->th = th;
    return RGBD_OK;
}

ProjWork work_view(const ProjWS* w)
{
    ProjWork k{};
    k.qcap = w->qcap; k.tcap = w->tcap;
    k.cell_off = w->d_cell_off; k.s_rec = w->d_srec; k.s_desc = w->d_sdesc;
    k.uv = w->d_uv; k.win = w->d_win; k.status = w->d_status; k.keys = w->d_keys; k.more = w->d_more;
    k.head = w->d_head; k.res = w->d_res; k.minq = w->d_minq; k.taken = w->d_taken; k.out = w->d_out;
    k.out_count = w->d_count;
    return k;
}

// the three launches over npairs pairs; max_q / max_t = the most queries / trains any pair can have
rgbd_status run_pairs(rgbd_ctx* c, const ProjFrames& f, const ProjCfg& g, const ProjWork& k, int max_q, int max_t, int npairs, bool debug,
                      bool assign)
{
    const hipStream_t st = c->stream;
    int tk = timer_begin(c, "k_proj_grid");
    RGBD_TRY(c, launch_proj_grid(f, g, k, npairs, st), "proj_grid");
    timer_end(c, tk);
    tk = timer_begin(c, "k_proj_search");
    RGBD_TRY(c, launch_proj_search(f, g, k, max_q, max_t, npairs, debug, st), "proj_search");
    timer_end(c, tk);
    if (!assign) return RGBD_OK;
    tk = timer_begin(c, "k_proj_assign");
    RGBD_TRY(c, launch_proj_assign(f, g, k, max_t, npairs, st), "proj_assign");
    timer_end(c, tk);
    return RGBD_OK;
}

// one pair from host buffers, staged as frames 0 (F1) and 1 (F2) of `cap` rows
rgbd_status stage_pair(rgbd_ctx* c, const float* xyz1, const uint8_t* desc1, const uint8_t* outlier1, int n1, const float* Tcw1,
                       const rgbd_keypoint* kun2, const float* xyz2, const uint8_t* desc2, int n2, const float* Tcw2,
                       ProjWS** wout, ProjFrames* f)
{
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    ProjWS* w = nullptr;
    if ((s = ws_get(c, 1, n1, n2, &w))) return s;
    const size_t cap = (size_t)std::max(n1, n2);
    s = check_hip(c, w->d_kun.reserve(2 * cap * 7), "projection keypoints");
    if (!s) s = check_hip(c, w->d_xyz.reserve(2 * cap * 3), "projection xyz");
    if (!s) s = check_hip(c, w->d_desc.reserve(2 * cap * 32), "projection descriptors");
    if (!s) s = check_hip(c, w->d_outlier.reserve(2 * cap), "projection outlier flags");
    if (!s) s = check_hip(c, w->d_poses.reserve(32), "projection poses");
    if (!s) s = check_hip(c, w->d_fcount.reserve(2), "projection frame counts");
    if (s) return s;
    const hipStream_t st = c->stream;
    const int counts[2] = {n1, n2}, pairs[2] = {0, 1};
    s = check_hip(c, hipMemcpyAsync(w->d_fcount, counts, 8, hipMemcpyHostToDevice, st), "projection counts up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_pairs, pairs, 8, hipMemcpyHostToDevice, st), "projection pairs up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_poses, Tcw1, 64, hipMemcpyHostToDevice, st), "projection pose up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_poses + 16, Tcw2, 64, hipMemcpyHostToDevice, st), "projection pose up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_xyz, xyz1, (size_t)n1 * 12, hipMemcpyHostToDevice, st), "projection xyz up");
    if (!s && n2 > 0) s = check_hip(c, hipMemcpyAsync(w->d_xyz + cap * 3, xyz2, (size_t)n2 * 12, hipMemcpyHostToDevice, st), "projection xyz up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_desc, desc1, (size_t)n1 * 32, hipMemcpyHostToDevice, st), "projection desc up");
    if (!s && n2 > 0) s = check_hip(c, hipMemcpyAsync(w->d_desc + cap * 32, desc2, (size_t)n2 * 32, hipMemcpyHostToDevice, st), "projection desc up");
    if (!s && n2 > 0) s = check_hip(c, hipMemcpyAsync(w->d_kun + cap * 7, kun2, (size_t)n2 * 28, hipMemcpyHostToDevice, st), "projection keypoints up");
    if (!s && outlier1) s = check_hip(c, hipMemcpyAsync(w->d_outlier, outlier1, (size_t)n1, hipMemcpyHostToDevice, st), "projection flags up");
    if (s) return s;
    *f = ProjFrames{w->d_fcount, w->d_kun, w->d_xyz, w->d_desc, outlier1 ? w->d_outlier.get() : nullptr, w->d_poses,
                    w->d_pairs, w->d_pairs + 1, (int)cap};
    *wout = w;
    return RGBD_OK;
}

bool pair_args_ok(const float* xyz1, const uint8_t* desc1, int n1, const float* Tcw1, const rgbd_keypoint* kun2, const float* xyz2,
                  const uint8_t* desc2, int n2, const float* Tcw2)
{
    if (n1 < 0 || n2 < 0 || !Tcw1 || !Tcw2) return false;
    if (n1 > 0 && (!xyz1 || !desc1)) return false;
    if (n2 > 0 && (!kun2 || !xyz2 || !desc2)) return false;
    return true;
}

}  // namespace

extern "C" {

rgbd_status rgbd_image_bounds(rgbd_ctx* c, rgbd_bounds* out)
{
    if (!c || !out) return RGBD_ERR_ARG;
    if (!c->bounds_set) {
        if (c->cam.k1 == 0.0f) {   // Core/Frame.cpp:309-314
            c->bounds = rgbd_bounds{0.0f, (float)c->W, 0.0f, (float)c->H};
        } else {
            rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
            if (s) return s;
            if (!c->d_cfg) return fail(c, RGBD_ERR_HIP, "image bounds: the context has no device workspace");
            DevBuf<float> d_b;
            float b[4] = {0, 0, 0, 0};
            if ((s = check_hip(c, d_b.alloc(4), "image bounds"))) return s;
            RGBD_TRY(c, launch_proj_bounds(c->d_cfg, d_b, c->stream), "proj_bounds");
            s = check_hip(c, hipMemcpyAsync(b, d_b, 16, hipMemcpyDeviceToHost, c->stream), "image bounds read");
            if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
            if (s) return s;
            c->bounds = rgbd_bounds{b[0], b[1], b[2], b[3]};
        }
        c->bounds_set = true;
    }
    *out = c->bounds;
    return RGBD_OK;
}

rgbd_status rgbd_projection_match(rgbd_ctx* c, const float* xyz1, const uint8_t* desc1, const uint8_t* outlier1, int32_t n1,
                                  const float* Tcw1, const rgbd_keypoint* kun2, const float* xyz2, const uint8_t* desc2,
                                  int32_t n2, const float* Tcw2, const rgbd_bounds* bounds, float th, rgbd_dmatch* out,
                                  int32_t cap, int32_t* m)
{
    if (!c || !m || cap < 0 || (cap > 0 && !out)) return RGBD_ERR_ARG;
    *m = 0;
    if (!th_ok(th)) return fail(c, RGBD_ERR_ARG, "projection match: th must be finite and in [0, 65536]");
    if (!pair_args_ok(xyz1, desc1, n1, Tcw1, kun2, xyz2, desc2, n2, Tcw2)) return fail(c, RGBD_ERR_ARG, "projection match: null input");
    if (n2 > kProjMaxTrain) return fail(c, RGBD_ERR_UNSUPPORTED, "projection match: more than 65536 train rows (16-bit position in the rank key)");
    if (n1 == 0 || n2 == 0) return RGBD_OK;
    ProjCfg g{};
    rgbd_status s = make_cfg(c, bounds, th, &g);
    if (s) return s;
    ProjWS* w = nullptr;
    ProjFrames f{};
    if ((s = stage_pair(c, xyz1, desc1, outlier1, n1, Tcw1, kun2, xyz2, desc2, n2, Tcw2, &w, &f))) return s;
    if ((s = run_pairs(c, f, g, work_view(w), n1, n2, 1, false, true))) return s;
    int cnt = 0;
    s = check_hip(c, hipMemcpyAsync(&cnt, w->d_count, 4, hipMemcpyDeviceToHost, c->stream), "projection count");
    if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
    if (s) return s;
    *m = cnt;
    const int rd = std::min(cnt, cap);
    if (rd > 0) {
        s = check_hip(c, hipMemcpyAsync(out, w->d_out, (size_t)rd * sizeof(rgbd_dmatch), hipMemcpyDeviceToHost, c->stream), "projection matches");
        if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
        if (s) return s;
    }
    return cnt > cap ? fail(c, RGBD_ERR_CAPACITY, "projection match capacity") : RGBD_OK;
}

rgbd_status rgbd_debug_projection(rgbd_ctx* c, const float* xyz1, const uint8_t* desc1, const uint8_t* outlier1, int32_t n1,
                                  const float* Tcw1, const rgbd_keypoint* kun2, const float* xyz2, const uint8_t* desc2,
                                  int32_t n2, const float* Tcw2, const rgbd_bounds* bounds, float th, uint32_t* uv_bits,
                                  int32_t* status, int32_t* cand, int32_t cand_cap, int32_t* cand_count)
{
    if (!c || cand_cap < 0 || (cand_cap > 0 && !cand)) return RGBD_ERR_ARG;
    if (!th_ok(th)) return fail(c, RGBD_ERR_ARG, "projection match: th must be finite and in [0, 65536]");
    if (!pair_args_ok(xyz1, desc1, n1, Tcw1, kun2, xyz2, desc2, n2, Tcw2)) return fail(c, RGBD_ERR_ARG, "projection match: null input");
    if (n1 > 0 && (!uv_bits || !status || !cand_count)) return fail(c, RGBD_ERR_ARG, "projection debug: null output");
    if (n2 > kProjMaxTrain) return fail(c, RGBD_ERR_UNSUPPORTED, "projection match: more than 65536 train rows (16-bit position in the rank key)");
    if (n1 == 0) return RGBD_OK;
    ProjCfg g{};
    rgbd_status s = make_cfg(c, bounds, th, &g);
    if (s) return s;
    ProjWS* w = nullptr;
    ProjFrames f{};
    if ((s = stage_pair(c, xyz1, desc1, outlier1, n1, Tcw1, kun2, xyz2, desc2, n2, Tcw2, &w, &f))) return s;
    s = check_hip(c, w->d_cand.reserve((size_t)n1 * cand_cap), "projection candidates");
    if (!s) s = check_hip(c, w->d_ccount.reserve(n1), "projection candidate counts");
    if (s) return s;
    ProjWork k = work_view(w);
    k.cand = w->d_cand;
    k.ccount = w->d_ccount;
    k.ccap = cand_cap;
    if ((s = run_pairs(c, f, g, k, n1, n2, 1, true, false))) return s;
    const hipStream_t st = c->stream;
    s = check_hip(c, hipMemcpyAsync(uv_bits, w->d_uv, (size_t)n1 * 8, hipMemcpyDeviceToHost, st), "projection uv read");
    if (!s) s = check_hip(c, hipMemcpyAsync(status, w->d_status, (size_t)n1 * 4, hipMemcpyDeviceToHost, st), "projection status read");
    if (!s) s = check_hip(c, hipMemcpyAsync(cand_count, w->d_ccount, (size_t)n1 * 4, hipMemcpyDeviceToHost, st), "projection counts read");
    if (!s && cand_cap > 0)
        s = check_hip(c, hipMemcpyAsync(cand, w->d_cand, (size_t)n1 * cand_cap * 4, hipMemcpyDeviceToHost, st), "projection candidates read");
    if (!s) s = check_hip(c, hipStreamSynchronize(st), "sync");
    return s;
}

rgbd_status rgbd_projection_match_batch(rgbd_ctx* c, int32_t P, const int32_t* qframe, const int32_t* tframe, const float* poses,
                                        const uint8_t* outlier, float th, rgbd_dmatch* out, int32_t* counts)
{
    if (!c || P < 0 || (P > 0 && (!qframe || !tframe || !poses || !out || !counts))) return RGBD_ERR_ARG;
    if (!th_ok(th)) return fail(c, RGBD_ERR_ARG, "projection match: th must be finite and in [0, 65536]");
    const int B = c->last_B, K = c->cfg.kp_cap;
    if (B < 1) return fail(c, RGBD_ERR_ARG, "projection match batch: no extracted batch");
    for (int p = 0; p < P; p++)
        if (qframe[p] >= B || (qframe[p] >= 0 && (tframe[p] < 0 || tframe[p] >= B)))
            return fail(c, RGBD_ERR_ARG, "projection match batch: frame index outside the last batch");
    if (K > kProjMaxTrain) return fail(c, RGBD_ERR_UNSUPPORTED, "projection match: more than 65536 train rows (16-bit position in the rank key)");
    if (P == 0) return RGBD_OK;
    ProjCfg g{};
    rgbd_status s = make_cfg(c, nullptr, th, &g);
    if (s) return s;
    if ((s = check_hip(c, hipSetDevice(c->device), "hipSetDevice"))) return s;
    if ((s = order_after_extraction(c))) return s;
    ProjWS* w = nullptr;
    if ((s = ws_get(c, P, K, K, &w))) return s;
    s = check_hip(c, w->d_poses.reserve((size_t)B * 16), "projection poses");
    if (!s && outlier) s = check_hip(c, w->d_outlier.reserve((size_t)B * K), "projection outlier flags");
    if (s) return s;
    const hipStream_t st = c->stream;
    // the pair list lives in the first 2 P entries of d_pairs (its capacity follows the workspace's pair count)
    s = check_hip(c, hipMemcpyAsync(w->d_pairs, qframe, (size_t)P * 4, hipMemcpyHostToDevice, st), "projection pairs up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_pairs + P, tframe, (size_t)P * 4, hipMemcpyHostToDevice, st), "projection pairs up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_poses, poses, (size_t)B * 64, hipMemcpyHostToDevice, st), "projection poses up");
    if (!s && outlier) s = check_hip(c, hipMemcpyAsync(w->d_outlier, outlier, (size_t)B * K, hipMemcpyHostToDevice, st), "projection flags up");
    if (s) return s;
    const ProjFrames f{c->out.count, c->out.kun, c->out.xyz, c->out.desc, outlier ? w->d_outlier.get() : nullptr, w->d_poses,
                       w->d_pairs, w->d_pairs + P, K};
    if ((s = run_pairs(c, f, g, work_view(w), K, K, P, false, true))) return s;
    s = check_hip(c, hipMemcpyAsync(counts, w->d_count, (size_t)P * 4, hipMemcpyDeviceToHost, st), "projection counts");
    if (!s) s = check_hip(c, hipStreamSynchronize(st), "sync");
    if (s) return s;
    // the workspace rows are qcap (>= K) long
    for (int p = 0; p < P && !s; p++)
        if (counts[p] > 0)
            s = check_hip(c, hipMemcpyAsync(out + (size_t)p * K, w->d_out + (size_t)p * w->qcap, (size_t)counts[p] * sizeof(rgbd_dmatch),
                                            hipMemcpyDeviceToHost, st), "projection matches");
    if (!s) s = check_hip(c, hipStreamSynchronize(st), "sync");
    return s;
}

}  // extern "C"
