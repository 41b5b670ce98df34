// gftt_host.cpp -- host side of the Shi-Tomasi GFTT + BRIEF front end (gftt.hip): Extractor(GFTT, BRIEF, NORMAL),
// behind the same extraction entry points as the ORBextractor, the SVO and the adaptive front ends.
//   Extractor::create(GFTT)       Features/Extractor.cpp:178-181  -> gftt_configure (GfttCfg)
//   Extractor::detectAndCompute   Features/Extractor.cpp:50-61    -> GfttWS::run (one launch chain)
//   Frame::undistortKeyPoints + uprojectCamera (Core/Frame.cpp:91-117, 251-281) -> k_undistort
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "brief_front.h"
#include "gftt_dev.h"
#include "launch.h"

namespace rgbd {

struct GfttWS : FrontEnd {
    GfttCfg cfg{};
    BriefFront bf;                 // one level: gray + box sums
    DevBuf<uint32_t> d_maxkey;     // [B]
    DevBuf<uint64_t> d_keys;       // [B][cand_cap]
    DevBuf<int> d_ncand;           // [B]
    DevBuf<uint64_t> d_corners;    // [B][nfeatures]
    DevBuf<int> d_ncorner, d_ranks;   // [B]
    DevBuf<float> d_eig;           // rgbd_gftt_debug_eig staging, [H][W]
    DevBuf<uint64_t> d_sel_keys, d_sel_out;   // rgbd_gftt_select staging
    DevBuf<int> d_sel_n;           // its ncorner, ranks

    rgbd_status alloc(rgbd_ctx* c) override;
    rgbd_status run(rgbd_ctx* c, const uint8_t* d_bgr, const uint16_t* d_depth, int B, bool from_gray,
                    const ExtractHook* after_fast) override;
    BriefFront* brief() override { return &bf; }
};

namespace {

GfttWS* ws(rgbd_ctx* c) { return dynamic_cast<GfttWS*>(c->front.get()); }   // null: not a GFTT context

rgbd_status not_gftt(rgbd_ctx* c) { return fail(c, RGBD_ERR_ARG, "not a GFTT context (rgbd_create_gftt)"); }

// integer d2 < min_distance^2 (f64) <=> d2 < ceil(min_distance^2); 0: no spacing test (min_distance < 1)
int dist_limit(double min_distance) { return min_distance < 1.0 ? 0 : (int)std::ceil(min_distance * min_distance); }

}  // namespace

rgbd_status gftt_configure(rgbd_ctx* c, const rgbd_gftt_params& p)
{
    // every refusal before anything is allocated
    if (p.nfeatures < 1 || p.nfeatures > kGfttMaxCorners) return fail(c, RGBD_ERR_UNSUPPORTED, "gftt: nfeatures must be 1..12288");
    if (!(p.quality_level > 0.0 && p.quality_level < 1.0)) return fail(c, RGBD_ERR_UNSUPPORTED, "gftt: 0 < quality_level < 1");
    if (!std::isfinite(p.min_distance) || p.min_distance < 0.0 || p.min_distance > 64.0)
        return fail(c, RGBD_ERR_UNSUPPORTED, "gftt: min_distance must be finite and in [0, 64]");
    if (p.cand_cap < 0 || p.cand_cap > kGfttMaxCandCap) return fail(c, RGBD_ERR_UNSUPPORTED, "gftt: cand_cap must be 1..1048576 (0: 32768)");
    if (c->W < 2 || c->H < 2 || c->W > 2047 || c->H > 2047) return fail(c, RGBD_ERR_UNSUPPORTED, "gftt: image sides 2..2047");
    GfttCfg g{};
    g.W = c->W;
    g.H = c->H;
    g.nfeatures = p.nfeatures;
    g.cand_cap = p.cand_cap > 0 ? p.cand_cap : kGfttDefaultCandCap;
    g.chunk = gftt_default_chunk(p.nfeatures);
    g.dist_lim = dist_limit(p.min_distance);
    g.border = kBriefBorder;
    g.kp_cap = p.nfeatures;
    g.quality_level = p.quality_level;
    GfttWS* w = new GfttWS();
    c->front.reset(w);
    w->cfg = g;
    w->bf.one_level(c->W, c->H, g.kp_cap);
    c->cfg.kp_cap = g.kp_cap;   // the output arrays (kps, desc, xyz, knn) are sized by it
    return RGBD_OK;
}

rgbd_status GfttWS::alloc(rgbd_ctx* c)
{
    const GfttCfg& g = cfg;
    const size_t B = (size_t)c->maxB;
    rgbd_status s = bf.alloc(c, "gftt", "gray");
    if (!s) s = check_hip(c, d_maxkey.alloc(B), "gftt maxima");
    if (!s) s = check_hip(c, d_keys.alloc(B * g.cand_cap), "gftt candidates");
    if (!s) s = check_hip(c, d_ncand.alloc(B), "gftt candidate counts");
    if (!s) s = check_hip(c, d_corners.alloc(B * g.nfeatures), "gftt corners");
    if (!s) s = check_hip(c, d_ncorner.alloc(B), "gftt corner counts");
    if (!s) s = check_hip(c, d_ranks.alloc(B), "gftt ranks");
    if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
    return s;
}

rgbd_status GfttWS::run(rgbd_ctx* c, const uint8_t* d_bgr, const uint16_t* d_depth, int B, bool from_gray,
                        const ExtractHook* after_fast)
{
    const GfttCfg& g = cfg;
    const hipStream_t st = c->stream;
    const size_t fb = (size_t)bf.cfg.frame_bytes;
    rgbd_status s = check_hip(c, hipMemsetAsync(d_maxkey, 0, 4 * (size_t)B, st), "clear gftt maxima");
    if (!s) s = check_hip(c, hipMemsetAsync(d_ncand, 0, 4 * (size_t)B, st), "clear gftt counts");
    if (!s) s = bf.run_pyramid(c, d_bgr, B, from_gray);
    if (s) return s;
    int tk = timer_begin(c, "k_gftt_max");
    RGBD_TRY(c, launch_gftt_max(bf.d_pyr, fb, g, d_maxkey, B, st), "gftt_max");
    timer_end(c, tk);
    tk = timer_begin(c, "k_gftt_cand");
    RGBD_TRY(c, launch_gftt_cand(bf.d_pyr, fb, g, d_maxkey, d_keys, d_ncand, c->d_err, B, st), "gftt_cand");
    timer_end(c, tk);
    // e.g. the deferred PnPRansac solves of earlier pipelined steps (pnp_host.cpp)
    if ((s = call_hook(after_fast, 1)) || (s = call_hook(after_fast, 2))) return s;
    tk = timer_begin(c, "k_gftt_select");
    RGBD_TRY(c, launch_gftt_select(d_keys, d_ncand, 0, g, d_corners, d_ncorner, d_ranks, c->out.count, c->out.kps, B, st),
             "gftt_select");
    timer_end(c, tk);
    return bf.run_describe(c, d_depth, B);
}

}  // namespace rgbd

using namespace rgbd;

extern "C" {

rgbd_status rgbd_gftt_debug_eig(rgbd_ctx* c, int32_t b, float* out)
{
    if (!c || !out) return RGBD_ERR_ARG;
    if (!ws(c)) return not_gftt(c);
    if (b < 0 || b >= c->last_B) return fail(c, RGBD_ERR_ARG, "gftt: frame index outside the last batch");
    GfttWS* w = ws(c);
    const GfttCfg& g = w->cfg;
    const size_t px = (size_t)g.W * g.H;
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (!s && !w->d_eig) s = check_hip(c, w->d_eig.alloc(px), "gftt map");
    if (s) return s;
    RGBD_TRY(c, launch_gftt_eig(w->bf.d_pyr + (size_t)b * w->bf.cfg.frame_bytes, g, w->d_eig, c->stream), "gftt_eig");
    s = check_hip(c, hipMemcpyAsync(out, w->d_eig, px * 4, hipMemcpyDeviceToHost, c->stream), "read gftt map");
    return s ? s : check_hip(c, hipStreamSynchronize(c->stream), "sync");
}

rgbd_status rgbd_gftt_debug_corners(rgbd_ctx* c, int32_t b, uint32_t* max_bits, int32_t* n_candidates, int32_t* xy, float* val,
                                    int32_t cap, int32_t* n)
{
    if (!c) return RGBD_ERR_ARG;
    if (!ws(c)) return not_gftt(c);
    if (b < 0 || b >= c->last_B) return fail(c, RGBD_ERR_ARG, "gftt: frame index outside the last batch");
    if (cap < 0) return fail(c, RGBD_ERR_ARG, "gftt: negative output capacity");
    GfttWS* w = ws(c);
    const GfttCfg& g = w->cfg;
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    uint32_t mk = 0;
    int nc = 0, m = 0;
    s = check_hip(c, hipMemcpyAsync(&mk, w->d_maxkey + b, 4, hipMemcpyDeviceToHost, c->stream), "read gftt maximum");
    if (!s) s = check_hip(c, hipMemcpyAsync(&nc, w->d_ncand + b, 4, hipMemcpyDeviceToHost, c->stream), "read gftt count");
    if (!s) s = check_hip(c, hipMemcpyAsync(&m, w->d_ncorner + b, 4, hipMemcpyDeviceToHost, c->stream), "read gftt corners");
    if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
    if (s) return s;
    if (max_bits) {
        const float M = gftt_decode_max(mk);
        std::memcpy(max_bits, &M, 4);
    }
    if (n_candidates) *n_candidates = nc;
    if (n) *n = m;
    if ((xy || val) && m > cap) return fail(c, RGBD_ERR_CAPACITY, "output capacity smaller than the frame's corner count");
    if (m == 0 || (!xy && !val)) return RGBD_OK;
    std::vector<uint64_t> keys((size_t)m);
    s = check_hip(c, hipMemcpyAsync(keys.data(), w->d_corners + (size_t)b * g.nfeatures, (size_t)m * 8, hipMemcpyDeviceToHost,
                                    c->stream), "read gftt corner list");
    if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
    if (s) return s;
    for (int i = 0; i < m; i++) {
        const uint32_t idx = (uint32_t)keys[i], bits = (uint32_t)(keys[i] >> 32);
        if (xy) {
            xy[2 * i] = (int32_t)(idx % (uint32_t)g.W);
            xy[2 * i + 1] = (int32_t)(idx / (uint32_t)g.W);
        }
        if (val) std::memcpy(val + i, &bits, 4);
    }
    return RGBD_OK;
}

rgbd_status rgbd_gftt_debug_ranks(rgbd_ctx* c, int32_t b, int32_t* ranks)
{
    if (!c || !ranks) return RGBD_ERR_ARG;
    if (!ws(c)) return not_gftt(c);
    if (b < 0 || b >= c->last_B) return fail(c, RGBD_ERR_ARG, "gftt: frame index outside the last batch");
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (!s) s = check_hip(c, hipMemcpyAsync(ranks, ws(c)->d_ranks + b, 4, hipMemcpyDeviceToHost, c->stream), "read gftt ranks");
    return s ? s : check_hip(c, hipStreamSynchronize(c->stream), "sync");
}

rgbd_status rgbd_gftt_select(rgbd_ctx* c, const int32_t* xy, const float* val, int32_t n, int32_t W, int32_t H,
                             double min_distance, int32_t max_corners, int32_t chunk, int32_t* out_idx, int32_t* m)
{
    if (!c || !m || n < 0 || (n > 0 && (!xy || !val)) || !out_idx) return RGBD_ERR_ARG;
    if (!ws(c)) return not_gftt(c);
    *m = 0;
    if (W < 1 || H < 1 || W > 2047 || H > 2047 || n > kGfttMaxCandCap || max_corners < 1 || max_corners > kGfttMaxCorners ||
        chunk < 0 || chunk > kGfttMaxChunk || !std::isfinite(min_distance) || min_distance < 0.0 || min_distance > 64.0)
        return fail(c, RGBD_ERR_ARG, "gftt select: sides 1..2047, n <= 1048576, max_corners 1..12288, chunk 0..4096, min_distance in [0, 64]");
    if (n == 0) return RGBD_OK;
    std::vector<uint64_t> keys((size_t)n);
    std::unordered_map<uint32_t, int32_t> where;
    where.reserve((size_t)n * 2);
    for (int i = 0; i < n; i++) {
        const int x = xy[2 * i], y = xy[2 * i + 1];
        uint32_t bits;
        std::memcpy(&bits, val + i, 4);
        if (x < 0 || x >= W || y < 0 || y >= H || !(val[i] > 0.0f) || !std::isfinite(val[i]))
            return fail(c, RGBD_ERR_ARG, "gftt select: points inside the image with positive finite values");
        const uint32_t idx = (uint32_t)(y * W + x);
        if (!where.emplace(idx, i).second) return fail(c, RGBD_ERR_ARG, "gftt select: the points must be distinct");
        keys[(size_t)i] = gftt_key(bits, idx);
    }
    GfttWS* w = ws(c);
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    if ((s = check_hip(c, w->d_sel_keys.reserve((size_t)n), "gftt select keys"))) return s;   // every call ends synchronised
    if (!w->d_sel_n) {   // the one allocated last
        s = check_hip(c, w->d_sel_out.alloc((size_t)kGfttMaxCorners), "gftt select corners");
        if (!s) s = check_hip(c, w->d_sel_n.alloc(2), "gftt select counts");
        if (s) return s;
    }
    GfttCfg g = w->cfg;   // the extraction's kernel on the caller's list and parameters
    g.W = W;
    g.H = H;
    g.nfeatures = max_corners;
    g.kp_cap = max_corners;
    g.cand_cap = n;
    g.chunk = chunk > 0 ? chunk : gftt_default_chunk(max_corners);
    g.dist_lim = dist_limit(min_distance);
    s = check_hip(c, hipMemcpyAsync(w->d_sel_keys, keys.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream), "gftt select up");
    if (s) return s;
    RGBD_TRY(c, launch_gftt_select(w->d_sel_keys, nullptr, n, g, w->d_sel_out, w->d_sel_n, w->d_sel_n + 1, nullptr, nullptr, 1,
                                   c->stream), "gftt_select");
    int cnt = 0;
    s = check_hip(c, hipMemcpyAsync(&cnt, w->d_sel_n, 4, hipMemcpyDeviceToHost, c->stream), "gftt select count");
    if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
    if (s) return s;
    if (cnt < 0 || cnt > max_corners) return fail(c, RGBD_ERR_HIP, "gftt select: corrupt corner count");
    if (cnt) {
        s = check_hip(c, hipMemcpyAsync(keys.data(), w->d_sel_out, (size_t)cnt * 8, hipMemcpyDeviceToHost, c->stream), "gftt select down");
        if (!s) s = check_hip(c, hipStreamSynchronize(c->stream), "sync");
        if (s) return s;
    }
    for (int i = 0; i < cnt; i++) out_idx[i] = where[(uint32_t)keys[(size_t)i]];
    *m = cnt;
    return RGBD_OK;
}

}  // extern "C"
