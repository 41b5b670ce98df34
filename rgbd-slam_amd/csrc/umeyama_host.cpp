// umeyama_host.cpp -- C ABI of the Umeyama RANSAC (umeyama.hip): Ransac::compute (Solver/Ransac.cpp:46-181) for one
// problem, a batch of problems, and the pairs of the last extraction.  The solve of every form is one k_umeyama
// launch; the hard limits are checked before any copy or launch (DESIGN.md "Umeyama RANSAC definition").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>

#include "context.h"
#include "umeyama_dev.h"

using namespace rgbd;

namespace rgbd {

struct UmWS {
    DevBuf<float> d_pts;
    DevBuf<UmProb> d_probs;
    DevBuf<int> d_tables;
    DevBuf<int32_t> d_rngs, d_inl;
    DevBuf<UmRes> d_res;
    // rgbd_ransac_umeyama_frames
    DevBuf<rgbd_dmatch> d_matches;
    DevBuf<int> d_counts, d_pairs, d_gated, d_err;
    // rgbd_debug_ransac_umeyama
    DevBuf<int32_t> d_dpos, d_dcount, d_dacc;
    DevBuf<uint8_t> d_dsneg;
    // bound tables by gated count, for tab_ratio (glibc log / pow, computed once per distinct count)
    std::map<int, std::vector<int>> tabs;
    double tab_ratio = -1.0;
};

void umeyama_free(rgbd_ctx* c)
{
    delete c->umeyama;
    c->umeyama = nullptr;
}

}  // namespace rgbd

namespace {

// the hard limits; nullptr when the parameters pass
const char* make_prm(const rgbd_umeyama_params* q, UmPrm* p)
{
    if (q->error_version == 3) return "ransac umeyama: MAHALANOBIS_ERROR reads an uninitialised covariance in the reference";
    if (q->error_version == 1 || q->error_version == 2) return "ransac umeyama: the reprojection versions need the camera the reference never sets";
    if (q->error_version != 0 && q->error_version != 4) return "ransac umeyama: unknown error_version";
    if (q->used_pairs < 3 || q->used_pairs > kUmMaxPairs) return "ransac umeyama: used_pairs outside [3, 8]";
    if (q->min_matches < q->used_pairs) return "ransac umeyama: min_matches below used_pairs (the reference's sampler would not end)";
    if (!(q->min_inlier_ratio >= 0.05 && q->min_inlier_ratio <= 1.0)) return "ransac umeyama: min_inlier_ratio outside [0.05, 1]";
    p->adaptive = q->error_version == 4 ? 1 : 0;
    p->used_pairs = q->used_pairs;
    p->min_matches = q->min_matches;
    p->max_bound = um_iters(q->min_inlier_ratio);
    p->thr = q->thr_euclidean;
    p->min_ratio = q->min_inlier_ratio;
    return nullptr;
}

UmWS* ws_get(rgbd_ctx* c)
{
    if (!c->umeyama) c->umeyama = new UmWS();
    return c->umeyama;
}

// the concatenated bound tables of the problems' gated counts; probs[p].tab_off set
void build_tables(UmWS* w, const UmPrm& prm, const std::vector<int>& gated, std::vector<UmProb>& probs, std::vector<int>& tables)
{
    if (w->tab_ratio != prm.min_ratio) {
        w->tabs.clear();
        w->tab_ratio = prm.min_ratio;
    }
    std::map<int, int> at;
    tables.clear();
    for (size_t p = 0; p < probs.size(); p++) {
        const int M = gated[p];
        probs[p].tab_off = 0;
        if (!probs[p].run || M < prm.min_matches) continue;
        auto f = at.find(M);
        if (f == at.end()) {
            std::vector<int>& t = w->tabs[M];
            if (t.empty()) {
                t.resize((size_t)M + 1);
                um_bound_table(M, prm.min_ratio, t.data());
            }
            f = at.emplace(M, (int)tables.size()).first;
            tables.insert(tables.end(), t.begin(), t.end());
        }
        probs[p].tab_off = f->second;
    }
    if (tables.empty()) tables.push_back(0);
}

struct UmDebugOut {
    int32_t* pos;       // [cap][used_pairs]
    int32_t* count;     // [cap]
    uint8_t* sneg;      // [cap]
    int32_t cap;
    int32_t* accepts;   // [acc_cap][3]
    int32_t acc_cap;
    int32_t* n_accepts;
    int32_t* best_count;
};

int dbg_cap(const UmPrm& prm)
{
    const int mb = std::max(prm.max_bound, kUmIters0);
    return (mb + kUmThreads - 1) / kUmThreads * kUmThreads;
}

// The solve over problems already on the device (w->d_pts rows, probs with tab_off set): upload the descriptors,
// tables and generators, one launch, read back.  rngs: [P][33] in / out.
rgbd_status solve_dev(rgbd_ctx* c, UmWS* w, const UmPrm& prm, const std::vector<UmProb>& probs, const std::vector<int>& tables,
                      size_t rows, int max_m, rgbd_rng* rngs, std::vector<UmRes>& res, std::vector<int32_t>& inl,
                      const UmDebugOut* dbg)
{
    const size_t P = probs.size();
    rgbd_status s = check_hip(c, w->d_probs.reserve(P), "ransac umeyama problems");
    if (!s) s = check_hip(c, w->d_tables.reserve(tables.size()), "ransac umeyama tables");
    if (!s) s = check_hip(c, w->d_rngs.reserve(33 * P), "ransac umeyama generators");
    if (!s) s = check_hip(c, w->d_inl.reserve(std::max<size_t>(rows, 1)), "ransac umeyama inliers");
    if (!s) s = check_hip(c, w->d_res.reserve(P), "ransac umeyama results");
    UmDbg d{nullptr, nullptr, nullptr, nullptr, 0};
    if (!s && dbg) {
        const size_t cap = (size_t)dbg_cap(prm);
        s = check_hip(c, w->d_dpos.reserve(cap * kUmMaxPairs), "ransac umeyama debug");
        if (!s) s = check_hip(c, w->d_dcount.reserve(cap), "ransac umeyama debug");
        if (!s) s = check_hip(c, w->d_dsneg.reserve(cap), "ransac umeyama debug");
        if (!s) s = check_hip(c, w->d_dacc.reserve(3 * (size_t)(kUmMaxM + 1)), "ransac umeyama debug");
        d = UmDbg{w->d_dpos, w->d_dcount, w->d_dsneg, w->d_dacc, (int32_t)cap};
    }
    if (s) return s;
    static_assert(sizeof(rgbd_rng) == 33 * 4, "rgbd_rng is 33 words");
    const hipStream_t st = c->stream;
    s = check_hip(c, hipMemcpyAsync(w->d_probs, probs.data(), P * sizeof(UmProb), hipMemcpyHostToDevice, st), "ransac umeyama problems up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_tables, tables.data(), tables.size() * 4, hipMemcpyHostToDevice, st), "ransac umeyama tables up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_rngs, rngs, P * sizeof(rgbd_rng), hipMemcpyHostToDevice, st), "ransac umeyama generators up");
    if (!s) s = check_hip(c, hipMemsetAsync(w->d_res, 0, P * sizeof(UmRes), st), "ransac umeyama results clear");
    if (!s && dbg) s = check_hip(c, hipMemsetAsync(w->d_dcount, 0, (size_t)d.cap * 4, st), "ransac umeyama debug clear");
    if (!s && dbg) s = check_hip(c, hipMemsetAsync(w->d_dpos, 0, (size_t)d.cap * kUmMaxPairs * 4, st), "ransac umeyama debug clear");
    if (!s && dbg) s = check_hip(c, hipMemsetAsync(w->d_dsneg, 0, (size_t)d.cap, st), "ransac umeyama debug clear");
    if (!s && dbg) s = check_hip(c, hipMemsetAsync(w->d_dacc, 0, 3 * (size_t)(kUmMaxM + 1) * 4, st), "ransac umeyama debug clear");
    if (s) return s;
    const int tk = timer_begin(c, "k_umeyama");
    RGBD_TRY(c, launch_umeyama(w->d_pts, w->d_probs, prm, w->d_tables, w->d_rngs, w->d_inl, w->d_res, d, max_m, (int)P, st), "umeyama");
    timer_end(c, tk);
    res.resize(P);
    inl.resize(std::max<size_t>(rows, 1));
    s = check_hip(c, hipMemcpyAsync(res.data(), w->d_res, P * sizeof(UmRes), hipMemcpyDeviceToHost, st), "ransac umeyama results");
    if (!s && rows) s = check_hip(c, hipMemcpyAsync(inl.data(), w->d_inl, rows * 4, hipMemcpyDeviceToHost, st), "ransac umeyama inliers");
    if (!s) s = check_hip(c, hipMemcpyAsync(rngs, w->d_rngs, P * sizeof(rgbd_rng), hipMemcpyDeviceToHost, st), "ransac umeyama generators");
    std::vector<int32_t> hp;
    if (!s && dbg) {
        hp.resize((size_t)dbg->cap * kUmMaxPairs);
        const size_t n = (size_t)std::min(dbg->cap, d.cap);
        s = check_hip(c, hipMemcpyAsync(hp.data(), w->d_dpos, n * kUmMaxPairs * 4, hipMemcpyDeviceToHost, st), "ransac umeyama debug");
        if (!s) s = check_hip(c, hipMemcpyAsync(dbg->count, w->d_dcount, n * 4, hipMemcpyDeviceToHost, st), "ransac umeyama debug");
        if (!s) s = check_hip(c, hipMemcpyAsync(dbg->sneg, w->d_dsneg, n, hipMemcpyDeviceToHost, st), "ransac umeyama debug");
        if (!s) s = check_hip(c, hipMemcpyAsync(dbg->accepts, w->d_dacc, 3 * (size_t)std::min(dbg->acc_cap, kUmMaxM + 1) * 4, hipMemcpyDeviceToHost, st), "ransac umeyama debug");
    }
    if (!s) s = check_hip(c, hipStreamSynchronize(st), "sync");
    if (s) return s;
    if (dbg) {
        const size_t n = (size_t)std::min(dbg->cap, d.cap);
        for (size_t h = 0; h < n; h++)
            for (int k = 0; k < prm.used_pairs; k++) dbg->pos[h * prm.used_pairs + k] = hp[h * kUmMaxPairs + k];
        *dbg->n_accepts = res[0].n_accepts;
        *dbg->best_count = res[0].best_count;
    }
    return RGBD_OK;
}

struct UmHostProblem {
    const float* xyz1;
    int32_t n1;
    const float* xyz2;
    int32_t n2;
    const rgbd_dmatch* m;
    int32_t count;
    uint8_t* flags2;
};

// F2's flags and the inlier list from the final positions (:46-51, :76): every match's trainIdx is flagged outlier
// (the gated ones and a failed call's included), then the final inliers' are flagged inlier
void finish_problem(const rgbd_dmatch* m, int count, const UmRes& r, const int32_t* pos, uint8_t* flags2, rgbd_dmatch* inliers)
{
    for (int i = 0; i < count; i++) flags2[m[i].trainIdx] = 1;
    for (int k = 0; k < r.n_inliers; k++) {
        const rgbd_dmatch& a = m[pos[k]];
        inliers[k] = a;
        flags2[a.trainIdx] = 0;
    }
}

rgbd_status solve_host(rgbd_ctx* c, int P, const UmHostProblem* hp, const rgbd_umeyama_params* prm_in, rgbd_rng* rngs, float* T12,
                       rgbd_dmatch* inliers, int32_t* n_inliers, int32_t* iterations, int32_t* ok, const UmDebugOut* dbg)
{
    if (!c || P < 0) return RGBD_ERR_ARG;
    if (!prm_in) return fail(c, RGBD_ERR_ARG, "ransac umeyama: null parameters");
    UmPrm prm{};
    if (const char* why = make_prm(prm_in, &prm)) return fail(c, RGBD_ERR_UNSUPPORTED, why);
    if (P > 0 && (!hp || !rngs || !T12 || !n_inliers || !iterations || !ok)) return fail(c, RGBD_ERR_ARG, "ransac umeyama: null argument");
    size_t rows = 0;
    int max_m = 0;
    for (int p = 0; p < P; p++) {
        const UmHostProblem& h = hp[p];
        if (h.count < 0 || h.n1 < 0 || h.n2 < 0) return fail(c, RGBD_ERR_ARG, "ransac umeyama: negative count");
        if (h.count > kUmMaxM) return fail(c, RGBD_ERR_UNSUPPORTED, "ransac umeyama: more than 4096 matches per problem");
        if (h.count > 0 && (!h.xyz1 || !h.xyz2 || !h.m || !h.flags2 || !inliers)) return fail(c, RGBD_ERR_ARG, "ransac umeyama: null argument");
        for (int i = 0; i < h.count; i++)
            if ((unsigned)h.m[i].queryIdx >= (unsigned)h.n1 || (unsigned)h.m[i].trainIdx >= (unsigned)h.n2)
                return fail(c, RGBD_ERR_ARG, "ransac umeyama: a match index outside its frame");
        rows += (size_t)h.count;
        max_m = std::max(max_m, h.count);
    }
    if (P == 0) return RGBD_OK;
    std::vector<float> pts(std::max<size_t>(rows, 1) * 6);
    std::vector<UmProb> probs(P);
    std::vector<int> gated(P, 0);
    size_t off = 0;
    for (int p = 0; p < P; p++) {
        const UmHostProblem& h = hp[p];
        probs[p] = UmProb{(int)off, h.count, 0, 1};
        for (int i = 0; i < h.count; i++) {
            float* r = &pts[6 * (off + i)];
            std::memcpy(r, h.xyz1 + 3 * (size_t)h.m[i].queryIdx, 12);
            std::memcpy(r + 3, h.xyz2 + 3 * (size_t)h.m[i].trainIdx, 12);
            gated[p] += um_gated_out(r[2], r[5]) ? 0 : 1;
        }
        off += (size_t)h.count;
    }
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    UmWS* w = ws_get(c);
    std::vector<int> tables;
    build_tables(w, prm, gated, probs, tables);
    if ((s = check_hip(c, w->d_pts.reserve(pts.size()), "ransac umeyama points"))) return s;
    if ((s = check_hip(c, hipMemcpyAsync(w->d_pts, pts.data(), pts.size() * 4, hipMemcpyHostToDevice, c->stream), "ransac umeyama points up"))) return s;
    std::vector<UmRes> res;
    std::vector<int32_t> inl;
    if ((s = solve_dev(c, w, prm, probs, tables, rows, max_m, rngs, res, inl, dbg))) return s;
    for (int p = 0; p < P; p++) {
        const UmHostProblem& h = hp[p];
        std::memcpy(T12 + 16 * (size_t)p, res[p].T, 64);
        n_inliers[p] = res[p].n_inliers;
        iterations[p] = res[p].iterations;
        ok[p] = res[p].ok;
        if (h.count > 0) finish_problem(h.m, h.count, res[p], inl.data() + probs[p].off, h.flags2, inliers + probs[p].off);
    }
    return RGBD_OK;
}

// cv::Mat::inv() of a 4x4 f32 matrix as DESIGN.md defines it (unpinned): Gaussian elimination with partial
// pivoting on [A | I], every operation f32; a zero pivot gives the zero matrix
void inv4(const float* A0, float* X)
{
    float A[4][4], B[4][4];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            A[i][j] = A0[4 * i + j];
            B[i][j] = i == j ? 1.0f : 0.0f;
        }
    for (int k = 0; k < 4; k++) {
        int piv = k;
        for (int i = k + 1; i < 4; i++)
            if (std::fabs(A[i][k]) > std::fabs(A[piv][k])) piv = i;
        if (!(std::fabs(A[piv][k]) > 0.0f)) {
            for (int i = 0; i < 16; i++) X[i] = 0.0f;
            return;
        }
        if (piv != k)
            for (int j = 0; j < 4; j++) {
                std::swap(A[k][j], A[piv][j]);
                std::swap(B[k][j], B[piv][j]);
            }
        for (int i = k + 1; i < 4; i++) {
            const float f = A[i][k] / A[k][k];
            for (int j = k + 1; j < 4; j++) A[i][j] = A[i][j] - f * A[k][j];
            for (int j = 0; j < 4; j++) B[i][j] = B[i][j] - f * B[k][j];
        }
    }
    for (int j = 0; j < 4; j++)
        for (int i = 3; i >= 0; i--) {
            float v = B[i][j];
            for (int k = i + 1; k < 4; k++) v = v - A[i][k] * X[4 * k + j];
            X[4 * i + j] = v / A[i][i];
        }
}

}  // namespace

extern "C" {

rgbd_status rgbd_ransac_umeyama_batch(rgbd_ctx* c, int32_t P, const float* xyz1, const int32_t* n1, const float* xyz2,
                                      const int32_t* n2, const rgbd_dmatch* m12, const int32_t* counts,
                                      const rgbd_umeyama_params* prm, rgbd_rng* rngs, uint8_t* flags2, float* T12,
                                      rgbd_dmatch* inliers, int32_t* n_inliers, int32_t* iterations_run, int32_t* ok)
{
    if (!c || P < 0) return RGBD_ERR_ARG;
    if (P > 0 && (!n1 || !n2 || !counts)) return fail(c, RGBD_ERR_ARG, "ransac umeyama: null argument");
    std::vector<UmHostProblem> hp(P);
    size_t o1 = 0, o2 = 0, om = 0;
    for (int p = 0; p < P; p++) {
        if (n1[p] < 0 || n2[p] < 0 || counts[p] < 0) return fail(c, RGBD_ERR_ARG, "ransac umeyama: negative count");
        hp[p] = UmHostProblem{xyz1 ? xyz1 + 3 * o1 : nullptr, n1[p], xyz2 ? xyz2 + 3 * o2 : nullptr, n2[p],
                              m12 ? m12 + om : nullptr, counts[p], flags2 ? flags2 + o2 : nullptr};
        o1 += (size_t)n1[p];
        o2 += (size_t)n2[p];
        om += (size_t)counts[p];
    }
    return solve_host(c, P, hp.data(), prm, rngs, T12, inliers, n_inliers, iterations_run, ok, nullptr);
}

rgbd_status rgbd_ransac_umeyama(rgbd_ctx* c, const float* xyz1, int32_t n1, const float* xyz2, int32_t n2,
                                const rgbd_dmatch* m12, int32_t m, const rgbd_umeyama_params* prm, rgbd_rng* rng,
                                uint8_t* flags2, float* T12, rgbd_dmatch* inliers, int32_t* n_inliers,
                                int32_t* iterations_run, int32_t* ok)
{
    const UmHostProblem h{xyz1, n1, xyz2, n2, m12, m, flags2};
    return solve_host(c, 1, &h, prm, rng, T12, inliers, n_inliers, iterations_run, ok, nullptr);
}

rgbd_status rgbd_debug_ransac_umeyama(rgbd_ctx* c, const float* xyz1, int32_t n1, const float* xyz2, int32_t n2,
                                      const rgbd_dmatch* m12, int32_t m, const rgbd_umeyama_params* prm, rgbd_rng* rng,
                                      uint8_t* flags2, float* T12, rgbd_dmatch* inliers, int32_t* n_inliers,
                                      int32_t* iterations_run, int32_t* ok, int32_t hyp_cap, int32_t* hyp_pos,
                                      int32_t* hyp_count, uint8_t* hyp_sneg, int32_t* best_count, int32_t accept_cap,
                                      int32_t* accepts, int32_t* n_accepts)
{
    if (!c) return RGBD_ERR_ARG;
    if (hyp_cap < 0 || accept_cap < 0 || !hyp_pos || !hyp_count || !hyp_sneg || !best_count || !accepts || !n_accepts)
        return fail(c, RGBD_ERR_ARG, "ransac umeyama debug: null output");
    const UmDebugOut d{hyp_pos, hyp_count, hyp_sneg, hyp_cap, accepts, accept_cap, n_accepts, best_count};
    const UmHostProblem h{xyz1, n1, xyz2, n2, m12, m, flags2};
    return solve_host(c, 1, &h, prm, rng, T12, inliers, n_inliers, iterations_run, ok, &d);
}

rgbd_status rgbd_ransac_umeyama_frames(rgbd_ctx* c, int32_t P, const int32_t* qframe, const int32_t* tframe,
                                       const rgbd_dmatch* matches, const int32_t* counts, const rgbd_umeyama_params* prm_in,
                                       rgbd_rng* rngs, uint8_t* flags2, float* T12, rgbd_dmatch* inliers,
                                       int32_t* n_inliers, int32_t* iterations_run, int32_t* ok)
{
    if (!c || P < 0) return RGBD_ERR_ARG;
    if (!prm_in) return fail(c, RGBD_ERR_ARG, "ransac umeyama: null parameters");
    UmPrm prm{};
    if (const char* why = make_prm(prm_in, &prm)) return fail(c, RGBD_ERR_UNSUPPORTED, why);
    if (P > 0 && (!qframe || !tframe || !matches || !counts || !rngs || !flags2 || !T12 || !inliers || !n_inliers || !iterations_run || !ok))
        return fail(c, RGBD_ERR_ARG, "ransac umeyama frames: null argument");
    const int B = c->last_B, K = c->cfg.kp_cap;
    if (P > 0 && B < 1) return fail(c, RGBD_ERR_ARG, "ransac umeyama frames: no extracted batch");
    int max_m = 0;
    bool any = false;
    for (int p = 0; p < P; p++) {
        if (qframe[p] < 0) continue;
        if (qframe[p] >= B || tframe[p] < 0 || tframe[p] >= B)
            return fail(c, RGBD_ERR_UNSUPPORTED, "ransac umeyama frames: frame index outside the last batch");
        if (counts[p] < 0 || counts[p] > K) return fail(c, RGBD_ERR_ARG, "ransac umeyama frames: match count outside [0, kp_cap]");
        if (counts[p] > kUmMaxM) return fail(c, RGBD_ERR_UNSUPPORTED, "ransac umeyama: more than 4096 matches per problem");
        for (int i = 0; i < counts[p]; i++) {
            const rgbd_dmatch& m = matches[(size_t)p * K + i];
            if ((unsigned)m.queryIdx >= (unsigned)K || (unsigned)m.trainIdx >= (unsigned)K)
                return fail(c, RGBD_ERR_UNSUPPORTED, "ransac umeyama frames: a match index outside its frame");
        }
        max_m = std::max(max_m, counts[p]);
        any = true;
    }
    for (int p = 0; p < P; p++) {
        for (int k = 0; k < 16; k++) T12[16 * (size_t)p + k] = (k % 5 == 0) ? 1.0f : 0.0f;
        n_inliers[p] = iterations_run[p] = ok[p] = 0;
    }
    if (!any) return RGBD_OK;
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    if ((s = order_after_extraction(c))) return s;
    UmWS* w = ws_get(c);
    const size_t PK = (size_t)P * K;
    s = check_hip(c, w->d_pts.reserve(6 * PK), "ransac umeyama points");
    if (!s) s = check_hip(c, w->d_matches.reserve(PK), "ransac umeyama matches");
    if (!s) s = check_hip(c, w->d_counts.reserve((size_t)P), "ransac umeyama counts");
    if (!s) s = check_hip(c, w->d_pairs.reserve(2 * (size_t)P), "ransac umeyama pairs");
    if (!s) s = check_hip(c, w->d_gated.reserve((size_t)P), "ransac umeyama gated counts");
    if (!s) s = check_hip(c, w->d_err.reserve(1), "ransac umeyama flag");
    if (s) return s;
    const hipStream_t st = c->stream;
    s = check_hip(c, hipMemcpyAsync(w->d_matches, matches, PK * sizeof(rgbd_dmatch), hipMemcpyHostToDevice, st), "ransac umeyama matches up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_counts, counts, (size_t)P * 4, hipMemcpyHostToDevice, st), "ransac umeyama counts up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_pairs, qframe, (size_t)P * 4, hipMemcpyHostToDevice, st), "ransac umeyama pairs up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_pairs + P, tframe, (size_t)P * 4, hipMemcpyHostToDevice, st), "ransac umeyama pairs up");
    if (!s) s = check_hip(c, hipMemsetAsync(w->d_err, 0, 4, st), "ransac umeyama flag clear");
    if (s) return s;
    const int tk = timer_begin(c, "k_umeyama_gather");
    RGBD_TRY(c, launch_umeyama_gather(w->d_matches, w->d_counts, w->d_pairs, w->d_pairs + P, c->out.xyz, K, P, w->d_pts, w->d_gated,
                                      w->d_err, st), "umeyama_gather");
    timer_end(c, tk);
    std::vector<int> gated(P, 0);
    int err = 0;
    s = check_hip(c, hipMemcpyAsync(gated.data(), w->d_gated, (size_t)P * 4, hipMemcpyDeviceToHost, st), "ransac umeyama gated counts");
    if (!s) s = check_hip(c, hipMemcpyAsync(&err, w->d_err, 4, hipMemcpyDeviceToHost, st), "ransac umeyama flag");
    if (!s) s = check_hip(c, hipStreamSynchronize(st), "sync");
    if (s) return s;
    if (err) return fail(c, RGBD_ERR_UNSUPPORTED, "ransac umeyama frames: a match index outside its frame");
    std::vector<UmProb> probs(P);
    for (int p = 0; p < P; p++) probs[p] = UmProb{(int)((size_t)p * K), qframe[p] < 0 ? 0 : counts[p], 0, qframe[p] < 0 ? 0 : 1};
    std::vector<int> tables;
    build_tables(w, prm, gated, probs, tables);
    std::vector<UmRes> res;
    std::vector<int32_t> inl;
    if ((s = solve_dev(c, w, prm, probs, tables, PK, max_m, rngs, res, inl, nullptr))) return s;
    for (int p = 0; p < P; p++) {
        if (qframe[p] < 0) continue;
        std::memcpy(T12 + 16 * (size_t)p, res[p].T, 64);
        n_inliers[p] = res[p].n_inliers;
        iterations_run[p] = res[p].iterations;
        ok[p] = res[p].ok;
        finish_problem(matches + (size_t)p * K, counts[p], res[p], inl.data() + (size_t)p * K, flags2 + (size_t)p * K,
                       inliers + (size_t)p * K);
    }
    return RGBD_OK;
}

void rgbd_ransac_umeyama_pose(const float* T12, const float* Tcw1, float* Tcw2)
{
    float inv[16];
    inv4(T12, inv);
    matmul4(inv, Tcw1, Tcw2);
}

}  // extern "C"
