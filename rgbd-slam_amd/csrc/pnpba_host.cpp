// pnpba_host.cpp -- C ABI of the motion-only bundle adjustment (pnpba.hip): PnPSolver::compute
// (Solver/PnPSolver.cpp:31-150) for one problem, a batch of problems, and the pairs of the last extraction.
// Every form is one k_pnpba launch; the loop never returns to the host (DESIGN.md "Motion-only BA definition").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "context.h"
#include "pnp_dev.h"
#include "pnpba_dev.h"

using namespace rgbd;

namespace rgbd {

struct BaWS {
    DevBuf<float> d_Xw, d_obs, d_Tin, d_poses;
    DevBuf<BaProb> d_probs;
    DevBuf<uint8_t> d_mask;
    DevBuf<BaRes> d_res;
    // rgbd_pnp_solver_frames
    DevBuf<rgbd_dmatch> d_matches;
    DevBuf<int> d_counts, d_pairs, d_err;
    // rgbd_debug_pnp_solver
    DevBuf<BaRound> d_rounds;
    DevBuf<double> d_chi2;
    DevBuf<uint8_t> d_level;
};

void pnpba_free(rgbd_ctx* c)
{
    delete c->pnpba;
    c->pnpba = nullptr;
}

}  // namespace rgbd

namespace {

const rgbd_pnp_solver_params kBaDefaults{4, 10, 5.991, 3, 10};

// the parameters as the kernel reads them; false when they are out of range
bool make_prm(const rgbd_pnp_solver_params* in, BaPrm* p)
{
    const rgbd_pnp_solver_params& q = in ? *in : kBaDefaults;
    if (q.rounds < 1 || q.rounds > kBaMaxRounds || q.iterations < 1 || !std::isfinite(q.chi2_threshold) || !(q.chi2_threshold > 0))
        return false;
    p->rounds = q.rounds;
    p->iterations = q.iterations;
    p->robust_rounds = q.robust_rounds;
    p->min_edges = q.min_edges;
    p->chi2_threshold = q.chi2_threshold;
    p->delta = std::sqrt(q.chi2_threshold);
    p->delta2 = p->delta * p->delta;
    return true;
}

BaWS* ws_get(rgbd_ctx* c)
{
    if (!c->pnpba) c->pnpba = new BaWS();
    return c->pnpba;
}

rgbd_status ws_edges(rgbd_ctx* c, BaWS* w, size_t nedges, size_t P)
{
    rgbd_status s = check_hip(c, w->d_Xw.reserve(3 * nedges), "pnp solver Xw");
    if (!s) s = check_hip(c, w->d_obs.reserve(2 * nedges), "pnp solver obs");
    if (!s) s = check_hip(c, w->d_mask.reserve(nedges), "pnp solver mask");
    if (!s) s = check_hip(c, w->d_Tin.reserve(16 * P), "pnp solver poses");
    if (!s) s = check_hip(c, w->d_probs.reserve(P), "pnp solver problems");
    if (!s) s = check_hip(c, w->d_res.reserve(P), "pnp solver results");
    return s;
}

struct BaDebugOut {
    double* est;       // [rounds][7]
    int32_t* iters;    // [rounds]
    int32_t* trials;   // [rounds]
    double* lam;       // [rounds]
    double* nu;        // [rounds]
    double* chi2;      // [rounds][M]
    uint8_t* level;    // [rounds][M]
    int32_t* rounds_run;
};

// P concatenated problems from host buffers: upload, one launch, read back.  Results are written for the
// problems with ok = 1 only.  dbg (one problem) may be null.
rgbd_status solve_host(rgbd_ctx* c, int P, const int32_t* counts, const float* Xw, const float* obs, const float* K4,
                       const float* Tcw_in, const rgbd_pnp_solver_params* prm_in, float* Tcw_out, uint8_t* masks,
                       int32_t* n_inliers, int32_t* ok, const BaDebugOut* dbg)
{
    if (!c || P < 0) return RGBD_ERR_ARG;
    if (P > 0 && (!counts || !K4 || !Tcw_in || !Tcw_out || !n_inliers || !ok)) return fail(c, RGBD_ERR_ARG, "pnp solver: null argument");
    BaPrm prm{};
    if (!make_prm(prm_in, &prm)) return fail(c, RGBD_ERR_ARG, "pnp solver: rounds in [1, 16], iterations >= 1 and a finite chi2_threshold > 0");
    size_t nedges = 0;
    int max_m = 0;
    for (int p = 0; p < P; p++) {
        if (counts[p] < 0) return fail(c, RGBD_ERR_ARG, "pnp solver: negative edge count");
        if (counts[p] > kPnpMaxM) return fail(c, RGBD_ERR_UNSUPPORTED, "pnp solver: more than 4096 edges per problem");
        nedges += (size_t)counts[p];
        max_m = std::max(max_m, counts[p]);
    }
    if (nedges > 0 && (!Xw || !obs || !masks)) return fail(c, RGBD_ERR_ARG, "pnp solver: null edge arrays");
    if (P == 0) return RGBD_OK;
    if (max_m < 3) {   // nothing to launch: every problem returns false
        for (int p = 0; p < P; p++) ok[p] = 0;
        if (dbg) *dbg->rounds_run = 0;
        return RGBD_OK;
    }
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    BaWS* w = ws_get(c);
    if ((s = ws_edges(c, w, nedges, (size_t)P))) return s;
    const size_t M0 = (size_t)counts[0];
    if (dbg) {
        s = check_hip(c, w->d_rounds.reserve((size_t)prm.rounds), "pnp solver debug rounds");
        if (!s) s = check_hip(c, w->d_chi2.reserve((size_t)prm.rounds * M0), "pnp solver debug chi2");
        if (!s) s = check_hip(c, w->d_level.reserve((size_t)prm.rounds * M0), "pnp solver debug levels");
        if (s) return s;
    }
    std::vector<BaProb> probs(P);
    size_t off = 0;
    for (int p = 0; p < P; p++) {
        probs[p] = BaProb{(int)off, counts[p]};
        off += (size_t)counts[p];
    }
    const hipStream_t st = c->stream;
    s = check_hip(c, hipMemcpyAsync(w->d_Xw, Xw, nedges * 12, hipMemcpyHostToDevice, st), "pnp solver Xw up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_obs, obs, nedges * 8, hipMemcpyHostToDevice, st), "pnp solver obs up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_Tin, Tcw_in, (size_t)P * 64, hipMemcpyHostToDevice, st), "pnp solver poses up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_probs, probs.data(), (size_t)P * sizeof(BaProb), hipMemcpyHostToDevice, st), "pnp solver problems up");
    if (!s && dbg) s = check_hip(c, hipMemsetAsync(w->d_rounds, 0, (size_t)prm.rounds * sizeof(BaRound), st), "pnp solver debug clear");
    if (!s && dbg) s = check_hip(c, hipMemsetAsync(w->d_chi2, 0, (size_t)prm.rounds * M0 * 8, st), "pnp solver debug clear");
    if (!s && dbg) s = check_hip(c, hipMemsetAsync(w->d_level, 0, (size_t)prm.rounds * M0, st), "pnp solver debug clear");
    if (s) return s;
    const BaCam K{(double)K4[0], (double)K4[1], (double)K4[2], (double)K4[3]};
    const int tk = timer_begin(c, "k_pnpba");
    RGBD_TRY(c, launch_pnpba(w->d_Xw, w->d_obs, w->d_probs, w->d_Tin, K, prm, max_m, P, w->d_mask, w->d_res,
                             dbg ? w->d_rounds.get() : nullptr, dbg ? w->d_chi2.get() : nullptr,
                             dbg ? w->d_level.get() : nullptr, (int)M0, st), "pnpba");
    timer_end(c, tk);
    std::vector<BaRes> res(P);
    std::vector<uint8_t> hm(nedges);
    std::vector<BaRound> hr(dbg ? prm.rounds : 0);
    s = check_hip(c, hipMemcpyAsync(res.data(), w->d_res, (size_t)P * sizeof(BaRes), hipMemcpyDeviceToHost, st), "pnp solver results");
    if (!s) s = check_hip(c, hipMemcpyAsync(hm.data(), w->d_mask, nedges, hipMemcpyDeviceToHost, st), "pnp solver masks");
    if (!s && dbg) {
        s = check_hip(c, hipMemcpyAsync(hr.data(), w->d_rounds, hr.size() * sizeof(BaRound), hipMemcpyDeviceToHost, st), "pnp solver debug rounds");
        if (!s) s = check_hip(c, hipMemcpyAsync(dbg->chi2, w->d_chi2, (size_t)prm.rounds * M0 * 8, hipMemcpyDeviceToHost, st), "pnp solver debug chi2");
        if (!s) s = check_hip(c, hipMemcpyAsync(dbg->level, w->d_level, (size_t)prm.rounds * M0, hipMemcpyDeviceToHost, st), "pnp solver debug levels");
    }
    if (!s) s = check_hip(c, hipStreamSynchronize(st), "sync");
    if (s) return s;
    for (int p = 0; p < P; p++) {
        ok[p] = res[p].ok;
        if (!res[p].ok) continue;
        std::memcpy(Tcw_out + 16 * (size_t)p, res[p].T, 64);
        n_inliers[p] = res[p].n_inliers;
        if (counts[p] > 0) std::memcpy(masks + probs[p].off, hm.data() + probs[p].off, (size_t)counts[p]);
    }
    if (dbg) {
        *dbg->rounds_run = res[0].ok ? res[0].rounds_run : 0;
        for (int r = 0; r < prm.rounds; r++) {
            std::memcpy(dbg->est + 7 * (size_t)r, hr[r].est, 56);
            dbg->iters[r] = hr[r].iters;
            dbg->trials[r] = hr[r].trials;
            dbg->lam[r] = hr[r].lam;
            dbg->nu[r] = hr[r].nu;
        }
    }
    return RGBD_OK;
}

}  // namespace

extern "C" {

rgbd_status rgbd_pnp_solver_batch(rgbd_ctx* c, int32_t P, const int32_t* counts, const float* Xw, const float* obs,
                                  const float* K4, const float* Tcw_in, const rgbd_pnp_solver_params* prm, float* Tcw_out,
                                  uint8_t* masks, int32_t* n_inliers, int32_t* ok)
{
    return solve_host(c, P, counts, Xw, obs, K4, Tcw_in, prm, Tcw_out, masks, n_inliers, ok, nullptr);
}

rgbd_status rgbd_pnp_solver(rgbd_ctx* c, const float* Xw, const float* obs, int32_t M, const float* K4, const float* Tcw_in,
                            const rgbd_pnp_solver_params* prm, float* Tcw_out, uint8_t* outlier_mask, int32_t* n_inliers,
                            int32_t* ok)
{
    return solve_host(c, 1, &M, Xw, obs, K4, Tcw_in, prm, Tcw_out, outlier_mask, n_inliers, ok, nullptr);
}

rgbd_status rgbd_debug_pnp_solver(rgbd_ctx* c, const float* Xw, const float* obs, int32_t M, const float* K4,
                                  const float* Tcw_in, const rgbd_pnp_solver_params* prm, float* Tcw_out,
                                  uint8_t* outlier_mask, int32_t* n_inliers, int32_t* ok, int32_t* rounds_run,
                                  double* round_est, int32_t* round_iters, int32_t* round_trials, double* round_lambda,
                                  double* round_nu, double* edge_chi2, uint8_t* edge_level)
{
    if (!c) return RGBD_ERR_ARG;
    if (!rounds_run || !round_est || !round_iters || !round_trials || !round_lambda || !round_nu || (M > 0 && (!edge_chi2 || !edge_level)))
        return fail(c, RGBD_ERR_ARG, "pnp solver debug: null output");
    const BaDebugOut d{round_est, round_iters, round_trials, round_lambda, round_nu, edge_chi2, edge_level, rounds_run};
    return solve_host(c, 1, &M, Xw, obs, K4, Tcw_in, prm, Tcw_out, outlier_mask, n_inliers, ok, &d);
}

rgbd_status rgbd_pnp_solver_frames(rgbd_ctx* c, int32_t P, const int32_t* qframe, const int32_t* tframe, const float* poses,
                                   const rgbd_dmatch* matches, const int32_t* counts, int32_t as_written,
                                   const rgbd_pnp_solver_params* prm_in, float* Tcw_out, uint8_t* masks, int32_t* n_inliers,
                                   int32_t* ok)
{
    if (!c || P < 0) return RGBD_ERR_ARG;
    if (P > 0 && (!qframe || !tframe || !poses || !matches || !counts || !Tcw_out || !masks || !n_inliers || !ok))
        return fail(c, RGBD_ERR_ARG, "pnp solver frames: null argument");
    BaPrm prm{};
    if (!make_prm(prm_in, &prm)) return fail(c, RGBD_ERR_ARG, "pnp solver: rounds in [1, 16], iterations >= 1 and a finite chi2_threshold > 0");
    const int B = c->last_B, K = c->cfg.kp_cap;
    if (B < 1) return fail(c, RGBD_ERR_ARG, "pnp solver frames: no extracted batch");
    int max_m = 0;
    for (int p = 0; p < P; p++) {
        if (qframe[p] >= B || (qframe[p] >= 0 && (tframe[p] < 0 || tframe[p] >= B)))
            return fail(c, RGBD_ERR_ARG, "pnp solver frames: frame index outside the last batch");
        if (qframe[p] < 0) continue;
        if (counts[p] < 0 || counts[p] > K) return fail(c, RGBD_ERR_ARG, "pnp solver frames: match count outside [0, kp_cap]");
        if (counts[p] > kPnpMaxM) return fail(c, RGBD_ERR_UNSUPPORTED, "pnp solver: more than 4096 edges per problem");
        max_m = std::max(max_m, counts[p]);
    }
    if (P == 0) return RGBD_OK;
    if (max_m < 3) {   // every pair skipped or short: nothing to launch
        for (int p = 0; p < P; p++) ok[p] = 0;
        return RGBD_OK;
    }
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    if ((s = order_after_extraction(c))) return s;
    BaWS* w = ws_get(c);
    const size_t PK = (size_t)P * K;
    if ((s = ws_edges(c, w, PK, (size_t)P))) return s;
    s = check_hip(c, w->d_matches.reserve(PK), "pnp solver matches");
    if (!s) s = check_hip(c, w->d_counts.reserve((size_t)P), "pnp solver counts");
    if (!s) s = check_hip(c, w->d_pairs.reserve(2 * (size_t)P), "pnp solver pairs");
    if (!s) s = check_hip(c, w->d_poses.reserve(16 * (size_t)B), "pnp solver frame poses");
    if (!s) s = check_hip(c, w->d_err.reserve(1), "pnp solver flag");
    if (s) return s;
    const hipStream_t st = c->stream;
    s = check_hip(c, hipMemcpyAsync(w->d_matches, matches, PK * sizeof(rgbd_dmatch), hipMemcpyHostToDevice, st), "pnp solver matches up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_counts, counts, (size_t)P * 4, hipMemcpyHostToDevice, st), "pnp solver counts up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_pairs, qframe, (size_t)P * 4, hipMemcpyHostToDevice, st), "pnp solver pairs up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_pairs + P, tframe, (size_t)P * 4, hipMemcpyHostToDevice, st), "pnp solver pairs up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->d_poses, poses, (size_t)B * 64, hipMemcpyHostToDevice, st), "pnp solver poses up");
    if (!s) s = check_hip(c, hipMemsetAsync(w->d_err, 0, 4, st), "pnp solver flag clear");
    if (s) return s;
    int tk = timer_begin(c, "k_pnpba_gather");
    RGBD_TRY(c, launch_pnpba_gather(w->d_matches, w->d_counts, w->d_pairs, w->d_pairs + P, w->d_poses, c->out.xyz, c->out.kun, K,
                                    as_written ? 1 : 0, P, w->d_Xw, w->d_obs, w->d_probs, w->d_Tin, w->d_err, st), "pnpba_gather");
    timer_end(c, tk);
    const BaCam Kc{(double)c->cam.fx, (double)c->cam.fy, (double)c->cam.cx, (double)c->cam.cy};
    tk = timer_begin(c, "k_pnpba");
    RGBD_TRY(c, launch_pnpba(w->d_Xw, w->d_obs, w->d_probs, w->d_Tin, Kc, prm, max_m, P, w->d_mask, w->d_res, nullptr, nullptr,
                             nullptr, 0, st), "pnpba");
    timer_end(c, tk);
    std::vector<BaRes> res(P);
    std::vector<uint8_t> hm(PK);
    int err = 0;
    s = check_hip(c, hipMemcpyAsync(res.data(), w->d_res, (size_t)P * sizeof(BaRes), hipMemcpyDeviceToHost, st), "pnp solver results");
    if (!s) s = check_hip(c, hipMemcpyAsync(hm.data(), w->d_mask, PK, hipMemcpyDeviceToHost, st), "pnp solver masks");
    if (!s) s = check_hip(c, hipMemcpyAsync(&err, w->d_err, 4, hipMemcpyDeviceToHost, st), "pnp solver flag");
    if (!s) s = check_hip(c, hipStreamSynchronize(st), "sync");
    if (s) return s;
    if (err) return fail(c, RGBD_ERR_ARG, "pnp solver frames: a match index outside [0, kp_cap)");
    for (int p = 0; p < P; p++) {
        ok[p] = res[p].ok;
        if (!res[p].ok) continue;
        std::memcpy(Tcw_out + 16 * (size_t)p, res[p].T, 64);
        n_inliers[p] = res[p].n_inliers;
        std::memcpy(masks + (size_t)p * K, hm.data() + (size_t)p * K, (size_t)counts[p]);
    }
    return RGBD_OK;
}

}  // extern "C"
