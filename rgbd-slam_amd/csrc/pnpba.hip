// pnpba.hip -- motion-only bundle adjustment, PnPSolver::compute (Solver/PnPSolver.cpp:31-150), on gfx950.
// Operator: DESIGN.md "Motion-only BA definition" (tests/pnp_solver_model.py is the same text as numpy).
//
//   k_pnpba         one 256-thread workgroup per problem; the whole rounds x iterations x trials loop of the
//                   Levenberg-Marquardt schedule runs inside the one launch.  The edges (Xw, obs as floats) are
//                   staged in LDS once.  One pass = every lane evaluates its edges l, l + 256, ... at the pose in
//                   LDS and adds their 28 terms in sequence, the 16-lane rows are reduced on DPP, lanes 0..27 of
//                   wave 0 add the 16 row sums, and thread 0 runs the serial part (accept / reject, Cholesky,
//                   exponential) and publishes the next pose.  Every pass evaluates all 28 sums, so an accepted
//                   trial's H, b and chi are the next iteration's: an iteration costs one pass per trial.
//   k_pnpba_gather  the edges of rgbd_pnp_solver_frames from the last extraction's outputs and the match lists.
//
// Control flow is decided once per pass by thread 0 and read by everyone from LDS.  Two workgroup barriers per
// pass order every shared word: thread 0 writes ctl / Rt only between barrier A (after the row sums are stored)
// and barrier B; every other thread reads them only between B and the next A.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "dispatch.h"
#include "pnp_dev.h"
#include "pnpba_dev.h"
#include "wave_dev.h"

namespace rgbd {

namespace {

enum { kCtlEval = 0, kCtlDone = 1 };

struct BaLds {
    double red[kBaSums * 16];   // row sums: [term][row]
    double sums[kBaSums];       // the pass's 28 sums
    double Rt[12];              // the pose the next pass evaluates; at a round's end the last pose evaluated
    double Rtf[12];             // at a round's end: the round's final estimate
    BaEst est_in;
    int ctl;
    int n_in;                   // level-0 edges after the last classification
};

// x of lane l - S within each 16-lane row (DPP row_shr:S), 0 where the row has no such lane; after the levels
// S = 1, 2, 4, 8 lane 15 of a row holds the row's natural-order binary tree
template <int S>
__device__ __forceinline__ double ba_row_shr(double x)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(u & 0xFFFFFFFFull), 0x110 + S, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(u >> 32), 0x110 + S, 0xF, 0xF, false);
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// A problem's edges as the passes read them: the LDS stage [M][5] = Xw, obs.  RGBD_BA_EDGES_GLOBAL (experiment
// builds, profiles/pnp_solver/README.md) reads the global rows again in every pass instead.
struct BaEdges {
    const float* lds;
    const float* Xw;
    const float* obs;
};

__device__ __forceinline__ void ba_edge(const BaEdges& E, int i, float* ed)
{
#ifdef RGBD_BA_EDGES_GLOBAL
    ed[0] = E.Xw[3 * i]; ed[1] = E.Xw[3 * i + 1]; ed[2] = E.Xw[3 * i + 2];
    ed[3] = E.obs[2 * i]; ed[4] = E.obs[2 * i + 1];
#else
#pragma unroll
    for (int k = 0; k < 5; k++) ed[k] = E.lds[5 * i + k];
#endif
}

// p = R Xw + t and the raw chi2 of edge i
__device__ __forceinline__ double ba_chi2(const BaEdges& E, int i, const double* Rt, const BaCam& K, double* p, double* ex, double* ey)
{
    float ed[5];
    ba_edge(E, i, ed);
    const double X = (double)ed[0], Y = (double)ed[1], Z = (double)ed[2];
    p[0] = ((Rt[0] * X + Rt[1] * Y) + Rt[2] * Z) + Rt[9];
    p[1] = ((Rt[3] * X + Rt[4] * Y) + Rt[5] * Z) + Rt[10];
    p[2] = ((Rt[6] * X + Rt[7] * Y) + Rt[8] * Z) + Rt[11];
    *ex = (double)ed[3] - ((p[0] / p[2]) * K.fx + K.cx);
    *ey = (double)ed[4] - ((p[1] / p[2]) * K.fy + K.cy);
    return *ex * *ex + *ey * *ey;
}

// one pass: the 28 sums over the lane's active edges (bit j of `inactive` = edge tid + 256 j is at level 1) at
// L.Rt, left in L.sums for wave 0.  Ends after barrier A; the caller's barrier B follows thread 0's serial part.
__device__ __forceinline__ void ba_pass(BaLds& L, const BaEdges& edges, int M, unsigned inactive, const BaCam& K, bool robust,
                                        double delta, double delta2)
{
    const int tid = threadIdx.x, lane = tid & 63;
    double Rt[12];
#pragma unroll
    for (int i = 0; i < 12; i++) Rt[i] = L.Rt[i];
    double acc[kBaSums];
#pragma unroll
    for (int k = 0; k < kBaSums; k++) acc[k] = 0.0;
    for (int i = tid, j = 0; i < M; i += kBaThreads, j++) {
        if ((inactive >> j) & 1u) continue;
        double p[3], ex, ey;
        const double chi2 = ba_chi2(edges, i, Rt, K, p, &ex, &ey);
        const double x = p[0], y = p[1];
        const double iz = 1.0 / p[2];
        const double iz2 = iz * iz;
        const double J0[6] = {((x * y) * iz2) * K.fx, -((1.0 + (x * x) * iz2) * K.fx), (y * iz) * K.fx, -(iz * K.fx), 0.0,
                              (x * iz2) * K.fx};
        const double J1[6] = {(1.0 + (y * y) * iz2) * K.fy, -(((x * y) * iz2) * K.fy), -((x * iz) * K.fy), 0.0, -(iz * K.fy),
                              (y * iz2) * K.fy};
        double rho = chi2, w = 1.0;
        if (robust && !(chi2 <= delta2)) {
            const double s = sqrt(chi2);
            rho = (2.0 * s) * delta - delta2;
            w = delta / s;
        }
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++) acc[k++] += w * (J0[a] * J0[b] + J1[a] * J1[b]);
#pragma unroll
        for (int a = 0; a < 6; a++) acc[k++] += w * (J0[a] * ex + J1[a] * ey);
        acc[27] += rho;
    }
#pragma unroll
    for (int k = 0; k < kBaSums; k++) {
        acc[k] += ba_row_shr<1>(acc[k]);
        acc[k] += ba_row_shr<2>(acc[k]);
        acc[k] += ba_row_shr<4>(acc[k]);
        acc[k] += ba_row_shr<8>(acc[k]);
    }
    if ((lane & 15) == 15)
#pragma unroll
        for (int k = 0; k < kBaSums; k++) L.red[k * 16 + (tid >> 4)] = acc[k];
    __syncthreads();   // barrier A
    if (tid < 64) {
        if (tid < kBaSums) {
            double r[16];
#pragma unroll
            for (int i = 0; i < 16; i++) r[i] = L.red[tid * 16 + i];
#pragma unroll
            for (int s2 = 1; s2 < 16; s2 <<= 1)
#pragma unroll
                for (int i = 0; i < 16; i += 2 * s2) r[i] += r[i + s2];
            L.sums[tid] = r[0];
        }
        wave_lds_sync();
    }
}

}  // namespace

__global__ __launch_bounds__(kBaThreads) void k_pnpba(const float* __restrict__ Xw, const float* __restrict__ obs,
                                                      const BaProb* __restrict__ probs, const float* __restrict__ Tin,
                                                      BaCam K, BaPrm prm,
                                                      uint8_t* __restrict__ mask, BaRes* __restrict__ res,
                                                      BaRound* __restrict__ dbg_rounds, double* __restrict__ dbg_chi2,
                                                      uint8_t* __restrict__ dbg_level, int dbg_stride)
{
    extern __shared__ __align__(16) unsigned char ba_dyn[];
    __shared__ BaLds L;
    float* stage = reinterpret_cast<float*>(ba_dyn);   // [M][5]: Xw, obs
    const int tid = threadIdx.x, pb = blockIdx.x;
    const BaProb pr = probs[pb];
    const int M = pr.count;
    if (M < 3) {   // uniform: PnPSolver.cpp:99-100
        if (tid == 0) res[pb].ok = 0;
        return;
    }
    const BaEdges edges{stage, Xw + 3 * (size_t)pr.off, obs + 2 * (size_t)pr.off};
#ifndef RGBD_BA_EDGES_GLOBAL
    for (int i = tid; i < M; i += kBaThreads) {
        float* e = stage + 5 * i;
        e[0] = edges.Xw[3 * i]; e[1] = edges.Xw[3 * i + 1]; e[2] = edges.Xw[3 * i + 2];
        e[3] = edges.obs[2 * i]; e[4] = edges.obs[2 * i + 1];
    }
#endif
    // thread 0's serial state
    BaEst est{}, trial{};
    double cur[kBaSums];   // the sums at est
    double lam = 0.0, nu = 2.0, chi = 0.0, scale = 1e-3;
    int it = 0, ntr = 0, trials = 0;
    bool last_is_trial = false;
    if (tid == 0) {
        ba_from_pose(Tin + 16 * (size_t)pb, &est);
        L.est_in = est;
        L.n_in = M;
    }
    unsigned inactive = 0;   // bit j: edge tid + 256 j is at level 1
    int rounds_run = 0;
    __syncthreads();
    for (int rnd = 0; rnd < prm.rounds; rnd++) {
        const bool robust = rnd < prm.robust_rounds;
        const int n_act = L.n_in;   // uniform: written before the barrier that ended the last round
        if (tid == 0) {
            est = L.est_in;         // every round restarts from Tcw_in (PnPSolver.cpp:103)
            ba_Rt(est, L.Rt);
            L.ctl = n_act > 0 ? kCtlEval : kCtlDone;
            it = ntr = trials = 0;
            last_is_trial = false;
        }
        __syncthreads();   // barrier B of the round's first pass
        bool first = true;
        while (L.ctl == kCtlEval) {
            ba_pass(L, edges, M, inactive, K, robust, prm.delta, prm.delta2);
            if (tid == 0) {
                bool done = false, solved = true;   // solved: L.sums holds an evaluation (of est when first, else of trial)
                for (;;) {
                    if (first) {
#pragma unroll
                        for (int k = 0; k < kBaSums; k++) cur[k] = L.sums[k];
                        chi = cur[27];
                        double m = 0.0;
                        const int dg[6] = {0, 6, 11, 15, 18, 20};
#pragma unroll
                        for (int a = 0; a < 6; a++)
                            if (fabs(cur[dg[a]]) > m) m = fabs(cur[dg[a]]);
                        lam = 1e-5 * m;
                        first = false;
                    } else {
                        const double chi_new = solved ? L.sums[27] : DBL_MAX;
                        const double rho = (chi - chi_new) / scale;
                        ntr++;
                        trials++;
                        if (rho > 0 && isfinite(chi_new)) {
                            if (solved) {
                                est = trial;
#pragma unroll
                                for (int k = 0; k < kBaSums; k++) cur[k] = L.sums[k];
                                last_is_trial = false;
                            }
                            const double tmp = 2.0 * rho - 1.0;
                            double alpha = 1.0 - (tmp * tmp) * tmp;
                            if (2.0 / 3.0 < alpha) alpha = 2.0 / 3.0;
                            if (!(1.0 / 3.0 < alpha)) alpha = 1.0 / 3.0;
                            lam = lam * alpha;
                            nu = 2.0;
                        } else {
                            lam = lam * nu;
                            nu = nu * 2.0;
                            if (solved) last_is_trial = true;
                        }
                        if (!(rho < 0 && ntr < kBaMaxTrials)) {   // the iteration ends
                            it++;
                            if (ntr == kBaMaxTrials || rho == 0 || !isfinite(lam) || it == prm.iterations) {
                                done = true;
                                break;
                            }
                            // the next iteration evaluates at est again: the sums it would get are cur
                            ntr = 0;
                            chi = cur[27];
                            last_is_trial = false;
                        }
                    }
                    double d[6];
                    solved = ba_chol_solve(cur, lam, d);
                    if (!solved) {
                        scale = 1e-3;
                        continue;
                    }
                    ba_exp_times(d, est, &trial);
                    double sc = 0.0;
#pragma unroll
                    for (int a = 0; a < 6; a++) sc = sc + d[a] * (lam * d[a] + (-cur[21 + a]));
                    scale = sc + 1e-3;
                    break;
                }
                if (done) {
                    // L.Rt stays the last pose evaluated when that was a rejected trial
                    if (!last_is_trial) ba_Rt(est, L.Rt);
                    L.ctl = kCtlDone;
                } else {
                    ba_Rt(trial, L.Rt);
                }
            }
            first = false;
            __syncthreads();   // barrier B
        }
        // ---- classification (PnPSolver.cpp:107-129): an active edge on the last evaluation, the others at the estimate
        if (tid == 0) {
            ba_Rt(est, L.Rtf);
            L.n_in = 0;
        }
        __syncthreads();
        {
            double Ra[12], Rf[12];
#pragma unroll
            for (int i = 0; i < 12; i++) { Ra[i] = L.Rt[i]; Rf[i] = L.Rtf[i]; }
            int n0 = 0;
            for (int i = tid, j = 0; i < M; i += kBaThreads, j++) {
                const bool act = !((inactive >> j) & 1u);
                double p[3], ex, ey;
                const double chi2 = ba_chi2(edges, i, act ? Ra : Rf, K, p, &ex, &ey);
                const bool out = chi2 > prm.chi2_threshold;
                inactive = out ? (inactive | (1u << j)) : (inactive & ~(1u << j));
                n0 += out ? 0 : 1;
                if (dbg_chi2) {
                    dbg_chi2[((size_t)pb * prm.rounds + rnd) * dbg_stride + i] = chi2;
                    dbg_level[((size_t)pb * prm.rounds + rnd) * dbg_stride + i] = out ? 1 : 0;
                }
            }
            if (n0) atomicAdd(&L.n_in, n0);
        }
        if (tid == 0 && dbg_rounds) {
            BaRound& r = dbg_rounds[(size_t)pb * prm.rounds + rnd];
#pragma unroll
            for (int i = 0; i < 4; i++) r.est[i] = est.q[i];
#pragma unroll
            for (int i = 0; i < 3; i++) r.est[4 + i] = est.t[i];
            r.lam = lam;
            r.nu = nu;
            r.iters = it;
            r.trials = trials;
        }
        rounds_run = rnd + 1;
        __syncthreads();   // n_in complete; Rt / Rtf / ctl free for the next round
        if (M < prm.min_edges) break;   // PnPSolver.cpp:131-132
    }
    for (int i = tid, j = 0; i < M; i += kBaThreads, j++) mask[pr.off + i] = (inactive >> j) & 1u;
    if (tid == 0) {
        BaRes& r = res[pb];
        double Rt[12];
        ba_Rt(est, Rt);
#pragma unroll
        for (int a = 0; a < 3; a++) {
#pragma unroll
            for (int b = 0; b < 3; b++) r.T[4 * a + b] = (float)Rt[3 * a + b];
            r.T[4 * a + 3] = (float)Rt[9 + a];
        }
        r.T[12] = r.T[13] = r.T[14] = 0.0f;
        r.T[15] = 1.0f;
        r.n_inliers = L.n_in;
        r.ok = 1;
        r.rounds_run = rounds_run;
    }
}

// Edges of pair p from the last extraction: obs = the train frame's undistorted keypoint, Xw = unprojectWorld of
// the train frame's own point (as_written, PnPSolver.cpp:65) or of the query frame's; the guess = the train
// frame's pose.  Rows [p K, p K + counts[p]) of the edge arrays; an index outside [0, K) raises *err.
__global__ __launch_bounds__(256) void k_pnpba_gather(const rgbd_dmatch* __restrict__ matches, const int* __restrict__ counts,
                                                      const int* __restrict__ qf, const int* __restrict__ tf,
                                                      const float* __restrict__ poses, const float* __restrict__ xyz,
                                                      const float* __restrict__ kun, int K, int as_written,
                                                      float* __restrict__ Xw, float* __restrict__ obs,
                                                      BaProb* __restrict__ probs, float* __restrict__ Tin, int* __restrict__ err)
{
    const int p = blockIdx.x, tid = threadIdx.x;
    const int q = qf[p];
    const int n = q < 0 ? 0 : counts[p];
    if (tid == 0) probs[p] = BaProb{p * K, n};
    if (q < 0) return;
    const int t = tf[p];
    if (tid < 16) Tin[16 * (size_t)p + tid] = poses[16 * (size_t)t + tid];
    const int src = as_written ? t : q;
    const float* T = poses + 16 * (size_t)src;
    for (int i = tid; i < n; i += 256) {
        const rgbd_dmatch m = matches[(size_t)p * K + i];
        const size_t o = (size_t)p * K + i;
        if ((unsigned)m.queryIdx >= (unsigned)K || (unsigned)m.trainIdx >= (unsigned)K) {
            *err = 1;
            Xw[3 * o] = Xw[3 * o + 1] = Xw[3 * o + 2] = 0.0f;
            obs[2 * o] = obs[2 * o + 1] = 0.0f;
            continue;
        }
        const int pi = as_written ? m.trainIdx : m.queryIdx;
        const float* X = xyz + ((size_t)src * K + pi) * 3;
        const float Xc[3] = {X[0], X[1], X[2]};
        float xw[3];
        ba_unproject_world(T, Xc, xw);
        Xw[3 * o] = xw[0]; Xw[3 * o + 1] = xw[1]; Xw[3 * o + 2] = xw[2];
        const float* u = kun + ((size_t)t * K + m.trainIdx) * 7;
        obs[2 * o] = u[0];
        obs[2 * o + 1] = u[1];
    }
}

hipError_t launch_pnpba(const float* Xw, const float* obs, const BaProb* probs, const float* Tin, const BaCam& K,
                        const BaPrm& prm, int max_m, int P, uint8_t* mask, BaRes* res, BaRound* dbg_rounds,
                        double* dbg_chi2, uint8_t* dbg_level, int dbg_stride, hipStream_t st)
{
    if (max_m < 0 || max_m > kPnpMaxM) return hipErrorInvalidValue;
    const size_t lds = (size_t)(max_m > 0 ? max_m : 1) * 5 * sizeof(float);
    return dispatch(k_pnpba, dim3(P), dim3(kBaThreads), lds, st, Xw, obs, probs, Tin, K, prm, mask, res,
                    dbg_rounds, dbg_chi2, dbg_level, dbg_stride);
}

hipError_t launch_pnpba_gather(const rgbd_dmatch* matches, const int* counts, const int* qf, const int* tf, const float* poses,
                               const float* xyz, const float* kun, int K, int as_written, int P, float* Xw, float* obs,
                               BaProb* probs, float* Tin, int* err, hipStream_t st)
{
    return dispatch(k_pnpba_gather, dim3(P), dim3(256), 0, st, matches, counts, qf, tf, poses, xyz, kun, K, as_written, Xw,
                    obs, probs, Tin, err);
}

}  // namespace rgbd
