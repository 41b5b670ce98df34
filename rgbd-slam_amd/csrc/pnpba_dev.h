// pnpba_dev.h -- the motion-only bundle adjustment of PnPSolver::compute (Solver/PnPSolver.cpp:31-150): argument
// blocks shared by pnpba.hip and pnpba_host.cpp, and the serial f64 pieces of DESIGN.md "Motion-only BA
// definition" (quaternion estimate, g2o's SE3Quat::exp, the unpivoted 6 x 6 Cholesky), each a literal restatement
// of that text: the operation order here is the definition's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rgbd_hip.h"
#include "gn6_dev.h"

namespace rgbd {

constexpr int kBaThreads = 256;    // lanes of the strided sums
constexpr int kBaSums = 28;        // 21 of H (upper, row-major), 6 of sum w J^T err, sum rho
constexpr int kBaMaxTrials = 10;   // g2o's maxTrialsAfterFailure
constexpr int kBaMaxRounds = 16;   // rounds a call may ask for

struct BaPrm {
    int rounds, iterations, robust_rounds, min_edges;
    double chi2_threshold, delta, delta2;   // delta = sqrt(threshold), delta2 = delta * delta
};

struct BaCam { double fx, fy, cx, cy; };   // K4 widened

struct BaProb { int off, count; };   // a problem's edges: rows [off, off + count) of the edge arrays

struct BaRes {
    float T[16];
    int n_inliers, ok, rounds_run, pad;
};

// per problem and round (rgbd_debug_pnp_solver)
struct BaRound {
    double est[7];   // qx qy qz qw tx ty tz
    double lam, nu;
    int iters, trials;
};

struct BaEst { double q[4], t[3]; };   // g2o's SE3Quat: unit quaternion (x y z w), translation

// the branch of Eigen's Quaterniond(Matrix3d) for a non-positive trace, largest diagonal entry I (static indices)
template <int I>
__device__ __forceinline__ void ba_quat_branch(const double* m, double* q)
{
    constexpr int J = (I + 1) % 3, K = (I + 2) % 3;
    double s = sqrt(((m[4 * I] - m[4 * J]) - m[4 * K]) + 1.0);
    q[I] = 0.5 * s;
    s = 0.5 / s;
    q[3] = (m[3 * K + J] - m[3 * J + K]) * s;
    q[J] = (m[3 * J + I] + m[3 * I + J]) * s;
    q[K] = (m[3 * K + I] + m[3 * I + K]) * s;
}

// Eigen's Quaterniond(Matrix3d); m row-major
__device__ inline void ba_quat_from_R(const double* m, double* q)
{
    const double t = (m[0] + m[4]) + m[8];
    if (t > 0) {
        double s = sqrt(t + 1.0);
        q[3] = 0.5 * s;
        s = 0.5 / s;
        q[0] = (m[7] - m[5]) * s;
        q[1] = (m[2] - m[6]) * s;
        q[2] = (m[3] - m[1]) * s;
        return;
    }
    int i = 0;
    double mii = m[0];
    if (m[4] > mii) { i = 1; mii = m[4]; }
    if (m[8] > mii) i = 2;
    if (i == 0) ba_quat_branch<0>(m, q);
    else if (i == 1) ba_quat_branch<1>(m, q);
    else ba_quat_branch<2>(m, q);
}

// SE3Quat::normalizeRotation: the sign first (w >= 0), then every component divided by the norm
__device__ inline void ba_normalize(double* q)
{
    if (q[3] < 0)
#pragma unroll
        for (int i = 0; i < 4; i++) q[i] = -q[i];
    const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = q[i] / n;
}

// Eigen's Quaterniond::toRotationMatrix, then t: Rt[12] = R row-major, t
__device__ inline void ba_Rt(const BaEst& e, double* Rt)
{
    const double x = e.q[0], y = e.q[1], z = e.q[2], w = e.q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    Rt[0] = 1.0 - (tyy + tzz); Rt[1] = txy - twz;         Rt[2] = txz + twy;
    Rt[3] = txy + twz;         Rt[4] = 1.0 - (txx + tzz); Rt[5] = tyz - twx;
    Rt[6] = txz - twy;         Rt[7] = tyz + twx;         Rt[8] = 1.0 - (txx + tyy);
    Rt[9] = e.t[0]; Rt[10] = e.t[1]; Rt[11] = e.t[2];
}

// Converter::toSE3Quat of a float row-major 4 x 4
__device__ inline void ba_from_pose(const float* T, BaEst* e)
{
    double R[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) R[3 * r + c] = (double)T[4 * r + c];
        e->t[r] = (double)T[4 * r + 3];
    }
    ba_quat_from_R(R, e->q);
    ba_normalize(e->q);
}

// out = exp(d) * e with g2o's SE3Quat::exp, d = (omega, upsilon)
__device__ inline void ba_exp_times(const double* d, const BaEst& e, BaEst* out)
{
    const double wx = d[0], wy = d[1], wz = d[2];
    const double th2 = (wx * wx + wy * wy) + wz * wz;
    const double th = sqrt(th2);
    const double xy = wx * wy, xz = wx * wz, yz = wy * wz;
    const double Om[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
    const double Om2[9] = {-(wy * wy + wz * wz), xy, xz, xy, -(wx * wx + wz * wz), yz, xz, yz, -(wx * wx + wy * wy)};
    double a = 1.0, b = 0.5, c = 1.0 / 6.0;
    if (!(th < 1e-5)) {
        double sn, cs;
        sincos_poly(th, &sn, &cs);
        a = sn / th;
        b = (1.0 - cs) / th2;
        c = (th - sn) / (th2 * th);
    }
    double R[9], V[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const double id = (i % 4 == 0) ? 1.0 : 0.0;
        R[i] = (id + a * Om[i]) + b * Om2[i];
        V[i] = (id + b * Om[i]) + c * Om2[i];
    }
#pragma unroll
    for (int r = 0; r < 3; r++)
        out->t[r] = ((R[3 * r] * e.t[0] + R[3 * r + 1] * e.t[1]) + R[3 * r + 2] * e.t[2]) +
                    ((V[3 * r] * d[3] + V[3 * r + 1] * d[4]) + V[3 * r + 2] * d[5]);
    double qa[4];
    ba_quat_from_R(R, qa);
    ba_normalize(qa);
    const double ax = qa[0], ay = qa[1], az = qa[2], aw = qa[3];
    const double bx = e.q[0], by = e.q[1], bz = e.q[2], bw = e.q[3];
    out->q[0] = ((aw * bx + ax * bw) + ay * bz) - az * by;
    out->q[1] = ((aw * by + ay * bw) + az * bx) - ax * bz;
    out->q[2] = ((aw * bz + az * bw) + ax * by) - ay * bx;
    out->q[3] = ((aw * bw - ax * bx) - ay * by) - az * bz;
    ba_normalize(out->q);
}

// (H + lam I) d = b by unpivoted Cholesky, S = the 28 sums (b = -S[21..26]); false when a pivot is not > 0
__device__ inline bool ba_chol_solve(const double* S, double lam, double* d)
{
    double A[6][6], L[6][6];
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = a; b < 6; b++) {
            A[a][b] = S[k];
            A[b][a] = S[k];
            k++;
        }
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double s = A[j][j] + lam;
#pragma unroll
        for (int m = 0; m < j; m++) s = s - L[j][m] * L[j][m];
        if (!(s > 0)) return false;
        L[j][j] = sqrt(s);
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            s = A[i][j];
#pragma unroll
            for (int m = 0; m < j; m++) s = s - L[i][m] * L[j][m];
            L[i][j] = s / L[j][j];
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = -S[21 + i];
#pragma unroll
        for (int m = 0; m < i; m++) s = s - L[i][m] * y[m];
        y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int m = i + 1; m < 6; m++) s = s - L[m][i] * d[m];
        d[i] = s / L[i][i];
    }
    return true;
}

// Frame::unprojectWorld in float (DESIGN.md "Projection match definition" step 2): mOw = -Rcw^T tcw, then
// Rwc x + mOw as one gemm (double sums in k order, one rounding each)
__device__ inline void ba_unproject_world(const float* T, const float* X, float* xw)
{
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double o = 0.0, a = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            o += (double)T[4 * k + r] * (double)T[4 * k + 3];
            a += (double)T[4 * k + r] * (double)X[k];
        }
        const float Ow = (float)(o * -1.0);
        xw[r] = (float)(a + (double)Ow);
    }
}

// launchers (pnpba.hip).  max_m = the largest edge count of the P problems (sizes the LDS edge stage)
hipError_t launch_pnpba(const float* Xw, const float* obs, const BaProb* probs, const float* Tin, const BaCam& K,
                        const BaPrm& prm, int max_m, int P, uint8_t* mask, BaRes* res, BaRound* dbg_rounds, double* dbg_chi2,
                        uint8_t* dbg_level, int dbg_stride, hipStream_t st);
hipError_t launch_pnpba_gather(const rgbd_dmatch* matches, const int* counts, const int* qf, const int* tf, const float* poses,
                               const float* xyz, const float* kun, int K, int as_written, int P, float* Xw, float* obs,
                               BaProb* probs, float* Tin, int* err, hipStream_t st);

}  // namespace rgbd
