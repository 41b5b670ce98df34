// gn6_dev.h -- the oracle's definitions of the three f64 pieces every 6-parameter Gauss-Newton step here uses:
// sin / cos by range reduction + Taylor polynomials, the Rodrigues exponential of a rotation vector and the
// 6 x 6 solve by Gaussian elimination with partial pivoting.  Shared by GICP's Gauss-Newton (gicp.hip) and
// solvePnPRansac's refinement (pnp.hip): one definition, so both solvers keep the oracle's operations in the
// oracle's order together.  (The two gn_terms are different functions and stay with their solvers.)
#pragma once
#include <hip/hip_runtime.h>

namespace rgbd {

__device__ inline void sincos_poly(double x, double* s_out, double* c_out)
{
    const double PIO2_1 = 1.57079632673412561417e+00, PIO2_1T = 6.07710050650619224932e-11;
    const double INV_PIO2 = 6.36619772367581382433e-01;
    const double kd = floor(x * INV_PIO2 + 0.5);
    const long k = (long)kd;
    const double r = (x - kd * PIO2_1) - kd * PIO2_1T;
    const double r2 = r * r;
    double s = -1.0 / 121645100408832000.0;
    s = s * r2 + 1.0 / 355687428096000.0;
    s = s * r2 - 1.0 / 1307674368000.0;
    s = s * r2 + 1.0 / 6227020800.0;
    s = s * r2 - 1.0 / 39916800.0;
    s = s * r2 + 1.0 / 362880.0;
    s = s * r2 - 1.0 / 5040.0;
    s = s * r2 + 1.0 / 120.0;
    s = s * r2 - 1.0 / 6.0;
    s = s * r2 + 1.0;
    const double sr = s * r;
    double c = -1.0 / 6402373705728000.0;
    c = c * r2 + 1.0 / 20922789888000.0;
    c = c * r2 - 1.0 / 87178291200.0;
    c = c * r2 + 1.0 / 479001600.0;
    c = c * r2 - 1.0 / 3628800.0;
    c = c * r2 + 1.0 / 40320.0;
    c = c * r2 - 1.0 / 720.0;
    c = c * r2 + 1.0 / 24.0;
    c = c * r2 - 0.5;
    c = c * r2 + 1.0;
    switch ((int)(k & 3)) {
    case 0: *c_out = c; *s_out = sr; break;
    case 1: *c_out = -sr; *s_out = c; break;
    case 2: *c_out = -c; *s_out = -sr; break;
    default: *c_out = sr; *s_out = -c; break;
    }
}

__device__ inline void rodrigues_exp(const double w[3], double R[9])
{
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double th = sqrt(th2);
    if (th < 1e-300) {
        for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    double sn, c;
    sincos_poly(th, &sn, &c);
    const double k[3] = {w[0] / th, w[1] / th, w[2] / th};
    const double c1 = 1.0 - c;
    R[0] = c + c1 * k[0] * k[0];         R[1] = c1 * k[0] * k[1] - sn * k[2]; R[2] = c1 * k[0] * k[2] + sn * k[1];
    R[3] = c1 * k[1] * k[0] + sn * k[2]; R[4] = c + c1 * k[1] * k[1];         R[5] = c1 * k[1] * k[2] - sn * k[0];
    R[6] = c1 * k[2] * k[0] - sn * k[1]; R[7] = c1 * k[2] * k[1] + sn * k[0]; R[8] = c + c1 * k[2] * k[2];
}

// H x = -g; false when a pivot is exactly 0 (x is then not written)
__device__ __forceinline__ bool solve6(const double* H, const double* g, double x[6])
{
    double A[6][7];
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j < 6; j++) A[i][j] = H[i * 6 + j];
        A[i][6] = -g[i];
    }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        int p = k;
        double ap = fabs(A[k][k]);
#pragma unroll
        for (int i = k + 1; i < 6; i++)
            if (fabs(A[i][k]) > ap) { p = i; ap = fabs(A[i][k]); }
        // row swap k <-> p with static indices (p is run-time)
#pragma unroll
        for (int i = k + 1; i < 6; i++)
            if (i == p)
#pragma unroll
                for (int j = 0; j < 7; j++) { const double tt = A[k][j]; A[k][j] = A[i][j]; A[i][j] = tt; }
        if (A[k][k] == 0.0) ok = false;
#pragma unroll
        for (int i = k + 1; i < 6; i++) {
            const double f = A[i][k] / A[k][k];
#pragma unroll
            for (int j = k; j < 7; j++) A[i][j] -= f * A[k][j];
        }
    }
    if (!ok) return false;
#pragma unroll
    for (int k = 5; k >= 0; k--) {
        double sacc = A[k][6];
#pragma unroll
        for (int j = k + 1; j < 6; j++) sacc -= A[k][j] * x[j];
        x[k] = sacc / A[k][k];
    }
    return true;
}

}  // namespace rgbd
