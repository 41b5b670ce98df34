// umeyama_dev.h -- the rules of the Umeyama RANSAC, Ransac::compute (Solver/Ransac.cpp), written once for the
// kernel (umeyama.hip), the host (umeyama_host.cpp) and tests/umeyama_loop_check.cpp.  Operator: DESIGN.md
// "Umeyama RANSAC definition"; tests/umeyama_ransac_model.py is the same text as numpy.  Every operation is f32
// in the order written (the build's -ffp-contract=off keeps a * b + c two roundings).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cfloat>
#include <climits>
#include <cmath>

#include "ransac_dev.h"

namespace rgbd {

constexpr int kUmMaxM = 4096;      // matches per problem (24 B each in LDS)
constexpr int kUmMaxPairs = 8;     // used_pairs in [3, 8]
constexpr int kUmThreads = 256;    // one workgroup = one round of hypotheses
constexpr int kUmIters0 = 487;     // computeRANSACIteration(0.20), Ransac.cpp:26

struct UmPrm {
    int32_t adaptive;       // ADAPTIVE_ERROR: the threshold is scaled by the F1 point's z (:267-268)
    int32_t used_pairs;
    int32_t min_matches;
    int32_t max_bound;      // iters(min_inlier_ratio): no accepted bound is above it
    double thr;             // inlierThresholdEuclidean
    double min_ratio;       // minimalInlierRatioThreshold
};

struct UmProb {
    int32_t off;            // first match row
    int32_t count;          // match rows
    int32_t tab_off;        // the problem's bound table in the table buffer (count of gated matches + 1 entries)
    int32_t run;            // 0: a skipped pair
};

struct UmRes {
    float T[16];
    int32_t n_inliers;
    int32_t iterations;
    int32_t ok;
    int32_t best_count;
    int32_t n_accepts;
    int32_t gated;
    int32_t pad[2];
};

// ---------------------------------------------------------------- iteration bounds (host: glibc log / pow)
// computeRANSACIteration (:449-454), the exponent always 3; the conversion saturates (a deviation,
// the reference's is undefined from 2^31 on)
inline int um_iters(double r)
{
    const double q = std::log(1 - 0.98) / std::log(1 - std::pow(r, 3));
    if (!(q < 2147483648.0)) return q != q ? INT_MIN : INT_MAX;
    if (q <= -2147483649.0) return INT_MIN;
    return (int)q;
}

// bound[c], c = 0..M: the loop bound after a model with c of M inliers is accepted (:442-445)
inline void um_bound_table(int M, double min_ratio, int* bound)
{
    const int cap = um_iters(min_ratio);
    for (int c = 0; c <= M; c++) {
        const int b = um_iters((double)((float)c / (float)M));
        bound[c] = b < cap ? b : cap;
    }
}

// glibc rand() on a 33-word state (state[31], f, r), for host loops
struct UmHostGen {
    int32_t* s;
    int random_int(int M)
    {
        int f = s[31], r = s[32];
        const uint32_t val = (uint32_t)s[f] + (uint32_t)s[r];
        s[f] = (int32_t)val;
        if (++f >= 31) {
            f = 0;
            ++r;
        } else if (++r >= 31) {
            r = 0;
        }
        s[31] = f;
        s[32] = r;
        return glibc_random_int((int32_t)(val >> 1), M);
    }
};

// ---------------------------------------------------------------- the sampler (:183-208)
// Random::randomInt(0, M - 1) until n distinct positions are chosen; pos in draw order; every draw counts
template <class Gen>
__host__ __device__ inline void um_sample(Gen& g, int M, int n, int* pos, int& calls)
{
    int k = 0;
    while (k < n) {
        const int id = g.random_int(M);
        calls++;
        bool used = false;
#pragma unroll
        for (int j = 0; j < kUmMaxPairs; j++) used = used || (j < k && pos[j] == id);
        if (!used) {
#pragma unroll
            for (int j = 0; j < kUmMaxPairs; j++)
                if (j == k) pos[j] = id;
            k++;
        }
    }
}

// ---------------------------------------------------------------- Eigen 3.3 JacobiSVD<Matrix3f>, full U and V
// the f32 instance of oracle/orc_solver.cpp svd3 (FLT_MIN, FLT_EPSILON in the thresholds); y / |y| is +-1
// exactly for the y != 0 it is reached with, so copysign
struct UmRot { float c, s; };

__host__ __device__ inline void um_rot_rows(float A[3][3], int p, int q, UmRot j)
{
    if (j.c == 1.0f && j.s == 0.0f) return;
    for (int i = 0; i < 3; i++) {
        const float xi = A[p][i], yi = A[q][i];
        A[p][i] = j.c * xi + j.s * yi;
        A[q][i] = -j.s * xi + j.c * yi;
    }
}

__host__ __device__ inline void um_rot_cols(float A[3][3], int p, int q, UmRot j)
{
    const float c = j.c, s = -j.s;
    if (c == 1.0f && s == 0.0f) return;
    for (int i = 0; i < 3; i++) {
        const float xi = A[i][p], yi = A[i][q];
        A[i][p] = c * xi + s * yi;
        A[i][q] = -s * xi + c * yi;
    }
}

__host__ __device__ inline UmRot um_make_jacobi(float x, float y, float z)
{
    const float deno = 2.0f * fabsf(y);
    if (deno < FLT_MIN) return UmRot{1.0f, 0.0f};
    const float tau = (x - z) / deno;
    const float w = sqrtf(tau * tau + 1.0f);
    const float t = (tau > 0.0f) ? 1.0f / (tau + w) : 1.0f / (tau - w);
    const float sign_t = t > 0.0f ? 1.0f : -1.0f;
    const float n = 1.0f / sqrtf(t * t + 1.0f);
    UmRot r;
    r.s = ((-sign_t * copysignf(1.0f, y)) * fabsf(t)) * n;
    r.c = n;
    return r;
}

__host__ __device__ inline void um_jacobi_2x2(const float A[3][3], int p, int q, UmRot* jl, UmRot* jr)
{
    float m00 = A[p][p], m01 = A[p][q], m10 = A[q][p], m11 = A[q][q];
    UmRot r1;
    const float t = m00 + m11;
    const float d = m10 - m01;
    if (fabsf(d) < FLT_MIN) {
        r1.s = 0.0f;
        r1.c = 1.0f;
    } else {
        const float u = t / d;
        const float tmp = sqrtf(1.0f + u * u);
        r1.s = 1.0f / tmp;
        r1.c = u / tmp;
    }
    if (!(r1.c == 1.0f && r1.s == 0.0f)) {
        const float a0 = r1.c * m00 + r1.s * m10, b0 = -r1.s * m00 + r1.c * m10;
        const float a1 = r1.c * m01 + r1.s * m11, b1 = -r1.s * m01 + r1.c * m11;
        m00 = a0; m10 = b0; m01 = a1; m11 = b1;
    }
    *jr = um_make_jacobi(m00, m01, m11);
    const float jtc = jr->c, jts = -jr->s;
    jl->c = r1.c * jtc - r1.s * jts;
    jl->s = r1.c * jts + r1.s * jtc;
}

__host__ __device__ inline void um_svd3(const float M[3][3], float U[3][3], float V[3][3])
{
    float scale = 0.0f;
    bool finite = true;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const float a = fabsf(M[i][j]);
            if (!(a <= FLT_MAX)) finite = false;   // inf or NaN
            if (a > scale) scale = a;
        }
    if (!finite) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) U[i][j] = V[i][j] = __builtin_nanf("");
        return;
    }
    if (scale == 0.0f) scale = 1.0f;
    float W[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            W[i][j] = M[i][j] / scale;
            U[i][j] = V[i][j] = (i == j) ? 1.0f : 0.0f;
        }
    float maxDiag = fmaxf(fmaxf(fabsf(W[0][0]), fabsf(W[1][1])), fabsf(W[2][2]));
    bool finished = false;
    int sweeps = 0;
    while (!finished && sweeps < 64) {
        finished = true;
        sweeps++;
        for (int p = 1; p < 3; ++p)
            for (int q = 0; q < p; ++q) {
                const float threshold = fmaxf(FLT_MIN, (2.0f * FLT_EPSILON) * maxDiag);
                if (fabsf(W[p][q]) > threshold || fabsf(W[q][p]) > threshold) {
                    finished = false;
                    UmRot jl, jr;
                    um_jacobi_2x2(W, p, q, &jl, &jr);
                    um_rot_rows(W, p, q, jl);
                    um_rot_cols(U, p, q, UmRot{jl.c, -jl.s});
                    um_rot_cols(W, p, q, jr);
                    um_rot_cols(V, p, q, jr);
                    maxDiag = fmaxf(maxDiag, fmaxf(fabsf(W[p][p]), fabsf(W[q][q])));
                }
            }
    }
    float S[3];
    for (int i = 0; i < 3; i++) {
        const float a = W[i][i];
        S[i] = fabsf(a);
        if (a < 0.0f)
            for (int r = 0; r < 3; r++) U[r][i] = -U[r][i];
    }
    for (int i = 0; i < 3; i++) S[i] *= scale;
    for (int i = 0; i < 3; i++) {
        int pos = i;
        float mx = S[i];
        for (int j = i + 1; j < 3; j++)
            if (S[j] > mx) { mx = S[j]; pos = j; }
        if (mx == 0.0f) break;
        if (pos != i) {
            const float ts = S[i]; S[i] = S[pos]; S[pos] = ts;
            for (int r = 0; r < 3; r++) {
                const float t1 = U[r][i]; U[r][i] = U[r][pos]; U[r][pos] = t1;
                const float t2 = V[r][i]; V[r][i] = V[r][pos]; V[r][pos] = t2;
            }
        }
    }
}

__host__ __device__ inline float um_det3(const float A[3][3])
{
    return (A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0])) +
           A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
}

// ---------------------------------------------------------------- Eigen::umeyama(src, dst, false) (:231)
// from sigma and the two means: Rt = R (row-major 9) then t (3); false = "model failed", isnan(T(0, 0)) (:240);
// *sneg = the S = (1, 1, -1) branch was taken
__host__ __device__ inline bool um_model(const float sigma[3][3], const float* dmean, const float* smean, float* Rt, bool* sneg)
{
    float U[3][3], V[3][3];
    um_svd3(sigma, U, V);
    const bool neg = um_det3(U) * um_det3(V) < 0.0f;
    const float S[3] = {1.0f, 1.0f, neg ? -1.0f : 1.0f};
    for (int i = 0; i < 3; i++) {
        const float u0 = U[i][0] * S[0], u1 = U[i][1] * S[1], u2 = U[i][2] * S[2];
        for (int j = 0; j < 3; j++) Rt[3 * i + j] = (u0 * V[j][0] + u1 * V[j][1]) + u2 * V[j][2];
    }
    for (int i = 0; i < 3; i++)
        Rt[9 + i] = dmean[i] - ((Rt[3 * i] * smean[0] + Rt[3 * i + 1] * smean[1]) + Rt[3 * i + 2] * smean[2]);
    *sneg = neg;
    return !(Rt[0] != Rt[0]);
}

// the whole fit over n >= 1 point pairs, sequential sums in point order: get(i, p) fills p[0..2] = the F1 point
// (dst) and p[3..5] = the F2 point (src)
template <class Get>
__host__ __device__ inline bool um_fit(const Get& get, int n, float* Rt, bool* sneg)
{
    const float inv_n = 1.0f / (float)n;
    float mean[6], p[6];
    get(0, mean);
    for (int i = 1; i < n; i++) {
        get(i, p);
        for (int k = 0; k < 6; k++) mean[k] = mean[k] + p[k];
    }
    for (int k = 0; k < 6; k++) mean[k] = mean[k] * inv_n;
    float sigma[3][3];
    for (int i = 0; i < n; i++) {
        get(i, p);
        for (int k = 0; k < 6; k++) p[k] = p[k] - mean[k];
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) {
                const float v = p[a] * p[3 + b];
                sigma[a][b] = i == 0 ? v : sigma[a][b] + v;
            }
    }
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) sigma[a][b] = sigma[a][b] * inv_n;
    return um_model(sigma, mean, mean + 3, Rt, sneg);
}

__host__ __device__ inline void um_identity(float* Rt)
{
    for (int i = 0; i < 12; i++) Rt[i] = (i < 9 && i % 4 == 0) ? 1.0f : 0.0f;
}

// ---------------------------------------------------------------- the scoring predicate (:259-276)
// p: the F1 point then the F2 point
__host__ __device__ inline bool um_inlier(const float* Rt, const float* p, int adaptive, double thr)
{
    const float ex = ((Rt[0] * p[3] + Rt[1] * p[4]) + Rt[2] * p[5]) + Rt[9];
    const float ey = ((Rt[3] * p[3] + Rt[4] * p[4]) + Rt[5] * p[5]) + Rt[10];
    const float ez = ((Rt[6] * p[3] + Rt[7] * p[4]) + Rt[8] * p[5]) + Rt[11];
    const float dx = ex - p[0], dy = ey - p[1], dz = ez - p[2];
    const float nrm = sqrtf((dx * dx + dy * dy) + dz * dz);
    double t = thr;
    if (adaptive) t = t * (double)p[2];
    return (double)nrm < t;
}

// the depth gate (:78-81): strict comparisons, so a NaN z is kept
__host__ __device__ inline bool um_gated_out(float z1, float z2)
{
    return z1 < 0.1f || z1 > 6.0f || z2 < 0.1f || z2 > 6.0f;
}

// ---------------------------------------------------------------- the loop (:95-157, :429-447)
struct UmLoop {
    int i = 0;                 // the running for's index
    int bound = kUmIters0;     // mRANSACParams.iterationCount
    int best = 0;              // inliers of the best model; its ratio float(best) / float(M) is strictly
                               // increasing in best for every M <= 4096, so the ratio test is a count test
    int best_i = -1;
};

// iteration s.i with outcome count (< 0: the model failed); false = the loop had ended before it
__host__ __device__ inline bool um_step(UmLoop& s, int count, const int* bound_tab)
{
    if (s.i >= s.bound) return false;
    if (count > s.best) {   // strictly greater: a tie keeps the earlier model
        s.best = count;
        s.best_i = s.i;
        s.bound = bound_tab[count];
    }
    s.i++;
    return true;
}

// bestInlierRatio < minimalInlierRatioThreshold (:168)
__host__ __device__ inline bool um_below_ratio(int best, int M, double min_ratio)
{
    return (double)((float)best / (float)M) < min_ratio;
}

// ---------------------------------------------------------------- Eigen's isIdentity(1e-5f) (:55)
__host__ __device__ inline bool um_is_identity(const float* T)
{
    const float prec = 1e-5f;
    for (int j = 0; j < 4; j++)
        for (int i = 0; i < 4; i++) {
            const float a = T[4 * i + j];
            if (i == j) {
                if (!(fabsf(a - 1.0f) <= fminf(fabsf(a), 1.0f) * prec)) return false;
            } else if (!(fabsf(a) <= 1.0f * prec)) {
                return false;
            }
        }
    return true;
}

__host__ __device__ inline void um_T16(const float* Rt, float* T)
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T[4 * i + j] = Rt[3 * i + j];
        T[4 * i + 3] = Rt[9 + i];
    }
    T[12] = T[13] = T[14] = 0.0f;
    T[15] = 1.0f;
}

struct UmDbg {
    int32_t* pos;      // [cap][8] sample positions (gated order) per evaluated hypothesis
    int32_t* count;    // [cap] inliers, -1 where the model failed
    uint8_t* sneg;     // [cap] the S = -1 branch
    int32_t* accepts;  // [kUmMaxM + 1][3] iteration, count, new bound
    int32_t cap;
};

size_t um_lds_bytes(int max_m);
hipError_t launch_umeyama(const float* pts, const UmProb* probs, const UmPrm& prm, const int* tables, int32_t* rngs,
                          int32_t* inl, UmRes* res, const UmDbg& dbg, int max_m, int P, hipStream_t st);
hipError_t launch_umeyama_gather(const void* matches, const int* counts, const int* qf, const int* tf, const float* xyz,
                                 int K, int P, float* pts, int* gated, int* err, hipStream_t st);

}  // namespace rgbd
