// ransac_dev.h -- RansacSE3 hypothesis-kernel interface (host <-> device).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rgbd {

constexpr int kRansacMaxM = 2304;   // LDS-resident matches per RansacSE3 call (<= 147 KB)

struct RansacDev {
    int32_t M;          // used matches (sorted by distance)
    int32_t H;          // hypotheses (the identity slot is block H)
    int32_t SS;         // sample size (stride of the sample table)
    int32_t MWcap;      // mask words per hypothesis in masks_out
    uint32_t minTh;     // mMinInlierTh
    float maxMahal;     // mMaxMahalanobisDistance
    double C;           // depthCovariance sticky value
    double rcx, rcy;    // raster_cov_x / raster_cov_y (Solver/SolverSE3.cpp:218-225)
};

struct HypOut {
    float T[16];
    double err;
    int32_t n;
    int32_t pad;
};

// ------------------------------------------------------------------ the loop rules of RansacSE3::compute
// Written once for the host loop (solver.cpp) and the device loop (lane_replay_dev.h); semantics:
// oracle/orc_solver.cpp.  tests/ransac_loop_check.cpp runs them on the CPU.

// Random::randomInt(0, M - 1) (System/Random.cpp:16-20) from one rand() output
__host__ __device__ inline int glibc_random_int(int32_t r, int M)
{
    return int(((double)r / ((double)2147483647 + 1.0)) * (double)M);
}

// RansacSE3::sampleMatches (:135-159): the ids of one hypothesis in std::set order (ascending, distinct),
// two g.random_int(M) draws per attempt, each attempt adding 2 to `calls`.  Returns the number of ids (SS
// unless M < SS or the safety stop ended the loop).
template <class Gen>
__host__ __device__ inline int sample_matches(Gen& g, int M, int SS, int* ids, int& calls)
{
    int n = 0, safety = 0;
    while (n < SS && M >= SS) {
        int id1 = g.random_int(M);
        const int id2 = g.random_int(M);
        calls += 2;
        if (id1 > id2) id1 = id2;
        int pos = 0;
        while (pos < n && ids[pos] < id1) pos++;
        if (pos == n || ids[pos] != id1) {
            for (int k = n; k > pos; k--) ids[k] = ids[k - 1];
            ids[pos] = id1;
            n++;
        }
        if (++safety > 10000) break;
    }
    return n;
}

struct Se3Loop {                   // the sequential loop's state (:56-103)
    float rmse = 1e6f;
    int bestH = -1;                // hypothesis of the best model, -1 if none
    int validIters = 0;
    size_t bestN = 0;
};

// The accept rule (:88-102) for hypothesis h with outcome o, in loop iteration n of a call with M matches:
// n takes the two += 10 steps; false = the loop breaks.  The reference compares nr with mvDMatches.size() * 0.5
// (a size_t times a double); M * 0.5 (an int times a double) is the same value: M >= 0 is that size, and both
// conversions to double are exact.
__host__ __device__ inline bool se3_accept(Se3Loop& s, int h, const HypOut& o, int M, uint32_t minTh, int& n)
{
    if (o.n <= 0) return true;
    s.validIters++;
    const size_t nr = (size_t)o.n;
    if (o.err <= (double)s.rmse && nr >= s.bestN && nr >= minTh) {
        s.rmse = (float)o.err;
        s.bestH = h;
        s.bestN = nr;
        if (nr > M * 0.5) n += 10;
        if (nr > M * 0.75) n += 10;
        if (nr > M * 0.8) return false;
    }
    return true;
}

// the identity fallback (:105-117) applies when no iteration was valid and the identity's outcome passes this
__host__ __device__ inline bool se3_identity_ok(const HypOut& id, uint32_t minTh, float maxMahal)
{
    return (uint32_t)id.n > minTh && id.err < (double)maxMahal;
}

size_t ransac_lds_bytes(int M);
hipError_t launch_ransac_hyp(const float* pts, const int* samples, const int* scount, const RansacDev& prm, HypOut* out,
                       uint32_t* masks, hipStream_t st);

}  // namespace rgbd
