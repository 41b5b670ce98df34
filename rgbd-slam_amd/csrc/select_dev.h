// select_dev.h -- libstdc++'s std::nth_element (introselect) and cv::KeyPointsFilter::retainBest on one workgroup,
// bit-exact in the element order they leave: k_svo_select / k_adp_frame (retainBest) and k_adp_select
// (VideoGridAdaptedFeatureDetector's keepStrongest).  Device code, included by the kernels' translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "wave_dev.h"

// profiling builds of svo.hip stamp the selection's stages; everywhere else the stamps are no-ops
#ifndef SEL_PROF
#define SEL_PROF(k) do { } while (0)
#define SEL_PROF_V(k, v) do { } while (0)
#endif

namespace rgbd {

// ------------------------------------------------------------------ retainBest on one workgroup
// cv::KeyPointsFilter::retainBest (OpenCV 3.4) = libstdc++ std::nth_element(begin, begin + n - 1, end,
// response >) + std::partition(begin + n, end, response >= boundary).  Both are Hoare-style: the k-th
// "left stopper" and the k-th "right stopper" (counted from the right) swap while the left one lies
// before the right one; since the scans only meet untouched elements or the previous pair's swapped
// ones, the k-th swap pairs the k-th stoppers of the ORIGINAL range.  That is computed here with block
// ranks: every pair swaps at once, and libstdc++'s element order is reproduced exactly.  The rest of
// introselect (median-of-3, depth limit 2 lg n with the heap-select fallback, final insertion sort)
// runs on one lane.  R = responses, I = payload (u16), posL / posR = rank -> position scratch.
struct SelLds {
    int wa[32];      // wave totals of block_scan2, two buffers
    int phase;       // block_scan2 buffer parity
    int first_false; // pair_swap: rank of the first left stopper that does not swap
};

// exclusive block scan of (a, b) (each < 2^16 in total) in thread order: one packed DPP scan per wave,
// the wave totals through LDS (double-buffered by the caller's phase bit, so one barrier per call)
__device__ __forceinline__ void block_scan2(int a, int b, int& ea, int& eb, int& ta, int& tb, SelLds& sh)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int v = a | (b << 16);
    const int iv = wave_incl_scan(v);
    int* buf = sh.wa + (sh.phase & 1) * 16;
    if (lane == 63) buf[w] = iv;
    __syncthreads();
    int pre = 0, tot = 0;
    for (int i = 0; i < nw; i++) {
        const int x = buf[i];
        pre += i < w ? x : 0;
        tot += x;
    }
    if (threadIdx.x == 0) sh.phase++;   // read by no one before the next barrier
    const int ex = pre + iv - v;
    ea = ex & 0xffff;
    eb = ex >> 16;
    ta = tot & 0xffff;
    tb = tot >> 16;
}

// Pair the left stoppers (mode 0: !(x > p); mode 1: !(x >= p)) with the right stoppers (mode 0: !(p > x);
// mode 1: x >= p) of [a, e) and swap every pair whose left stopper lies before its right one.  Returns K
// (swaps), L_K (the K-th left stopper, INT_MAX if none) and R_{K-1} (-1 if K == 0); TB = right stoppers.
// Each thread owns a contiguous run of <= 32 elements (flags as bit masks, nothing else kept in
// registers); a swap is done by the owner of its left stopper, and pairs are disjoint, so it needs no
// staging: read both, write both.
__device__ int pair_swap(float* R, uint16_t* I, uint16_t* posL, uint16_t* posR, int a, int e, float p, int mode,
                         int& LK, int& RK1, int& TB, SelLds& sh)
{
    const int T = blockDim.x, tid = threadIdx.x;
    const int E = (e - a + T - 1) / T;
    const int base = a + tid * E, hi = min(base + E, e);
    if (tid == 0) sh.first_false = INT_MAX;   // ordered before the atomics by block_scan2's barrier
    unsigned fA = 0, fB = 0;
    int ca = 0, cb = 0;
    for (int i = base; i < hi; i++) {
        const float v = R[i];
        const bool A = mode == 0 ? !(v > p) : !(v >= p);
        const bool Bq = mode == 0 ? !(p > v) : (v >= p);
        fA |= (unsigned)A << (i - base);
        fB |= (unsigned)Bq << (i - base);
        ca += A;
        cb += Bq;
    }
    int ea, eb, TA;
    block_scan2(ca, cb, ea, eb, TA, TB, sh);
    int ka = ea, kb = eb, ff = INT_MAX;
    unsigned sA = 0;
    for (int i = base; i < hi; i++) {
        const int j = i - base;
        const int A = (fA >> j) & 1, Bq = (fB >> j) & 1;
        if (A) {
            posL[ka] = (uint16_t)i;
            if (TB - kb - Bq >= ka + 1) sA |= 1u << j;   // the right stopper of rank ka lies after i
            else ff = min(ff, ka);
        }
        if (Bq) posR[TB - 1 - kb] = (uint16_t)i;
        ka += A;
        kb += Bq;
    }
    // swapping is a prefix of the left-stopper ranks: K = the first rank that does not swap (else TA)
    if (ff != INT_MAX) atomicMin(&sh.first_false, ff);
    __syncthreads();
    const int K = min(sh.first_false, TA);
    LK = K < TA ? (int)posL[K] : INT_MAX;
    RK1 = K > 0 ? (int)posR[K - 1] : -1;
    ka = ea;
    for (int i = base; i < hi; i++) {
        const int j = i - base;
        if ((sA >> j) & 1) {
            const int q = posR[ka];
            const float r = R[i];
            R[i] = R[q];
            R[q] = r;
            const uint16_t t = I[i];
            I[i] = I[q];
            I[q] = t;
        }
        ka += (fA >> j) & 1;
    }
    __syncthreads();
    return K;
}

__device__ __forceinline__ void el_swap(float* R, uint16_t* I, int a, int b)
{
    const float r = R[a];
    R[a] = R[b];
    R[b] = r;
    const uint16_t t = I[a];
    I[a] = I[b];
    I[b] = t;
}

// libstdc++ __adjust_heap / __push_heap with comp(a, b) = a > b (one lane)
__device__ void adjust_heap(float* R, uint16_t* I, int first, int hole, int len, float vr, uint16_t vi)
{
    const int top = hole;
    int child = hole;
    while (child < (len - 1) / 2) {
        child = 2 * (child + 1);
        if (R[first + child] > R[first + child - 1]) child--;
        R[first + hole] = R[first + child];
        I[first + hole] = I[first + child];
        hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) {
        child = 2 * (child + 1);
        R[first + hole] = R[first + child - 1];
        I[first + hole] = I[first + child - 1];
        hole = child - 1;
    }
    int parent = (hole - 1) / 2;
    while (hole > top && R[first + parent] > vr) {
        R[first + hole] = R[first + parent];
        I[first + hole] = I[first + parent];
        hole = parent;
        parent = (hole - 1) / 2;
    }
    R[first + hole] = vr;
    I[first + hole] = vi;
}

// std::__heap_select(first, middle, last) + iter_swap(first, nth): introselect's depth-limit fallback
__device__ void heap_select_one_lane(float* R, uint16_t* I, int first, int middle, int last, int nth)
{
    const int len = middle - first;
    if (len >= 2) {
        int parent = (len - 2) / 2;
        for (;;) {
            adjust_heap(R, I, first, parent, len, R[first + parent], I[first + parent]);
            if (parent == 0) break;
            parent--;
        }
    }
    for (int i = middle; i < last; i++)
        if (R[i] > R[first]) {   // __pop_heap(first, middle, i)
            const float vr = R[i];
            const uint16_t vi = I[i];
            R[i] = R[first];
            I[i] = I[first];
            adjust_heap(R, I, first, 0, len, vr, vi);
        }
    el_swap(R, I, first, nth);
}

// std::__insertion_sort(first, last) with comp = greater (one lane)
__device__ void insertion_sort_one_lane(float* R, uint16_t* I, int f, int l)
{
    if (f == l) return;
    for (int i = f + 1; i < l; i++) {
        const float vr = R[i];
        const uint16_t vi = I[i];
        int j = i;
        if (vr > R[f]) {
            for (; j > f; j--) { R[j] = R[j - 1]; I[j] = I[j - 1]; }
        } else {
            while (vr > R[j - 1]) { R[j] = R[j - 1]; I[j] = I[j - 1]; j--; }
        }
        R[j] = vr;
        I[j] = vi;
    }
}

// std::__move_median_to_first(result, a, b, c) with comp = greater (one lane)
__device__ void median_to_first(float* R, uint16_t* I, int result, int a, int b, int c)
{
    if (R[a] > R[b]) {
        if (R[b] > R[c]) el_swap(R, I, result, b);
        else if (R[a] > R[c]) el_swap(R, I, result, c);
        else el_swap(R, I, result, a);
    } else if (R[a] > R[c]) el_swap(R, I, result, a);
    else if (R[b] > R[c]) el_swap(R, I, result, c);
    else el_swap(R, I, result, b);
}

// std::nth_element(begin, begin + nth, end, response >) over R[0..n) (0 <= nth < n): libstdc++'s __introselect
// depth_limit < 0: libstdc++'s 2 * lg(n); an explicit value pins the heap-select fallback in the tests
__device__ void introselect_block(float* R, uint16_t* I, uint16_t* posL, uint16_t* posR, int n, int nth, SelLds& sh,
                                  int depth_limit = -1)
{
    int f = 0, l = n;
    int depth = depth_limit >= 0 ? depth_limit : 2 * (31 - __clz(n));
    bool heap = false;
    int it = 0;
    while (l - f > 3) {
        if (depth == 0) {
            if (threadIdx.x == 0) heap_select_one_lane(R, I, f, nth + 1, l, nth);
            __syncthreads();
            heap = true;
            break;
        }
        --depth;
        if (threadIdx.x == 0) median_to_first(R, I, f, f + 1, f + (l - f) / 2, l - 1);
        __syncthreads();
        const float p = R[f];
        int LK, RK1, TB;
        const int K = pair_swap(R, I, posL, posR, f + 1, l, p, 0, LK, RK1, TB, sh);
        const int cut = min(K == 0 ? LK : min(LK, RK1), l);   // (the min with l never binds: median-of-3 sentinels)
        if (cut <= nth) f = cut;
        else l = cut;
        SEL_PROF(2 + min(it, 40));
        it++;
    }
    SEL_PROF_V(60, it);
    (void)it;
    if (!heap) {
        if (threadIdx.x == 0) insertion_sort_one_lane(R, I, f, l);
        __syncthreads();
    }
}

// retainBest(n_points = nkeep) over R[0..n) (n > nkeep >= 1): returns the kept count (block-uniform)
__device__ int retain_best_block(float* R, uint16_t* I, uint16_t* posL, uint16_t* posR, int n, int nkeep, SelLds& sh,
                                 int depth_limit = -1)
{
    introselect_block(R, I, posL, posR, n, nkeep - 1, sh, depth_limit);
    // std::partition(begin + nkeep, end, response >= R[nkeep - 1]): the kept prefix grows by the preds
    const float amb = R[nkeep - 1];
    int LK, RK1, TB;
    SEL_PROF(45);
    pair_swap(R, I, posL, posR, nkeep, n, amb, 1, LK, RK1, TB, sh);
    SEL_PROF(46);
    return nkeep + TB;
}

}  // namespace rgbd
