// fast.hip -- the reference's plain FAST front end on gfx950: Extractor(FAST, BRIEF, NORMAL)
//   cv::FastFeatureDetector::create()  Features/Extractor.cpp:168-171: cv::FAST(gray, 10, true, TYPE_9_16)  -> k_adp_score + k_fast_rows
//   Extractor::detectAndCompute        Features/Extractor.cpp:50-61: retainBest(nfeatures)                   -> k_fast_select
// then BRIEF-32 (k_svo_brief on k_svo_pyramid's box sums) and k_undistort, as for the SVO front end; or, for
// Extractor(FAST, ORB, NORMAL), cv::ORB::create()->compute()'s provided-keypoints path (:216-218): runByImageBorder(31),
// the ORB2 path's level-0 blur and k_fast_orb_describe, the 256 tests of bit_pattern_31_ steered by the keypoint's
// stored angle (-1: compute() does not recompute it).
//
// The detector is adaptive.hip's identity on the whole image: the corners of cv::FAST at threshold t >= 1 after its
// 3x3 suppression are the strict 3x3 maxima of the threshold-free score S = max(M, 1) - 1 with S >= t, in raster
// order.  Score and maxima stay two passes (k_adp_score as it is, then k_fast_rows on its map): the map is 1 B per
// pixel and stays in L2 between them.
//
// A rich frame has 11,000 .. 32,000 corners at threshold 10, more than select_dev.h's LDS selection holds (12,288).
// k_fast_select therefore runs libstdc++'s introselect in two tiers: Hoare pair-swap passes on a per-frame global
// scratch (R f32, I u16, posL / posR u16: 10 B per element, L2-resident) while the live range [f, l) is longer than
// kFastLdsTier, then select_dev.h's introselect_block on that range in LDS with the depth budget that is left, and
// retainBest's closing partition over the global tail.  The element order is libstdc++'s on both tiers.
#include <hip/hip_runtime.h>

#include "dispatch.h"

#include <climits>
#include <cstdint>

#include "fast_dev.h"
#include "orb_math_dev.h"
#include "orb_pattern_dev.h"
#include "select_dev.h"

namespace rgbd {

// ------------------------------------------------------------------ block scans with 32-bit totals
struct BigLds {
    int wa[16], wb[16];
    int first_false;   // pair_swap_g: rank of the first left stopper that does not swap
};

// exclusive block scan of (a, b) in thread order, totals up to 2^31: two DPP wave scans, wave totals through LDS
__device__ __forceinline__ void block_scan_pair(int a, int b, int& ea, int& eb, int& ta, int& tb, BigLds& sh)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int ia = wave_incl_scan(a), ib = wave_incl_scan(b);
    __syncthreads();   // the previous call's readers are done
    if (lane == 63) {
        sh.wa[w] = ia;
        sh.wb[w] = ib;
    }
    __syncthreads();
    int pa = 0, pb = 0;
    ta = 0;
    tb = 0;
    for (int i = 0; i < nw; i++) {
        const int x = sh.wa[i], y = sh.wb[i];
        pa += i < w ? x : 0;
        pb += i < w ? y : 0;
        ta += x;
        tb += y;
    }
    ea = pa + ia - a;
    eb = pb + ib - b;
}

// ------------------------------------------------------------------ the raster corner list
// One workgroup per image row and frame, thread t owns columns [t E, (t + 1) E) (E = ceil(W / 256) <= 8), so thread
// order is raster order.  LIST = false counts the row's maxima; LIST = true sums the counts of the rows above and
// stores the row's maxima behind them.  cv::FAST's score buffer is 0 outside [3, W - 3) x [3, H - 3).  The map is 0
// in rows outside that range and in columns below 3; where its rows are wider than the image (sstride > W, the ORB
// pyramid's padded rows) its columns from W - 3 on hold scores of ring pixels past the image, so column W - 3 is
// taken as 0 here, not read.  Every neighbour of a pixel inside the range lies inside the map.
template <bool LIST>
__global__ __launch_bounds__(kFastRowThreads) void k_fast_rows(FastCfg g, const uint8_t* __restrict__ smap, int* __restrict__ rowc,
                                                               uint32_t* __restrict__ cand, int* __restrict__ ncand,
                                                               int* __restrict__ err)
{
    __shared__ BigLds sh;
    const int tid = threadIdx.x, y = blockIdx.x, b = blockIdx.y;
    const int W = g.W, H = g.H, SS = g.sstride;
    const uint8_t* S = smap + (size_t)b * SS * H;
    const int E = (W + kFastRowThreads - 1) / kFastRowThreads;
    const int x0 = tid * E;
    const int xa = max(x0, 3), xe = min(min(x0 + E, W), W - 3);
    unsigned keep = 0;
    int cnt = 0;
    if (y >= 3 && y < H - 3) {
        const uint8_t* r0 = S + (size_t)(y - 1) * SS;
        const uint8_t* r1 = r0 + SS;
        const uint8_t* r2 = r1 + SS;
        for (int x = xa; x < xe; x++) {
            const int s = r1[x];
            if (s < g.thr) continue;
            const int right = x + 1 < W - 3 ? max(max((int)r0[x + 1], (int)r1[x + 1]), (int)r2[x + 1]) : 0;
            const int nb = max(max(max((int)r0[x - 1], (int)r0[x]), max(right, (int)r1[x - 1])), max((int)r2[x - 1], (int)r2[x]));
            if (s > nb) {
                keep |= 1u << (x - x0);
                cnt++;
            }
        }
    }
    int above = 0;
    if (LIST)
        for (int r = tid; r < y; r += kFastRowThreads) above += rowc[b * H + r];
    int off, pre, tot, prefix;
    block_scan_pair(cnt, above, off, pre, tot, prefix, sh);
    if (!LIST) {
        if (tid == 0) rowc[b * H + y] = tot;
        return;
    }
    off += prefix;
    uint32_t* L = cand + (size_t)b * g.cand_cap;
    for (int j = 0; j < E; j++)
        if ((keep >> j) & 1u) {
            if (off < g.cand_cap) L[off] = adp_pack(x0 + j, y, (int)S[(size_t)y * SS + x0 + j]);
            off++;
        }
    if (y == H - 1 && tid == 0) {   // the last row holds no corner: prefix is the frame's count
        ncand[b] = prefix + tot;
        if (prefix + tot > g.cand_cap) atomicOr(err + b, kFastErrCand);
    }
}

// ------------------------------------------------------------------ retainBest on up to 65,536 elements
// pair_swap (select_dev.h) on global arrays with up to 64 elements per thread: the same pairing of the k-th left
// stopper with the k-th right stopper, flags as 64-bit masks, ranks from block_scan_pair.
__device__ int pair_swap_g(float* R, uint16_t* I, uint16_t* posL, uint16_t* posR, int a, int e, float p, int mode, int& LK,
                           int& RK1, int& TB, BigLds& sh)
{
    const int T = blockDim.x, tid = threadIdx.x;
    const int E = (e - a + T - 1) / T;
    const int base = a + tid * E, hi = min(base + E, e);
    if (tid == 0) sh.first_false = INT_MAX;   // ordered before the atomics by block_scan_pair's barriers
    unsigned long long fA = 0, fB = 0;
    int ca = 0, cb = 0;
    for (int i = base; i < hi; i++) {
        const float v = R[i];
        const bool A = mode == 0 ? !(v > p) : !(v >= p);
        const bool Bq = mode == 0 ? !(p > v) : (v >= p);
        fA |= (unsigned long long)A << (i - base);
        fB |= (unsigned long long)Bq << (i - base);
        ca += A;
        cb += Bq;
    }
    int ea, eb, TA;
    block_scan_pair(ca, cb, ea, eb, TA, TB, sh);
    int ka = ea, kb = eb, ff = INT_MAX;
    unsigned long long sA = 0;
    for (int i = base; i < hi; i++) {
        const int j = i - base;
        const int A = (int)((fA >> j) & 1), Bq = (int)((fB >> j) & 1);
        if (A) {
            posL[ka] = (uint16_t)i;
            if (TB - kb - Bq >= ka + 1) sA |= 1ull << j;   // the right stopper of rank ka lies after i
            else ff = min(ff, ka);
        }
        if (Bq) posR[TB - 1 - kb] = (uint16_t)i;
        ka += A;
        kb += Bq;
    }
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
            el_swap(R, I, i, q);
        }
        ka += (int)((fA >> j) & 1);
    }
    __syncthreads();
    return K;
}

// retainBest(nkeep) over gR / gI [0, n) (kFastMaxCandCap >= n > nkeep >= 1): the kept count (block-uniform), the kept
// elements' payloads in gI[0, count).  depth_limit as for introselect_block; the budget 2 lg n is taken from n and
// carried from the global tier into the LDS tier.
__device__ int retain_best_tiered(float* gR, uint16_t* gI, uint16_t* gPL, uint16_t* gPR, unsigned char* smem, int n, int nkeep,
                                  int depth_limit, SelLds& sh, BigLds& bs)
{
    const int T = blockDim.x, tid = threadIdx.x;
    float* R = reinterpret_cast<float*>(smem);
    uint16_t* I = reinterpret_cast<uint16_t*>(R + kFastLdsTier);
    uint16_t* posL = I + kFastLdsTier;
    uint16_t* posR = posL + kFastLdsTier;
    if (tid == 0) sh.phase = 0;
    __syncthreads();
    if (n <= kFastLdsTier) {   // the whole selection in LDS
        for (int i = tid; i < n; i += T) {
            R[i] = gR[i];
            I[i] = gI[i];
        }
        __syncthreads();
        const int m = retain_best_block(R, I, posL, posR, n, nkeep, sh, depth_limit);
        __syncthreads();
        for (int i = tid; i < m; i += T) gI[i] = I[i];
        __syncthreads();
        return m;
    }
    const int nth = nkeep - 1;
    int f = 0, l = n;
    int depth = depth_limit >= 0 ? depth_limit : 2 * (31 - __clz(n));
    bool heap = false;
    while (l - f > kFastLdsTier) {
        if (depth == 0) {
            if (tid == 0) heap_select_one_lane(gR, gI, f, nth + 1, l, nth);
            __syncthreads();
            heap = true;
            break;
        }
        --depth;
        if (tid == 0) median_to_first(gR, gI, f, f + 1, f + (l - f) / 2, l - 1);
        __syncthreads();
        const float p = gR[f];
        int LK, RK1, TB;
        const int K = pair_swap_g(gR, gI, gPL, gPR, f + 1, l, p, 0, LK, RK1, TB, bs);
        const int cut = min(K == 0 ? LK : min(LK, RK1), l);
        if (cut <= nth) f = cut;
        else l = cut;
    }
    if (!heap) {   // [f, l) fits the LDS tier: the rest of introselect there
        const int len = l - f;
        for (int i = tid; i < len; i += T) {
            R[i] = gR[f + i];
            I[i] = gI[f + i];
        }
        __syncthreads();
        introselect_block(R, I, posL, posR, len, nth - f, sh, depth);
        __syncthreads();
        for (int i = tid; i < len; i += T) {
            gR[f + i] = R[i];
            gI[f + i] = I[i];
        }
        __syncthreads();
    }
    // std::partition(begin + nkeep, end, response >= R[nkeep - 1]) over the global tail
    const float amb = gR[nkeep - 1];
    int LK, RK1, TB;
    pair_swap_g(gR, gI, gPL, gPR, nkeep, n, amb, 1, LK, RK1, TB, bs);
    return nkeep + TB;
}

// One workgroup per frame: retainBest(nfeatures) when the frame has more corners, then the descriptor's
// runByImageBorder (stable) and the keypoints as cv::KeyPoint(x, y, 7.f, -1, score), octave 0, class_id -1.
__global__ __launch_bounds__(kFastThreads) void k_fast_select(FastCfg g, FastBufs w, int* __restrict__ counts, float* __restrict__ kps,
                                                              int* __restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ SelLds sh;
    __shared__ BigLds bs;
    const int tid = threadIdx.x, T = blockDim.x, b = blockIdx.x;
    const size_t fo = (size_t)b * g.cand_cap;
    const uint32_t* L = w.cand + fo;
    float* gR = w.R + fo;
    uint16_t* gI = w.I + fo;
    const int n = w.ncand[b];
    if (n > g.cand_cap) {   // flagged by k_fast_rows
        if (tid == 0) counts[b] = 0;
        return;
    }
    int m = n;
    const bool retain = n > g.nfeatures;
    if (retain) {
        for (int i = tid; i < n; i += T) {
            gR[i] = (float)adp_s(L[i]);
            gI[i] = (uint16_t)i;
        }
        __syncthreads();
        m = retain_best_tiered(gR, gI, w.posL + fo, w.posR + fo, smem, n, g.nfeatures, -1, sh, bs);
    }
    if (m > g.kp_cap) {
        if (tid == 0) {
            atomicOr(err + b, kFastErrKeep);
            counts[b] = 0;
        }
        return;
    }
    const int E = (m + T - 1) / T, base = tid * E, hi = min(base + E, m);
    int keep = 0;
    for (int i = base; i < hi; i++) {
        const uint32_t e = L[retain ? (int)gI[i] : i];
        const int x = adp_x(e), y = adp_y(e);
        keep += x >= g.border && x < g.W - g.border && y >= g.border && y < g.H - g.border;
    }
    int o, d0, total, d1;
    block_scan_pair(keep, 0, o, d0, total, d1, bs);
    for (int i = base; i < hi; i++) {
        const uint32_t e = L[retain ? (int)gI[i] : i];
        const int x = adp_x(e), y = adp_y(e);
        if (!(x >= g.border && x < g.W - g.border && y >= g.border && y < g.H - g.border)) continue;
        float* K = kps + ((size_t)b * g.kp_cap + o) * 7;   // o < total <= m <= kp_cap
        K[0] = (float)x;
        K[1] = (float)y;
        K[2] = 7.0f;
        K[3] = -1.0f;
        K[4] = (float)adp_s(e);
        reinterpret_cast<int*>(K)[5] = 0;
        reinterpret_cast<int*>(K)[6] = -1;
        o++;
    }
    if (tid == 0) counts[b] = total;
}

// ------------------------------------------------------------------ steered BRIEF at the stored angle, one wave per keypoint
// k_cvorb_describe's test loop (lane = descriptor byte) without IC_Angle: cv::ORB::compute() on provided keypoints
// steers by KeyPoint::angle as it stands.  A keypoint lies at least 31 px inside the image and the rotated tests
// reach at most 18 px.
constexpr int kFastDescWaves = 4;
__constant__ CvPattern c_fast_pattern = make_cv_pattern();

__global__ __launch_bounds__(64 * kFastDescWaves) void k_fast_orb_describe(const uint8_t* __restrict__ blur, size_t frame_bytes, int st,
                                                                           FastCfg g, const int* __restrict__ counts,
                                                                           const float* __restrict__ kps, uint8_t* __restrict__ desc)
{
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int o = blockIdx.x * kFastDescWaves + (int)(threadIdx.x >> 6);
    if (o >= counts[b]) return;   // wave-uniform
    const size_t slot = (size_t)b * g.kp_cap + o;
    const float* K = kps + slot * 7;
    const int x = __float2int_rn(K[0]), y = __float2int_rn(K[1]);   // cvRound(kpt.pt) at layer scale 1
    float a, bs;
    cos_sin_f(K[3] * (float)(M_PI / 180.f), &a, &bs);
    if (lane < 32) {
        const uint8_t* ctr = blur + (size_t)b * frame_bytes + (size_t)y * st + x;
        int byte = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint32_t pw = c_fast_pattern.v[8 * lane + i];
            const float x0 = (float)(int8_t)(pw & 0xFFu), y0 = (float)(int8_t)((pw >> 8) & 0xFFu);
            const float x1 = (float)(int8_t)((pw >> 16) & 0xFFu), y1 = (float)(int8_t)(pw >> 24);
            const int t0 = ctr[(ptrdiff_t)__float2int_rn(x0 * bs + y0 * a) * st + __float2int_rn(x0 * a - y0 * bs)];
            const int t1 = ctr[(ptrdiff_t)__float2int_rn(x1 * bs + y1 * a) * st + __float2int_rn(x1 * a - y1 * bs)];
            byte |= (t0 < t1) << i;
        }
        desc[slot * 32 + lane] = (uint8_t)byte;
    }
}

__global__ __launch_bounds__(kFastThreads) void k_fast_retain_test(FastBufs w, int n, int nkeep, int depth_limit, int* __restrict__ order,
                                                                   int* __restrict__ m)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ SelLds sh;
    __shared__ BigLds bs;
    for (int i = threadIdx.x; i < n; i += blockDim.x) w.I[i] = (uint16_t)i;
    __syncthreads();
    int mm = n;
    if (n > nkeep) mm = nkeep > 0 ? retain_best_tiered(w.R, w.I, w.posL, w.posR, smem, n, nkeep, depth_limit, sh, bs) : 0;
    for (int i = threadIdx.x; i < mm; i += blockDim.x) order[i] = w.I[i];
    if (threadIdx.x == 0) *m = mm;
}

// ------------------------------------------------------------------ launchers
constexpr size_t kFastSelLds = (size_t)kFastLdsTier * 10 + 16;

hipError_t launch_fast_rows(const FastCfg& g, const FastBufs& w, int* err, int B, hipStream_t st)
{
    if (g.W > kFastRowThreads * 8 || g.thr < 1 || g.sstride < g.W) return hipErrorInvalidValue;   // a thread's columns are a 32-bit mask
    const hipError_t e = dispatch(k_fast_rows<false>, dim3(g.H, B), dim3(kFastRowThreads), 0, st, g, w.smap, w.rowc, w.cand, w.ncand,
                                  err);
    if (e != hipSuccess) return e;
    return dispatch(k_fast_rows<true>, dim3(g.H, B), dim3(kFastRowThreads), 0, st, g, w.smap, w.rowc, w.cand, w.ncand, err);
}

hipError_t launch_fast_select(const FastCfg& g, const FastBufs& w, int* counts, float* kps, int* err, int B, hipStream_t st)
{
    if (g.cand_cap > kFastMaxCandCap || g.nfeatures < 1) return hipErrorInvalidValue;   // 16-bit payloads and positions
    return dispatch(k_fast_select, dim3(B), dim3(kFastThreads), kFastSelLds, st, g, w, counts, kps, err);
}

hipError_t launch_fast_orb_describe(const uint8_t* blur, size_t frame_bytes, int stride, const FastCfg& g, const int* counts,
                                    const float* kps, uint8_t* desc, int B, hipStream_t st)
{
    if (g.border < 19) return hipErrorInvalidValue;   // the rotated tests' reach
    return dispatch(k_fast_orb_describe, dim3((g.kp_cap + kFastDescWaves - 1) / kFastDescWaves, B), dim3(64 * kFastDescWaves), 0, st,
                    blur, frame_bytes, stride, g, counts, kps, desc);
}

hipError_t launch_fast_retain_test(const FastBufs& w, int n, int nkeep, int depth_limit, int* order, int* m, hipStream_t st)
{
    if (n < 0 || n > kFastMaxCandCap) return hipErrorInvalidValue;
    return dispatch(k_fast_retain_test, dim3(1), dim3(kFastThreads), kFastSelLds, st, w, n, nkeep, depth_limit, order, m);
}

}  // namespace rgbd
