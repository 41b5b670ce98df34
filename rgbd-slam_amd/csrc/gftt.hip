// gftt.hip -- the reference's Extractor(GFTT, BRIEF, NORMAL) on gfx950: cv::GFTTDetector(nfeatures, 0.01, 3, 3,
// false, 0.04) (Features/Extractor.cpp:178-181), i.e. OpenCV 3.x's goodFeaturesToTrack restated (DESIGN.md,
// "GFTT + BRIEF definition"; tests/gftt_model.py is its executable form):
//   cornerMinEigenVal (Sobel 3x3, covariance products, 3x3 box sums, min eigenvalue)  -> gftt_tile_eig
//   minMaxLoc + threshold(TOZERO) + dilate + the candidate scan                        -> k_gftt_max, k_gftt_cand
//   std::sort(greaterThanPtr) + the min-distance greedy + runByImageBorder             -> k_gftt_select
// then BRIEF-32 (k_svo_brief on k_svo_pyramid's box sums) and k_undistort, as for the SVO front end.
//
// The eigenvalue map is never stored: pass A keeps the frame's maximum, pass B recomputes e per tile with a
// one-pixel halo, thresholds it and emits the candidates (an f32 map per frame would be written and read once
// each; the arithmetic is cheap beside that traffic).  The maximum and the emission are order-free: the
// maximum by an atomic on an order-preserving key, the candidates because their rank keys are unique and the
// selection sorts them.
#include <hip/hip_runtime.h>

#include "dispatch.h"

#include <cstdint>

#include "gftt_dev.h"
#include "wave_dev.h"

namespace rgbd {

// ------------------------------------------------------------------ the minimum-eigenvalue map of one tile
constexpr int kGtW = 64, kGtH = 16, kGtThreads = 256;

// BORDER_REFLECT_101, then clamped: coordinates more than one reflection out only address staging cells
// whose values are never used
__device__ __forceinline__ int gftt_r101(int i, int n)
{
    i = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
    return min(max(i, 0), n - 1);
}

// order-preserving u32 image of a float (no NaNs here): larger float <=> larger key, every key > 0
__device__ __forceinline__ uint32_t gftt_ord(float f)
{
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

template <int HALO>
struct GfttTile {
    static constexpr int EW = kGtW + 2 * HALO, EH = kGtH + 2 * HALO;   // e: the tile and its halo
    static constexpr int PW = EW + 2, PH = EH + 2;                     // covariance products: one more
    static constexpr int GW = PW + 2, GH = PH + 2;                     // gray: one more again
    uint8_t G[GH * GW];
    float P[3][PH * PW];
    float E[EH * EW];
};

// Fills t.E with e at the image pixels of the tile [x0, x0 + 64) x [y0, y0 + 16) and its HALO (cells outside
// the image hold 0 and are never read as neighbours of a candidate).  All f32 except the box sums, which are
// f64 in the order (l + c) + r, then (t + m) + b, rounded once.  Ends with a barrier.
template <int HALO>
__device__ void gftt_tile_eig(GfttTile<HALO>& t, const uint8_t* __restrict__ img, int W, int H, int x0, int y0)
{
    using T = GfttTile<HALO>;
    const int tid = threadIdx.x;
    for (int i = tid; i < T::GH * T::GW; i += kGtThreads) {
        const int r = i / T::GW, c = i - r * T::GW;
        const int y = gftt_r101(y0 - HALO - 2 + r, H), x = gftt_r101(x0 - HALO - 2 + c, W);
        t.G[i] = img[(size_t)y * W + x];
    }
    __syncthreads();
    const float s = (float)(1.0 / (4 * 3 * 255));
    for (int i = tid; i < T::PH * T::PW; i += kGtThreads) {
        const int r = i / T::PW, c = i - r * T::PW;
        const int y = y0 - HALO - 1 + r, x = x0 - HALO - 1 + c;
        float xx = 0.0f, xy = 0.0f, yy = 0.0f;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const uint8_t* q = t.G + (r + 1) * T::GW + (c + 1);
            const int a00 = q[-T::GW - 1], a01 = q[-T::GW], a02 = q[-T::GW + 1];
            const int a10 = q[-1], a12 = q[1];
            const int a20 = q[T::GW - 1], a21 = q[T::GW], a22 = q[T::GW + 1];
            const int dx = (a02 - a00) + 2 * (a12 - a10) + (a22 - a20);
            const int dy = (a20 - a00) + 2 * (a21 - a01) + (a22 - a02);
            const float Dx = (float)dx * s, Dy = (float)dy * s;
            xx = Dx * Dx;
            xy = Dx * Dy;
            yy = Dy * Dy;
        }
        t.P[0][i] = xx;
        t.P[1][i] = xy;
        t.P[2][i] = yy;
    }
    __syncthreads();
    for (int i = tid; i < T::EH * T::EW; i += kGtThreads) {
        const int r = i / T::EW, c = i - r * T::EW;
        const int y = y0 - HALO + r, x = x0 - HALO + c;
        float e = 0.0f;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            // REFLECT_101 on the product maps: column -1 is column 1, column W is column W - 2
            const int xo = x0 - HALO - 1, yo = y0 - HALO - 1;
            const int cx[3] = {(x - 1 < 0 ? 1 : x - 1) - xo, x - xo, (x + 1 >= W ? W - 2 : x + 1) - xo};
            const int ry[3] = {(y - 1 < 0 ? 1 : y - 1) - yo, y - yo, (y + 1 >= H ? H - 2 : y + 1) - yo};
            float S[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                double rows[3];
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const float* p = t.P[k] + ry[j] * T::PW;
                    rows[j] = ((double)p[cx[0]] + (double)p[cx[1]]) + (double)p[cx[2]];
                }
                S[k] = (float)((rows[0] + rows[1]) + rows[2]);
            }
            const float a = S[0] * 0.5f, b = S[1], cc = S[2] * 0.5f;
            e = (a + cc) - sqrtf((a - cc) * (a - cc) + b * b);
        }
        t.E[i] = e;
    }
    __syncthreads();
}

// pass A: the frame's largest e, as an order-preserving key (maxkey[b] cleared to 0 before the launch)
__global__ __launch_bounds__(kGtThreads) void k_gftt_max(const uint8_t* __restrict__ gray, size_t frame_bytes, GfttCfg g,
                                                         uint32_t* __restrict__ maxkey)
{
    __shared__ GfttTile<0> t;
    __shared__ uint32_t best;
    const int tid = threadIdx.x, b = blockIdx.z, x0 = blockIdx.x * kGtW, y0 = blockIdx.y * kGtH;
    if (tid == 0) best = 0;
    gftt_tile_eig<0>(t, gray + (size_t)b * frame_bytes, g.W, g.H, x0, y0);
    uint32_t m = 0;
    for (int i = tid; i < kGtH * kGtW; i += kGtThreads) {
        const int r = i / kGtW, c = i - r * kGtW;
        if (x0 + c < g.W && y0 + r < g.H) m = max(m, gftt_ord(t.E[i]));
    }
    if (m) atomicMax(&best, m);
    __syncthreads();
    if (tid == 0 && best) atomicMax(maxkey + b, best);
}

// the raw map of one frame (rgbd_gftt_debug_eig): the same tile code, stored
__global__ __launch_bounds__(kGtThreads) void k_gftt_eig(const uint8_t* __restrict__ gray, GfttCfg g, float* __restrict__ out)
{
    __shared__ GfttTile<0> t;
    const int tid = threadIdx.x, x0 = blockIdx.x * kGtW, y0 = blockIdx.y * kGtH;
    gftt_tile_eig<0>(t, gray, g.W, g.H, x0, y0);
    for (int i = tid; i < kGtH * kGtW; i += kGtThreads) {
        const int r = i / kGtW, c = i - r * kGtW;
        if (x0 + c < g.W && y0 + r < g.H) out[(size_t)(y0 + r) * g.W + x0 + c] = t.E[i];
    }
}

// pass B: thr = (float)((double)M * quality_level); a pixel with 1 <= x < W-1, 1 <= y < H-1 is a candidate
// when its thresholded value (e > thr ? e : 0) is not 0 and equals the largest thresholded value of its 3x3
// neighbourhood.  A tile's candidates are collected in LDS and appended to the frame's list with one atomic.
__global__ __launch_bounds__(kGtThreads) void k_gftt_cand(const uint8_t* __restrict__ gray, size_t frame_bytes, GfttCfg g,
                                                          const uint32_t* __restrict__ maxkey, uint64_t* __restrict__ keys,
                                                          int* __restrict__ ncand, int* __restrict__ err)
{
    __shared__ GfttTile<1> t;
    __shared__ uint64_t L[kGtW * kGtH];
    __shared__ int nl, base;
    using T = GfttTile<1>;
    const int tid = threadIdx.x, b = blockIdx.z, x0 = blockIdx.x * kGtW, y0 = blockIdx.y * kGtH;
    if (tid == 0) nl = 0;
    gftt_tile_eig<1>(t, gray + (size_t)b * frame_bytes, g.W, g.H, x0, y0);
    const float M = gftt_decode_max(maxkey[b]);
    const float thr = (float)((double)M * g.quality_level);
    for (int i = tid; i < kGtH * kGtW; i += kGtThreads) {
        const int r = i / kGtW, c = i - r * kGtW;
        const int x = x0 + c, y = y0 + r;
        if (x < 1 || x >= g.W - 1 || y < 1 || y >= g.H - 1) continue;
        const float* q = t.E + (r + 1) * T::EW + (c + 1);
        const float e = q[0];
        const float v = e > thr ? e : 0.0f;
        if (v == 0.0f) continue;
        float mx = v;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const float w = q[dy * T::EW + dx];
                mx = fmaxf(mx, w > thr ? w : 0.0f);
            }
        if (v == mx) L[atomicAdd(&nl, 1)] = gftt_key(__float_as_uint(e), (uint32_t)(y * g.W + x));
    }
    __syncthreads();
    const int n = nl;
    if (n == 0) return;
    if (tid == 0) {
        base = atomicAdd(ncand + b, n);
        if (base + n > g.cand_cap) atomicOr(err + b, kGfttErrFlag);
    }
    __syncthreads();
    uint64_t* K = keys + (size_t)b * g.cand_cap;
    for (int i = tid; i < n; i += kGtThreads)
        if (base + i < g.cand_cap) K[base + i] = L[i];
}

// ------------------------------------------------------------------ rank + spacing + keypoints, one workgroup per frame
// The greedy consumes little more than one rank per accepted corner, so the list is not sorted whole.  Per pass:
//   1. the next `chunk` ranks below the previous pass's last key: a radix select (six 11-bit digits of the
//      64-bit key, histograms in LDS) finds the chunk's smallest key, a gather collects the chunk (keys are
//      unique, so exactly that many lie in the range), a bitonic sort in LDS puts it in rank order;
//   2. the spacing on the chunk: candidates within min_distance of a corner accepted by an earlier pass are
//      rejected; then rounds in which an undecided candidate is rejected if an accepted higher-ranked one of
//      the chunk lies within min_distance, and accepted if none is accepted and none undecided.  A decision
//      only reads final states (an undecided neighbour defers it), so the outcome is the sequential walk's
//      whatever the interleaving; rounds run until nothing is undecided (a monotone ridge is a chain as long
//      as the ridge);
//   3. the accepted ones are appended in rank order, up to nfeatures.
// Walking the ranks in chunks is the sequential walk, so the result is exact.
constexpr uint32_t kQxy = (1u << 22) - 1;   // Q: x (11 bits) | y << 11 | state << 22 (0 undecided, 1 accepted, 2 rejected)

struct GfttSelLds {
    int hist[2048];
    int wsum[16];
    int digit, kk, flag, slots, last;
};

__device__ __forceinline__ int gftt_block_scan(int v, int& total, GfttSelLds& sh)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int iv = wave_incl_scan(v);
    if (lane == 63) sh.wsum[w] = iv;
    __syncthreads();
    int pre = 0, tot = 0;
    for (int i = 0; i < nw; i++) {
        const int x = sh.wsum[i];
        pre += i < w ? x : 0;
        tot += x;
    }
    __syncthreads();
    total = tot;
    return pre + iv - v;
}

__device__ __forceinline__ bool gftt_near(uint32_t a, uint32_t b, int lim)
{
    const int dx = (int)(a & 2047u) - (int)(b & 2047u), dy = (int)((a >> 11) & 2047u) - (int)((b >> 11) & 2047u);
    return dx * dx + dy * dy < lim;
}

__global__ __launch_bounds__(kGfttSelThreads) void k_gftt_select(const uint64_t* __restrict__ keys, const int* __restrict__ ncand,
                                                                 int n_fixed, GfttCfg g, uint64_t* __restrict__ corners,
                                                                 int* __restrict__ ncorner, int* __restrict__ ranks,
                                                                 int* __restrict__ counts, float* __restrict__ kps, int P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ GfttSelLds sh;
    uint64_t* S = reinterpret_cast<uint64_t*>(smem);       // [P] the chunk in rank order
    uint32_t* Q = reinterpret_cast<uint32_t*>(S + P);      // [P] its positions and states
    uint32_t* A = Q + P;                                   // [nfeatures] accepted corners' positions
    const int tid = threadIdx.x, T = blockDim.x, b = blockIdx.x;
    const uint64_t* K = keys + (size_t)b * g.cand_cap;
    const int n = min(ncand ? ncand[b] : n_fixed, g.cand_cap);
    const int nfeat = g.nfeatures, lim = g.dist_lim;
    uint64_t* C = corners + (size_t)b * nfeat;
    uint64_t bound = ~0ull;      // keys of earlier passes are >= bound
    int consumed = 0, nacc = 0, used = 0;
    while (nacc < nfeat && consumed < n) {
        const int k = min(g.chunk, n - consumed);
        // 1a. T0 = the k-th largest key below bound (0: the pass takes all that remain)
        uint64_t T0 = 0;
        if (k < n - consumed) {
            int kk = k;
            for (int p = 5; p >= 0; p--) {
                const int shift = 11 * p;
                for (int i = tid; i < 2048; i += T) sh.hist[i] = 0;
                __syncthreads();
                // the high digits of most keys agree (eigenvalues share their exponent bits): a wave whose keys
                // all fall into one bin adds its count once
                for (int i0 = 0; i0 < n; i0 += T) {
                    const int i = i0 + tid;
                    const uint64_t key = i < n ? K[i] : 0ull;
                    const uint64_t hi = p == 5 ? 0ull : key >> (shift + 11);
                    const bool in = i < n && key < bound && hi == T0;
                    const int d = in ? (int)((key >> shift) & 2047u) : -1;
                    const unsigned long long mask = __ballot(in);
                    if (mask == 0) continue;
                    const int leader = __ffsll(mask) - 1;
                    const int f = __shfl(d, leader);
                    if (__all(!in || d == f)) {
                        if ((tid & 63) == leader) atomicAdd(&sh.hist[f], __popcll(mask));
                    } else if (in) {
                        atomicAdd(&sh.hist[d], 1);
                    }
                }
                __syncthreads();
                if (tid < 64) {   // lane l owns bins 2047 - 32 l down to 2016 - 32 l: descending digits
                    const int top = 2047 - 32 * tid;
                    int s = 0;
                    for (int j = 0; j < 32; j++) s += sh.hist[top - j];
                    const int incl = wave_incl_scan(s);
                    int c = incl - s;
                    if (c < kk && kk <= incl) {
                        for (int j = 0; j < 32; j++) {
                            const int c2 = c + sh.hist[top - j];
                            if (kk <= c2) {
                                sh.digit = top - j;
                                sh.kk = kk - c;
                                break;
                            }
                            c = c2;
                        }
                    }
                }
                __syncthreads();
                T0 = (T0 << 11) | (uint64_t)sh.digit;
                kk = sh.kk;
            }
        }
        // 1b. gather and sort (descending); Pp = the power of two at or above k
        int Pp = 1;
        while (Pp < k) Pp *= 2;
        if (tid == 0) sh.slots = 0;
        for (int i = tid; i < Pp; i += T) S[i] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += T) {
            const uint64_t key = K[i];
            if (key < bound && key >= T0) {
                const int slot = atomicAdd(&sh.slots, 1);
                if (slot < k) S[slot] = key;
            }
        }
        for (int size = 2; size <= Pp; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                __syncthreads();
                for (int i = tid; i < Pp / 2; i += T) {
                    const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                    const uint64_t a = S[lo], c = S[hi];
                    if ((a < c) == ((lo & size) == 0)) {
                        S[lo] = c;
                        S[hi] = a;
                    }
                }
            }
        __syncthreads();
        // 2. positions; candidates near a corner of an earlier pass are rejected
        for (int i = tid; i < k; i += T) {
            const uint32_t idx = (uint32_t)S[i];
            const uint32_t y = idx / (uint32_t)g.W, x = idx - y * (uint32_t)g.W;
            uint32_t q = x | (y << 11);
            if (lim == 0)
                q |= 1u << 22;
            else
                for (int a = 0; a < nacc; a++)
                    if (gftt_near(q, A[a], lim)) {
                        q |= 2u << 22;
                        break;
                    }
            Q[i] = q;
        }
        if (lim != 0) {
            int more;
            do {
                __syncthreads();
                if (tid == 0) sh.flag = 0;
                __syncthreads();
                // Within a round other threads store Q[j] while it is read here: a word changes once, from
                // undecided to its final state, and a stale "undecided" only defers the decision.  The accesses
                // are relaxed atomics, so each is one whole-word load or store and none is repeated or torn.
                for (int i = tid; i < k; i += T) {
                    const uint32_t q = __atomic_load_n(&Q[i], __ATOMIC_RELAXED);
                    if (q >> 22) continue;
                    int st = 1;   // accepted unless a neighbour says otherwise
                    for (int j = 0; j < i; j++) {
                        const uint32_t o = __atomic_load_n(&Q[j], __ATOMIC_RELAXED);
                        if ((o >> 22) == 2u || !gftt_near(q, o, lim)) continue;
                        if ((o >> 22) == 1u) {
                            st = 2;
                            break;
                        }
                        st = 0;
                    }
                    if (st)
                        __atomic_store_n(&Q[i], q | ((uint32_t)st << 22), __ATOMIC_RELAXED);
                    else
                        sh.flag = 1;
                }
                __syncthreads();
                more = sh.flag;
            } while (more);
        }
        __syncthreads();
        // 3. append the accepted in rank order
        const int E = (k + T - 1) / T, lo = tid * E, hi = min(lo + E, k);
        int cnt = 0;
        for (int i = lo; i < hi; i++) cnt += (Q[i] >> 22) == 1u;
        if (tid == 0) sh.last = -1;
        int tot;
        int pos = nacc + gftt_block_scan(cnt, tot, sh);
        for (int i = lo; i < hi; i++)
            if ((Q[i] >> 22) == 1u) {
                if (pos < nfeat) {
                    A[pos] = Q[i] & kQxy;
                    C[pos] = S[i];
                    if (pos == nfeat - 1) sh.last = i;
                }
                pos++;
            }
        __syncthreads();
        if (nacc + tot >= nfeat) {
            used = consumed + sh.last + 1;
            nacc = nfeat;
            break;
        }
        nacc += tot;
        consumed += k;
        used = consumed;
        bound = S[k - 1];
        __syncthreads();   // S, Q and sh are rewritten by the next pass
    }
    __syncthreads();
    if (tid == 0) {
        ncorner[b] = nacc;
        ranks[b] = used;
    }
    if (!kps) return;
    // runByImageBorder(28) (a stable remove_if), then cv::KeyPoint(x, y, 3.f): angle -1, response 0, octave 0,
    // class_id -1
    const int E = (nacc + T - 1) / T, lo = tid * E, hi = min(lo + E, nacc);
    int keep = 0;
    for (int i = lo; i < hi; i++) {
        const int x = (int)(A[i] & 2047u), y = (int)(A[i] >> 11);
        keep += x >= g.border && x < g.W - g.border && y >= g.border && y < g.H - g.border;
    }
    int total;
    int o = gftt_block_scan(keep, total, sh);
    for (int i = lo; i < hi; i++) {
        const int x = (int)(A[i] & 2047u), y = (int)(A[i] >> 11);
        if (!(x >= g.border && x < g.W - g.border && y >= g.border && y < g.H - g.border)) continue;
        float* Kp = kps + ((size_t)b * g.kp_cap + o) * 7;
        Kp[0] = (float)x;
        Kp[1] = (float)y;
        Kp[2] = 3.0f;
        Kp[3] = -1.0f;
        Kp[4] = 0.0f;
        reinterpret_cast<int*>(Kp)[5] = 0;
        reinterpret_cast<int*>(Kp)[6] = -1;
        o++;
    }
    if (tid == 0) counts[b] = total;
}

// ------------------------------------------------------------------ launchers
hipError_t launch_gftt_max(const uint8_t* gray, size_t frame_bytes, const GfttCfg& g, uint32_t* maxkey, int B, hipStream_t st)
{
    return dispatch(k_gftt_max, dim3((g.W + kGtW - 1) / kGtW, (g.H + kGtH - 1) / kGtH, B), dim3(kGtThreads), 0, st, gray,
                    frame_bytes, g, maxkey);
}

hipError_t launch_gftt_cand(const uint8_t* gray, size_t frame_bytes, const GfttCfg& g, const uint32_t* maxkey, uint64_t* keys,
                            int* ncand, int* err, int B, hipStream_t st)
{
    return dispatch(k_gftt_cand, dim3((g.W + kGtW - 1) / kGtW, (g.H + kGtH - 1) / kGtH, B), dim3(kGtThreads), 0, st, gray,
                    frame_bytes, g, maxkey, keys, ncand, err);
}

hipError_t launch_gftt_eig(const uint8_t* gray, const GfttCfg& g, float* out, hipStream_t st)
{
    return dispatch(k_gftt_eig, dim3((g.W + kGtW - 1) / kGtW, (g.H + kGtH - 1) / kGtH), dim3(kGtThreads), 0, st, gray, g, out);
}

hipError_t launch_gftt_select(const uint64_t* keys, const int* ncand, int n_fixed, const GfttCfg& g, uint64_t* corners,
                              int* ncorner, int* ranks, int* counts, float* kps, int B, hipStream_t st)
{
    if (g.chunk < 1 || g.chunk > kGfttMaxChunk || g.nfeatures < 1 || g.nfeatures > kGfttMaxCorners || g.W < 1 || g.W > 2047 ||
        g.H < 1 || g.H > 2047 || g.cand_cap < 1)
        return hipErrorInvalidValue;
    int P = 1;
    while (P < g.chunk) P *= 2;
    const size_t lds = (size_t)P * 12 + (size_t)g.nfeatures * 4;
    return dispatch(k_gftt_select, dim3(B), dim3(kGfttSelThreads), lds, st, keys, ncand, n_fixed, g, corners, ncorner, ranks,
                    counts, kps, P);
}

}  // namespace rgbd
