// project.hip -- projection-guided matching on gfx950.
//
// Reference: Matcher::projectionMatch (Features/Matcher.cpp:35-104) over Frame::unprojectWorld
//   (Core/Frame.cpp:317-327), Frame::getFeaturesInArea (:179-229) and the 64 x 48 grid of
//   assignFeaturesToGrid / posInGrid (:75-89, :231-241).  The operator is DESIGN.md "Projection match
//   definition"; this file follows its step numbers.
//
// Per pair (query frame F1, train frame F2), three launches:
//   k_proj_grid    one workgroup: a stable counting sort of F2's keypoints by cell column x 48 + cell row.  A
//                  query's candidates are then at most 64 contiguous runs of the sorted array (one per cell
//                  column of its window), and a keypoint's sorted position IS its rank in the reference's
//                  visiting order, so the rank key (distance << 16 | position) orders candidates as the
//                  reference's strict '<' scan does.
//   k_proj_search  one lane per query: steps 1-7, then the kProjKeys smallest keys with distance <= TH_HIGH
//                  among the z-valid candidates, ascending, and a flag when more exist.  Train sets of up to
//                  kSearchLdsTrains keypoints take the LDS form (k_proj_search_lds: one workgroup per pair, the
//                  sorted train set staged in LDS once), larger ones read it from global memory.
//   k_proj_assign  one workgroup: the greedy assignment of step 8, exact, in rounds (below).
// Loop bounds: the grid's placement loop runs once per distinct cell of a 64-keypoint chunk (<= 64); a window
// scan visits <= 64 runs of <= n2 keypoints; the assignment runs <= n1 + 1 rounds (the lowest unresolved query
// is final in every round).
#include <hip/hip_runtime.h>

#include "dispatch.h"
#include "project_dev.h"
#include "rgbd_internal.h"
#include "undistort_dev.h"

namespace rgbd {

// ---------------------------------------------------------------- image bounds
// Frame::computeImageBounds (Core/Frame.cpp:283-315): the corners (0,0), (W,0), (0,H), (W,H) through
// k_undistort's undistortion; out = (min_x, max_x, min_y, max_y)
__global__ void k_proj_bounds(const ExtractCfg* __restrict__ cfgp, float* __restrict__ out)
{
    const ExtractCfg& cfg = *cfgp;
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float W = (float)cfg.W, H = (float)cfg.H;
    const float cxs[4] = {0.f, W, 0.f, W}, cys[4] = {0.f, 0.f, H, H};
    float x[4], y[4];
#pragma unroll
    for (int i = 0; i < 4; i++) undistort_point(cfg, cxs[i], cys[i], &x[i], &y[i]);
    out[0] = fminf(x[0], x[2]);
    out[1] = fmaxf(x[1], x[3]);
    out[2] = fminf(y[0], y[1]);
    out[3] = fmaxf(y[2], y[3]);
}

// ---------------------------------------------------------------- grid
// round(): half away from zero, exact (v - trunc(v) is exact in f32)
__device__ __forceinline__ float round_away(float v)
{
    const float t = truncf(v);
    return fabsf(v - t) >= 0.5f ? t + copysignf(1.0f, v) : t;
}

// posInGrid (Core/Frame.cpp:231-241): column x 48 + row, or -1 outside the grid (NaN included)
__device__ __forceinline__ int proj_cell(const ProjCfg& g, float x, float y)
{
    const float fc = round_away((x - g.min_x) * g.winv), fr = round_away((y - g.min_y) * g.hinv);
    if (!(fc >= 0.f && fc < (float)kProjCols && fr >= 0.f && fr < (float)kProjRows)) return -1;
    return (int)fc * kProjRows + (int)fr;
}

constexpr int kGridThreads = 512;
constexpr int kGridWaves = kGridThreads / 64;
constexpr int kGridPer = kProjCells / kGridThreads;   // cells scanned per thread
static_assert(kGridPer * kGridThreads == kProjCells, "the cell scan gives every thread the same number of cells");
static_assert((kGridWaves & (kGridWaves - 1)) == 0, "cells are dealt to the waves by their low bits");

__global__ __launch_bounds__(kGridThreads) void k_proj_grid(ProjFrames f, ProjCfg g, ProjWork w)
{
    __shared__ int cnt[kProjCells];   // the histogram, then every cell's next free position
    __shared__ int wsum[kGridWaves];
    const int p = blockIdx.x;
    if (f.qf[p] < 0) return;   // pair not requested
    const int tframe = f.tf[p];
    const int n2 = min(f.counts[tframe], w.tcap);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* kun = f.kun + (size_t)tframe * f.cap * 7;
    for (int i = tid; i < kProjCells; i += kGridThreads) cnt[i] = 0;
    __syncthreads();
    for (int i = tid; i < n2; i += kGridThreads) {
        const int c = proj_cell(g, kun[(size_t)i * 7], kun[(size_t)i * 7 + 1]);
        if (c >= 0) atomicAdd(&cnt[c], 1);
    }
    __syncthreads();
    // exclusive scan of the cell counts: kGridPer consecutive cells per thread
    int loc[kGridPer], s = 0;
#pragma unroll
    for (int k = 0; k < kGridPer; k++) {
        loc[k] = cnt[kGridPer * tid + k];
        s += loc[k];
    }
    int inc = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int excl = inc - s;
    for (int i = 0; i < wv; i++) excl += wsum[i];
    int* cell_off = w.cell_off + (size_t)p * (kProjCells + 1);
#pragma unroll
    for (int k = 0; k < kGridPer; k++) {
        cell_off[kGridPer * tid + k] = excl;
        cnt[kGridPer * tid + k] = excl;
        excl += loc[k];
    }
    if (tid == kGridThreads - 1) cell_off[kProjCells] = excl;
    __syncthreads();
    // stable placement: every wave walks all keypoints in index order, 64 at a time, and places those whose
    // cell it owns (cell % kGridWaves), one distinct cell of the chunk per step, so a cell's members keep
    // their index order and no two waves touch one cursor.  This pass only decides positions (the pair's minq
    // row, free until k_proj_assign, holds them); the data moves in the parallel pass after it
    uint32_t* pos_of = w.minq + (size_t)p * w.tcap;
    volatile int* cursor = cnt;
    float nx = 0.f, ny = 0.f;   // the next chunk's keypoint, loaded one chunk ahead
    if (lane < n2) {
        nx = kun[(size_t)lane * 7];
        ny = kun[(size_t)lane * 7 + 1];
    }
    for (int base = 0; base < n2; base += 64) {
        const int i = base + lane;
        const float x = nx, y = ny;
        if (i + 64 < n2) {
            nx = kun[(size_t)(i + 64) * 7];
            ny = kun[(size_t)(i + 64) * 7 + 1];
        }
        const int c = i < n2 ? proj_cell(g, x, y) : -1;
        const bool mine = c >= 0 && (c & (kGridWaves - 1)) == wv;
        int pos = -1;
        unsigned long long pend = __ballot(mine);
        while (pend) {   // <= 64 steps: every step retires at least the leader
            const int leader = __ffsll((long long)pend) - 1;
            const int lc = __shfl(c, leader, 64);
            const unsigned long long same = __ballot(mine && c == lc);
            const int cur = cursor[lc];   // every lane reads before the leader's store: one wave, LDS in order
            if (mine && c == lc) pos = cur + __popcll(same & ((1ull << lane) - 1ull));
            if (lane == leader) cursor[lc] = cur + __popcll(same);
            pend &= ~same;
        }
        if (mine) pos_of[i] = (uint32_t)pos;
        else if (i < n2 && c < 0 && wv == 0) pos_of[i] = kProjEmpty;   // in no cell
    }
    __syncthreads();
    float4* s_rec = w.s_rec + (size_t)p * w.tcap;
    uint4* s_desc = w.s_desc + (size_t)p * w.tcap * 2;
    const float* xyz = f.xyz + (size_t)tframe * f.cap * 3;
    const uint4* desc = reinterpret_cast<const uint4*>(f.desc + (size_t)tframe * f.cap * 32);
    for (int i = tid; i < n2; i += kGridThreads) {
        const uint32_t pos = pos_of[i];
        if (pos == kProjEmpty) continue;
        const uint32_t iw = (uint32_t)i | (xyz[(size_t)i * 3 + 2] > 0 ? 0x10000u : 0u);
        s_rec[pos] = make_float4(kun[(size_t)i * 7], kun[(size_t)i * 7 + 1], __uint_as_float(iw), 0.f);
        s_desc[2 * (size_t)pos] = desc[2 * (size_t)i];
        s_desc[2 * (size_t)pos + 1] = desc[2 * (size_t)i + 1];
    }
}

// ---------------------------------------------------------------- window scan
__device__ __forceinline__ int hamming(const uint32_t (&q)[8], const uint4& a, const uint4& b)
{
    return __popc(q[0] ^ a.x) + __popc(q[1] ^ a.y) + __popc(q[2] ^ a.z) + __popc(q[3] ^ a.w) + __popc(q[4] ^ b.x) +
           __popc(q[5] ^ b.y) + __popc(q[6] ^ b.z) + __popc(q[7] ^ b.w);
}

// one key into the ascending array (keys are unique: the position is part of the key); true when a key fell
// off the end
__device__ __forceinline__ bool key_insert(uint32_t (&a)[kProjKeys], uint32_t key)
{
#pragma unroll
    for (int i = 0; i < kProjKeys; i++) {
        const uint32_t lo = min(a[i], key);
        key = max(a[i], key);
        a[i] = lo;
    }
    return key != kProjEmpty;
}

// step 7: the window's cells column by column, rows inside a column, members in index order = <= 64 runs of
// the sorted array; fn(position, index word, descriptor) for every member with |dx| < th and |dy| < th.  The
// next column's run bounds and the next member's record and descriptor are loaded one step ahead, so a member
// costs one memory round trip (the descriptor of a member that fails the distance test is loaded in vain:
// about three in four at th = 5, 32 B each, from L2).
template <typename F>
__device__ __forceinline__ void scan_window(const ProjCfg& g, float u, float v, uint32_t win, const int* __restrict__ cell_off,
                                            const float4* __restrict__ s_rec, const uint4* __restrict__ s_desc, F&& fn)
{
    const int c0 = win & 0xFF, c1 = (win >> 8) & 0xFF, r0 = (win >> 16) & 0xFF, r1 = win >> 24;
    int nb = cell_off[c0 * kProjRows + r0], ne = cell_off[c0 * kProjRows + r1 + 1];
    for (int ix = c0; ix <= c1; ix++) {
        const int b = nb, e = ne;
        if (ix < c1) {
            nb = cell_off[(ix + 1) * kProjRows + r0];
            ne = cell_off[(ix + 1) * kProjRows + r1 + 1];
        }
        if (b >= e) continue;
        float4 nr = s_rec[b];
        uint4 nd0 = s_desc[2 * (size_t)b], nd1 = s_desc[2 * (size_t)b + 1];
        for (int pos = b; pos < e; pos++) {
            const float4 rec = nr;
            const uint4 d0 = nd0, d1 = nd1;
            if (pos + 1 < e) {
                nr = s_rec[pos + 1];
                nd0 = s_desc[2 * (size_t)(pos + 1)];
                nd1 = s_desc[2 * (size_t)(pos + 1) + 1];
            }
            if (fabsf(rec.x - u) < g.th && fabsf(rec.y - v) < g.th) fn(pos, __float_as_uint(rec.z), d0, d1);
        }
    }
}

__device__ __forceinline__ void load_desc(const uint8_t* desc, size_t row, uint32_t (&qd)[8])
{
    const uint4* r = reinterpret_cast<const uint4*>(desc + row * 32);
    const uint4 a = r[0], b = r[1];
    qd[0] = a.x; qd[1] = a.y; qd[2] = a.z; qd[3] = a.w;
    qd[4] = b.x; qd[5] = b.y; qd[6] = b.z; qd[7] = b.w;
}

// ---------------------------------------------------------------- search
// cv::Mat arithmetic (DESIGN.md "cv::Mat conventions"): every product sum of a gemm runs in double in k order
// and is rounded to float once
// One query: steps 1-7 and the kept keys.  cell_off / s_rec / s_desc: the pair's sorted train set, in global
// memory or staged in LDS.
template <bool DEBUG>
__device__ __forceinline__ void search_one(const ProjFrames& f, const ProjCfg& g, const ProjWork& w, int p, int qframe, int tframe,
                                           int q, const int* __restrict__ cell_off, const float4* __restrict__ s_rec,
                                           const uint4* __restrict__ s_desc)
{
    const size_t qo = (size_t)p * w.qcap + q;
    const size_t row = (size_t)qframe * f.cap + q;
    int status = kProjSearched;
    float u = 0.f, v = 0.f;
    uint32_t win = 0;
    const float* X = f.xyz + row * 3;
    if (f.outlier && f.outlier[row]) status = kProjOutlier;        // step 1
    else if (!(X[2] > 0)) status = kProjNoDepth;
    else {
        const float* T1 = f.poses + (size_t)qframe * 16;
        const float* T2 = f.poses + (size_t)tframe * 16;
        float xw[3], xc[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {   // step 2: mOw = -Rcw^T tcw, then Rwc x + mOw as one gemm
            double o = 0.0, a = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                o += (double)T1[4 * k + r] * (double)T1[4 * k + 3];
                a += (double)T1[4 * k + r] * (double)X[k];
            }
            const float Ow = (float)(o * -1.0);
            xw[r] = (float)(a + (double)Ow);
        }
#pragma unroll
        for (int r = 0; r < 3; r++) {   // step 3: Rcw xw + tcw as one gemm
            double a = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) a += (double)T2[4 * r + k] * (double)xw[k];
            xc[r] = (float)(a + (double)T2[4 * r + 3]);
        }
        const float inv = 1.0f / xc[2];   // step 4
        if (inv < 0) status = kProjBehind;
        else {
            u = (g.fx * xc[0]) * inv + g.cx;
            v = (g.fy * xc[1]) * inv + g.cy;
            if (!(u >= g.min_x && u <= g.max_x && v >= g.min_y && v <= g.max_y)) status = kProjOutside;   // step 5, NaN skipped
            else {   // step 6; the comparisons run on the floats, so no out-of-range float is converted
                const float c0f = floorf(((u - g.min_x) - g.th) * g.winv), c1f = ceilf(((u - g.min_x) + g.th) * g.winv);
                const float r0f = floorf(((v - g.min_y) - g.th) * g.hinv), r1f = ceilf(((v - g.min_y) + g.th) * g.hinv);
                if (!(c0f < (float)kProjCols) || !(c1f >= 0.f) || !(r0f < (float)kProjRows) || !(r1f >= 0.f)) status = kProjNoCells;
                else {
                    const int c0 = c0f > 0.f ? (int)c0f : 0, c1 = c1f < (float)(kProjCols - 1) ? (int)c1f : kProjCols - 1;
                    const int r0 = r0f > 0.f ? (int)r0f : 0, r1 = r1f < (float)(kProjRows - 1) ? (int)r1f : kProjRows - 1;
                    win = (uint32_t)c0 | (uint32_t)c1 << 8 | (uint32_t)r0 << 16 | (uint32_t)r1 << 24;
                }
            }
        }
    }
    w.uv[qo] = make_float2(u, v);
    w.win[qo] = win;
    w.status[qo] = status;
    uint32_t keys[kProjKeys];
#pragma unroll
    for (int i = 0; i < kProjKeys; i++) keys[i] = kProjEmpty;
    bool more = false;
    int ncand = 0;
    if (status == kProjSearched) {
        uint32_t qd[8];
        load_desc(f.desc, row, qd);
        scan_window(g, u, v, win, cell_off, s_rec, s_desc, [&](int pos, uint32_t iw, const uint4& d0, const uint4& d1) {
            if (DEBUG) {
                if (ncand < w.ccap) w.cand[(size_t)q * w.ccap + ncand] = (int)(iw & 0xFFFFu);
                ncand++;
            }
            if (!(iw & 0x10000u)) return;   // isValidObs(i2)
            const int d = hamming(qd, d0, d1);
            if (d <= kProjThHigh) more |= key_insert(keys, (uint32_t)d << 16 | (uint32_t)pos);
        });
    }
    if (DEBUG) w.ccount[q] = ncand;
    uint4* ko = reinterpret_cast<uint4*>(w.keys + qo * kProjKeys);
#pragma unroll
    for (int i = 0; i < kProjKeys / 4; i++) ko[i] = make_uint4(keys[4 * i], keys[4 * i + 1], keys[4 * i + 2], keys[4 * i + 3]);
    w.more[qo] = more ? 1 : 0;
    w.head[qo] = 0;
    w.res[qo] = keys[0] == kProjEmpty ? kProjNoMatch : kProjUnresolved;
}

// Global form: one lane per query, any train count.
constexpr int kSearchThreads = 256;
template <bool DEBUG>
__global__ __launch_bounds__(kSearchThreads) void k_proj_search(ProjFrames f, ProjCfg g, ProjWork w)
{
    const int p = blockIdx.y;
    const int qframe = f.qf[p];
    if (qframe < 0) return;
    const int n1 = min(f.counts[qframe], w.qcap);
    const int q = blockIdx.x * kSearchThreads + threadIdx.x;
    if (q >= n1) return;
    search_one<DEBUG>(f, g, w, p, qframe, f.tf[p], q, w.cell_off + (size_t)p * (kProjCells + 1), w.s_rec + (size_t)p * w.tcap,
                      w.s_desc + (size_t)p * w.tcap * 2);
}

// LDS form, for train sets of up to kSearchLdsTrains keypoints (lds_trains of them fit this launch): one workgroup
// per pair stages the cell offsets and the sorted records and descriptors (48 B per train) in LDS once, then its
// lanes take the pair's queries; a window scan then costs LDS round trips, not global ones.
constexpr int kSearchLdsThreads = 1024;
constexpr int kSearchLdsTrains = 3072;
constexpr int kSearchLdsCells = (kProjCells + 1 + 3) & ~3;   // ints, so the records after them stay 16-byte aligned
template <bool DEBUG>
__global__ __launch_bounds__(kSearchLdsThreads) void k_proj_search_lds(ProjFrames f, ProjCfg g, ProjWork w, int lds_trains)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t search_lds[];
    int* l_off = reinterpret_cast<int*>(search_lds);
    float4* l_rec = reinterpret_cast<float4*>(l_off + kSearchLdsCells);
    uint4* l_desc = reinterpret_cast<uint4*>(l_rec + lds_trains);
    const int p = blockIdx.x;
    const int qframe = f.qf[p];
    if (qframe < 0) return;
    const int tframe = f.tf[p];
    const int n1 = min(f.counts[qframe], w.qcap);
    const int* cell_off = w.cell_off + (size_t)p * (kProjCells + 1);
    const int ns = min(cell_off[kProjCells], lds_trains);   // trains inside the grid
    const float4* s_rec = w.s_rec + (size_t)p * w.tcap;
    const uint4* s_desc = w.s_desc + (size_t)p * w.tcap * 2;
    for (int i = threadIdx.x; i <= kProjCells; i += kSearchLdsThreads) l_off[i] = cell_off[i];
    for (int i = threadIdx.x; i < ns; i += kSearchLdsThreads) l_rec[i] = s_rec[i];
    for (int i = threadIdx.x; i < 2 * ns; i += kSearchLdsThreads) l_desc[i] = s_desc[i];
    __syncthreads();
    for (int q = threadIdx.x; q < n1; q += kSearchLdsThreads) search_one<DEBUG>(f, g, w, p, qframe, tframe, q, l_off, l_rec, l_desc);
}

// ---------------------------------------------------------------- greedy assignment
// Step 8 is sequential in query order: a query takes its best candidate that no earlier query took.  The same
// result in rounds.  Every round:
//   a. an unresolved query drops the keys at the head of its list whose train is taken; an empty list resolves it
//      to "no match" (a truncated list is first rebuilt from the window, taken trains skipped);
//   b. it writes its index into minq[t] (atomic min) for every train t left on its list (a truncated list: for
//      every untaken candidate of its window);
//   c. it takes the train t at its head when minq[t] is its own index.
// c is what the sequential loop does: no earlier unresolved query lists t at all, so none can take it before
// this query's turn; the earlier resolved ones did not; and every train this query prefers to t is taken
// already.  The lowest unresolved query always passes c (or resolves in a), so n1 rounds suffice.
// minq and taken live in LDS when the pair's train set fits (LDS = true, max_t <= kAssignLdsTrains trains: 5 bytes
// each), else in the pair's global rows.
#ifndef RGBD_PROJ_ASSIGN_THREADS
#define RGBD_PROJ_ASSIGN_THREADS 512   // 1023 fr1 pairs, th 5: 256 / 512 / 1024 threads -> 0.087 / 0.086 / 0.096 ms (profiles/projection_match)
#endif
constexpr int kAssignThreads = RGBD_PROJ_ASSIGN_THREADS;
constexpr int kAssignWaves = kAssignThreads / 64;
constexpr int kAssignLdsTrains = 8192;

template <bool LDS>
__global__ __launch_bounds__(kAssignThreads) void k_proj_assign(ProjFrames f, ProjCfg g, ProjWork w, int lds_trains)
{
    extern __shared__ uint32_t assign_lds[];   // LDS: minq[lds_trains], then taken[lds_trains]
    __shared__ int s_any;
    __shared__ int wtot[kAssignWaves];
    const int p = blockIdx.x;
    const int qframe = f.qf[p];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (qframe < 0) {
        if (tid == 0) w.out_count[p] = 0;
        return;
    }
    const int tframe = f.tf[p];
    const int n1 = min(f.counts[qframe], w.qcap), n2 = min(f.counts[tframe], w.tcap);
    const size_t qb = (size_t)p * w.qcap, tb = (size_t)p * w.tcap;
    uint32_t* keys = w.keys + qb * kProjKeys;
    int* head = w.head + qb;
    int* res = w.res + qb;
    uint8_t* more = w.more + qb;
    uint32_t* minq = LDS ? assign_lds : w.minq + tb;
    uint8_t* taken = LDS ? reinterpret_cast<uint8_t*>(assign_lds + lds_trains) : w.taken + tb;
    const int* cell_off = w.cell_off + (size_t)p * (kProjCells + 1);
    const float4* s_rec = w.s_rec + tb;
    const uint4* s_desc = w.s_desc + tb * 2;
    for (int t = tid; t < n2; t += kAssignThreads) taken[t] = 0;
    for (int round = 0; round <= n1; round++) {
        if (tid == 0) s_any = 0;
        for (int t = tid; t < n2; t += kAssignThreads) minq[t] = kProjEmpty;
        __syncthreads();
        for (int q = tid; q < n1; q += kAssignThreads) {
            if (res[q] != kProjUnresolved) continue;
            uint32_t* kq = keys + (size_t)q * kProjKeys;
            int h = head[q];
            while (h < kProjKeys && kq[h] != kProjEmpty && taken[kq[h] & 0xFFFFu]) h++;   // a
            const bool trunc = more[q] != 0;
            if (h == kProjKeys || kq[h] == kProjEmpty) {
                if (!trunc) {
                    res[q] = kProjNoMatch;
                    continue;
                }
                // the kept keys are used up and more candidates exist: the list again from the window
                uint32_t nk[kProjKeys];
#pragma unroll
                for (int i = 0; i < kProjKeys; i++) nk[i] = kProjEmpty;
                uint32_t qd[8];
                load_desc(f.desc, (size_t)qframe * f.cap + q, qd);
                const float2 uv = w.uv[qb + q];
                bool m2 = false;
                scan_window(g, uv.x, uv.y, w.win[qb + q], cell_off, s_rec, s_desc, [&](int pos, uint32_t iw, const uint4& d0, const uint4& d1) {
                    if (!(iw & 0x10000u) || taken[pos]) return;
                    const int d = hamming(qd, d0, d1);
                    if (d <= kProjThHigh) m2 |= key_insert(nk, (uint32_t)d << 16 | (uint32_t)pos);
                });
#pragma unroll
                for (int i = 0; i < kProjKeys; i++) kq[i] = nk[i];
                more[q] = m2 ? 1 : 0;
                h = 0;
                if (nk[0] == kProjEmpty) {
                    res[q] = kProjNoMatch;
                    continue;
                }
            }
            head[q] = h;
            s_any = 1;
            if (more[q]) {   // b, a truncated list: every untaken candidate of the window
                uint32_t qd[8];
                load_desc(f.desc, (size_t)qframe * f.cap + q, qd);
                const float2 uv = w.uv[qb + q];
                scan_window(g, uv.x, uv.y, w.win[qb + q], cell_off, s_rec, s_desc, [&](int pos, uint32_t iw, const uint4& d0, const uint4& d1) {
                    if (!(iw & 0x10000u) || taken[pos]) return;
                    if (hamming(qd, d0, d1) <= kProjThHigh) atomicMin(&minq[pos], (uint32_t)q);
                });
            } else {
                for (int i = h; i < kProjKeys && kq[i] != kProjEmpty; i++) atomicMin(&minq[kq[i] & 0xFFFFu], (uint32_t)q);
            }
        }
        __syncthreads();
        if (!s_any) break;   // uniform: read between two barriers
        for (int q = tid; q < n1; q += kAssignThreads) {   // c
            if (res[q] != kProjUnresolved) continue;
            const uint32_t key = keys[(size_t)q * kProjKeys + head[q]];
            const uint32_t pos = key & 0xFFFFu;
            if (__hip_atomic_load(&minq[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (uint32_t)q) {
                res[q] = (int)key;
                taken[pos] = 1;
            }
        }
        __syncthreads();
    }
    __syncthreads();
    // the matches in query order
    rgbd_dmatch* out = w.out + qb;
    int base = 0;
    for (int q0 = 0; q0 < n1; q0 += kAssignThreads) {
        const int q = q0 + tid;
        const int r = q < n1 ? res[q] : kProjNoMatch;
        const bool on = r >= 0;
        const unsigned long long b = __ballot(on);
        if (lane == 0) wtot[wv] = __popcll(b);
        __syncthreads();
        int off = base, tot = 0;
        for (int i = 0; i < kAssignWaves; i++) {
            if (i < wv) off += wtot[i];
            tot += wtot[i];
        }
        if (on) {
            rgbd_dmatch m;
            m.queryIdx = q;
            m.trainIdx = (int)(__float_as_uint(s_rec[r & 0xFFFF].z) & 0xFFFFu);
            m.imgIdx = -1;
            m.distance = (float)(r >> 16);
            out[off + __popcll(b & ((1ull << lane) - 1ull))] = m;
        }
        base += tot;
        __syncthreads();
    }
    if (tid == 0) w.out_count[p] = base;
}

}  // namespace rgbd

#include "launch.h"
namespace rgbd {

hipError_t launch_proj_bounds(const ExtractCfg* d_cfg, float* out4, hipStream_t st)
{
    return dispatch(k_proj_bounds, dim3(1), dim3(64), 0, st, d_cfg, out4);
}

hipError_t launch_proj_grid(const ProjFrames& f, const ProjCfg& g, const ProjWork& w, int npairs, hipStream_t st)
{
    return dispatch(k_proj_grid, dim3(npairs), dim3(kGridThreads), 0, st, f, g, w);
}

hipError_t launch_proj_search(const ProjFrames& f, const ProjCfg& g, const ProjWork& w, int max_q, int max_t, int npairs,
                              bool debug, hipStream_t st)
{
    if (max_t <= kSearchLdsTrains) {
        const int lt = max_t > 0 ? max_t : 1;
        const size_t lds = (size_t)kSearchLdsCells * 4 + (size_t)lt * 48;
        if (debug) return dispatch(k_proj_search_lds<true>, dim3(npairs), dim3(kSearchLdsThreads), lds, st, f, g, w, lt);
        return dispatch(k_proj_search_lds<false>, dim3(npairs), dim3(kSearchLdsThreads), lds, st, f, g, w, lt);
    }
    const dim3 grid((max_q + kSearchThreads - 1) / kSearchThreads, npairs);
    if (debug) return dispatch(k_proj_search<true>, grid, dim3(kSearchThreads), 0, st, f, g, w);
    return dispatch(k_proj_search<false>, grid, dim3(kSearchThreads), 0, st, f, g, w);
}

hipError_t launch_proj_assign(const ProjFrames& f, const ProjCfg& g, const ProjWork& w, int max_t, int npairs, hipStream_t st)
{
    if (max_t <= kAssignLdsTrains) {
        const int lt = (max_t + 3) & ~3;
        return dispatch(k_proj_assign<true>, dim3(npairs), dim3(kAssignThreads), (size_t)lt * 5, st, f, g, w, lt);
    }
    return dispatch(k_proj_assign<false>, dim3(npairs), dim3(kAssignThreads), 0, st, f, g, w, 0);
}

}  // namespace rgbd
