// cvorb.hip -- OpenCV's ORB on gfx950: the reference's Extractor(ORB, ORB, NORMAL)
//   cv::ORB::create(nfeatures, scaleFactor, nlevels)->detect   Features/Extractor.cpp:163-166, 52   -> k_cvorb_score, k_cvorb_list,
//                                                                                                    k_cvorb_select
//   Extractor::detectAndCompute: retainBest(nfeatures)          Features/Extractor.cpp:56-57       -> k_cvorb_frame
//   cv::ORB::create()->compute (the provided-keypoints path)    Features/Extractor.cpp:216-218, 59 -> k_cvorb_frame, k_cvorb_describe
// on the ORB2 path's pyramid and blurred pyramid (k_pyramid / k_pyr_tail and the blur blocks of the k_fast grid), then
// k_undistort.  DESIGN.md, "OpenCV ORB definition"; tests/cvorb_model.py is its executable form.
//
// cv::FAST's score (cornerScore<16>) of a corner found at threshold t >= 1 is S = M - 1, M the largest arc minimum
// over both polarities, whatever t was; a pixel is a corner at t iff S >= t, and the survivors of the strict 3x3
// suppression are the strict maxima of the S map among the corners (adaptive.hip).  A neighbour below t cannot
// suppress a corner, so the map only holds S where S >= t and 0 elsewhere.
#include <hip/hip_runtime.h>

#include "dispatch.h"

#include <cstdint>

#include "cvorb_dev.h"
#include "orb_math_dev.h"
#include "orb_pattern_dev.h"
#include "select_dev.h"

namespace rgbd {

__constant__ CvPattern c_cv_pattern = make_cv_pattern();

// ------------------------------------------------------------------ the FAST-9 score map of every level
// One thread per pixel of the part of a level the list reads: x in [e - 1, w - e], y in [e - 1, h - e] (the border
// filter's range and its one-pixel suppression margin; e >= 22, so every ring lies inside the level).  A 9-arc of
// the 16-ring holds pixel k or k + 8 for every k, so a pixel whose ring pixels 0 and 8 (or 4 and 12) both lie
// within t of the centre is no corner at t: most pixels leave after four loads.
constexpr int kScW = 64, kScH = 4;

__global__ __launch_bounds__(kScW * kScH) void k_cvorb_score(const uint8_t* __restrict__ pyr, uint8_t* __restrict__ score,
                                                             CvorbCfg g, int tiles_x)
{
    const int l = blockIdx.y, b = blockIdx.z;
    const int w = g.lw[l], h = g.lh[l], st = g.lstride[l], e = g.edge;
    const int rw = w - 2 * e + 2, rh = h - 2 * e + 2;   // the computed range's sides
    if (rw <= 2 || rh <= 2) return;                     // the level keeps nothing
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x = e - 1 + tx * kScW + (int)(threadIdx.x % kScW), y = e - 1 + ty * kScH + (int)(threadIdx.x / kScW);
    if (x > w - e || y > h - e) return;
    const size_t base = (size_t)b * g.frame_pyr_bytes + g.loff[l];
    const uint8_t* p = pyr + base + (size_t)y * st + x;
    const int t = g.thr, v = p[0];
    int out = 0;
    const int d0 = p[3 * st] - v, d8 = p[-3 * st] - v, d4 = p[3] - v, d12 = p[-3] - v;
    const bool dead = (abs(d0) <= t && abs(d8) <= t) || (abs(d4) <= t && abs(d12) <= t);
    if (!dead) {
        int d[16];
        d[0] = d0;                      d[1] = p[3 * st + 1] - v;   d[2] = p[2 * st + 2] - v;   d[3] = p[st + 3] - v;
        d[4] = d4;                      d[5] = p[-st + 3] - v;      d[6] = p[-2 * st + 2] - v;  d[7] = p[-3 * st + 1] - v;
        d[8] = d8;                      d[9] = p[-3 * st - 1] - v;  d[10] = p[-2 * st - 2] - v; d[11] = p[-st - 3] - v;
        d[12] = d12;                    d[13] = p[st - 3] - v;      d[14] = p[2 * st - 2] - v;  d[15] = p[3 * st - 1] - v;
        int mn2[16], mx2[16], mn4[16], mx4[16];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            mn2[k] = min(d[k], d[(k + 1) & 15]);
            mx2[k] = max(d[k], d[(k + 1) & 15]);
        }
#pragma unroll
        for (int k = 0; k < 16; k++) {
            mn4[k] = min(mn2[k], mn2[(k + 2) & 15]);
            mx4[k] = max(mx2[k], mx2[(k + 2) & 15]);
        }
        int M = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) {   // arc k .. k+8 = (k .. k+3), (k+4 .. k+7) and k+8
            const int amin = min(min(mn4[k], mn4[(k + 4) & 15]), d[(k + 8) & 15]);
            const int amax = max(max(mx4[k], mx4[(k + 4) & 15]), d[(k + 8) & 15]);
            M = max(M, max(amin, -amax));
        }
        const int S = max(M, 1) - 1;
        out = S >= t ? S : 0;
    }
    score[base + (size_t)y * st + x] = (uint8_t)out;
}

// ------------------------------------------------------------------ the level's corners in raster order
// cv::FAST(level, t, nonmax = true) followed by runByImageBorder(e) = the strict 3x3 maxima of the score map at x in
// [e, w - e), y in [e, h - e), in raster order.  The range's rows are cut into kCvListStrips strips, one workgroup
// per (strip, level, frame), and the kernel runs twice: the counting pass leaves every strip's count, the writing pass
// starts each strip at the sum of the counts above it.  Inside a strip the rows are cut into 16-px segments at
// 16-byte aligned columns (rows are 64-B padded, levels 256-B aligned), numbered in raster order; thread t of round r
// owns segment kListThreads r + t, so an ordered block scan gives every corner its slot (k_adp_cells' scheme).  A
// segment reads three 16-byte rows and their two neighbour columns; columns outside [e - 1, w - e] are never
// written by k_cvorb_score and hold the buffer's initial 0.  The count goes on past cand_cap.
constexpr int kListSeg = 16;
constexpr int kListThreads = 512;

template <bool kWrite>
__global__ __launch_bounds__(kListThreads) void k_cvorb_list(const uint8_t* __restrict__ score, CvorbCfg g,
                                                             uint32_t* __restrict__ cand, int* __restrict__ nstrip,
                                                             int* __restrict__ nfast, int* __restrict__ err)
{
    __shared__ SelLds sh;
    const int tid = threadIdx.x, l = blockIdx.x / kCvListStrips, s = blockIdx.x - l * kCvListStrips, b = blockIdx.y;
    const int w = g.lw[l], h = g.lh[l], st = g.lstride[l], e = g.edge;
    const int sw = w - 2 * e, shh = h - 2 * e;
    const int c = b * g.nlevels + l;
    if (sw <= 0 || shh <= 0) {
        if (kWrite && s == 0 && tid == 0) nfast[c] = 0;
        return;
    }
    const int r0 = shh * s / kCvListStrips, r1 = shh * (s + 1) / kCvListStrips;   // the strip's rows of the range
    const int a0 = e & ~(kListSeg - 1);                                            // the first segment's column (>= 16)
    const int segs = (w - e - a0 + kListSeg - 1) / kListSeg, nseg = segs * (r1 - r0);
    const uint8_t* S = score + (size_t)b * g.frame_pyr_bytes + g.loff[l];
    uint32_t* L = cand + (size_t)c * g.cand_cap;
    int* NS = nstrip + (size_t)c * kCvListStrips;
    if (tid == 0) sh.phase = 0;
    __syncthreads();
    int stored = 0;                             // block-uniform: corners so far (writing pass: of the whole level)
    if (kWrite)
        for (int k = 0; k < s; k++) stored += NS[k];
    for (int base = 0; base < nseg; base += kListThreads) {
        const int seg = base + tid;
        int v1[kListSeg + 2];
        unsigned keep = 0;                      // bit i: pixel i of the segment is a corner
        int cnt = 0, lxs = 0, ly = 0;
        if (seg < nseg) {
            const int ry = seg / segs;
            ly = e + r0 + ry;
            lxs = a0 + kListSeg * (seg - ry * segs);
            int cm[kListSeg + 2];
            const uint8_t* q = S + (size_t)(ly - 1) * st + lxs;   // 16-B aligned; lxs - 1 >= 15 and lxs + 16 < w
            const uint4 t4 = *reinterpret_cast<const uint4*>(q), m4 = *reinterpret_cast<const uint4*>(q + st),
                        b4 = *reinterpret_cast<const uint4*>(q + 2 * st);
            const uint32_t tw[4] = {t4.x, t4.y, t4.z, t4.w}, mw[4] = {m4.x, m4.y, m4.z, m4.w}, bw[4] = {b4.x, b4.y, b4.z, b4.w};
            cm[0] = max((int)q[-1], (int)q[2 * st - 1]);
            v1[0] = q[st - 1];
            cm[kListSeg + 1] = max((int)q[kListSeg], (int)q[2 * st + kListSeg]);
            v1[kListSeg + 1] = q[st + kListSeg];
#pragma unroll
            for (int j = 0; j < kListSeg; j++) {
                const int sh8 = 8 * (j & 3);
                cm[j + 1] = max((int)((tw[j >> 2] >> sh8) & 255u), (int)((bw[j >> 2] >> sh8) & 255u));
                v1[j + 1] = (int)((mw[j >> 2] >> sh8) & 255u);
            }
#pragma unroll
            for (int i = 0; i < kListSeg; i++) {
                const int s = v1[i + 1];
                const int nb = max(max(max(cm[i], cm[i + 1]), cm[i + 2]), max(v1[i], v1[i + 2]));
                if (s >= 1 && s > nb && lxs + i >= e && lxs + i < w - e) {
                    keep |= 1u << i;
                    cnt++;
                }
            }
        }
        int off, d0, tot, d1;
        block_scan2(cnt, 0, off, d0, tot, d1, sh);
        off += stored;
        if (kWrite) {
#pragma unroll
            for (int i = 0; i < kListSeg; i++)
                if ((keep >> i) & 1u) {
                    if (off < g.cand_cap) L[off] = pack_key(lxs + i, ly, v1[i + 1]);
                    off++;
                }
        }
        stored += tot;
        __syncthreads();   // block_scan2's phase bit is read by the next round
    }
    if (tid == 0) {
        if (!kWrite) {
            NS[s] = stored;
        } else if (s == kCvListStrips - 1) {   // the last strip ends at the level's count
            nfast[c] = stored;
            if (stored > g.cand_cap) atomicOr(err + b, kCvorbErrCand);
        }
    }
}

// ------------------------------------------------------------------ retainBest(2 N), Harris, retainBest(N)
// HarrisResponses (blockSize 7, k = 0.04) at a level position at least 4 px inside the level: int32 sums of the
// 3x3 Sobel-like gradients over the 7x7 block, then f32 left to right.
__device__ __forceinline__ float harris_at(const uint8_t* __restrict__ img, int st, int x0, int y0, float ssq)
{
    int a = 0, b = 0, c = 0;
    const uint8_t* p0 = img + (size_t)(y0 - 4) * st + (x0 - 4);
    int r0[9], r1[9], r2[9];   // three consecutive rows of the 9 x 9 patch
#pragma unroll
    for (int j = 0; j < 9; j++) {
        r0[j] = p0[j];
        r1[j] = p0[st + j];
    }
    for (int i = 0; i < 7; i++) {
        const uint8_t* q = p0 + (size_t)(i + 2) * st;
#pragma unroll
        for (int j = 0; j < 9; j++) r2[j] = q[j];
#pragma unroll
        for (int j = 0; j < 7; j++) {
            const int Ix = (r1[j + 2] - r1[j]) * 2 + (r0[j + 2] - r0[j]) + (r2[j + 2] - r2[j]);
            const int Iy = (r2[j + 1] - r0[j + 1]) * 2 + (r2[j] - r0[j]) + (r2[j + 2] - r0[j + 2]);
            a += Ix * Ix;
            b += Iy * Iy;
            c += Ix * Iy;
        }
#pragma unroll
        for (int j = 0; j < 9; j++) {
            r0[j] = r1[j];
            r1[j] = r2[j];
        }
    }
    const float fa = (float)a, fb = (float)b, fc = (float)c;
    const float s = fa + fb;
    return ((fa * fb - fc * fc) - (0.04f * s) * s) * ssq;
}

// One workgroup per (level, frame): the list's scores into LDS, retainBest(2 N) (select_dev.h: libstdc++'s element
// order), the Harris response of every survivor on the unblurred level, retainBest(N) on it.  Both survivor lists
// are kept (s1 / h1, s2 / h2) for k_cvorb_frame and the debug reader.  A level whose list overflowed is left empty:
// its frame is flagged.
__global__ __launch_bounds__(kCvorbThreads) void k_cvorb_select(const uint8_t* __restrict__ pyr, CvorbCfg g,
                                                                const uint32_t* __restrict__ cand, const int* __restrict__ nfast,
                                                                uint32_t* __restrict__ s1, float* __restrict__ h1, int* __restrict__ n1,
                                                                uint32_t* __restrict__ s2, float* __restrict__ h2, int* __restrict__ n2)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ SelLds sh;
    const int tid = threadIdx.x, T = blockDim.x, l = blockIdx.x, b = blockIdx.y;
    const int c = b * g.nlevels + l, cap = g.cand_cap, N = g.N[l];
    float* R = reinterpret_cast<float*>(smem);
    uint16_t* I = reinterpret_cast<uint16_t*>(R + cap);
    uint16_t* posL = I + cap;
    uint16_t* posR = posL + cap;
    const size_t lo = (size_t)c * cap;
    const uint32_t* L = cand + lo;
    int n = nfast[c];
    if (n > cap) n = 0;
    for (int i = tid; i < n; i += T) {
        R[i] = (float)key_s(L[i]);
        I[i] = (uint16_t)i;
    }
    if (tid == 0) sh.phase = 0;
    __syncthreads();
    int m1 = n;
    if (n > 2 * N) m1 = N > 0 ? retain_best_block(R, I, posL, posR, n, 2 * N, sh) : 0;
    __syncthreads();
    const uint8_t* img = pyr + (size_t)b * g.frame_pyr_bytes + g.loff[l];
    for (int i = tid; i < m1; i += T) {
        const uint32_t k = L[I[i]];
        const float hr = harris_at(img, g.lstride[l], key_x(k), key_y(k), g.ssq);
        s1[lo + i] = k;
        h1[lo + i] = hr;
        R[i] = hr;
    }
    __syncthreads();
    int m2 = m1;
    if (m1 > N) m2 = N > 0 ? retain_best_block(R, I, posL, posR, m1, N, sh) : 0;
    __syncthreads();
    for (int i = tid; i < m2; i += T) {
        s2[lo + i] = L[I[i]];
        h2[lo + i] = R[i];
    }
    if (tid == 0) {
        n1[c] = m1;
        n2[c] = m2;
    }
}

// ------------------------------------------------------------------ levels -> the frame's keypoints (one frame per block)
// 1. the levels' survivors concatenated level-major, responses into LDS
// 2. retainBest(nfeatures) over all of them when more than nfeatures (it fires only when a level kept ties)
// 3. cv::ORB::compute's runByImageBorder((W, H), 31) on cvRound of the scaled points (stable), and its regrouping
//    by octave, stable within an octave: an ordered scan per level pair.  On a list whose octaves already do not
//    decrease the regrouping changes nothing, so it is not tested for.
// Keypoints are written as cv::KeyPoint(x s, y s, 31 s, angle (k_cvorb_describe), Harris, octave, -1), their level
// positions to fsel.
__global__ __launch_bounds__(kCvorbThreads) void k_cvorb_frame(CvorbCfg g, const uint32_t* __restrict__ s2, const float* __restrict__ h2,
                                                               const int* __restrict__ n2, uint32_t* __restrict__ fsel,
                                                               int* __restrict__ counts, float* __restrict__ kps, int* __restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ SelLds sh;
    __shared__ int pre[kMaxLevels + 1];
    const int tid = threadIdx.x, T = blockDim.x, b = blockIdx.x;
    const int nl = g.nlevels, cap = g.cand_cap, FC = g.frame_cap;
    float* R = reinterpret_cast<float*>(smem);
    uint16_t* I = reinterpret_cast<uint16_t*>(R + FC);
    uint16_t* posL = I + FC;
    uint16_t* posR = posL + FC;
    if (tid == 0) {
        sh.phase = 0;
        int s = 0;
        for (int l = 0; l < nl; l++) {
            pre[l] = s;
            s += n2[b * nl + l];
        }
        for (int l = nl; l <= kMaxLevels; l++) pre[l] = s;
    }
    __syncthreads();
    const int n = pre[nl];
    if (n > FC) {   // more than the selection holds: the frame fails
        if (tid == 0) {
            atomicOr(err + b, kCvorbErrKeep);
            counts[b] = 0;
        }
        return;
    }
    for (int l = 0; l < nl; l++) {
        const int nk = pre[l + 1] - pre[l];
        const float* hl = h2 + (size_t)(b * nl + l) * cap;
        for (int i = tid; i < nk; i += T) {
            R[pre[l] + i] = hl[i];
            I[pre[l] + i] = (uint16_t)(pre[l] + i);
        }
    }
    __syncthreads();
    int m = n;
    if (n > g.nfeatures) m = retain_best_block(R, I, posL, posR, n, g.nfeatures, sh);
    __syncthreads();
    // each thread owns a contiguous run of the list; posL[i] = the element's level, or 255 when the border drops it
    const int E = (m + T - 1) / T, base = tid * E, hi = min(base + E, m);
    const bool any = g.W > 2 * kCvorbDescBorder && g.H > 2 * kCvorbDescBorder;
    for (int i = base; i < hi; i++) {
        const int idx = I[i];
        int l = 0;
        while (idx >= pre[l + 1]) l++;
        const uint32_t k = s2[(size_t)(b * nl + l) * cap + (idx - pre[l])];
        const int cx = __float2int_rn((float)key_x(k) * g.scale[l]), cy = __float2int_rn((float)key_y(k) * g.scale[l]);
        const bool keep = any && cx >= kCvorbDescBorder && cx < g.W - kCvorbDescBorder && cy >= kCvorbDescBorder &&
                          cy < g.H - kCvorbDescBorder;
        posL[i] = (uint16_t)(keep ? l : 255);
    }
    int done = 0;   // block-uniform: keypoints of the lower levels
    for (int lp = 0; lp < nl; lp += 2) {
        int ca = 0, cb = 0;
        for (int i = base; i < hi; i++) {
            ca += posL[i] == lp;
            cb += posL[i] == lp + 1;
        }
        int ea, eb, ta, tb;
        block_scan2(ca, cb, ea, eb, ta, tb, sh);
        int oa = done + ea, ob = done + ta + eb;
        for (int i = base; i < hi; i++) {
            const int lv = posL[i];
            if (lv != lp && lv != lp + 1) continue;
            const int o = lv == lp ? oa++ : ob++;
            if (o >= g.kp_cap) continue;
            const int idx = I[i];
            const uint32_t k = s2[(size_t)(b * nl + lv) * cap + (idx - pre[lv])];
            float* K = kps + ((size_t)b * g.kp_cap + o) * 7;
            K[0] = (float)key_x(k) * g.scale[lv];
            K[1] = (float)key_y(k) * g.scale[lv];
            K[2] = g.size[lv];
            K[3] = -1.0f;
            K[4] = R[i];
            reinterpret_cast<int*>(K)[5] = lv;
            reinterpret_cast<int*>(K)[6] = -1;
            fsel[(size_t)b * g.kp_cap + o] = (uint32_t)key_x(k) | ((uint32_t)key_y(k) << 11) | ((uint32_t)lv << 22);
        }
        done += ta + tb;
        __syncthreads();   // block_scan2's phase bit is read by the next round
    }
    if (tid == 0) {
        counts[b] = min(done, g.kp_cap);
        if (done > g.kp_cap) atomicOr(err + b, kCvorbErrKeep);
    }
}

// ------------------------------------------------------------------ angle + steered BRIEF, one wave per keypoint
// IC_Angle on the unblurred level (lane = disk row, integer moments), then the 256 tests of bit_pattern_31_ on the
// blurred level (lane = descriptor byte).  A keypoint lies at least 22 px inside its level, so the radius-15 disk
// and the rotated tests (|offset| <= 18) stay inside it.
constexpr int kCvDescWaves = 4;

__global__ __launch_bounds__(64 * kCvDescWaves) void k_cvorb_describe(const uint8_t* __restrict__ pyr, const uint8_t* __restrict__ blur,
                                                                      CvorbCfg g, const uint32_t* __restrict__ fsel,
                                                                      const int* __restrict__ counts, float* __restrict__ kps,
                                                                      uint8_t* __restrict__ desc)
{
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int o = blockIdx.x * kCvDescWaves + (int)(threadIdx.x >> 6);
    if (o >= counts[b]) return;   // wave-uniform
    const size_t slot = (size_t)b * g.kp_cap + o;
    const uint32_t k = fsel[slot];
    const int x = (int)(k & 2047u), y = (int)((k >> 11) & 2047u), l = (int)(k >> 22);
    const int st = g.lstride[l];
    const size_t base = (size_t)b * g.frame_pyr_bytes + g.loff[l] + (size_t)y * st + x;
    int m10 = 0, m01 = 0;
    if (lane < 31) {
        const int v = lane - 15;
        const int d = g.umax[v < 0 ? -v : v];
        const uint8_t* row = pyr + base + (ptrdiff_t)v * st;
        int s = 0;
        for (int u = -d; u <= d; u++) {
            const int val = row[u];
            m10 += u * val;
            s += val;
        }
        m01 = v * s;
    }
    m10 = __builtin_amdgcn_readlane(wave_incl_scan(m10), 63);
    m01 = __builtin_amdgcn_readlane(wave_incl_scan(m01), 63);
    const float angle = fast_atan2_deg((float)m01, (float)m10);
    float a, bs;
    cos_sin_f(angle * (float)(M_PI / 180.f), &a, &bs);
    if (lane < 32) {
        const uint8_t* ctr = blur + base;
        int byte = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint32_t pw = c_cv_pattern.v[8 * lane + i];
            const float x0 = (float)(int8_t)(pw & 0xFFu), y0 = (float)(int8_t)((pw >> 8) & 0xFFu);
            const float x1 = (float)(int8_t)((pw >> 16) & 0xFFu), y1 = (float)(int8_t)(pw >> 24);
            const int t0 = ctr[(ptrdiff_t)__float2int_rn(x0 * bs + y0 * a) * st + __float2int_rn(x0 * a - y0 * bs)];
            const int t1 = ctr[(ptrdiff_t)__float2int_rn(x1 * bs + y1 * a) * st + __float2int_rn(x1 * a - y1 * bs)];
            byte |= (t0 < t1) << i;
        }
        desc[slot * 32 + lane] = (uint8_t)byte;
    }
    if (lane == 0) kps[slot * 7 + 3] = angle;
}

// ------------------------------------------------------------------ launchers
hipError_t launch_cvorb_score(const uint8_t* pyr, const CvorbCfg& g, const CvorbBufs& w, int B, hipStream_t st)
{
    // level 0's computed range bounds every level's tile grid; a smaller level's spare blocks leave at once
    const int rw = g.lw[0] - 2 * g.edge + 2, rh = g.lh[0] - 2 * g.edge + 2;
    if (rw <= 2 || rh <= 2) return hipSuccess;
    const int tx = (rw + kScW - 1) / kScW, ty = (rh + kScH - 1) / kScH;
    return dispatch(k_cvorb_score, dim3(tx * ty, g.nlevels, B), dim3(kScW * kScH), 0, st, pyr, w.score, g, tx);
}

hipError_t launch_cvorb_list(const CvorbCfg& g, const CvorbBufs& w, int* err, int B, hipStream_t st)
{
    // the segments' 16-byte row loads
    if (g.frame_pyr_bytes % 16 != 0) return hipErrorInvalidValue;
    for (int l = 0; l < g.nlevels; l++)
        if (g.lstride[l] % 16 != 0 || g.loff[l] % 16 != 0) return hipErrorInvalidValue;
    const dim3 grid(g.nlevels * kCvListStrips, B);
    const hipError_t e = dispatch(k_cvorb_list<false>, grid, dim3(kListThreads), 0, st, w.score, g, w.cand, w.nstrip, w.nfast, err);
    if (e != hipSuccess) return e;
    return dispatch(k_cvorb_list<true>, grid, dim3(kListThreads), 0, st, w.score, g, w.cand, w.nstrip, w.nfast, err);
}

hipError_t launch_cvorb_select(const uint8_t* pyr, const CvorbCfg& g, const CvorbBufs& w, int B, hipStream_t st)
{
    return dispatch(k_cvorb_select, dim3(g.nlevels, B), dim3(kCvorbThreads), (size_t)g.cand_cap * 10 + 16, st, pyr, g, w.cand,
                    w.nfast, w.s1, w.h1, w.n1, w.s2, w.h2, w.n2);
}

hipError_t launch_cvorb_frame(const CvorbCfg& g, const CvorbBufs& w, int* counts, float* kps, int* err, int B, hipStream_t st)
{
    return dispatch(k_cvorb_frame, dim3(B), dim3(kCvorbThreads), (size_t)g.frame_cap * 10 + 16, st, g, w.s2, w.h2, w.n2, w.fsel,
                    counts, kps, err);
}

hipError_t launch_cvorb_describe(const uint8_t* pyr, const uint8_t* blur, const CvorbCfg& g, const CvorbBufs& w, const int* counts,
                                 float* kps, uint8_t* desc, int B, hipStream_t st)
{
    return dispatch(k_cvorb_describe, dim3((g.kp_cap + kCvDescWaves - 1) / kCvDescWaves, B), dim3(64 * kCvDescWaves), 0, st, pyr,
                    blur, g, w.fsel, counts, kps, desc);
}

}  // namespace rgbd
