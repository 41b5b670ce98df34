// adaptive.hip -- the reference's adaptive front end on gfx950: Extractor(FAST, BRIEF, ADAPTIVE)
//   DetectorAdjuster::detect            Features/DetectorAdjuster.cpp:23-39: cv::FAST(roi, (int)mThresh)   -> k_adp_score + k_adp_cells
//   VideoDynamicAdaptedFeatureDetector  Features/VideoDynamicAdaptedFeatureDetector.cpp:24-44: the tries    -> k_adp_chain
//   VideoGridAdaptedFeatureDetector     Features/VideoGridAdaptedFeatureDetector.cpp:24-84: keepStrongest   -> k_adp_select
//   Extractor::detectAndCompute         Features/Extractor.cpp:50-61: retainBest(nfeatures)                 -> k_adp_frame
// then BRIEF-32 (k_svo_brief on k_svo_pyramid's box sums) and k_undistort, as for the SVO front end.
//
// cv::FAST's score (cornerScore<16>) of a corner found at threshold t >= 1 is S = M - 1, M the largest arc
// minimum over both polarities, whatever t was; a pixel is a corner at t iff M > t, i.e. S >= t.  A neighbour
// that suppresses a corner scores at least as much, so it is a corner at t too: the survivors of the strict
// 3x3 non-maximum suppression at t are the strict maxima of the S map with S >= t.  One pixel pass therefore
// serves every threshold the adjuster tries, and its loop only needs the counts n(t) of the maxima.
#include <hip/hip_runtime.h>

#include "dispatch.h"

#include <cstdint>

#include "adaptive_dev.h"
#include "fast_tile_dev.h"
#include "select_dev.h"

namespace rgbd {

// ------------------------------------------------------------------ the threshold-free FAST-9 score map
constexpr int kScTW = 64, kScTH = 32;
constexpr int kScHy = 3, kScHx = 8;                 // staged halo: 3 rows, 8 columns (dword-aligned)
constexpr int kScGW = kScTW + 2 * kScHx;            // 80 staged columns: x0-8 .. x0+71
constexpr int kScGH = kScTH + 2 * kScHy;            // 38 staged rows: y0-3 .. y0+34

// One 256-thread workgroup per 64 x 32 tile of a frame's gray image: S = max(M, 1) - 1 where the ring lies in
// the image (x in [3, W-3), y in [3, H-3)), else 0.
__global__ __launch_bounds__(256) void k_adp_score(const uint8_t* __restrict__ gray, size_t frame_bytes,
                                                   uint8_t* __restrict__ smap, AdpCfg g)
{
    __shared__ __attribute__((aligned(16))) uint8_t G[kScGH * kScGW];
    __shared__ __attribute__((aligned(16))) uint32_t PI[kScGH * kScGW];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int x0 = blockIdx.x * kScTW, y0 = blockIdx.y * kScTH;
    const int W = g.W, H = g.H;
    const uint8_t* img = gray + (size_t)b * frame_bytes;
    uint8_t* out = smap + (size_t)b * W * H;
    const bool al4 = ((W | (int)(frame_bytes & 3)) & 3) == 0;
    // 1. stage rows y0-3 .. y0+34, columns x0-8 .. x0+71 as dwords (zero outside the image)
    for (int i = tid; i < kScGH * (kScGW / 4); i += 256) {
        const int r = i / (kScGW / 4), q = i - r * (kScGW / 4);
        const int y = y0 - kScHy + r, x = x0 - kScHx + 4 * q;
        uint32_t v = 0;
        if (y >= 0 && y < H) {
            const uint8_t* row = img + (size_t)y * W;
            if (al4 && x >= 0 && x + 4 <= W) {
                v = *reinterpret_cast<const uint32_t*>(row + x);
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (x + k >= 0 && x + k < W) v |= (uint32_t)row[x + k] << (8 * k);
            }
        }
        reinterpret_cast<uint32_t*>(G)[i] = v;
    }
    __syncthreads();
    // pair image PI[r][c] = G[r][c] | G[r][c+1] << 16, four entries per task
    for (int i = tid; i < kScGH * (kScGW / 4); i += 256) {
        const int q = i % (kScGW / 4);
        const uint32_t v = reinterpret_cast<const uint32_t*>(G)[i];
        const uint32_t nb = q + 1 < kScGW / 4 ? (uint32_t)G[4 * i + 4] : 0u;
        uint4 o;
        o.x = (v & 0xffu) | ((v & 0xff00u) << 8);
        o.y = ((v >> 8) & 0xffu) | ((v & 0xff0000u));
        o.z = ((v >> 16) & 0xffu) | ((v >> 24) << 16);
        o.w = (v >> 24) | (nb << 16);
        reinterpret_cast<uint4*>(PI)[i] = o;
    }
    __syncthreads();
    // 2. one pixel pair per task
    for (int task = tid; task < kScTH * (kScTW / 2); task += 256) {
        const int ty = task / (kScTW / 2), tx = 2 * (task - ty * (kScTW / 2));
        const int X = x0 + tx, Y = y0 + ty;
        if (Y >= H || X >= W) continue;
        const u16x2 m = fast9_m2(PI, kScGW, ty + kScHy, tx + kScHx);
        uint8_t s[2];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const bool dom = X + k >= 3 && X + k < W - 3 && Y >= 3 && Y < H - 3;
            s[k] = (uint8_t)(dom ? max((int)m[k], 1) - 1 : 0);
        }
        uint8_t* o = out + (size_t)Y * W + X;
        o[0] = s[0];
        if (X + 1 < W) o[1] = s[1];
    }
}

// ------------------------------------------------------------------ cell lists + histograms
// One workgroup per (frame, cell).  cv::FAST treats the ROI as an image of its own: corners are tested at
// local x in [3, w-3), y in [3, h-3), and the strict 3x3 suppression sees score 0 outside that range.  The
// scan range is cut into segments of up to 16 pixels of one row; segments are numbered in raster order and
// thread t of round r owns segment 1024 r + t, so thread order is raster order and an ordered block scan
// gives each stored maximum its slot: the list's order never depends on arrival order.  A thread loads its
// segment's three score rows with their one-pixel margins unconditionally (zero outside the scan range) and
// shares the vertical maxima of the 18 columns among the 16 pixels.
constexpr int kCellSeg = 16;

__global__ __launch_bounds__(kAdpThreads) void k_adp_cells(const uint8_t* __restrict__ smap, AdpCfg g,
                                                           uint32_t* __restrict__ list, int* __restrict__ nlist,
                                                           int* __restrict__ nge)
{
    __shared__ SelLds sh;
    __shared__ int hist[256];
    const int tid = threadIdx.x, cell = blockIdx.x, b = blockIdx.y;
    const int c = b * g.ncells + cell;
    int x0, y0, x1, y1;
    adp_roi(g, cell, x0, y0, x1, y1);
    const int w = x1 - x0, h = y1 - y0;
    const int sw = w - 6, shh = h - 6;          // the scan range (both >= 1: ROIs are at least 7 x 7)
    const int segs = (sw + kCellSeg - 1) / kCellSeg, nseg = segs * shh;
    const uint8_t* S = smap + (size_t)b * g.W * g.H + (size_t)y0 * g.W + x0;
    uint32_t* L = list + (size_t)c * g.cell_cap;
    if (tid < 256) hist[tid] = 0;
    if (tid == 0) sh.phase = 0;
    __syncthreads();
    int stored = 0;                             // block-uniform: maxima with S >= tmin so far
    for (int base = 0; base < nseg; base += kAdpThreads) {
        const int seg = base + tid;
        int v[3][kCellSeg + 2];
        unsigned keep = 0;                      // bit i: pixel i of the segment is a stored maximum
        int cnt = 0, lxs = 0, ly = 0;
        if (seg < nseg) {
            const int ry = seg / segs;
            ly = 3 + ry;
            lxs = 3 + kCellSeg * (seg - ry * segs);
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const int yy = ly + r - 1;
                const bool rowin = yy >= 3 && yy < h - 3;
                const uint8_t* q = S + (size_t)(rowin ? yy : ly) * g.W;   // (an address inside the ROI either way)
#pragma unroll
                for (int j = 0; j < kCellSeg + 2; j++) {
                    const int xx = lxs - 1 + j;
                    v[r][j] = (rowin && xx >= 3 && xx < w - 3) ? (int)q[xx] : 0;
                }
            }
            int cm[kCellSeg + 2];
#pragma unroll
            for (int j = 0; j < kCellSeg + 2; j++) cm[j] = max(v[0][j], v[2][j]);
#pragma unroll
            for (int i = 0; i < kCellSeg; i++) {
                const int s = v[1][i + 1];      // 0 past the row's end: never a maximum
                const int nb = max(max(max(cm[i], cm[i + 1]), cm[i + 2]), max(v[1][i], v[1][i + 2]));
                if (s >= 1 && s > nb) {
                    atomicAdd(&hist[s], 1);     // a count: its order does not matter
                    if (s >= g.tmin) {
                        keep |= 1u << i;
                        cnt++;
                    }
                }
            }
        }
        int off, d0, tot, d1;
        block_scan2(cnt, 0, off, d0, tot, d1, sh);
        off += stored;
#pragma unroll
        for (int i = 0; i < kCellSeg; i++)
            if ((keep >> i) & 1u) {
                if (off < g.cell_cap) L[off] = adp_pack(lxs + i, ly, v[1][i + 1]);
                off++;
            }
        stored += tot;
        __syncthreads();   // block_scan2's phase bit is read by the next round
    }
    __syncthreads();
    if (tid == 0) nlist[c] = min(stored, g.cell_cap);
    if (tid < 256) {
        int s = 0;
        for (int t = tid; t < 256; t++) s += hist[t];
        nge[(size_t)c * 256 + tid] = s;
    }
}

// ------------------------------------------------------------------ the threshold chain
// VideoDynamicAdaptedFeatureDetector::detect per cell, the cells' thresholds carried through the batch's
// frames in order: thread = cell.  n(t) is a lookup in the frame's suffix counts; the double multiply and
// the (int) truncation are the host's.  cv::FAST clamps its threshold to [0, 255].
__global__ __launch_bounds__(kAdpMaxCells) void k_adp_chain(const int* __restrict__ nge, AdpCfg g, double* __restrict__ state,
                                                            double* __restrict__ before, int* __restrict__ used,
                                                            int* __restrict__ tries, int B)
{
    const int cell = threadIdx.x;
    if (cell >= g.ncells) return;
    double th = state[cell];
    for (int b = 0; b < B; b++) {
        const int c = b * g.ncells + cell;
        before[c] = th;
        int it = g.iterations, t = 0, ntry = 0;
        do {
            t = min(max((int)th, 0), 255);
            const int n = nge[(size_t)c * 256 + t];
            ntry++;
            if (n < g.grid_min) {               // DetectorAdjuster::tooFew
                th *= g.decrease;
                if (th < g.min_thresh) th = g.min_thresh;
            } else if (n > g.grid_max) {        // DetectorAdjuster::tooMany
                th *= g.increase;
                if (th > g.max_thresh) th = g.max_thresh;
                break;
            } else
                break;
            it--;
        } while (it > 0 && th > g.min_thresh && th < g.max_thresh);   // DetectorAdjuster::good
        used[c] = t;
        tries[c] = ntry;
    }
    state[cell] = th;
}

// ------------------------------------------------------------------ keepStrongest per (frame, cell)
// The stored maxima with S >= the threshold the chain used, in raster order (cv::FAST's output), then
// std::nth_element(begin, begin + maxPerCell, end, |response| >) and the first maxPerCell kept.
__global__ __launch_bounds__(kAdpThreads) void k_adp_select(const uint32_t* __restrict__ list, const int* __restrict__ nlist,
                                                            const int* __restrict__ nge, const int* __restrict__ used,
                                                            AdpCfg g, uint32_t* __restrict__ sel, int* __restrict__ nsel,
                                                            int* __restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ SelLds sh;
    const int tid = threadIdx.x, T = blockDim.x, cell = blockIdx.x, b = blockIdx.y;
    const int c = b * g.ncells + cell;
    const int cap = g.cell_cap;
    float* R = reinterpret_cast<float*>(smem);
    uint16_t* I = reinterpret_cast<uint16_t*>(R + cap);
    uint16_t* posL = I + cap;
    uint16_t* posR = posL + cap;
    const uint32_t* L = list + (size_t)c * cap;
    const int ns = nlist[c], t = used[c];
    if (tid == 0) sh.phase = 0;
    __syncthreads();
    const int E = (ns + T - 1) / T, base = tid * E, hi = min(base + E, ns);
    int cnt = 0;
    for (int i = base; i < hi; i++) cnt += adp_s(L[i]) >= t;
    int off, d0, m, d1;
    block_scan2(cnt, 0, off, d0, m, d1, sh);
    for (int i = base; i < hi; i++) {
        const int s = adp_s(L[i]);
        if (s >= t) {
            R[off] = (float)s;
            I[off] = (uint16_t)i;
            off++;
        }
    }
    // a maximum at the threshold used that the list did not hold: the frame's capacity flag
    if (tid == 0 && m != nge[(size_t)c * 256 + t]) atomicOr(err + b, 4);
    __syncthreads();
    int keep = m;
    if (m > g.max_per_cell) {
        introselect_block(R, I, posL, posR, m, g.max_per_cell, sh);
        keep = g.max_per_cell;
    }
    int x0, y0, x1, y1;
    adp_roi(g, cell, x0, y0, x1, y1);
    uint32_t* O = sel + (size_t)c * g.max_per_cell;
    for (int i = tid; i < keep; i += T) {
        const uint32_t e = L[I[i]];
        O[i] = adp_pack(adp_x(e) + x0, adp_y(e) + y0, adp_s(e));
    }
    if (tid == 0) nsel[c] = keep;
}

// ------------------------------------------------------------------ cells -> keypoints (one frame per block)
// 1. the cells' survivors concatenated row-major (aggregateKeypointsPerGridCell) -> R / I
// 2. retainBest(nfeatures) when more than nfeatures (Extractor::detectAndCompute :56-57)
// 3. runByImageBorder(28) (stable remove_if), keypoints written as cv::KeyPoint(x, y, 7.f, -1, score), octave
//    0, class_id -1 (cv::FAST's)
__global__ __launch_bounds__(kAdpThreads) void k_adp_frame(const uint32_t* __restrict__ sel, const int* __restrict__ nsel,
                                                           AdpCfg g, int* __restrict__ counts, float* __restrict__ kps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ SelLds sh;
    __shared__ int pre[kAdpMaxCells + 1];
    const int tid = threadIdx.x, T = blockDim.x, b = blockIdx.x;
    const int NM = g.kp_cap;                    // ncells * max_per_cell
    float* R = reinterpret_cast<float*>(smem);
    uint16_t* I = reinterpret_cast<uint16_t*>(R + NM);
    uint16_t* posL = I + NM;
    uint16_t* posR = posL + NM;
    const uint32_t* Sb = sel + (size_t)b * NM;
    if (tid == 0) {
        sh.phase = 0;
        int s = 0;
        for (int k = 0; k < g.ncells; k++) {
            pre[k] = s;
            s += nsel[b * g.ncells + k];
        }
        pre[g.ncells] = s;
    }
    __syncthreads();
    const int n = pre[g.ncells];
    for (int k = 0; k < g.ncells; k++) {
        const int nk = pre[k + 1] - pre[k];
        for (int i = tid; i < nk; i += T) {
            const int slot = k * g.max_per_cell + i;
            R[pre[k] + i] = (float)adp_s(Sb[slot]);
            I[pre[k] + i] = (uint16_t)slot;
        }
    }
    __syncthreads();
    int m = n;
    if (n > g.nfeatures) m = g.nfeatures > 0 ? retain_best_block(R, I, posL, posR, n, g.nfeatures, sh) : 0;
    const int E2 = (m + T - 1) / T, base2 = tid * E2;
    int keep = 0;
    for (int j = 0; j < E2; j++) {
        const int i = base2 + j;
        if (i >= m) break;
        const uint32_t e = Sb[I[i]];
        const int x = adp_x(e), y = adp_y(e);
        keep += x >= g.border && x < g.W - g.border && y >= g.border && y < g.H - g.border;
    }
    int o, d2, total, d3;
    block_scan2(keep, 0, o, d2, total, d3, sh);
    for (int j = 0; j < E2; j++) {
        const int i = base2 + j;
        if (i >= m) break;
        const uint32_t e = Sb[I[i]];
        const int x = adp_x(e), y = adp_y(e);
        if (!(x >= g.border && x < g.W - g.border && y >= g.border && y < g.H - g.border)) continue;
        if (o < g.kp_cap) {
            float* K = kps + ((size_t)b * g.kp_cap + o) * 7;
            K[0] = (float)x;
            K[1] = (float)y;
            K[2] = 7.0f;
            K[3] = -1.0f;
            K[4] = (float)adp_s(e);
            reinterpret_cast<int*>(K)[5] = 0;
            reinterpret_cast<int*>(K)[6] = -1;
        }
        o++;
    }
    if (tid == 0) counts[b] = min(total, g.kp_cap);
}

__global__ __launch_bounds__(kAdpThreads) void k_adp_keep_test(const float* __restrict__ resp, int n, int nth,
                                                               int depth_limit, int* __restrict__ order)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ SelLds sh;
    float* R = reinterpret_cast<float*>(smem);
    uint16_t* I = reinterpret_cast<uint16_t*>(R + n);
    uint16_t* posL = I + n;
    uint16_t* posR = posL + n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        R[i] = resp[i];
        I[i] = (uint16_t)i;
    }
    if (threadIdx.x == 0) sh.phase = 0;
    __syncthreads();
    int keep = n;
    if (n > nth) {
        introselect_block(R, I, posL, posR, n, nth, sh, depth_limit);
        keep = nth;
    }
    for (int i = threadIdx.x; i < keep; i += blockDim.x) order[i] = I[i];
}

// ------------------------------------------------------------------ launchers
hipError_t launch_adp_score(const uint8_t* gray, size_t frame_bytes, uint8_t* smap, const AdpCfg& g, int B, hipStream_t st)
{
    return dispatch(k_adp_score, dim3((g.W + kScTW - 1) / kScTW, (g.H + kScTH - 1) / kScTH, B), dim3(256), 0, st, gray,
                    frame_bytes, smap, g);
}

hipError_t launch_adp_cells(const uint8_t* smap, const AdpCfg& g, uint32_t* list, int* nlist, int* nge, int B, hipStream_t st)
{
    return dispatch(k_adp_cells, dim3(g.ncells, B), dim3(kAdpThreads), 0, st, smap, g, list, nlist, nge);
}

hipError_t launch_adp_chain(const int* nge, const AdpCfg& g, double* state, double* before, int* used, int* tries, int B,
                            hipStream_t st)
{
    return dispatch(k_adp_chain, dim3(1), dim3(kAdpMaxCells), 0, st, nge, g, state, before, used, tries, B);
}

hipError_t launch_adp_select(const uint32_t* list, const int* nlist, const int* nge, const int* used, const AdpCfg& g,
                             uint32_t* sel, int* nsel, int* err, int B, hipStream_t st)
{
    return dispatch(k_adp_select, dim3(g.ncells, B), dim3(kAdpThreads), (size_t)g.cell_cap * 10 + 16, st, list, nlist, nge,
                    used, g, sel, nsel, err);
}

hipError_t launch_adp_frame(const uint32_t* sel, const int* nsel, const AdpCfg& g, int* counts, float* kps, int B,
                            hipStream_t st)
{
    return dispatch(k_adp_frame, dim3(B), dim3(kAdpThreads), (size_t)g.kp_cap * 10 + 16, st, sel, nsel, g, counts, kps);
}

hipError_t launch_adp_keep_test(const float* resp, int n, int nth, int depth_limit, int* order, hipStream_t st)
{
    return dispatch(k_adp_keep_test, dim3(1), dim3(kAdpThreads), (size_t)n * 10 + 16, st, resp, n, nth, depth_limit, order);
}

}  // namespace rgbd
