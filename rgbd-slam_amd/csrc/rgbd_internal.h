// rgbd_internal.h -- configuration blocks shared by the host runtime and the gfx950 kernels.
//
// All geometry is computed once on the host (geometry.cpp) with the reference's own
// float/double semantics and passed to kernels by value (kernel-argument SGPRs), so
// the kernels never re-derive a float-rounded size or budget.
#pragma once
#include <stddef.h>
#include <stdint.h>

// host-only translation units (geometry.cpp, the check programs under tests/) include this header without HIP
#ifdef __HIPCC__
#define RGBD_HD __host__ __device__
#else
#define RGBD_HD
#endif

namespace rgbd {

constexpr int kMaxLevels = 12;
// k_describe reads kMaxLevels selection counts from each frame's row of nlevels unconditionally (and relies on
// ExtractCfg::sel_off_tab being INT32_MAX above nlevels, so no count above nlevels is ever summed): the counts
// buffer carries kMaxLevels entries of slack after the last frame's row.  launch_describe checks the size.
inline size_t sel_count_elems(int max_batch, int nlevels) { return (size_t)max_batch * nlevels + kMaxLevels; }
constexpr int kCellStride = 48;
#define RGBD_PYR_THREADS 512
constexpr int kPyrThreads = RGBD_PYR_THREADS;  // k_pyramid: threads per strip workgroup
#ifndef RGBD_PYR_STRIPS
#define RGBD_PYR_STRIPS 16
#endif
constexpr int kPyrStrips = RGBD_PYR_STRIPS;  // k_pyramid: horizontal strips per frame (one workgroup each; 10 / 12 / 16 ->
                                             // 3.685-3.697 / 3.695-3.701 / 3.664-3.669 ms per step: a 16th of 640 x 480 is
                                             // 39 KB of LDS, four workgroups per CU, profiles/blur_level0)
constexpr int kPyrLdsLimit = 150 * 1024;     // k_pyramid: most LDS a strip workgroup may ask for (level buffers + resize rows)
#define RGBD_BLUR_TH 48   // r04 (level blur of levels 1-7 in the k_fast grid): 16 / 32 / 48 rows -> 230.5k / 232.6k / 233.3k frames/s (profiles/r04_ab_blur_rows)
constexpr int kBlurTH = RGBD_BLUR_TH;        // level blur: rows per strip (one thread per 4-px column quad)
// bench.py's --full byte model (its PB_LEVELS, held to this line by tests/test_abi.py) charges the blurred bytes of
// this many levels to k_pyramid.  No code reads it: k_pyramid blurs nothing since level 0 moved to k_fast's tile
// waves, so that model's k_pyramid / k_fast figures are off by level 0's bytes ("Roofline accounting")
#define RGBD_PB_LEVELS 1
#ifndef RGBD_PYR_STRIP_LEVELS
#define RGBD_PYR_STRIP_LEVELS 4
#endif
// levels 0 .. kPyrStripLevels-1 are computed by k_pyramid's strips, the smaller ones after them by
// k_pyr_tail (one workgroup per frame; r06 A/B: 3 / 4 / 5 / all strip levels -> 228.4k / 229.6k / 226k / 225.7k
// frames/s, profiles/r06_ab/ab25-ab26)
constexpr int kPyrStripLevels = RGBD_PYR_STRIP_LEVELS;
#ifndef RGBD_PYR_TAIL_THREADS
#define RGBD_PYR_TAIL_THREADS 256
#endif
constexpr int kPyrTailThreads = RGBD_PYR_TAIL_THREADS;   // k_pyr_tail: threads per frame workgroup (256 / 512 alike, ab25)

struct LevelCfg {
    int32_t w, h, stride;      // level image, row stride in the pyramid buffer
    int32_t off;               // byte offset of the level inside one frame's pyramid
    int32_t minBX, maxBX, minBY, maxBY;   // ComputeKeyPointsOctTree borders (:619-622)
    int32_t cell_begin, cell_count;       // this level's FAST cells in the cell table
    int32_t N;                 // mnFeaturesPerLevel[level]
    int32_t nIni;              // DistributeOctTree root count (:420)
    float hX;                  // root width (:422)
    float scale;               // mvScaleFactor[level]
    float size;                // (float)(int)(PATCH_SIZE * scale) (:680)
    int32_t key_off;           // offset of this level's candidate region in a frame's key scratch
    int32_t key_cap;           // capacity of that region (sum of its cells' slot capacity, up to a multiple of 4)
    int32_t sel_off;           // offset of this level's selected-keypoint slots (per frame)
    int32_t rsx_off, rsy_off;  // resize tables (level l from l-1): x entries / y entries
    int32_t rs_xmax;           // first dx whose tap sx+1 falls outside the source row
    int32_t rs_simd;           // VResizeLinearVec_32s8u coverage [0, rs_simd)
    int32_t qx_off;            // this level's QuadX entries (k_pyramid's per-quad horizontal taps)
    double rs_scale_x, rs_scale_y;   // 1 / ((double)dst / src) of cv::resize (level l from l-1)
};

struct ExtractCfg {
    int32_t W, H, nlevels;
    int32_t frame_pyr_bytes;   // one frame's pyramid (all levels, padded rows)
    int32_t n_cells;           // FAST cells over all levels
    int32_t cell_cap;          // max NMS survivors of any cell (king-graph bound)
    int32_t dist_kc;           // quadtree: candidates per level whose round state fits in LDS (else HBM)
    int32_t keys_per_frame;    // key scratch entries per frame
    int32_t sel_per_frame;     // selected-keypoint slots per frame (sum of N+3)
    int32_t node_cap;          // quadtree node capacity (power of two)
    int32_t scan_cap;          // LDS scan scratch: max(node_cap, cells of any level) + 1
    int32_t kp_cap;            // output keypoints per frame
    int32_t ini_th, min_th;
    int32_t umax[16];
    // IC_Angle row weights for v_dot4 (row v + 15, dword k covers columns u = 4k - 15 .. 4k - 12):
    // ic_wu byte = u + 16 inside the disk (|u| <= umax[|v|]) else 0; ic_w1 byte = 1 inside else 0
    alignas(16) uint32_t ic_wu[31][8];
    alignas(16) uint32_t ic_w1[31][8];
    // camera
    float fx, fy, cx, cy, invfx, invfy;
    float k1, k2, p1, p2, k3;
    float depth_factor;
    int32_t undistort;
    // k_pyramid: rows [strip_r0, strip_r1) of each level computed (level > 0) or staged (level 0) by
    // strip s; a strip's rows include the halo its next level reads, so strips never exchange data
    int16_t strip_r0[kPyrStrips][kMaxLevels], strip_r1[kPyrStrips][kMaxLevels];
    int32_t pyr_top;           // levels [0, pyr_top) in the strips (min(nlevels, kPyrStripLevels)), the rest by k_pyr_tail
    int32_t pyr_lds;           // bytes of LDS per strip workgroup: even levels at 0, odd levels at pyr_lds_b
    int32_t pyr_lds_b;
    int32_t pyr_rsy_lds;       // bytes of the strip's resize row entries, staged after the level buffers
    // level blur of every level, inside the k_fast grid.  blur_thread: inner quads (x = 4 .. 4 * blur_tx[l]) of level l are threads [blur_t0[l], blur_t0[l + 1]),
    // strip-major; its edge quads (x = 0, then blur_ex[l] - 1 quads from 4 * (blur_tx[l] + 1)) are
    // threads blur_t0[kMaxLevels] + [blur_e0[l], blur_e0[l + 1])
    int32_t blur_t0[kMaxLevels + 1];
    int32_t blur_tx[kMaxLevels];
    int32_t blur_e0[kMaxLevels + 1];
    int32_t blur_ex[kMaxLevels];
    // level blur on the matrix cores (blur_tile_walk, RGBD_BLUR_MFMA): the levels it takes have no blur_thread
    // threads; level l owns the waves [blur_m0[l], blur_m0[l + 1]) ahead of the blur_thread blocks, strip-major:
    // blur_mt[l] 32-column tiles per strip of blur_ms[l] 32-row blocks; its tables (blur_tab.h) lie at byte
    // blur_tab_off[l] of the table buffer
    int32_t blur_m0[kMaxLevels + 1];
    int32_t blur_mt[kMaxLevels];
    int32_t blur_ms[kMaxLevels];
    int32_t blur_tab_off[kMaxLevels];
    // k_describe: lv[l].sel_off for l < nlevels, INT32_MAX above (one contiguous scalar load; a slot's level is
    // the count of levels >= 1 whose first slot it has reached, with no nlevels test)
    int32_t sel_off_tab[kMaxLevels];
    LevelCfg lv[kMaxLevels];
};

struct Cell {                  // one FAST ROI (rowRange/colRange of :655-660), level coordinates
    int16_t level, x0, y0, x1, y1, pad;
};

// k_fast, 0 / 1 for A/B builds: the leftover cells of a level's cell rows packed into full waves (host table +
// staging; 640 x 480: 229 -> 215 segments per frame, step 4.12 -> 4.06 ms, profiles/fast_pack_emit)
#ifndef RGBD_FAST_GATHER
#define RGBD_FAST_GATHER 1
#endif

// k_fast's blur blocks, 0 / 1 for A/B builds: 1 = levels of at least 64 x 32 px of a multi-level pyramid are
// blurred as 32 x 32 tiles on the matrix cores (blur_tile_walk), the smaller ones by blur_walk; 0 = blur_walk
// for all (profiles/blur_mfma)
#ifndef RGBD_BLUR_MFMA
#define RGBD_BLUR_MFMA 1
#endif
// 32-row blocks a tile wave walks down its 32-column strip after one warm-up block of horizontal sums: 2 / 4 / 7 /
// 13 (whole columns at 640 x 480) -> 3.927-3.963 / 3.843-3.872 / 3.796-3.844 / 3.790-3.794 ms per step against the
// parent's 3.905-3.933 (profiles/blur_mfma/ab_ms.txt); taller levels spread their blocks evenly over strips
#ifndef RGBD_BLUR_MS
#define RGBD_BLUR_MS 13
#endif
constexpr int kBlurMS = RGBD_BLUR_MS;

// k_fast's staged segment row.  A plain segment's cells lie side by side from a 16-B aligned start (<= 160 B);
// a gathered segment gives each of its 64 / lpc slots kFastRowBytes / (64 / lpc) bytes (48 / 64 / 96), which
// hold the cell's ROI row from its 4-B aligned start up to the last lane's 12-byte read (x1 + 6)
constexpr int kFastRowBytes = 192;
constexpr int kFastPlainRowBytes = 160;

struct FastSeg {               // k_fast: up to 64 / lpc cells of one level with one ROI height
    int32_t cell[4];           // slot k's cell (index into the cell table), k < ncell
    int16_t ncell;             // cells in the segment
    int16_t lpc;               // lanes per cell: 16 (interior <= 32 px wide, one DPP row) or the level's widest
                               // cell's pixel pairs, 17 .. 32 (so 3 cells of 17-21 pairs share a wave)
    int16_t gathered;          // 0: consecutive cells of one cell row, staged as one span; 1: the leftover cells
                               // of several cell rows (RGBD_FAST_GATHER), each staged into its own slot
    int16_t pad;
};

struct ResizeX { int16_t sx, a0, a1, pad; };   // xofs + ialpha
// k_pyramid's horizontal resize taps of one output quad (4 px): the quad's taps lie in the 12-byte source
// window wb .. wb + 11; pixel i's two taps are v_perm(sel[i]) of window dwords (pi_i, pi_i + 1) into a
// zero-extended u16 pair, dotted with wt[i] = (16 a0 | 16 a1 << 16) (weights x 16: the vertical pass
// then takes (r >> 4) << 8 as one mask); wbpi = wb | pi_bits << 16; simd bit i: pixel i in the SSE2
// vertical range [0, rs_simd)
struct QuadX { uint32_t wbpi; uint32_t sel[4]; uint32_t wt[4]; uint32_t simd; uint32_t pad[2]; };
struct ResizeY { int16_t sy0, sy1, b0, b1; };  // clipped source rows + ibeta

// packed candidate / selected keypoint: x (11 bits) | y (11 bits) | score (8 bits), coords
// relative to (minBorderX, minBorderY) of the level
RGBD_HD inline uint32_t pack_key(int x, int y, int s) { return (uint32_t)x | ((uint32_t)y << 11) | ((uint32_t)s << 22); }
RGBD_HD inline int key_x(uint32_t k) { return (int)(k & 2047u); }
RGBD_HD inline int key_y(uint32_t k) { return (int)((k >> 11) & 2047u); }
RGBD_HD inline int key_s(uint32_t k) { return (int)(k >> 22); }

}  // namespace rgbd
