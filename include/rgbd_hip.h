/*
 * rgbd_hip.h -- C ABI of the MI355X (gfx950) RGB-D tracking front end.
 *
 * Drop-in boundary for the reference hot path (toniortiz/rgbd-slam).  Every entry
 * point names the reference interface it replaces (file:line in the reference).
 * Plain pointers and sizes only; no C++/torch/OpenCV types cross this boundary.
 * Host-buffer entry points copy in/out; *_batch entry points take device pointers.
 *
 * Layout types mirror the reference's value types byte for byte:
 *   rgbd_keypoint == cv::KeyPoint (28 B), rgbd_dmatch == cv::DMatch (16 B),
 *   descriptors == cv::Mat N x 32 CV_8U rows, xyz == std::vector<cv::Point3f>.
 *
 * Errors: every call returns rgbd_status; RGBD_OK == 0.  rgbd_last_error() gives
 * the message.  Reference behaviour "bool false / identity pose = failure" is
 * reported through the `ok` out-parameters, not through rgbd_status.
 */
#ifndef RGBD_HIP_H
#define RGBD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rgbd_ctx rgbd_ctx;
typedef int32_t rgbd_status;

enum {
    RGBD_OK = 0,
    RGBD_ERR_ARG = 1,          /* bad argument / shape */
    RGBD_ERR_HIP = 2,          /* HIP runtime failure (no device, launch error, ...) */
    RGBD_ERR_CAPACITY = 3,     /* output capacity too small */
    RGBD_ERR_UNSUPPORTED = 4   /* configuration outside what the kernels support */
};

/* Extractor::setParameters(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
 * Features/Extractor.cpp:24-48 ; defaults (1000, 1.2f, 8, 20, 7) Features/Extractor.cpp:21 */
typedef struct {
    int32_t nfeatures;
    float scale_factor;
    int32_t nlevels;
    int32_t ini_th_fast;
    int32_t min_th_fast;
} rgbd_orb_params;

/* RGBDcamera + IntrinsicMatrix (Core/RGBDcamera.cpp:11-22, Core/IntrinsicMatrix.cpp:7-54).
 * depth_map_factor = 1/factor (RGBDcamera::mDepthMapFactor).  Distortion is applied
 * only when k1 != 0 (Core/Frame.cpp:256). */
typedef struct {
    float fx, fy, cx, cy;
    float k1, k2, p1, p2, k3;
    float depth_map_factor;
} rgbd_camera;

typedef struct {            /* cv::KeyPoint */
    float x, y, size, angle, response;
    int32_t octave, class_id;
} rgbd_keypoint;

typedef struct {            /* cv::DMatch */
    int32_t queryIdx, trainIdx, imgIdx;
    float distance;
} rgbd_dmatch;

/* RansacSE3(iters, minInlierTh, maxMahalanobisDist, sampleSize), Solver/SolverSE3.h:19.
 * Tracking uses (200, 10, 3.0f, 4), System/Tracking.cpp:129. */
typedef struct {
    int32_t iterations;
    uint32_t min_inlier_th;
    float max_mahalanobis;
    uint32_t sample_size;
} rgbd_ransac_params;

/* glibc rand() state (System/Random.cpp:10,19 use srand/rand): random_r TYPE_3. */
typedef struct {
    int32_t state[31];
    int32_t f, r;
} rgbd_rng;

/* RansacSE3::depthCovariance's function-static (Solver/SolverSE3.cpp:282-287), made explicit. */
typedef struct {
    double cov;
    int32_t set;
    int32_t pad;
} rgbd_sticky;

/* ------------------------------------------------------------------ context */
/* One context = one Extractor + RGBDcamera + device workspace, bound to one HIP device and
 * stream.  Not thread-safe (like ORBextractor, Features/ORBextractor.h:39); use one per thread. */
rgbd_status rgbd_create(int device, int width, int height, int max_batch, const rgbd_orb_params* orb,
                        const rgbd_camera* cam, rgbd_ctx** out);
void rgbd_destroy(rgbd_ctx* ctx);
const char* rgbd_last_error(const rgbd_ctx* ctx);
/* Upper bound on keypoints per frame (sum of per-level budgets + quadtree overshoot). */
int32_t rgbd_max_keypoints(const rgbd_ctx* ctx);
/* Use an external stream (hipStream_t) for all launches; NULL restores the context's own.  The new stream is
 * ordered behind the context's last extraction when that ran on another stream. */
rgbd_status rgbd_set_stream(rgbd_ctx* ctx, void* stream);

/* ------------------------------------------------------------------ extraction */
/* Extractor::detectAndCompute (Features/Extractor.h:40 -> ORBextractor::operator(),
 * Features/ORBextractor.cpp:706-766).  gray: host H x W u8 image with row step `step`. */
rgbd_status rgbd_detect_and_compute(rgbd_ctx* ctx, const uint8_t* gray, int32_t step, rgbd_keypoint* kps,
                                    uint8_t* desc, int32_t cap, int32_t* n);

/* Frame::Frame (Core/Frame.cpp:34-73): cvtColor + convertTo + extractFeatures +
 * undistortKeyPoints + uprojectCamera.  bgr: H x W x 3 u8, depth: H x W u16 (host). */
rgbd_status rgbd_frame(rgbd_ctx* ctx, const uint8_t* bgr, const uint16_t* depth, rgbd_keypoint* kps,
                       rgbd_keypoint* kps_un, uint8_t* desc, float* xyz, int32_t cap, int32_t* n);

/* Batched, device resident: d_bgr [B][H][W][3] u8, d_depth [B][H][W] u16 (device pointers).
 * Results stay on the device until read with rgbd_batch_frame / rgbd_batch_outputs. */
rgbd_status rgbd_extract_batch(rgbd_ctx* ctx, const void* d_bgr, const void* d_depth, int32_t B);
rgbd_status rgbd_batch_frame(rgbd_ctx* ctx, int32_t b, rgbd_keypoint* kps, rgbd_keypoint* kps_un,
                             uint8_t* desc, float* xyz, int32_t cap, int32_t* n);
/* Device pointers of the batch outputs: counts[B] i32, kps[B][K], kps_un[B][K], desc[B][K][32],
 * xyz[B][K][3] with K = rgbd_max_keypoints(). */
rgbd_status rgbd_batch_outputs(rgbd_ctx* ctx, void** counts, void** kps, void** kps_un, void** desc,
                               void** xyz);

/* Intermediate stages of the last batch, for parity tests (host copies). */
rgbd_status rgbd_debug_level(rgbd_ctx* ctx, int32_t b, int32_t level, uint8_t* out /* h*w */);
/* The blurred level (GaussianBlur 7x7 sigma 2 REFLECT_101 of the level, Features/ORBextractor.cpp:745-746)
 * the rBRIEF tests of the last extraction sampled (k_blur), h*w bytes. */
rgbd_status rgbd_debug_blurred(rgbd_ctx* ctx, int32_t b, int32_t level, uint8_t* out /* h*w */);
rgbd_status rgbd_debug_candidates(rgbd_ctx* ctx, int32_t b, int32_t level, int32_t* xys, int32_t cap,
                                  int32_t* n);
rgbd_status rgbd_debug_selected(rgbd_ctx* ctx, int32_t b, int32_t level, int32_t* xys, int32_t cap,
                                int32_t* n);
/* How the last extraction's quadtree of (frame b, level) was run: 0 = per-key round state, 1 = count / best-key
 * pyramids (no pass over the keys), 2 = the pyramid path abandoned for a node deeper than its bins (then the
 * per-key state), 3 = the pyramid path skipped up front (a tree of too few keys to fill).  The selection is the
 * same on every path. */
rgbd_status rgbd_debug_dist_path(rgbd_ctx* ctx, int32_t b, int32_t level, int32_t* path);

/* ------------------------------------------------------------------ SVO + BRIEF extractor */
/* Extractor(SVO, BRIEF, NORMAL), the reference's default front end (main.cpp:31): SVOextractor(nlevels, 5,
 * 20) (Features/Extractor.cpp:162-165; halfSample pyramid, FAST-10 + 3x3 NMS, Shi-Tomasi score, one keypoint
 * per 5x5 cell, Features/SVOextractor.cpp:86-137), retainBest(nfeatures) (Features/Extractor.cpp:56-57) and
 * cv::xfeatures2d::BriefDescriptorExtractor (32 bytes).  A context created this way runs it behind every
 * extraction entry point (rgbd_detect_and_compute, rgbd_frame, rgbd_extract_batch, the tracking chains).
 * Keypoints: size 0, angle -1, response = Shi-Tomasi score, octave = pyramid level (scale 2^level).
 * Shapes: the context builds the ORB geometry (1000 features, scale 1.2, 8 levels) before the SVO one, so it
 * inherits the ORB refusals (width a multiple of 16, every ORB level at least 48 px, the 48-px cell ROI rule,
 * height at most about twice the width); on top of them nlevels 1..8, even level widths above the last level,
 * at most 12288 grid cells (ceil(W / cell_size) * ceil(H / cell_size)) and sides of at most 2047 px, else
 * RGBD_ERR_UNSUPPORTED.  threshold: corners are found at this barrier and scored as the reference scores them,
 * max(m - 1, 20) (its score search starts at the literal 20, Features/SVOextractor.cpp:106-107). */
typedef struct {
    int32_t nfeatures;   /* 1000 (Extractor::setParameters) */
    int32_t nlevels;     /* 8 (1..8) */
    int32_t cell_size;   /* 5 */
    int32_t threshold;   /* FAST-10 barrier, 20 */
    int32_t max_keypoints;   /* output capacity per frame (rgbd_max_keypoints); 0: nfeatures + 64.  retainBest
                                keeps every tie of the boundary response, so more ties than the slack fail
                                loudly with RGBD_ERR_CAPACITY */
} rgbd_svo_params;
rgbd_status rgbd_create_svo(int device, int width, int height, int max_batch, const rgbd_svo_params* svo,
                            const rgbd_camera* cam, rgbd_ctx** out);
/* The 256 BRIEF tests, rows (y1, x1, y2, x2): bit t = SMOOTHED(y1, x1) < SMOOTHED(y2, x2), offsets in
 * [-24, 24].  OpenCV's own table (opencv_contrib xfeatures2d generated_32.i) is absent offline; the default
 * is a seeded stand-in drawn the same way (tools/gen_brief_pattern.py).  Load the real one here. */
rgbd_status rgbd_svo_set_brief_pattern(rgbd_ctx* ctx, const int8_t* pairs);
rgbd_status rgbd_svo_get_brief_pattern(rgbd_ctx* ctx, int8_t* pairs);
/* Intermediate stages of the last SVO batch (host copies, parity tests): a pyramid level (h x w), and the
 * grid keypoints with response > 20 in cell order before retainBest: xyl[i] = (x, y, level), resp[i]. */
rgbd_status rgbd_svo_debug_level(rgbd_ctx* ctx, int32_t b, int32_t level, uint8_t* out);
rgbd_status rgbd_svo_debug_grid(rgbd_ctx* ctx, int32_t b, int32_t* xyl, float* resp, int32_t cap, int32_t* n);
/* The device retainBest (libstdc++ nth_element + partition restated, k_svo_select's code) on n host
 * responses (n <= 12288): order[0..m) = the retained original indices in cv::KeyPointsFilter's order.
 * depth_limit < 0: introselect's own 2 lg n; >= 0 forces it (0 = the heap-select fallback). */
rgbd_status rgbd_svo_retain_best(rgbd_ctx* ctx, const float* resp, int32_t n, int32_t n_points, int32_t depth_limit,
                                 int32_t* order, int32_t* m);

/* ------------------------------------------------------------------ adaptive FAST + BRIEF extractor */
/* Extractor(FAST, BRIEF, ADAPTIVE) (Features/Extractor.cpp:24-61, 82-109): DetectorAdjuster ->
 * VideoDynamicAdaptedFeatureDetector -> VideoGridAdaptedFeatureDetector.  The frame is split into
 * grid_rows x grid_cols cells widened by edge_threshold; each cell runs cv::FAST on its ROI at its own
 * threshold (int)thresh, a double it carries from frame to frame and scales by `decrease` / `increase`
 * until the cell yields gridMin..gridMax corners (at most `iterations` tries), keeps its maxPerCell
 * strongest (std::nth_element at begin + maxPerCell), and the concatenated cells go through
 * retainBest(nfeatures) and cv::xfeatures2d::BriefDescriptorExtractor (32 bytes).  With maxFeatures =
 * (int)(min_features * 1.7): gridMin = round(min_features / (float)cells), gridMax = round(maxFeatures /
 * (float)cells), maxPerCell = maxFeatures / cells.  Keypoints: size 7, angle -1, response = the FAST score,
 * octave 0.  DESIGN.md, "Adaptive FAST + BRIEF definition".
 * The per-cell thresholds are the context's state: an extraction of B frames walks them through the frames
 * in order, and the next extraction starts where it ended (rgbd_adaptive_get / set_thresholds, _rewind).
 * Shapes: the refusals of a one-level ORB geometry (width a multiple of 16 and at least 64, the 48-px cell ROI
 * rule at level 0), sides of at most 2047 px, and RGBD_ERR_UNSUPPORTED
 * before any allocation unless 1 <= min_thresh <= init_thresh <= max_thresh <= 1e9, 0 < decrease < 1 <
 * increase, iterations in 1..32, a grid of 1..8 x 1..8, edge_threshold >= 0, every cell ROI at least 7 x 7,
 * 1 <= maxPerCell, maxFeatures <= 12288, nfeatures >= 0 and 1 <= cell_cap <= 12288. */
typedef struct {
    int32_t nfeatures;        /* 1000: retainBest(nfeatures) (Extractor::setParameters) */
    int32_t min_features;     /* 600 */
    int32_t grid_rows, grid_cols;   /* 3, 3 */
    int32_t edge_threshold;   /* 31: the cells' overlap margin */
    int32_t iterations;       /* 5: tries per cell and frame */
    int32_t cell_cap;         /* stored strict maxima per (frame, cell); 0: 8192.  A cell with more maxima at the
                                 threshold it used than were stored fails that frame with RGBD_ERR_CAPACITY */
    int32_t pad;
    double init_thresh;       /* 20 */
    double min_thresh;        /* 2 (>= 1) */
    double max_thresh;        /* 10000 */
    double increase;          /* 1.3 */
    double decrease;          /* 0.7 */
} rgbd_adaptive_params;
rgbd_status rgbd_create_adaptive(int device, int width, int height, int max_batch, const rgbd_adaptive_params* params,
                                 const rgbd_camera* cam, rgbd_ctx** out);
/* The cells' thresholds (grid_rows * grid_cols doubles, row-major), after the last extraction / for the next. */
rgbd_status rgbd_adaptive_get_thresholds(rgbd_ctx* ctx, double* thresh);
rgbd_status rgbd_adaptive_set_thresholds(rgbd_ctx* ctx, const double* thresh);
/* The next extraction starts from the thresholds in force before frame last_B - k of the last batch
 * (1 <= k <= last_B): a device-to-device copy queued on the context's stream, for batches that overlap by
 * k frames.  No host round trip. */
rgbd_status rgbd_adaptive_rewind(rgbd_ctx* ctx, int32_t k);
/* Cell `cell` of frame b of the last batch: the threshold before the frame (the double's bits), the integer
 * threshold of its last try, the number of tries, and the corners of that try in raster order as
 * (x, y, score) in ROI coordinates (what cv::FAST returned, before keepStrongest). */
rgbd_status rgbd_adaptive_debug_cell(rgbd_ctx* ctx, int32_t b, int32_t cell, uint64_t* thresh_before_bits,
                                     int32_t* thresh_used, int32_t* tries, int32_t* xys, int32_t cap, int32_t* n);
/* The device keepStrongest (std::nth_element(begin, begin + N, end, response >) restated, k_adp_select's
 * code) on n host responses (n <= 12288): order[0..min(n, N)) = the kept original indices in libstdc++'s
 * order.  depth_limit as for rgbd_svo_retain_best. */
rgbd_status rgbd_adaptive_keep_strongest(rgbd_ctx* ctx, const float* resp, int32_t n, int32_t N, int32_t depth_limit,
                                         int32_t* order);

/* ------------------------------------------------------------------ Shi-Tomasi GFTT + BRIEF extractor */
/* Extractor(GFTT, BRIEF, NORMAL) (Features/Extractor.cpp:50-61, 178-181): cv::GFTTDetector::create(nfeatures,
 * 0.01, 3, 3, false, 0.04), retainBest (never fires: at most nfeatures corners) and
 * cv::xfeatures2d::BriefDescriptorExtractor (32 bytes).  OpenCV 3.x's goodFeaturesToTrack restated: the minimum
 * eigenvalue e of the 3x3-summed Sobel covariance (f32, box sums in f64), thr = (float)(max e * quality_level),
 * candidates = interior pixels with e > thr that equal their thresholded 3x3 maximum, ranked by descending e
 * (equal values: the higher raster index first), then the sequential greedy that accepts a candidate unless an
 * accepted corner lies at integer dx*dx + dy*dy < min_distance^2, up to nfeatures.  Keypoints: size 3, angle -1,
 * response 0, octave 0, in acceptance order.  DESIGN.md, "GFTT + BRIEF definition"; tests/gftt_model.py.
 * The extractor has no frame-to-frame state.
 * Shapes: the refusals of a one-level ORB geometry (as for rgbd_create_adaptive), sides of 2..2047 px, and
 * RGBD_ERR_UNSUPPORTED before any allocation unless 1 <= nfeatures <= 12288, 0 < quality_level < 1,
 * min_distance finite in [0, 64] and 0 <= cand_cap <= 1048576. */
typedef struct {
    int32_t nfeatures;        /* 1000: maxCorners (Extractor::setParameters) */
    int32_t cand_cap;         /* stored candidates per frame; 0: 32768 (a uniform-noise 640 x 480 frame has about
                                 20,300).  A frame with more fails alone with RGBD_ERR_CAPACITY */
    double quality_level;     /* 0.01 */
    double min_distance;      /* 3; below 1 there is no spacing test */
} rgbd_gftt_params;
rgbd_status rgbd_create_gftt(int device, int width, int height, int max_batch, const rgbd_gftt_params* params,
                             const rgbd_camera* cam, rgbd_ctx** out);
/* The raw map e (width * height floats) of frame b of the last batch, recomputed from its gray image. */
rgbd_status rgbd_gftt_debug_eig(rgbd_ctx* ctx, int32_t b, float* out);
/* Frame b of the last batch: the bits of M = max e, the number of candidates found (it may exceed cand_cap),
 * and the accepted corners in acceptance order, before BRIEF's border filter, as (x, y) pairs with their
 * eigenvalues.  xy / val may be null to read the counts only. */
rgbd_status rgbd_gftt_debug_corners(rgbd_ctx* ctx, int32_t b, uint32_t* max_bits, int32_t* n_candidates, int32_t* xy,
                                    float* val, int32_t cap, int32_t* n);
/* How many ranks the greedy consumed on frame b of the last batch (all of them when the list ran out). */
rgbd_status rgbd_gftt_debug_ranks(rgbd_ctx* ctx, int32_t b, int32_t* ranks);
/* The device's rank + spacing stage (k_gftt_select, the code the extraction runs) on a host list of n distinct
 * points (x, y) inside W x H (sides <= 2047) with positive finite values: out_idx[0..m) = the accepted points'
 * list indices in acceptance order (room for min(n, max_corners)).  chunk = ranks per pass (1..4096; 0: the
 * default for max_corners); max_corners in 1..12288; n <= 1048576. */
rgbd_status rgbd_gftt_select(rgbd_ctx* ctx, const int32_t* xy, const float* val, int32_t n, int32_t W, int32_t H,
                             double min_distance, int32_t max_corners, int32_t chunk, int32_t* out_idx, int32_t* m);

/* ------------------------------------------------------------------ OpenCV ORB extractor */
/* Extractor(ORB, ORB, NORMAL) (Features/Extractor.cpp:50-61, 163-166, 216-218): cv::ORB::create(nfeatures,
 * scaleFactor, nlevels) as detector, retainBest(nfeatures), cv::ORB::create() as descriptor.  OpenCV 3.4's orb.cpp
 * restated: per pyramid level cv::FAST(fast_threshold, nonmax) over the whole level, runByImageBorder(
 * edge_threshold), retainBest(2 N_l) on the FAST score, the Harris response (7 x 7 block, k = 0.04), retainBest(N_l)
 * on it, IC_Angle, pt *= layerScale; then the frame-level retainBest and compute()'s provided-keypoints path
 * (runByImageBorder(31) at image scale, regrouping by octave, 7x7 sigma-2 blur, the 256 steered tests of
 * bit_pattern_31_).  Keypoints: size 31 * layerScale, response = Harris, class_id -1, level-major.  Fixed:
 * firstLevel 0, WTA_K 2, HARRIS_SCORE, patchSize 31, no mask.  DESIGN.md, "OpenCV ORB definition";
 * tests/cvorb_model.py.  No frame-to-frame state.  The pyramid and the blur are the ORB2 path's.
 * RGBD_ERR_UNSUPPORTED before any allocation: the ORB geometry's refusals for (width, height, scale_factor,
 * nlevels), a level size that differs from cv::ORB's, nfeatures outside 1..8192, fast_threshold outside 1..255,
 * edge_threshold outside 22..255 (22 = the descriptor's reach), cand_cap outside 0..12288, max_keypoints nonzero
 * and below nfeatures. */
typedef struct {
    int32_t nfeatures;        /* 1000 */
    float scale_factor;       /* 1.2f */
    int32_t nlevels;          /* 8 */
    int32_t edge_threshold;   /* 31 */
    int32_t fast_threshold;   /* 20 */
    int32_t cand_cap;         /* FAST corners stored per (frame, level) after the border filter; 0: 8192.  A frame with
                                 a level that has more fails alone with RGBD_ERR_CAPACITY */
    int32_t max_keypoints;    /* output capacity per frame; 0: nfeatures + nfeatures / 4.  retainBest keeps every tie of
                                 its boundary response, so a frame may keep more than nfeatures; one that keeps more
                                 than this fails alone with RGBD_ERR_CAPACITY */
} rgbd_cvorb_params;
rgbd_status rgbd_create_cvorb(int device, int width, int height, int max_batch, const rgbd_cvorb_params* params,
                              const rgbd_camera* cam, rgbd_ctx** out);
/* One level of frame b of the last batch, by stage:
 *   0  *n = the FAST corners after the border filter (the count goes on past cand_cap); nothing else is written
 *   1  the list after retainBest(2 N) in its order: xys[3 i ..] = (x, y, FAST score) in level coordinates
 *   2  harris[i] = the Harris response of entry i of stage 1's list
 *   3  the list after retainBest(N): xys and harris
 * xys / harris may be null; cap = entries they hold (RGBD_ERR_CAPACITY when the list is longer, *n still set).
 * On another kind of context: RGBD_ERR_ARG, "not a cv::ORB context". */
rgbd_status rgbd_cvorb_debug_level(rgbd_ctx* ctx, int32_t b, int32_t level, int32_t stage, int32_t* xys, float* harris,
                                   int32_t cap, int32_t* n);

/* ------------------------------------------------------------------ plain FAST extractor */
/* Extractor(FAST, BRIEF | ORB, NORMAL) (Features/Extractor.cpp:50-61, 168-171, 216-218, 224-226): cv::FastFeatureDetector::create()
 * over the whole image (cv::FAST(gray, threshold, nonmaxSuppression = true, TYPE_9_16), corners in [3, W - 3) x
 * [3, H - 3) in raster order, response = cornerScore<16>), retainBest(nfeatures) when there are more than nfeatures
 * corners (nth_element at nfeatures - 1, then every tie of the boundary response, in libstdc++'s element order),
 * then the descriptor.  RGBD_FAST_BRIEF: cv::xfeatures2d::BriefDescriptorExtractor (32 bytes, runByImageBorder(28));
 * rgbd_svo_set / get_brief_pattern work on such a context.  RGBD_FAST_ORB: cv::ORB::create()->compute() on the
 * provided keypoints: runByImageBorder(31), one level (every octave is 0), the 7x7 sigma-2 blur, the 256 tests of
 * bit_pattern_31_ steered by the keypoint's own angle, which compute() does not recompute: every descriptor is
 * steered by -1 degree; the BRIEF table entry points refuse such a context.  Keypoints: size 7, angle -1,
 * response = the FAST score, octave 0, class_id -1.  DESIGN.md, "Plain FAST definition"; tests/fast_model.py.  No
 * frame-to-frame state.
 * RGBD_ERR_UNSUPPORTED before any allocation: the refusals of a one-level ORB geometry (as for
 * rgbd_create_adaptive), sides above 2047 px, nfeatures outside 1..12288, threshold outside 1..255, a descriptor
 * other than the two named, cand_cap outside 0..65536, max_keypoints nonzero and outside nfeatures..65536. */
enum { RGBD_FAST_BRIEF = 0, RGBD_FAST_ORB = 1 };
typedef struct {
    int32_t nfeatures;        /* 1000: retainBest(nfeatures) (Extractor::setParameters) */
    int32_t threshold;        /* 10 (cv::FastFeatureDetector::create()'s default); 1..255 */
    int32_t descriptor;       /* RGBD_FAST_BRIEF | RGBD_FAST_ORB */
    int32_t cand_cap;         /* corners stored per frame before retainBest; 0: 32768, at most 65536 (a uniform-noise
                                 640 x 480 frame has 31,337).  A frame with more fails alone with RGBD_ERR_CAPACITY */
    int32_t max_keypoints;    /* output capacity per frame; 0: nfeatures + nfeatures / 4.  retainBest keeps every tie of
                                 its boundary response; a frame that keeps more than this (before the descriptor's
                                 border filter) fails alone with RGBD_ERR_CAPACITY */
} rgbd_fast_params;
rgbd_status rgbd_create_fast(int device, int width, int height, int max_batch, const rgbd_fast_params* params,
                             const rgbd_camera* cam, rgbd_ctx** out);
/* Frame b of the last batch: *n_candidates = the corners cv::FAST found (the count goes on past cand_cap), and the
 * stored ones in raster order, before retainBest, as xys[3 i ..] = (x, y, score); *n = how many were stored.  xys may
 * be null to read the counts only; cap = entries it holds (RGBD_ERR_CAPACITY when the list is longer).  On another
 * kind of context: RGBD_ERR_ARG, "not a FAST context". */
rgbd_status rgbd_fast_debug_corners(rgbd_ctx* ctx, int32_t b, int32_t* n_candidates, int32_t* xys, int32_t cap, int32_t* n);
/* The device retainBest of k_fast_select (both of its tiers: global scratch above 12288 live elements, LDS below) on
 * n host responses (n <= 65536): order[0..m) = the retained original indices in cv::KeyPointsFilter's order.
 * depth_limit as for rgbd_svo_retain_best. */
rgbd_status rgbd_fast_retain_best(rgbd_ctx* ctx, const float* resp, int32_t n, int32_t n_points, int32_t depth_limit,
                                  int32_t* order, int32_t* m);

/* ------------------------------------------------------------------ matching */
/* BFMatcher(NORM_HAMMING).knnMatch(k=2) (Features/Matcher.cpp:113): out[q] = {d1, i1, d2, i2}.
 * At most 65536 train rows (nt): the kernel's rank key holds the train index in 16 bits.  A larger nt
 * returns RGBD_ERR_UNSUPPORTED before anything is copied or launched; so does rgbd_match, which runs
 * rgbd_knn2 first. */
rgbd_status rgbd_knn2(rgbd_ctx* ctx, const uint8_t* desc_q, int32_t nq, const uint8_t* desc_t, int32_t nt,
                      int32_t* out);
/* Matcher::match (Features/Matcher.cpp:106-139): ratio test, unique train index (first query
 * wins), ref-outlier and both-depth-valid filters.  outlier_q: ref->mvbOutlier as u8;
 * z_q / z_t: mvKeys3Dc[i].z of ref / cur.  Output in query order. */
rgbd_status rgbd_match(rgbd_ctx* ctx, const uint8_t* desc_q, int32_t nq, const uint8_t* desc_t, int32_t nt,
                       const uint8_t* outlier_q, const float* z_q, const float* z_t, float nnratio,
                       int32_t discard_outliers, rgbd_dmatch* out, int32_t cap, int32_t* m);

/* Frame::computeImageBounds (Core/Frame.cpp:283-315): mnMinX, mnMaxX, mnMinY, mnMaxY.  k1 == 0: (0, W, 0, H);
 * otherwise from the four image corners undistorted like keypoints (cv::undistortPoints, k_undistort's code). */
typedef struct { float min_x, max_x, min_y, max_y; } rgbd_bounds;
/* The context's bounds, computed on first use (one small launch for a distorted camera) and cached. */
rgbd_status rgbd_image_bounds(rgbd_ctx* ctx, rgbd_bounds* out);

/* Matcher::projectionMatch(F1, F2, vMatches12, th) (Features/Matcher.cpp:35-104, Features/Matcher.h:26) over
 * Frame::unprojectWorld (Core/Frame.cpp:317-327), Frame::getFeaturesInArea with its default levels (-1, -1)
 * (:179-229) and the 64 x 48 grid of assignFeaturesToGrid / posInGrid (:75-89, :231-241); the operator is the
 * definition in DESIGN.md "Projection match definition".  F1: xyz1 = mvKeys3Dc (n1 x 3), desc1 (n1 x 32),
 * outlier1 = mvbOutlier as u8 (NULL: none), Tcw1 = its pose (row-major 4x4).  F2: kps_un2 = mvKeysUn (x and y
 * are read), xyz2 (z is read), desc2, Tcw2.  Camera = the context's; bounds NULL = the context's
 * (rgbd_image_bounds).  th finite in [0, 65536], else RGBD_ERR_ARG; n2 > 65536: RGBD_ERR_UNSUPPORTED (the rank
 * key holds a train position in 16 bits, as rgbd_knn2's).  Output in query order: {i1, i2, imgIdx -1 (the
 * three-argument cv::DMatch constructor), (float)distance}; *m = the match count, also when it exceeds cap
 * (RGBD_ERR_CAPACITY, the first cap matches written).  n1 == 0 or n2 == 0: RGBD_OK, *m = 0, nothing launched. */
rgbd_status rgbd_projection_match(rgbd_ctx* ctx, const float* xyz1, const uint8_t* desc1, const uint8_t* outlier1,
                                  int32_t n1, const float* Tcw1, const rgbd_keypoint* kps_un2, const float* xyz2,
                                  const uint8_t* desc2, int32_t n2, const float* Tcw2, const rgbd_bounds* bounds,
                                  float th, rgbd_dmatch* out, int32_t cap, int32_t* m);
/* The same over P pairs (qframe[p], tframe[p]) of the frames of the context's last rgbd_extract_batch, all pairs
 * in one pass (one workgroup chain per pair): poses = B x 16 Tcw (host), outlier = B x K u8 flags of the frames
 * as queries (host) or NULL, K = rgbd_max_keypoints.  out: P x K (host), counts[P].  qframe[p] < 0 skips pair p
 * (counts[p] = 0). */
rgbd_status rgbd_projection_match_batch(rgbd_ctx* ctx, int32_t P, const int32_t* qframe, const int32_t* tframe,
                                        const float* poses, const uint8_t* outlier, float th, rgbd_dmatch* out,
                                        int32_t* counts);
/* Parity hook, one pair with rgbd_projection_match's inputs: the geometry on its own, before the greedy
 * assignment.  Per query i1: uv_bits[2 i1 ..] = the f32 bits of (u, v) (Features/Matcher.cpp:63-64; 0 where not
 * computed: status 1-3); status[i1] = 0 searched, 1 outlier, 2 no depth, 3 behind the camera (invzc < 0), 4 out
 * of the image bounds or NaN, 5 no cell range (getFeaturesInArea's early returns, Core/Frame.cpp:185-199);
 * cand[i1 * cand_cap ..] = vIndices2 (:71) in visiting order, BEFORE the isValidObs and taken filters,
 * cand_count[i1] = its length (the first cand_cap are written). */
rgbd_status rgbd_debug_projection(rgbd_ctx* ctx, const float* xyz1, const uint8_t* desc1, const uint8_t* outlier1,
                                  int32_t n1, const float* Tcw1, const rgbd_keypoint* kps_un2, const float* xyz2,
                                  const uint8_t* desc2, int32_t n2, const float* Tcw2, const rgbd_bounds* bounds,
                                  float th, uint32_t* uv_bits, int32_t* status, int32_t* cand, int32_t cand_cap,
                                  int32_t* cand_count);

/* ------------------------------------------------------------------ solvers */
/* RansacSE3::compute (Solver/SolverSE3.cpp:23-133).  xyz1 = F1->mvKeys3Dc, xyz2 = F2->mvKeys3Dc
 * (N x 3 f32).  flags2 = F2->mvbOutlier (u8, updated when update_f2).  T21 row-major 4x4
 * (x2 = T21 x1), i.e. RansacSE3::mT21.  ok = the reference's bool result. */
rgbd_status rgbd_ransac_se3(rgbd_ctx* ctx, const float* xyz1, int32_t n1, const float* xyz2, int32_t n2,
                            const rgbd_dmatch* m12, int32_t m, const rgbd_ransac_params* prm, rgbd_rng* rng,
                            rgbd_sticky* sticky, int32_t update_f2, uint8_t* flags2, float* T21,
                            rgbd_dmatch* inliers, int32_t* n_inliers, float* rmse, int32_t* ok);

/* PnPRansac::compute (Solver/PnPRansac.cpp:14-56) -> cv::solvePnPRansac(v3D, v2D, K, noDist, r, t,
 * useExtrinsicGuess=false, 500, 3.0f, 0.85, inliers) (:39).  OpenCV is absent; the operator is the
 * definition in DESIGN.md "PnPRansac definition" (EPnP 5-point hypotheses on the cv::RNG((uint64)-1)
 * subset stream, float squared-pixel inlier test, RANSACUpdateNumIters, 10 Gauss-Newton steps on
 * the inliers).  min_matches: PnPRansac::compute returns false below 10 matches (:16, :35); 0 gives
 * the bare solvePnPRansac operator. */
typedef struct {
    int32_t iterations;          /* iterationsCount, 500 */
    float reprojection_error;    /* px, 3.0f */
    double confidence;           /* 0.85 */
    int32_t min_matches;         /* 10 in PnPRansac::compute */
    /* rgbd_pnp_track_*: 0 = every pair independent (Matcher discardOutliers = false); S >= 1 = the
     * reference's outlier-flag chain (Matcher::match discardOutliers = true, Features/Matcher.cpp:125-128,
     * on the flags PnPRansac::compute sets, Solver/PnPRansac.cpp:31,51) over S independent contiguous
     * runs of pairs (1 = one chain over the whole batch).  Ignored by rgbd_pnp_ransac(_batch). */
    int32_t flag_segments;
} rgbd_pnp_params;

/* One problem: p3 count x 3 f32 (object points), p2 count x 2 f32 (pixels, undistorted),
 * K4 = (fx, fy, cx, cy).  Out: R9 row-major (double), t3 (x_cam = R X + t), inlier_mask[count] u8
 * (the RANSAC inliers, optional), n_inliers, iters_run (RANSAC iterations), ok (the bool result). */
rgbd_status rgbd_pnp_ransac(rgbd_ctx* ctx, const float* p3, const float* p2, int32_t count, const float* K4,
                            const rgbd_pnp_params* prm, double* R9, double* t3, uint8_t* inlier_mask,
                            int32_t* n_inliers, int32_t* iters_run, int32_t* ok);
/* P independent problems in one pass (all hypotheses of all problems share launches): points of
 * problem p follow those of p-1 in p3 / p2 / masks; R9 [P][9], t3 [P][3], n_inliers / iters_run / ok [P]. */
rgbd_status rgbd_pnp_ransac_batch(rgbd_ctx* ctx, int32_t P, const int32_t* counts, const float* p3, const float* p2,
                                  const float* K4, const rgbd_pnp_params* prm, double* R9, double* t3,
                                  uint8_t* masks, int32_t* n_inliers, int32_t* iters_run, int32_t* ok);
/* The hidden state of the solve's schedule, for tests: the RANSAC iterations per problem that the NEXT
 * rgbd_pnp_ransac_batch (or tracking solve) evaluates in its first (k0) and second (k1) device chunk before the
 * host continues -- 8 and 16 on a fresh context, afterwards what the previous solve's iteration counts set (4..64
 * each).  Results do not depend on them (tests/test_gpu_pnp_edges.py).  No launch, no state change. */
rgbd_status rgbd_debug_pnp_chunks(rgbd_ctx* ctx, int32_t* k0, int32_t* k1);

/* PnPSolver::compute (Solver/PnPSolver.cpp:31-150): motion-only bundle adjustment of one pose from a guess and
 * 3D-2D matches -- one g2o SE(3) vertex, one EdgeSE3ProjectXYZOnlyPose per match under a Huber kernel, `rounds`
 * rounds of `iterations` Levenberg-Marquardt iterations, the edges reclassified against chi2_threshold between
 * rounds.  g2o is absent; the operator is the definition in DESIGN.md "Motion-only BA definition", the
 * reference's quirks included (every round restarts from the guess, an active edge is classified on the last
 * error evaluated, fewer than min_edges edges run one round).  Parity against g2o is unpinned. */
typedef struct {
    int32_t rounds;          /* 4 */
    int32_t iterations;      /* 10, per round */
    double  chi2_threshold;  /* 5.991; Huber delta = sqrt of it */
    int32_t robust_rounds;   /* 3: the kernel is removed after round index 2 */
    int32_t min_edges;       /* 10: fewer edges -> only round 0 */
} rgbd_pnp_solver_params;

/* One problem: Xw M x 3 f32 (world points), obs M x 2 f32 (undistorted pixels), K4 = (fx, fy, cx, cy), Tcw_in
 * the guess (row-major 4x4 float).  prm NULL = the reference's values above (rounds in [1, 16], iterations >= 1,
 * chi2_threshold finite and > 0, else RGBD_ERR_ARG).  Out: Tcw_out (row-major 4x4 float), outlier_mask[M] u8 = 1
 * where the edge ended flagged outlier, n_inliers, ok = the bool result: 0 for M < 3, and then nothing else is
 * written.  M > 4096: RGBD_ERR_UNSUPPORTED before any copy or launch.  Inputs must be finite. */
rgbd_status rgbd_pnp_solver(rgbd_ctx* ctx, const float* Xw, const float* obs, int32_t M, const float* K4,
                            const float* Tcw_in, const rgbd_pnp_solver_params* prm, float* Tcw_out,
                            uint8_t* outlier_mask, int32_t* n_inliers, int32_t* ok);
/* P independent problems in one launch (one workgroup each): the edges of problem p follow those of p-1 in Xw /
 * obs / masks; Tcw_in and Tcw_out [P][16], n_inliers / ok [P].  P = 0, or no problem with 3 edges: RGBD_OK and
 * nothing launched. */
rgbd_status rgbd_pnp_solver_batch(rgbd_ctx* ctx, int32_t P, const int32_t* counts, const float* Xw, const float* obs,
                                  const float* K4, const float* Tcw_in, const rgbd_pnp_solver_params* prm,
                                  float* Tcw_out, uint8_t* masks, int32_t* n_inliers, int32_t* ok);
/* The same over P pairs (qframe[p], tframe[p]) of the frames of the context's last rgbd_extract_batch, reading
 * rgbd_projection_match_batch's output as it stands: poses = B x 16 Tcw (host), matches = P x K (host), counts[P],
 * K = rgbd_max_keypoints (<= 4096).  Edge i of pair p: obs = the train frame's mvKeysUn[trainIdx]; Xw =
 * unprojectWorld(trainIdx) of the TRAIN frame under its own pose when as_written (Solver/PnPSolver.cpp:65), else
 * unprojectWorld(queryIdx) of the query frame under its pose; the guess = poses[tframe[p]]; the camera = the
 * context's.  masks: P x K by match position.  qframe[p] < 0 skips pair p (ok[p] = 0).  A match index outside
 * [0, K): RGBD_ERR_ARG. */
rgbd_status rgbd_pnp_solver_frames(rgbd_ctx* ctx, int32_t P, const int32_t* qframe, const int32_t* tframe,
                                   const float* poses, const rgbd_dmatch* matches, const int32_t* counts,
                                   int32_t as_written, const rgbd_pnp_solver_params* prm, float* Tcw_out,
                                   uint8_t* masks, int32_t* n_inliers, int32_t* ok);
/* Parity hook: rgbd_pnp_solver plus, per round r < rounds (zeros for a round not run; rounds_run = the rounds
 * run): round_est[7 r ..] = the round's final estimate (qx qy qz qw tx ty tz), round_iters / round_trials = the
 * LM iterations and trials run, round_lambda / round_nu = lambda and nu after the round; per round and edge
 * edge_chi2[r M + i] = the chi2 the classification read and edge_level[r M + i] = the level it set. */
rgbd_status rgbd_debug_pnp_solver(rgbd_ctx* ctx, const float* Xw, const float* obs, int32_t M, const float* K4,
                                  const float* Tcw_in, const rgbd_pnp_solver_params* prm, float* Tcw_out,
                                  uint8_t* outlier_mask, int32_t* n_inliers, int32_t* ok, int32_t* rounds_run,
                                  double* round_est, int32_t* round_iters, int32_t* round_trials,
                                  double* round_lambda, double* round_nu, double* edge_chi2, uint8_t* edge_level);

/* Ransac::compute (Solver/Ransac.cpp:46-181): the plain 3D-3D RANSAC -- unweighted rigid Eigen::umeyama on
 * used_pairs sampled matches, a Euclidean or depth-adaptive inlier test, an iteration count that adapts to the best
 * inlier ratio, and a re-fit on the winner's inliers.  Eigen is absent; the operator is the definition in DESIGN.md
 * "Umeyama RANSAC definition" (sequential f32 sums, the f32 JacobiSVD sweeps, a saturating iteration count).
 * Parity against the reference binary is unpinned.  error_version follows Ransac::ERROR_VERSION: 0 EUCLIDEAN_ERROR,
 * 4 ADAPTIVE_ERROR; 1, 2 (reprojection) and 3 (MAHALANOBIS_ERROR) are RGBD_ERR_UNSUPPORTED, as are used_pairs outside
 * [3, 8], min_matches < used_pairs, min_inlier_ratio outside [0.05, 1] and more than 4096 matches, all before any
 * copy or launch.  The parameters' iterationCount is ignored by the reference (:26) and has no field here. */
typedef struct {
    int32_t error_version;
    int32_t used_pairs;          /* usedPairs */
    int32_t min_matches;         /* minimalNumberOfMatches */
    int32_t pad;
    double  thr_euclidean;       /* inlierThresholdEuclidean (m; times the F1 point's z under ADAPTIVE_ERROR) */
    double  min_inlier_ratio;    /* minimalInlierRatioThreshold */
} rgbd_umeyama_params;

/* One pair: xyz1 = F1->mvKeys3Dc (n1 x 3 f32), xyz2 = F2->mvKeys3Dc, m12 the matches (queryIdx into F1, trainIdx into
 * F2; an index outside: RGBD_ERR_ARG).  rng in / out: glibc rand() after the last draw of the loop.  flags2 in / out =
 * F2->mvbOutlier (n2 bytes): every match's trainIdx is set 1, then the final inliers' 0.  Out: T12 row-major 4x4
 * (x1 = T12 x2: F2's camera points into F1's camera), inliers (capacity m) and n_inliers, iterations_run (RANSAC
 * iterations, 0 when fewer than min_matches pass the depth gate), ok = !T12.isIdentity(1e-5), the bool result. */
rgbd_status rgbd_ransac_umeyama(rgbd_ctx* ctx, const float* xyz1, int32_t n1, const float* xyz2, int32_t n2,
                                const rgbd_dmatch* m12, int32_t m, const rgbd_umeyama_params* prm, rgbd_rng* rng,
                                uint8_t* flags2, float* T12, rgbd_dmatch* inliers, int32_t* n_inliers,
                                int32_t* iterations_run, int32_t* ok);
/* P independent pairs in one launch (one workgroup each).  Pair p's clouds, flags, matches and inliers follow those
 * of pair p - 1 in xyz1 (n1[p] rows), xyz2 and flags2 (n2[p]), m12 and inliers (counts[p]); rngs, T12 [P][16],
 * n_inliers / iterations_run / ok [P].  P = 0: RGBD_OK and nothing launched. */
rgbd_status rgbd_ransac_umeyama_batch(rgbd_ctx* ctx, int32_t P, const float* xyz1, const int32_t* n1, const float* xyz2,
                                      const int32_t* n2, const rgbd_dmatch* m12, const int32_t* counts,
                                      const rgbd_umeyama_params* prm, rgbd_rng* rngs, uint8_t* flags2, float* T12,
                                      rgbd_dmatch* inliers, int32_t* n_inliers, int32_t* iterations_run, int32_t* ok);
/* The same over P pairs (F1 = frame qframe[p], F2 = frame tframe[p]) of the context's last rgbd_extract_batch, the
 * points read from the device-resident mvKeys3Dc.  matches, inliers and flags2 are P x K (host), K =
 * rgbd_max_keypoints, counts[P].  qframe[p] < 0 skips pair p (identity, ok 0, its rng and flags untouched).  A frame
 * or match index outside its range: RGBD_ERR_UNSUPPORTED. */
rgbd_status rgbd_ransac_umeyama_frames(rgbd_ctx* ctx, int32_t P, const int32_t* qframe, const int32_t* tframe,
                                       const rgbd_dmatch* matches, const int32_t* counts, const rgbd_umeyama_params* prm,
                                       rgbd_rng* rngs, uint8_t* flags2, float* T12, rgbd_dmatch* inliers,
                                       int32_t* n_inliers, int32_t* iterations_run, int32_t* ok);
/* Parity hook: rgbd_ransac_umeyama plus, per evaluated hypothesis h < min(iterations_run, hyp_cap): hyp_pos[h
 * used_pairs ..] = its sample (positions among the gated matches, in draw order), hyp_count[h] = its inliers (-1:
 * the model failed), hyp_sneg[h] = 1 where Umeyama took S = (1, 1, -1); best_count = the inliers of the loop's best
 * model; accepts[3 a ..] = (iteration, count, new bound) of acceptance a < min(n_accepts, accept_cap). */
rgbd_status rgbd_debug_ransac_umeyama(rgbd_ctx* ctx, const float* xyz1, int32_t n1, const float* xyz2, int32_t n2,
                                      const rgbd_dmatch* m12, int32_t m, const rgbd_umeyama_params* prm, rgbd_rng* rng,
                                      uint8_t* flags2, float* T12, rgbd_dmatch* inliers, int32_t* n_inliers,
                                      int32_t* iterations_run, int32_t* ok, int32_t hyp_cap, int32_t* hyp_pos,
                                      int32_t* hyp_count, uint8_t* hyp_sneg, int32_t* best_count, int32_t accept_cap,
                                      int32_t* accepts, int32_t* n_accepts);
/* Host only: Tcw2 = inv(T12) * Tcw1 (:53), the inverse as DESIGN.md defines it (f32 Gaussian elimination with
 * partial pivoting; cv::Mat::inv() itself is unpinned). */
void rgbd_ransac_umeyama_pose(const float* T12, const float* Tcw1, float* Tcw2);

/* Gicp (Solver/Gicp.cpp) over pcl::GeneralizedIterativeClosestPoint; Tracking sets max correspondence
 * distance 0.07 and 10 iterations (System/Tracking.cpp:147-151) on the ctor's 1e-9 transformation
 * epsilon (Solver/Gicp.cpp:12-15).  PCL is absent: DESIGN.md "GICP" defines the operator (PCL
 * covariances / correspondences / convergence restated; BFGS replaced by gn_iterations Gauss-Newton
 * steps per outer iteration). */
typedef struct {
    int32_t max_iterations;          /* 10 */
    int32_t k_correspondences;       /* 20 */
    double max_corr_dist;            /* 0.07 m */
    double transformation_epsilon;   /* 1e-9 */
    double rotation_epsilon;         /* 2e-3 */
    double gicp_epsilon;             /* 1e-3 */
    int32_t gn_iterations;           /* 4 */
    int32_t enable;                  /* tracking chains: run GICP when RansacSE3's rmse >= 0.8 */
} rgbd_gicp_params;

/* GeneralizedIterativeClosestPoint::align(out, guess): src / tgt M x 3 f32 (M <= 2048, M >= k),
 * guess row-major 4x4.  T = final_transformation_ (identity unless converged).  M < k: PCL computes no
 * covariances, RGBD_OK and not converged; M > 2048 or k outside [1, 32]: RGBD_ERR_UNSUPPORTED.  Coordinates
 * must be finite (the tracking chain passes valid-depth inliers; PCL's k-NN orders NaN differently). */
rgbd_status rgbd_gicp(rgbd_ctx* ctx, const float* src, const float* tgt, int32_t M, const float* guess,
                      const rgbd_gicp_params* prm, float* T, int32_t* converged, int32_t* iterations);
/* Gicp::compute (Solver/Gicp.cpp:21-35): < 20 pairs -> false; not converged or T.isIdentity() -> false. */
rgbd_status rgbd_gicp_compute(rgbd_ctx* ctx, const float* src, const float* tgt, int32_t M, const float* guess,
                              const rgbd_gicp_params* prm, float* T, int32_t* ok);
/* GICP stage of rgbd_track_batch (default: enabled with Tracking's settings); NULL restores the default. */
rgbd_status rgbd_set_tracking_gicp(rgbd_ctx* ctx, const rgbd_gicp_params* prm);

/* glibc srand(seed) restated (System/Random.cpp:10) so callers can seed deterministically. */
void rgbd_rng_seed(rgbd_rng* rng, uint32_t seed);

/* ------------------------------------------------------------------ tracking front end */
/* Tracking::visualOdometry over a device-resident sequence chunk (System/Tracking.cpp:121-163):
 * frame 0 of the chunk is the reference (pose = Tcw0); for b >= 1: Matcher(ratio).match(prev, cur)
 * -> RansacSE3 -> retry against the second reference -> GICP when rmse >= 0.8 (guess = mT21, clouds
 * = the RANSAC inliers; see rgbd_set_tracking_gicp) -> recover() on failure.  poses: B x 16 row-major Tcw out (in: poses[0..15] = Tcw of frame 0).
 * status[b] = 1 tracked, 0 recovered. n_inliers[b] = |mvInliers|. */
rgbd_status rgbd_track_batch(rgbd_ctx* ctx, const void* d_bgr, const void* d_depth, int32_t B, float nnratio,
                             const rgbd_ransac_params* prm, rgbd_rng* rng, rgbd_sticky* sticky, float* poses,
                             int32_t* status, int32_t* n_inliers);

/* Tracking's state carried from one chunk to the next (System/Tracking.cpp:39-73, 227-256).  Consecutive
 * chunks overlap by TWO frames: a continuing chunk's frames 0 and 1 are the previous chunk's last two
 * (already tracked; their features are extracted again, bit-identically), and tracking resumes at its
 * frame 2 with mpRefFrame.second / .first, their outlier flags, the keyframe and the last relative pose
 * exactly as the previous chunk left them, so a sequence split into chunks tracks bit-exactly as one chunk. */
typedef struct rgbd_track_state {
    float kf_pose[16];      /* mpLastKeyFrame->getPose() when the keyframe is before the chunk's frame 1 */
    float first_rel[16];    /* mRelativeFramePoses.back(): Tcr of the previous chunk's last frame */
    float ref2_pose[16];    /* pose of the previous chunk's second-to-last frame (as updateLastFrame left it) */
    int32_t first_is_kf;    /* the previous chunk's last frame is the last keyframe */
    int32_t valid;          /* 0: frame 0 starts the sequence (Tracking::initialize: keyframe) */
    uint8_t* flags2;        /* caller-owned, >= kp capacity bytes: outlier flags of the second-to-last frame */
    uint8_t* flags1;        /* caller-owned, >= kp capacity bytes: outlier flags of the last frame */
    int32_t flags_cap;      /* bytes of flags2 / flags1 (checked against rgbd_max_keypoints: RGBD_ERR_CAPACITY) */
} rgbd_track_state;

/* Tracking::track (System/Tracking.cpp:39-73) over a chunk: rgbd_track_batch's visualOdometry plus
 * updateLastFrame (the previous frame's pose rewritten as Tlr * pose(its keyframe), :242-247, which the
 * second-reference retry then reads), needKeyFrame / createKeyFrame (:201-240) and updateRelativePose
 * (:249-256), in the reference's float Mat arithmetic.  poses[b] = track()'s return for frame b (in: frame
 * 0's pose for a new sequence; for a continuing chunk (state->valid) poses[16..31] = the previous chunk's
 * last output, and frames 0 and 1 are not tracked again: their outputs are left as given, except poses[0]
 * = state->ref2_pose).  rel_poses (B x 16, optional) = mRelativeFramePoses; keyframe[b] (optional) = 1 when
 * frame b is a keyframe.  state in/out (zero it for a new sequence; flags2 / flags1 may be NULL, then a
 * continuing chunk starts with clear flags).  Replaces the tracker.track(frame) loop of main.cpp:43 for
 * this path. */
rgbd_status rgbd_track_batch_kf(rgbd_ctx* ctx, const void* d_bgr, const void* d_depth, int32_t B, float nnratio,
                                const rgbd_ransac_params* prm, rgbd_rng* rng, rgbd_sticky* sticky,
                                rgbd_track_state* state, float* poses, int32_t* status, int32_t* n_inliers,
                                float* rel_poses, int32_t* keyframe);

/* Tracking::visualOdometry (as rgbd_track_batch) over L independent lanes of ONE device-resident batch,
 * all lanes advanced together on the device (config 3's throughput form; a lane is a contiguous chunk of
 * the sequence tracked as its own chain, like the multi-GPU chunks).  lane_first[0..L]: lane l covers frames
 * lane_first[l] .. lane_first[l + 1] (its first frame is its reference: it starts the lane's chain with
 * clear outlier flags; lane_first[0] = 0, lane_first[L] = B - 1, strictly increasing), so consecutive lanes
 * share one frame.  rngs[l] / stickies[l] are lane l's RNG and sticky covariance (in/out).  Outputs are
 * lane-major: lane l owns rows lane_first[l] + l .. lane_first[l + 1] + l of poses ((B + L - 1) x 16),
 * status and n_inliers ((B + L - 1)); a lane's first row is its reference frame: poses in (lane 0: the
 * sequence's first pose; the others: the identity, so the chains stitch like rgbd-slam_amd/dist.py's),
 * status 1, n_inliers 0.  Equals rgbd_track_batch run on each lane's frames with its own RNG and sticky
 * state, bit for bit.  d_bgr = d_depth = NULL tracks the frames of the context's last rgbd_extract_batch
 * (of the same B), so a caller can run extraction and tracking as two calls (e.g. serialise the
 * extractions of several contexts, each overlapping another context's lane rounds).  If rgbd_set_stream
 * changed the context stream in between, the tracking launches wait on an event recorded after the
 * extraction, so no host synchronisation is needed between the two calls. */
rgbd_status rgbd_track_lanes(rgbd_ctx* ctx, const void* d_bgr, const void* d_depth, int32_t B, float nnratio,
                             const rgbd_ransac_params* prm, int32_t L, const int32_t* lane_first, rgbd_rng* rngs,
                             rgbd_sticky* stickies, float* poses, int32_t* status, int32_t* n_inliers);

/* Parity hook: the device's std::sort(vUsedMatches) (Solver/SolverSE3.cpp:52; libstdc++ introsort order
 * of DMatch::operator< on the distance) over n <= 2304 integer-valued distances: order[i] = the input index
 * at sorted position i.  depth_limit < 0: introsort's own 2 lg n; >= 0 forces it (0 = the heap-sort path). */
rgbd_status rgbd_debug_sort_matches(rgbd_ctx* ctx, const float* dist, int32_t n, int32_t depth_limit, int32_t* order);
/* k_fast's emission rank for 16-lane cells (the row_newbcast DPP sequence, csrc/extract.hip fast_rank16) on
 * its own: flags[rows][64] (0/1) -> slots[rows][64] (0xffffffff where the flag is clear) and counts[64], every
 * 16-lane row starting at slot 1000 x row.  Test hook for the rank k_fast's cell lists are built with. */
rgbd_status rgbd_debug_fast_rank16(rgbd_ctx* ctx, const uint8_t* flags, int32_t rows, uint32_t* slots, uint32_t* counts);
/* The Jacobi rotations' short sqrt / division sequences (csrc/pnp.hip sqrt_ge1, div_plain, rot_t) on their own:
 * sq[i] = sqrt(x[i]) for finite x[i] >= 1, q[i] = num[i] / den[i] for the operand ranges the Jacobi rotation and
 * the 3x3 SVD feed them (|den| in [1, 2^1000), num / den normal, |num| >= 2^-969 unless den == 1), t[i] =
 * sign(theta) / (|theta| + sqrt(theta^2 + 1)) for any non-NaN theta[i]; test hook for the claim that they return
 * the bits of the IEEE expressions (tests/test_gpu_pnp.py: the rotation's and the SVD's operand sets). */
rgbd_status rgbd_debug_rotation_ops(rgbd_ctx* ctx, const double* x, const double* num, const double* den,
                                    const double* theta, int32_t n, double* sq, double* q, double* t);
/* rgbd_gicp's covariance stage on its own (csrc/gicp.hip k_gicp_cov, launched with pts as source and as target):
 * cov[i] = the row-major 3x3 regularised covariance of pts[i] from its k nearest neighbours in pts, for every
 * point, including those that never get a correspondence and so never reach rgbd_gicp's result.  Checks as
 * rgbd_gicp: M > 2048 or k outside [1, 32] is RGBD_ERR_UNSUPPORTED; so is M < k (PCL computes no covariances,
 * rgbd_gicp reports not converged).  Coordinates must be finite (NaN orders differently in PCL's k-NN). */
rgbd_status rgbd_debug_gicp_cov(rgbd_ctx* ctx, const float* pts, int32_t M, int32_t k, double eps, double* cov /* M x 9 */);

/* Extract + match + PnPRansac over a device-resident chunk (the benchmark path named by the
 * north star; the reference's Tracking uses RansacSE3, see rgbd_track_batch).  For b >= 1:
 * Matcher(nnratio).match(F_{b-1}, F_b, m, discardOutliers=false) -> PnPRansac with F_{b-1}'s
 * mvKeys3Dc as object points and F_b's mvKeysUn as pixels (SURVEY A-9: the reference's own
 * PnPRansac reads F2's 3D; the C++ surface keeps that as an option) -> pose(b) = [R|t] pose(b-1),
 * else recover() (pose(b) = pose(b-1)).  All B-1 pairs are independent and solved in one pass.
 * poses: B x 16 row-major (in: poses[0..15]); status[b], n_inliers[b], n_matches[b] per frame. */
rgbd_status rgbd_pnp_track_batch(rgbd_ctx* ctx, const void* d_bgr, const void* d_depth, int32_t B, float nnratio,
                                 const rgbd_pnp_params* prm, float* poses, int32_t* status, int32_t* n_inliers,
                                 int32_t* n_matches);
/* The same step split for streaming callers: submit enqueues extraction, matching and the 3D-2D
 * gather and returns without waiting; collect waits for the OLDEST outstanding submission's solve
 * only, finishes its RANSAC (host continuation when a pair needs more than the first chunk) and
 * writes the outputs exactly as rgbd_pnp_track_batch would.  At most three submissions are
 * outstanding (each owns one of three workspaces), so the host work of step i overlaps the device
 * work of steps i+1 and i+2.  The device part of a submission's PnPRansac runs on the context's
 * high-priority solve stream; it is launched by the next submission right after that one's quadtree
 * kernel (ordered after both by events), so the latency-bound solve overlaps the description and the
 * following pyramid rather than the VALU-bound FAST; collect launches it itself if no submission
 * followed.  Consecutive submissions alternate between two sets of extraction outputs, and a
 * submission's knn-2 + gather run on a match stream, so they overlap the next extraction
 * (rgbd_batch_frame / rgbd_batch_outputs read the set of the latest submission).
 * The frames of a submission must stay valid until its collect. */
rgbd_status rgbd_pnp_track_submit(rgbd_ctx* ctx, const void* d_bgr, const void* d_depth, int32_t B, float nnratio,
                                  const rgbd_pnp_params* prm);
rgbd_status rgbd_pnp_track_collect(rgbd_ctx* ctx, float* poses, int32_t* status, int32_t* n_inliers,
                                   int32_t* n_matches);

/* ------------------------------------------------------------------ keyframe dense cloud */
/* Tracking::createKeyFrame's cloud (System/Tracking.cpp:234-237): Frame::createCloud(stride) samples
 * (z = depth * 1/factor > 0, RGBDcamera::unproject, BGR colour; Core/Frame.cpp:475-505), PCL PassThrough
 * on z (:537-549), VoxelGrid(leaf) (:516-524) and StatisticalOutlierRemoval(sor_k, sor_std)
 * (:526-535).  PCL is absent: its algorithms are the definitions in DESIGN.md "Keyframe cloud
 * definition" (one deviation: points of a voxel are summed in point order).  rgbd_point = the
 * pcl::PointXYZRGB payload (xyz + packed rgb bytes b, g, r, 0). */
typedef struct { float x, y, z; uint8_t b, g, r, pad; } rgbd_point;
typedef struct {
    int32_t stride;     /* createCloud(6) */
    float zmin, zmax;   /* passThroughFilter("z", 0.5, 4.0) */
    float leaf;         /* downsampleCloud(0.04f) */
    int32_t sor_k;      /* statisticalFilterCloud(50, 1.0), 1 <= sor_k <= 63 */
    double sor_std;
} rgbd_cloud_params;
/* One frame from host buffers (BGR8 + u16 depth of the context's size); *n points in out[cap]. */
rgbd_status rgbd_keyframe_cloud(rgbd_ctx* ctx, const uint8_t* bgr, const uint16_t* depth, const rgbd_cloud_params* prm,
                                rgbd_point* out, int32_t cap, int32_t* n);
/* The same from the Frame's own members, as Frame::createCloud reads them (Core/Frame.cpp:484-495): bgr =
 * mImColor, depth = mImDepth (H x W f32, already imDepth.convertTo(CV_32F, mDepthMapFactor), :48). */
rgbd_status rgbd_keyframe_cloud_f32(rgbd_ctx* ctx, const uint8_t* bgr, const float* depth, const rgbd_cloud_params* prm,
                                    rgbd_point* out, int32_t cap, int32_t* n);
/* The listed frames of a device-resident batch (B frames, as rgbd_extract_batch), one workgroup chain
 * per keyframe; keyframe k's points in out[k * cap ...], counts[k]. */
rgbd_status rgbd_keyframe_cloud_batch(rgbd_ctx* ctx, const void* d_bgr, const void* d_depth, int32_t B,
                                      const int32_t* frames, int32_t nkf, const rgbd_cloud_params* prm,
                                      rgbd_point* out, int32_t cap, int32_t* counts);

/* ------------------------------------------------------------------ pose graph (host) */
/* The keyframe pose graph of the reference's PoseGraph thread (Solver/PoseGraph.cpp): g2o
 * VertexSE3 (Twc) / EdgeSE3 (information info * I, RobustKernelHuber(delta)) optimised by
 * Levenberg-Marquardt (:40-57, :184-244, :368-386).  g2o is absent: the optimiser is the
 * definition in DESIGN.md "Pose graph" (g2o's error, oplus and LM schedule; numeric Jacobians,
 * dense Cholesky).  Host code; the edges' relative poses come from the device Matcher + RansacSE3. */
typedef struct rgbd_posegraph rgbd_posegraph;
rgbd_status rgbd_pg_create(rgbd_posegraph** out);
void rgbd_pg_destroy(rgbd_posegraph* g);
/* PoseGraph::createNode (:184-196): estimate = Twc (row-major 4x4), fixed (vertex 0 in the reference) */
rgbd_status rgbd_pg_add_vertex(rgbd_posegraph* g, int32_t id, const double* Twc, int32_t fixed);
rgbd_status rgbd_pg_set_fixed(rgbd_posegraph* g, int32_t id, int32_t fixed);
/* PoseGraph::createEdgeWithReference / createEdge (:198-244): measurement Z (x_from = Z x_to in
 * camera coordinates, i.e. RansacSE3::mT21 with F1 = to, F2 = from) or NULL for
 * setMeasurementFromState; *chi2 = the edge's robust chi2 at insertion (edge->chi2()). */
rgbd_status rgbd_pg_add_edge(rgbd_posegraph* g, int32_t from, int32_t to, const double* Z, double info,
                             double huber_delta, double* chi2);
/* PoseGraph::existEdge (:389-399): 1 if a == b or an edge joins them either way */
int32_t rgbd_pg_exist_edge(const rgbd_posegraph* g, int32_t a, int32_t b);
rgbd_status rgbd_pg_counts(const rgbd_posegraph* g, int32_t* vertices, int32_t* edges);
rgbd_status rgbd_pg_chi2(const rgbd_posegraph* g, double* chi2);
/* PoseGraph::optimize (:368-386): up to `iterations` LM iterations; the final robust chi2 */
rgbd_status rgbd_pg_optimize(rgbd_posegraph* g, int32_t iterations, double* chi2, int32_t* iterations_done);
rgbd_status rgbd_pg_vertex(const rgbd_posegraph* g, int32_t id, double* Twc);

/* ------------------------------------------------------------------ bag of words and the loop database */
/* DBoW3's vocabulary tree, transform and L1 score as the reference drives them (Frame::computeBoW, Core/Frame.cpp:243-249;
 * LoopDetector, PlaceRecognition/LoopDetector.cpp:22-84).  DBoW3 is absent: the operator is the definition in DESIGN.md
 * "Bag-of-words and loop detection definition", written from the reference's callers and recalled DBoW3 semantics;
 * parity with the library is unpinned.
 *
 * rgbd_voc_set uploads a tree of n_nodes nodes, node 0 the root: parent[i] (parent[0] ignored), descriptor[i] (32
 * bytes), weight[i], is_leaf[i], word_id[i] (read on leaves: 0 .. words - 1, once each).  The children of a node are
 * ordered by node id.  The vocabulary belongs to the context and is immutable until the next rgbd_voc_set /
 * rgbd_voc_clear.  RGBD_ERR_UNSUPPORTED before any copy: weighting / scoring other than TF_IDF / L1_NORM, desc_bytes
 * != 32, k outside [2, 32], L outside [1, 10], n_nodes >= 2^31, an inner node with 0 or more than k children (a leaf
 * root included), a node below level L, a weight that is not finite and >= 0.  A malformed tree: RGBD_ERR_ARG. */
enum { RGBD_VOC_TF_IDF = 0, RGBD_VOC_TF = 1, RGBD_VOC_IDF = 2, RGBD_VOC_BINARY = 3 };               /* DBoW3::WeightingType */
enum { RGBD_VOC_L1_NORM = 0, RGBD_VOC_L2_NORM = 1, RGBD_VOC_CHI_SQUARE = 2, RGBD_VOC_KL = 3,
       RGBD_VOC_BHATTACHARYYA = 4, RGBD_VOC_DOT_PRODUCT = 5 };                                      /* DBoW3::ScoringType */
rgbd_status rgbd_voc_set(rgbd_ctx* ctx, int32_t k, int32_t L, int32_t weighting, int32_t scoring, int32_t desc_bytes,
                         int64_t n_nodes, const int32_t* parent, const uint8_t* descriptor, const double* weight,
                         const uint8_t* is_leaf, const int32_t* word_id);
rgbd_status rgbd_voc_clear(rgbd_ctx* ctx);
/* Vocabulary::transform(features, BowVector, FeatureVector, levelsup) of n host descriptors (n x 32 bytes): the BoW
 * vector (bow_ids ascending, bow_vals, *n_words entries) and the feature vector as (fv_node, fv_idx) pairs ascending
 * (*n_fv entries); every output array holds n slots.  n > 4096: RGBD_ERR_UNSUPPORTED before any copy or launch; no
 * vocabulary or levelsup < 0: RGBD_ERR_ARG.  One k_bow_words and one k_bow_vector launch. */
rgbd_status rgbd_bow_transform(rgbd_ctx* ctx, const uint8_t* desc, int32_t n, int32_t levelsup, uint32_t* bow_ids,
                               double* bow_vals, int32_t* n_words, int32_t* fv_node, int32_t* fv_idx, int32_t* n_fv);
/* P frames in the same two launches: desc = the frames' descriptors one after the other (counts[p] rows each); frame
 * p's outputs start at its first descriptor's row, n_words[p] / n_fv[p] of them written. */
rgbd_status rgbd_bow_transform_batch(rgbd_ctx* ctx, int32_t P, const uint8_t* desc, const int32_t* counts, int32_t levelsup,
                                     uint32_t* bow_ids, double* bow_vals, int32_t* n_words, int32_t* fv_node,
                                     int32_t* fv_idx, int32_t* n_fv);
/* The same from the device descriptors of the last extraction (frame[p] in [0, B)): no descriptor crosses the host.
 * Frame p's outputs are the rgbd_max_keypoints slots from p * rgbd_max_keypoints. */
rgbd_status rgbd_bow_transform_frames(rgbd_ctx* ctx, int32_t P, const int32_t* frame, int32_t levelsup, uint32_t* bow_ids,
                                      double* bow_vals, int32_t* n_words, int32_t* fv_node, int32_t* fv_idx, int32_t* n_fv);
/* The descent alone: per descriptor the word id, its weight, the node id at level L - levelsup (0 when that level
 * is <= 0 or below the leaf) and the children taken (path: n x 10 bytes, 255 below the leaf). */
rgbd_status rgbd_debug_bow_words(rgbd_ctx* ctx, const uint8_t* desc, int32_t n, int32_t levelsup, int32_t* word,
                                 double* weight, int32_t* node, uint8_t* path);
/* L1Scoring::score(a, b) on the device; the argument order matters to the last bit.  Ids strictly ascending, at
 * most 4096 per vector. */
rgbd_status rgbd_bow_score(rgbd_ctx* ctx, const uint32_t* ids_a, const double* val_a, int32_t na, const uint32_t* ids_b,
                           const double* val_b, int32_t nb, double* score);
/* The keyframe database (LoopDetector::add's inverted file as the vectors themselves, device resident): add appends
 * one BoW vector, *entry = its index.  query scores one vector against every entry in one k_bow_score launch:
 * query_first != 0 is score(query, entry) (LoopDetector.cpp:70), 0 is score(entry, query) (:43); per entry the
 * score, the number of shared words and the smallest shared word id (-1: none).  *n_entries = the entry count; cap
 * below it: RGBD_ERR_CAPACITY.  An empty database launches nothing. */
rgbd_status rgbd_loopdb_add(rgbd_ctx* ctx, const uint32_t* ids, const double* vals, int32_t n, int32_t* entry);
rgbd_status rgbd_loopdb_query(rgbd_ctx* ctx, const uint32_t* ids, const double* vals, int32_t n, int32_t query_first,
                              int32_t cap, double* score, int32_t* n_shared, int32_t* min_shared, int32_t* n_entries);
rgbd_status rgbd_loopdb_clear(rgbd_ctx* ctx);
int32_t rgbd_loopdb_size(const rgbd_ctx* ctx);
/* LoopDetector::obtainCandidates' host rules (:48-83) over a query's arrays: the entries that share a word and are
 * not skipped (skip[e] != 0: the query itself and its connected keyframes), in the inverted file's order (smallest
 * shared word, then insertion), kept when score > min_score and abs(frame_id[e] - query_id) > interval; more than
 * five kept: std::sort by score descending and the first five.  out holds min(n, 5) entry indices. */
rgbd_status rgbd_loop_candidates(int32_t n, const double* score, const int32_t* n_shared, const int32_t* min_shared,
                                 const int32_t* frame_id, const uint8_t* skip, int32_t query_id, double min_score,
                                 int32_t interval, int32_t* out, int32_t* n_out);

/* ------------------------------------------------------------------ coloured occupancy map */
/* octomap::ColorOcTree as OctomapDrawer drives it (Drawer/OctomapDrawer.cpp:15-79; MapDrawer::drawOctomap,
 * Drawer/MapDrawer.cpp:48-71): every keyframe cloud is ray-cast into depth-16 voxels of `resolution` metres, each voxel
 * updated once per scan (occupied beats free), then coloured by the scan's points in cloud order.  octomap is absent: the
 * operator is the definition in DESIGN.md "Occupancy map definition", written from the reference's caller and recalled
 * octomap 1.9 semantics; parity with the library is unpinned.  Leaves only: no inner nodes, no pruning, no .ot file.
 *
 * The map is a device-resident open-addressing table of `capacity` voxels (a power of two) that belongs to the context
 * it was created on, runs on that context's stream, and must be destroyed before it.  RGBD_ERR_UNSUPPORTED before any
 * copy or launch: a null pointer, resolution <= 0 or not finite, a probability outside (0, 1), clamp_min >= clamp_max,
 * capacity < 64, above 2^30 or no power of two, more than 16384 points in a scan, a pose or origin that is not finite, a
 * maxrange that is NaN. */
typedef struct rgbd_occmap rgbd_occmap;
typedef struct {
    double resolution;                                  /* OctomapDrawer::reset: 0.08 */
    double prob_hit, prob_miss, clamp_min, clamp_max;   /* 0.9, 0.4, 0.001, 0.999; each becomes (float)log(p / (1 - p)) */
    int64_t capacity;                                   /* voxels the table holds */
} rgbd_occmap_params;
rgbd_status rgbd_occmap_create(rgbd_ctx* ctx, const rgbd_occmap_params* prm, rgbd_occmap** map);
void rgbd_occmap_destroy(rgbd_occmap* map);
rgbd_status rgbd_occmap_clear(rgbd_occmap* map);
rgbd_status rgbd_occmap_size(rgbd_occmap* map, int64_t* n);
/* insertPointCloud(cloud, origin, maxrange) + the colour fold of one scan: n rgbd_points in the camera frame (what
 * rgbd_keyframe_cloud* returns), Twc34 = the f32 [R' | Ow] (row-major 3x4) that takes them to the world on the device,
 * origin = the sensor's position, maxrange < 0 = none.  Points that are not finite, before or after the transform, are
 * skipped.  A scan whose voxels do not fit the table leaves the map exactly as it was: RGBD_ERR_CAPACITY. */
rgbd_status rgbd_occmap_insert(rgbd_occmap* map, const rgbd_point* pts, int32_t n, const float* Twc34, const float* origin,
                               double maxrange);
/* nscan scans queued without a host round trip between them: scan k's points are pts[k * cap ...], counts[k] of them
 * (rgbd_keyframe_cloud_batch's layout), its pose Twc34s[12 k ...] and origin origins[3 k ...].  The first scan that
 * does not fit and every scan after it are not applied: *applied = the scans applied, RGBD_ERR_CAPACITY when fewer than
 * nscan. */
rgbd_status rgbd_occmap_insert_batch(rgbd_occmap* map, const rgbd_point* pts, const int32_t* counts, int32_t cap, int32_t nscan,
                                     const float* Twc34s, const float* origins, double maxrange, int32_t* applied);
/* Every leaf with log-odds >= min_logodds (-INFINITY: all), ascending by (kx << 32) | (ky << 16) | kz: keys[3 i ...] =
 * (kx, ky, kz), logodds[i], rgb[3 i ...] = (r, g, b).  *n = the number of such leaves; above cap: RGBD_ERR_CAPACITY and
 * nothing written.  keys / logodds / rgb may be NULL with cap = 0 to count. */
rgbd_status rgbd_occmap_leaves(rgbd_occmap* map, float min_logodds, uint16_t* keys, float* logodds, uint8_t* rgb, int64_t cap,
                               int64_t* n);
/* Frame::updateSensor (Core/Frame.cpp:551-608), host only: from Tcw (row-major 4x4 f32) Rwc = Rcw^T and Ow = -Rcw^T tcw
 * (double sums, one rounding), R' = Eigen::Quaternionf(Rwc).toRotationMatrix() in f32; Twc34 = [R' | Ow], origin = Ow. */
rgbd_status rgbd_occmap_sensor_pose(const float* Tcw, float* Twc34, float* origin);

/* ------------------------------------------------------------------ measurement */
/* Per-kernel HIP-event timing on the context stream (off by default). */
rgbd_status rgbd_set_timing(rgbd_ctx* ctx, int32_t enable);
rgbd_status rgbd_reset_timing(rgbd_ctx* ctx);
/* Time only the launches of one kernel (e.g. "k_fast"); NULL times every kernel.  Each timed launch
 * costs an event pair on the stream, so a filter keeps the measured region close to the untimed one. */
rgbd_status rgbd_set_timing_filter(rgbd_ctx* ctx, const char* kernel);
int32_t rgbd_timing_count(const rgbd_ctx* ctx);
rgbd_status rgbd_timing_entry(rgbd_ctx* ctx, int32_t idx, const char** name, double* total_ms, int64_t* launches);
rgbd_status rgbd_synchronize(rgbd_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* RGBD_HIP_H */
