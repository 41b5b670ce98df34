"""rgbd-slam_amd -- MI355X (gfx950) RGB-D tracking front end, Python host binding.

ctypes binding of build/librgbd_hip.so (C ABI: include/rgbd_hip.h) plus thin classes
that mirror the reference's operator surfaces for this path:

  ORBextractor.detect_and_compute  <- Extractor::detectAndCompute  Features/Extractor.h:40
  Frame(bgr, depth, extractor)     <- Frame::Frame                 Core/Frame.cpp:34-73
  Matcher(nnratio).match(ref, cur) <- Matcher::match               Features/Matcher.cpp:106-139
  Context.projection_match(...)    <- Matcher::projectionMatch     Features/Matcher.cpp:35-104
  Context.pnp_solver(...)          <- PnPSolver::compute           Solver/PnPSolver.cpp:31-150
  Context.ransac_umeyama(...)      <- Ransac::compute              Solver/Ransac.cpp:46-181
  Context.bow_transform(desc)      <- Frame::computeBoW            Core/Frame.cpp:243-249
  Context.loopdb_add / loopdb_query, loop_candidates <- LoopDetector  PlaceRecognition/LoopDetector.cpp:22-84
  RansacSE3(...).compute(F1, F2, m) <- RansacSE3::compute          Solver/SolverSE3.cpp:23-133
  OccupancyMap(ctx).insert / insert_batch / leaves <- OctomapDrawer::insertCloud  Drawer/OctomapDrawer.cpp:38-79

The GPU library is mandatory: there is no CPU fallback.  Importing works without a GPU
(the library loads and exports its symbols); any compute call needs a HIP device and
raises RgbdError otherwise.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
# RGBD_HIP_LIB selects another in-tree build of the same library (e.g. build_prof/, the profiling variant)
LIB_PATH = os.environ.get("RGBD_HIP_LIB") or os.path.join(PKG_DIR, "build", "librgbd_hip.so")
HEADER = os.path.join(ROOT, "include", "rgbd_hip.h")

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])


POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"),
                        ("pad", "u1")])   # rgbd_point = pcl::PointXYZRGB payload


class RgbdError(RuntimeError):
    pass


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32)]


class Camera(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3",
                                         "depth_map_factor")]


class SvoParams(C.Structure):
    """rgbd_svo_params: Extractor(SVO, BRIEF, NORMAL), the reference's default (main.cpp:31)."""
    _fields_ = [("nfeatures", C.c_int32), ("nlevels", C.c_int32), ("cell_size", C.c_int32), ("threshold", C.c_int32),
                ("max_keypoints", C.c_int32)]


def svo_params(nfeatures=1000, nlevels=8, cell_size=5, threshold=20, max_keypoints=0) -> SvoParams:
    """setParameters(1000, ...) + SVOextractor(nlevels, 5, 20) (Features/Extractor.cpp:21, :162-165);
    max_keypoints 0 = nfeatures + 64 (retainBest's boundary ties beyond that raise RGBD_ERR_CAPACITY)."""
    return SvoParams(nfeatures, nlevels, cell_size, threshold, max_keypoints)


class AdaptiveParams(C.Structure):
    """rgbd_adaptive_params: Extractor(FAST, BRIEF, ADAPTIVE) (Features/Extractor.cpp:82-109)."""
    _fields_ = [("nfeatures", C.c_int32), ("min_features", C.c_int32), ("grid_rows", C.c_int32), ("grid_cols", C.c_int32),
                ("edge_threshold", C.c_int32), ("iterations", C.c_int32), ("cell_cap", C.c_int32), ("pad", C.c_int32),
                ("init_thresh", C.c_double), ("min_thresh", C.c_double), ("max_thresh", C.c_double),
                ("increase", C.c_double), ("decrease", C.c_double)]


def adaptive_params(nfeatures=1000, min_features=600, grid_rows=3, grid_cols=3, edge_threshold=31, iterations=5,
                    init_thresh=20.0, min_thresh=2.0, max_thresh=10000.0, increase=1.3, decrease=0.7,
                    cell_cap=0) -> AdaptiveParams:
    """The reference's values: setParameters(1000, ...), DetectorAdjuster(FAST, 20, 2, 10000, 1.3, 0.7), 600
    minimum features, 5 iterations, a 3 x 3 grid with edge threshold 31; cell_cap 0 = 8192 stored maxima
    per cell (a cell with more at the threshold it used raises RGBD_ERR_CAPACITY for that frame)."""
    return AdaptiveParams(nfeatures, min_features, grid_rows, grid_cols, edge_threshold, iterations, cell_cap, 0,
                          init_thresh, min_thresh, max_thresh, increase, decrease)


class GfttParams(C.Structure):
    """rgbd_gftt_params: Extractor(GFTT, BRIEF, NORMAL) (Features/Extractor.cpp:178-181)."""
    _fields_ = [("nfeatures", C.c_int32), ("cand_cap", C.c_int32), ("quality_level", C.c_double),
                ("min_distance", C.c_double)]


def gftt_params(nfeatures=1000, quality_level=0.01, min_distance=3.0, cand_cap=0) -> GfttParams:
    """The reference's values: GFTTDetector::create(nfeatures, 0.01, 3, ...); cand_cap 0 = 32768 stored
    candidates per frame (a frame with more raises RGBD_ERR_CAPACITY for that frame alone)."""
    return GfttParams(nfeatures, cand_cap, quality_level, min_distance)


class CvorbParams(C.Structure):
    """rgbd_cvorb_params: Extractor(ORB, ORB, NORMAL) (Features/Extractor.cpp:163-166, 216-218)."""
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("edge_threshold", C.c_int32), ("fast_threshold", C.c_int32), ("cand_cap", C.c_int32),
                ("max_keypoints", C.c_int32)]


def cvorb_params(nfeatures=1000, scale_factor=1.2, nlevels=8, edge_threshold=31, fast_threshold=20, cand_cap=0,
                 max_keypoints=0) -> CvorbParams:
    """cv::ORB::create(nfeatures, scaleFactor, nlevels)'s values.  cand_cap 0 = 8192 stored FAST corners per (frame,
    level), at most 12288; max_keypoints 0 = nfeatures + nfeatures / 4 (retainBest keeps ties).  A frame over
    either raises RGBD_ERR_CAPACITY for that frame alone."""
    return CvorbParams(nfeatures, scale_factor, nlevels, edge_threshold, fast_threshold, cand_cap, max_keypoints)


class FastParams(C.Structure):
    """rgbd_fast_params: Extractor(FAST, BRIEF | ORB, NORMAL) (Features/Extractor.cpp:168-171, 216-218, 224-226)."""
    _fields_ = [("nfeatures", C.c_int32), ("threshold", C.c_int32), ("descriptor", C.c_int32), ("cand_cap", C.c_int32),
                ("max_keypoints", C.c_int32)]


FAST_BRIEF, FAST_ORB = 0, 1


def fast_params(nfeatures=1000, threshold=10, descriptor="brief", cand_cap=0, max_keypoints=0) -> FastParams:
    """cv::FastFeatureDetector::create()'s values (threshold 10, nonmaxSuppression, TYPE_9_16).  descriptor "brief"
    (BriefDescriptorExtractor) or "orb" (cv::ORB::create()->compute()); cand_cap 0 = 32768 stored corners per frame,
    at most 65536; max_keypoints 0 = nfeatures + nfeatures / 4 (retainBest keeps ties).  A frame over either raises
    RGBD_ERR_CAPACITY for that frame alone."""
    d = {"brief": FAST_BRIEF, "orb": FAST_ORB}.get(descriptor, descriptor)
    return FastParams(nfeatures, threshold, int(d), cand_cap, max_keypoints)


class CloudParams(C.Structure):
    _fields_ = [("stride", C.c_int32), ("zmin", C.c_float), ("zmax", C.c_float), ("leaf", C.c_float),
                ("sor_k", C.c_int32), ("sor_std", C.c_double)]


def cloud_params(stride=6, zmin=0.5, zmax=4.0, leaf=0.04, sor_k=50, sor_std=1.0) -> CloudParams:
    """Tracking::createKeyFrame's values (System/Tracking.cpp:234-237)."""
    return CloudParams(stride, zmin, zmax, leaf, sor_k, sor_std)


class RansacParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("min_inlier_th", C.c_uint32), ("max_mahalanobis", C.c_float),
                ("sample_size", C.c_uint32)]


class Rng(C.Structure):
    _fields_ = [("state", C.c_int32 * 31), ("f", C.c_int32), ("r", C.c_int32)]


class Sticky(C.Structure):
    _fields_ = [("cov", C.c_double), ("set", C.c_int32), ("pad", C.c_int32)]


class TrackState(C.Structure):
    """rgbd_track_state: Tracking's state between chunks that overlap by two frames (zeroed = a new
    sequence).  Build it with track_state(), which also owns the two outlier-flag buffers."""
    _fields_ = [("kf_pose", C.c_float * 16), ("first_rel", C.c_float * 16), ("ref2_pose", C.c_float * 16),
                ("first_is_kf", C.c_int32), ("valid", C.c_int32), ("flags2", C.c_void_p), ("flags1", C.c_void_p),
                ("flags_cap", C.c_int32)]


def track_state(cap: int) -> TrackState:
    """A zeroed TrackState with caller-owned flag buffers of `cap` bytes, kept alive by the returned
    object; cap must be >= the context's keypoint capacity (Context.kp_cap; the library checks it and
    raises RGBD_ERR_CAPACITY otherwise).  Context.track_state() sizes it for the context."""
    cap = int(cap)
    if cap < 1:
        raise ValueError("track_state: cap must be >= 1 (use Context.track_state() or ctx.kp_cap)")
    ts = TrackState()
    ts._flag_buffers = (np.zeros(cap, np.uint8), np.zeros(cap, np.uint8))
    ts.flags2 = ts._flag_buffers[0].ctypes.data
    ts.flags1 = ts._flag_buffers[1].ctypes.data
    ts.flags_cap = cap
    return ts


class Bounds(C.Structure):
    """rgbd_bounds: Frame::computeImageBounds' mnMinX, mnMaxX, mnMinY, mnMaxY."""
    _fields_ = [(n, C.c_float) for n in ("min_x", "max_x", "min_y", "max_y")]


class PnpParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("reprojection_error", C.c_float), ("confidence", C.c_double),
                ("min_matches", C.c_int32), ("flag_segments", C.c_int32)]


class PnpSolverParams(C.Structure):
    """rgbd_pnp_solver_params: PnPSolver::compute's constants (Solver/PnPSolver.cpp:57, :102-132)."""
    _fields_ = [("rounds", C.c_int32), ("iterations", C.c_int32), ("chi2_threshold", C.c_double),
                ("robust_rounds", C.c_int32), ("min_edges", C.c_int32)]


class UmeyamaParams(C.Structure):
    """rgbd_umeyama_params: Ransac::parameters' fields that Ransac::compute reads (Solver/Ransac.h:21-29)."""
    _fields_ = [("error_version", C.c_int32), ("used_pairs", C.c_int32), ("min_matches", C.c_int32), ("pad", C.c_int32),
                ("thr_euclidean", C.c_double), ("min_inlier_ratio", C.c_double)]


class GicpParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("k_correspondences", C.c_int32), ("max_corr_dist", C.c_double),
                ("transformation_epsilon", C.c_double), ("rotation_epsilon", C.c_double),
                ("gicp_epsilon", C.c_double), ("gn_iterations", C.c_int32), ("enable", C.c_int32)]


class OccmapParams(C.Structure):
    """rgbd_occmap_params: OctomapDrawer::reset's values (Drawer/OctomapDrawer.cpp:15-25) and the table's capacity."""
    _fields_ = [("resolution", C.c_double), ("prob_hit", C.c_double), ("prob_miss", C.c_double),
                ("clamp_min", C.c_double), ("clamp_max", C.c_double), ("capacity", C.c_int64)]


_vp = C.c_void_p
_i32 = C.c_int32
_PI = C.POINTER(C.c_int32)
_SIGS = {
    "rgbd_create": (_i32, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(OrbParams), C.POINTER(Camera),
                           C.POINTER(_vp)]),
    "rgbd_create_svo": (_i32, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(SvoParams), C.POINTER(Camera),
                               C.POINTER(_vp)]),
    "rgbd_svo_set_brief_pattern": (_i32, [_vp, _vp]),
    "rgbd_svo_get_brief_pattern": (_i32, [_vp, _vp]),
    "rgbd_svo_debug_level": (_i32, [_vp, _i32, _i32, _vp]),
    "rgbd_svo_debug_grid": (_i32, [_vp, _i32, _vp, _vp, _i32, _PI]),
    "rgbd_svo_retain_best": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _PI]),
    "rgbd_create_adaptive": (_i32, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(AdaptiveParams), C.POINTER(Camera),
                                    C.POINTER(_vp)]),
    "rgbd_adaptive_get_thresholds": (_i32, [_vp, _vp]),
    "rgbd_adaptive_set_thresholds": (_i32, [_vp, _vp]),
    "rgbd_adaptive_rewind": (_i32, [_vp, _i32]),
    "rgbd_adaptive_debug_cell": (_i32, [_vp, _i32, _i32, C.POINTER(C.c_uint64), _PI, _PI, _vp, _i32, _PI]),
    "rgbd_adaptive_keep_strongest": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "rgbd_create_gftt": (_i32, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(GfttParams), C.POINTER(Camera),
                                C.POINTER(_vp)]),
    "rgbd_gftt_debug_eig": (_i32, [_vp, _i32, _vp]),
    "rgbd_gftt_debug_corners": (_i32, [_vp, _i32, C.POINTER(C.c_uint32), _PI, _vp, _vp, _i32, _PI]),
    "rgbd_gftt_debug_ranks": (_i32, [_vp, _i32, _PI]),
    "rgbd_gftt_select": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, C.c_double, _i32, _i32, _vp, _PI]),
    "rgbd_create_cvorb": (_i32, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(CvorbParams), C.POINTER(Camera),
                                 C.POINTER(_vp)]),
    "rgbd_cvorb_debug_level": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _i32, _PI]),
    "rgbd_create_fast": (_i32, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(FastParams), C.POINTER(Camera),
                                C.POINTER(_vp)]),
    "rgbd_fast_debug_corners": (_i32, [_vp, _i32, _PI, _vp, _i32, _PI]),
    "rgbd_fast_retain_best": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _PI]),
    "rgbd_destroy": (None, [_vp]),
    "rgbd_last_error": (C.c_char_p, [_vp]),
    "rgbd_max_keypoints": (_i32, [_vp]),
    "rgbd_set_stream": (_i32, [_vp, _vp]),
    "rgbd_detect_and_compute": (_i32, [_vp, _vp, _i32, _vp, _vp, _i32, _PI]),
    "rgbd_frame": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _PI]),
    "rgbd_extract_batch": (_i32, [_vp, _vp, _vp, _i32]),
    "rgbd_batch_frame": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _PI]),
    "rgbd_batch_outputs": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp),
                                  C.POINTER(_vp)]),
    "rgbd_debug_level": (_i32, [_vp, _i32, _i32, _vp]),
    "rgbd_debug_blurred": (_i32, [_vp, _i32, _i32, _vp]),
    "rgbd_debug_candidates": (_i32, [_vp, _i32, _i32, _vp, _i32, _PI]),
    "rgbd_debug_selected": (_i32, [_vp, _i32, _i32, _vp, _i32, _PI]),
    "rgbd_debug_dist_path": (_i32, [_vp, _i32, _i32, _PI]),
    "rgbd_knn2": (_i32, [_vp, _vp, _i32, _vp, _i32, _vp]),
    "rgbd_match": (_i32, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, C.c_float, _i32, _vp, _i32, _PI]),
    "rgbd_image_bounds": (_i32, [_vp, C.POINTER(Bounds)]),
    "rgbd_projection_match": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, C.POINTER(Bounds), C.c_float,
                                     _vp, _i32, _PI]),
    "rgbd_projection_match_batch": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, C.c_float, _vp, _vp]),
    "rgbd_debug_projection": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, C.POINTER(Bounds), C.c_float,
                                     _vp, _vp, _vp, _i32, _vp]),
    "rgbd_ransac_se3": (_i32, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, C.POINTER(RansacParams), C.POINTER(Rng),
                               C.POINTER(Sticky), _i32, _vp, _vp, _vp, _PI, C.POINTER(C.c_float), _PI]),
    "rgbd_rng_seed": (None, [C.POINTER(Rng), C.c_uint32]),
    "rgbd_track_batch": (_i32, [_vp, _vp, _vp, _i32, C.c_float, C.POINTER(RansacParams), C.POINTER(Rng),
                                C.POINTER(Sticky), _vp, _vp, _vp]),
    "rgbd_track_batch_kf": (_i32, [_vp, _vp, _vp, _i32, C.c_float, C.POINTER(RansacParams), C.POINTER(Rng),
                                   C.POINTER(Sticky), C.POINTER(TrackState), _vp, _vp, _vp, _vp, _vp]),
    "rgbd_track_lanes": (_i32, [_vp, _vp, _vp, _i32, C.c_float, C.POINTER(RansacParams), _i32, _vp, _vp, _vp, _vp, _vp,
                                _vp]),
    "rgbd_debug_sort_matches": (_i32, [_vp, _vp, _i32, _i32, _vp]),
    "rgbd_debug_fast_rank16": (_i32, [_vp, _vp, _i32, _vp, _vp]),
    "rgbd_debug_rotation_ops": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "rgbd_debug_gicp_cov": (_i32, [_vp, _vp, _i32, _i32, C.c_double, _vp]),
    "rgbd_pnp_ransac": (_i32, [_vp, _vp, _vp, _i32, _vp, C.POINTER(PnpParams), _vp, _vp, _vp, _PI, _PI, _PI]),
    "rgbd_pnp_ransac_batch": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, C.POINTER(PnpParams), _vp, _vp, _vp, _vp, _vp,
                                     _vp]),
    "rgbd_debug_pnp_chunks": (_i32, [_vp, _PI, _PI]),
    "rgbd_pnp_track_batch": (_i32, [_vp, _vp, _vp, _i32, C.c_float, C.POINTER(PnpParams), _vp, _vp, _vp, _vp]),
    "rgbd_pnp_track_submit": (_i32, [_vp, _vp, _vp, _i32, C.c_float, C.POINTER(PnpParams)]),
    "rgbd_pnp_track_collect": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "rgbd_pnp_solver": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, C.POINTER(PnpSolverParams), _vp, _vp, _PI, _PI]),
    "rgbd_pnp_solver_batch": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, C.POINTER(PnpSolverParams), _vp, _vp, _vp, _vp]),
    "rgbd_pnp_solver_frames": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, C.POINTER(PnpSolverParams), _vp, _vp, _vp,
                                      _vp]),
    "rgbd_debug_pnp_solver": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, C.POINTER(PnpSolverParams), _vp, _vp, _PI, _PI, _PI,
                                     _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rgbd_ransac_umeyama": (_i32, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, C.POINTER(UmeyamaParams), C.POINTER(Rng), _vp, _vp,
                                   _vp, _PI, _PI, _PI]),
    "rgbd_ransac_umeyama_batch": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(UmeyamaParams), _vp, _vp, _vp,
                                         _vp, _vp, _vp, _vp]),
    "rgbd_ransac_umeyama_frames": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, C.POINTER(UmeyamaParams), _vp, _vp, _vp, _vp, _vp,
                                          _vp, _vp]),
    "rgbd_debug_ransac_umeyama": (_i32, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, C.POINTER(UmeyamaParams), C.POINTER(Rng), _vp,
                                         _vp, _vp, _PI, _PI, _PI, _i32, _vp, _vp, _vp, _PI, _i32, _vp, _PI]),
    "rgbd_ransac_umeyama_pose": (None, [_vp, _vp, _vp]),
    "rgbd_voc_set": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "rgbd_voc_clear": (_i32, [_vp]),
    "rgbd_bow_transform": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _PI, _vp, _vp, _PI]),
    "rgbd_bow_transform_batch": (_i32, [_vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rgbd_bow_transform_frames": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rgbd_debug_bow_words": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "rgbd_bow_score": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _i32, C.POINTER(C.c_double)]),
    "rgbd_loopdb_add": (_i32, [_vp, _vp, _vp, _i32, _PI]),
    "rgbd_loopdb_query": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _PI]),
    "rgbd_loopdb_clear": (_i32, [_vp]),
    "rgbd_loopdb_size": (_i32, [_vp]),
    "rgbd_loop_candidates": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _i32, C.c_double, _i32, _vp, _PI]),
    "rgbd_gicp": (_i32, [_vp, _vp, _vp, _i32, _vp, C.POINTER(GicpParams), _vp, _PI, _PI]),
    "rgbd_gicp_compute": (_i32, [_vp, _vp, _vp, _i32, _vp, C.POINTER(GicpParams), _vp, _PI]),
    "rgbd_set_tracking_gicp": (_i32, [_vp, C.POINTER(GicpParams)]),
    "rgbd_set_timing": (_i32, [_vp, _i32]),
    "rgbd_reset_timing": (_i32, [_vp]),
    "rgbd_set_timing_filter": (_i32, [_vp, C.c_char_p]),
    "rgbd_timing_count": (_i32, [_vp]),
    "rgbd_timing_entry": (_i32, [_vp, _i32, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "rgbd_synchronize": (_i32, [_vp]),
    "rgbd_keyframe_cloud": (_i32, [_vp, _vp, _vp, C.POINTER(CloudParams), _vp, _i32, _PI]),
    "rgbd_keyframe_cloud_f32": (_i32, [_vp, _vp, _vp, C.POINTER(CloudParams), _vp, _i32, _PI]),
    "rgbd_keyframe_cloud_batch": (_i32, [_vp, _vp, _vp, _i32, _vp, _i32, C.POINTER(CloudParams), _vp, _i32, _vp]),
    "rgbd_occmap_create": (_i32, [_vp, C.POINTER(OccmapParams), C.POINTER(_vp)]),
    "rgbd_occmap_destroy": (None, [_vp]),
    "rgbd_occmap_clear": (_i32, [_vp]),
    "rgbd_occmap_size": (_i32, [_vp, C.POINTER(C.c_int64)]),
    "rgbd_occmap_insert": (_i32, [_vp, _vp, _i32, _vp, _vp, C.c_double]),
    "rgbd_occmap_insert_batch": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, C.c_double, _PI]),
    "rgbd_occmap_leaves": (_i32, [_vp, C.c_float, _vp, _vp, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    "rgbd_occmap_sensor_pose": (_i32, [_vp, _vp, _vp]),
    "rgbd_pg_create": (_i32, [C.POINTER(_vp)]),
    "rgbd_pg_destroy": (None, [_vp]),
    "rgbd_pg_add_vertex": (_i32, [_vp, _i32, _vp, _i32]),
    "rgbd_pg_set_fixed": (_i32, [_vp, _i32, _i32]),
    "rgbd_pg_add_edge": (_i32, [_vp, _i32, _i32, _vp, C.c_double, C.c_double, C.POINTER(C.c_double)]),
    "rgbd_pg_exist_edge": (_i32, [_vp, _i32, _i32]),
    "rgbd_pg_counts": (_i32, [_vp, _PI, _PI]),
    "rgbd_pg_chi2": (_i32, [_vp, C.POINTER(C.c_double)]),
    "rgbd_pg_optimize": (_i32, [_vp, _i32, C.POINTER(C.c_double), _PI]),
    "rgbd_pg_vertex": (_i32, [_vp, _i32, _vp]),
}

_lib = None


def build(force: bool = False) -> str:
    """Compile librgbd_hip.so for gfx950 in-tree (hipcc)."""
    args = ["make", "-s", "-C", PKG_DIR]
    if force:
        subprocess.run(args + ["clean"], check=True)
    subprocess.run(args, check=True)
    return LIB_PATH


def lib():
    """Load the HIP library; raises if it is missing (no CPU fallback exists)."""
    global _lib
    if _lib is None:
        # Bind to the same HIP runtime as torch (torch ships its own libamdhip64 with the same
        # SONAME); loading ours first would give the process two HIP runtimes.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        if not os.path.exists(LIB_PATH):
            raise RgbdError(f"{LIB_PATH} not built: run build() / __graft_entry__.build()")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def exported_symbols():
    return list(_SIGS)


def _ptr(a: np.ndarray):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def orb_params(nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th_fast=20, min_th_fast=7) -> OrbParams:
    """Extractor(ORB2, ORB2, NORMAL) + setParameters, Features/Extractor.cpp:15-48."""
    return OrbParams(nfeatures, scale_factor, nlevels, ini_th_fast, min_th_fast)


def camera(fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, factor=5000.0) -> Camera:
    """RGBDcamera(IntrinsicMatrix, ..., depthMapFactor=factor); mDepthMapFactor = 1/factor."""
    return Camera(fx, fy, cx, cy, k1, k2, p1, p2, k3, np.float32(1.0) / np.float32(factor))


def ransac_params(iters=200, min_inlier_th=10, max_mahalanobis=3.0, sample_size=4) -> RansacParams:
    return RansacParams(iters, min_inlier_th, max_mahalanobis, sample_size)


def pnp_params(iters=500, reproj=3.0, conf=0.85, min_matches=10, flag_segments=0) -> PnpParams:
    """PnPRansac::compute's solvePnPRansac arguments (Solver/PnPRansac.cpp:39) + its <10-match rule.
    flag_segments (rgbd_pnp_track_*): 0 = independent pairs (discardOutliers = false); S >= 1 = the
    reference's outlier-flag chain over S contiguous runs of pairs (1 = one chain)."""
    return PnpParams(iters, reproj, conf, min_matches, flag_segments)


def pnp_solver_params(rounds=4, iterations=10, chi2_threshold=5.991, robust_rounds=3, min_edges=10) -> PnpSolverParams:
    """PnPSolver::compute's schedule: 4 rounds of 10 LM iterations, chi2 5.991 (Huber delta = its root), the kernel
    removed after round index 2, fewer than 10 edges run one round (Solver/PnPSolver.cpp:57, :102-132)."""
    return PnpSolverParams(rounds, iterations, chi2_threshold, robust_rounds, min_edges)


EUCLIDEAN_ERROR, REPROJECTION_ERROR, EUCLIDEAN_AND_REPROJECTION_ERROR, MAHALANOBIS_ERROR, ADAPTIVE_ERROR = range(5)


def umeyama_params(error_version=EUCLIDEAN_ERROR, used_pairs=3, min_matches=10, thr=0.03,
                   min_inlier_ratio=0.1) -> UmeyamaParams:
    """Ransac::parameters (Solver/Ransac.h:21-29): errorVersion (Ransac::ERROR_VERSION), usedPairs,
    minimalNumberOfMatches, inlierThresholdEuclidean, minimalInlierRatioThreshold."""
    return UmeyamaParams(error_version, used_pairs, min_matches, 0, thr, min_inlier_ratio)


def gicp_params(max_iterations=10, max_corr=0.07, gn_iterations=4, enable=True) -> GicpParams:
    """Tracking's GICP settings (System/Tracking.cpp:147-151) over the Gicp ctor (Solver/Gicp.cpp:12-15)."""
    return GicpParams(max_iterations, 20, max_corr, 1e-9, 2e-3, 1e-3, gn_iterations, int(enable))


def occmap_params(resolution=0.08, prob_hit=0.9, prob_miss=0.4, clamp_min=0.001, clamp_max=0.999,
                  capacity=1 << 20) -> OccmapParams:
    """OctomapDrawer::reset (Drawer/OctomapDrawer.cpp:15-25); capacity = voxels the device table holds (a power of two)."""
    return OccmapParams(resolution, prob_hit, prob_miss, clamp_min, clamp_max, capacity)


def occmap_logodds(p: float) -> np.float32:
    """(float)log(p / (1 - p)) with the f64 libm log, as the library converts its probabilities."""
    import math
    return np.float32(math.log(p / (1.0 - p)))


def rng(seed: int) -> Rng:
    r = Rng()
    lib().rgbd_rng_seed(C.byref(r), seed)
    return r


def loop_candidates(score, n_shared, min_shared, frame_id, skip, query_id: int, min_score: float, interval: int = 10):
    """rgbd_loop_candidates: the entry indices LoopDetector::obtainCandidates returns, in its order (host only)."""
    score = np.ascontiguousarray(score, np.float64)
    ns, mw = np.ascontiguousarray(n_shared, np.int32), np.ascontiguousarray(min_shared, np.int32)
    fid, sk = np.ascontiguousarray(frame_id, np.int32), np.ascontiguousarray(skip, np.uint8)
    n = len(score)
    if not (len(ns) == len(mw) == len(fid) == len(sk) == n):
        raise ValueError("loop_candidates: array lengths differ")
    out, k = np.zeros(5, np.int32), C.c_int32(0)
    st = lib().rgbd_loop_candidates(n, _ptr(score), _ptr(ns), _ptr(mw), _ptr(fid), _ptr(sk), int(query_id), float(min_score),
                                    int(interval), _ptr(out), C.byref(k))
    if st != 0:
        raise RgbdError(f"loop_candidates: status {st}")
    return out[:k.value].copy()


class Context:
    """One extractor + camera + device workspace (rgbd_create)."""

    def __init__(self, width=640, height=480, max_batch=1, orb: OrbParams | None = None,
                 cam: Camera | None = None, device=0, svo: SvoParams | None = None,
                 adaptive: AdaptiveParams | None = None, gftt: GfttParams | None = None,
                 cvorb: CvorbParams | None = None, fast: FastParams | None = None):
        """svo: an Extractor(SVO, BRIEF, NORMAL) context (rgbd_create_svo) instead of the ORBextractor;
        adaptive: an Extractor(FAST, BRIEF, ADAPTIVE) context (rgbd_create_adaptive);
        gftt: an Extractor(GFTT, BRIEF, NORMAL) context (rgbd_create_gftt);
        cvorb: an Extractor(ORB, ORB, NORMAL) context, OpenCV's ORB (rgbd_create_cvorb);
        fast: an Extractor(FAST, BRIEF | ORB, NORMAL) context (rgbd_create_fast)."""
        if (svo is not None) + (adaptive is not None) + (gftt is not None) + (cvorb is not None) + (fast is not None) > 1:
            raise ValueError("Context: svo, adaptive, gftt, cvorb and fast are different extractors; give one")
        self.orb = orb or orb_params()
        self.cam = cam or camera(535.4, 539.2, 320.1, 247.6)
        self.svo = svo
        self.adaptive = adaptive
        self.gftt = gftt
        self.cvorb = cvorb
        self.fast = fast
        self.W, self.H = width, height
        h = C.c_void_p()
        if fast is not None:
            st = lib().rgbd_create_fast(device, width, height, max_batch, C.byref(fast), C.byref(self.cam), C.byref(h))
        elif cvorb is not None:
            st = lib().rgbd_create_cvorb(device, width, height, max_batch, C.byref(cvorb), C.byref(self.cam), C.byref(h))
        elif gftt is not None:
            st = lib().rgbd_create_gftt(device, width, height, max_batch, C.byref(gftt), C.byref(self.cam), C.byref(h))
        elif adaptive is not None:
            st = lib().rgbd_create_adaptive(device, width, height, max_batch, C.byref(adaptive), C.byref(self.cam),
                                            C.byref(h))
        elif svo is not None:
            st = lib().rgbd_create_svo(device, width, height, max_batch, C.byref(svo), C.byref(self.cam), C.byref(h))
        else:
            st = lib().rgbd_create(device, width, height, max_batch, C.byref(self.orb), C.byref(self.cam), C.byref(h))
        self._h = h
        if st != 0:
            msg = lib().rgbd_last_error(h).decode() if h.value else "rgbd_create failed"
            self.close()
            raise RgbdError(f"rgbd_create: {msg} (status {st})")
        self.kp_cap = lib().rgbd_max_keypoints(h)
        self._pending = []   # batch sizes of outstanding pnp_track_submit calls

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().rgbd_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st, what):
        if st != 0:
            raise RgbdError(f"{what}: {lib().rgbd_last_error(self._h).decode()} (status {st})")

    # --- extraction
    def detect_and_compute(self, gray: np.ndarray):
        gray = np.ascontiguousarray(gray, dtype=np.uint8)
        kps = np.zeros(self.kp_cap, KEYPOINT_DTYPE)
        desc = np.zeros((self.kp_cap, 32), np.uint8)
        n = C.c_int32(0)
        self._check(lib().rgbd_detect_and_compute(self._h, _ptr(gray), gray.strides[0], _ptr(kps), _ptr(desc),
                                                  self.kp_cap, C.byref(n)), "detect_and_compute")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def frame(self, bgr: np.ndarray, depth: np.ndarray):
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
        K = self.kp_cap
        kps, kun = np.zeros(K, KEYPOINT_DTYPE), np.zeros(K, KEYPOINT_DTYPE)
        desc, xyz = np.zeros((K, 32), np.uint8), np.zeros((K, 3), np.float32)
        n = C.c_int32(0)
        self._check(lib().rgbd_frame(self._h, _ptr(bgr), _ptr(depth), _ptr(kps), _ptr(kun), _ptr(desc), _ptr(xyz),
                                     K, C.byref(n)), "frame")
        m = n.value
        return dict(kps=kps[:m].copy(), kps_un=kun[:m].copy(), desc=desc[:m].copy(), xyz=xyz[:m].copy())

    def extract_batch(self, d_bgr: int, d_depth: int, B: int):
        self._check(lib().rgbd_extract_batch(self._h, C.c_void_p(d_bgr), C.c_void_p(d_depth), B), "extract_batch")

    def batch_frame(self, b: int):
        K = self.kp_cap
        kps, kun = np.zeros(K, KEYPOINT_DTYPE), np.zeros(K, KEYPOINT_DTYPE)
        desc, xyz = np.zeros((K, 32), np.uint8), np.zeros((K, 3), np.float32)
        n = C.c_int32(0)
        self._check(lib().rgbd_batch_frame(self._h, b, _ptr(kps), _ptr(kun), _ptr(desc), _ptr(xyz), K,
                                           C.byref(n)), "batch_frame")
        m = n.value
        return dict(kps=kps[:m].copy(), kps_un=kun[:m].copy(), desc=desc[:m].copy(), xyz=xyz[:m].copy())

    # --- adaptive FAST + BRIEF (rgbd_create_adaptive contexts)
    @property
    def adaptive_cells(self) -> int:
        return self.adaptive.grid_rows * self.adaptive.grid_cols if self.adaptive is not None else 0

    def adaptive_thresholds(self) -> np.ndarray:
        """The cells' thresholds (f64, row-major) the next extraction starts from."""
        out = np.zeros(max(self.adaptive_cells, 1), np.float64)
        self._check(lib().rgbd_adaptive_get_thresholds(self._h, _ptr(out)), "adaptive_thresholds")
        return out[:self.adaptive_cells].copy()

    def set_adaptive_thresholds(self, thresh: np.ndarray):
        thresh = np.ascontiguousarray(thresh, dtype=np.float64).reshape(-1)
        if len(thresh) != self.adaptive_cells:
            raise ValueError(f"set_adaptive_thresholds: {self.adaptive_cells} thresholds, one per cell")
        self._check(lib().rgbd_adaptive_set_thresholds(self._h, _ptr(thresh)), "set_adaptive_thresholds")

    def adaptive_rewind(self, k: int):
        """The next extraction starts from the thresholds before frame last_B - k of the last batch (a copy on
        the device, queued on the context's stream): for batches that overlap by k frames."""
        self._check(lib().rgbd_adaptive_rewind(self._h, int(k)), "adaptive_rewind")

    def adaptive_debug_cell(self, b: int, cell: int, cap=12288):
        """(threshold before as f64, threshold used, tries, corners (x, y, score) of the last try in raster
        order, ROI coordinates) of one cell of frame b of the last batch."""
        bits, used, tries, n = C.c_uint64(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        xys = np.zeros((cap, 3), np.int32)
        self._check(lib().rgbd_adaptive_debug_cell(self._h, b, cell, C.byref(bits), C.byref(used), C.byref(tries),
                                                   _ptr(xys), cap, C.byref(n)), "adaptive_debug_cell")
        before = float(np.array([bits.value], np.uint64).view(np.float64)[0])
        return before, used.value, tries.value, xys[:n.value].copy()

    def adaptive_keep_strongest(self, resp: np.ndarray, N: int, depth_limit: int = -1) -> np.ndarray:
        resp = np.ascontiguousarray(resp, dtype=np.float32)
        order = np.zeros(max(len(resp), 1), np.int32)
        self._check(lib().rgbd_adaptive_keep_strongest(self._h, _ptr(resp), len(resp), N, depth_limit, _ptr(order)),
                    "adaptive_keep_strongest")
        return order[:min(len(resp), N)].copy()

    # --- Shi-Tomasi GFTT + BRIEF (rgbd_create_gftt contexts)
    def gftt_debug_eig(self, b: int) -> np.ndarray:
        """The raw minimum-eigenvalue map e [H, W] f32 of frame b of the last batch."""
        out = np.zeros((self.H, self.W), np.float32)
        self._check(lib().rgbd_gftt_debug_eig(self._h, b, _ptr(out)), "gftt_debug_eig")
        return out

    def gftt_debug_corners(self, b: int):
        """Frame b of the last batch: dict(M = max e (f32), n_candidates, corners [m, 2] int32 (x, y) in
        acceptance order before BRIEF's border filter, vals [m] f32, ranks = ranks the greedy consumed)."""
        cap = self.gftt.nfeatures if self.gftt is not None else 1
        bits, nc, n, rk = C.c_uint32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        xy = np.zeros((cap, 2), np.int32)
        val = np.zeros(cap, np.float32)
        self._check(lib().rgbd_gftt_debug_corners(self._h, b, C.byref(bits), C.byref(nc), _ptr(xy), _ptr(val), cap,
                                                  C.byref(n)), "gftt_debug_corners")
        self._check(lib().rgbd_gftt_debug_ranks(self._h, b, C.byref(rk)), "gftt_debug_ranks")
        M = np.array([bits.value], np.uint32).view(np.float32)[0]
        return dict(M=M, n_candidates=nc.value, corners=xy[:n.value].copy(), vals=val[:n.value].copy(), ranks=rk.value)

    def gftt_select(self, xy: np.ndarray, val: np.ndarray, W: int, H: int, min_distance: float, max_corners: int,
                    chunk: int = 0) -> np.ndarray:
        """The device's rank + spacing stage on a host list of distinct points: the accepted points' indices in
        acceptance order.  chunk = ranks per pass (0: the default for max_corners)."""
        xy = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
        val = np.ascontiguousarray(val, dtype=np.float32).reshape(-1)
        if len(xy) != len(val):
            raise ValueError("gftt_select: one value per point")
        out = np.zeros(max(min(len(xy), max_corners), 1), np.int32)
        m = C.c_int32(0)
        self._check(lib().rgbd_gftt_select(self._h, _ptr(xy), _ptr(val), len(xy), W, H, float(min_distance), max_corners,
                                           chunk, _ptr(out), C.byref(m)), "gftt_select")
        return out[:m.value].copy()

    # --- OpenCV ORB (rgbd_create_cvorb contexts)
    def cvorb_debug_level(self, b: int, level: int):
        """One level of frame b of the last batch: dict(n_fast = FAST corners after the border filter (it counts past
        cand_cap), s1 [n1, 3] int32 (x, y, score) after retainBest(2 N) in its order, h1 [n1] f32 their Harris
        responses, s2 [n2, 3] / h2 [n2] after retainBest(N))."""
        cap = (self.cvorb.cand_cap or 8192) if self.cvorb is not None else 1
        n = C.c_int32(0)
        out = {}
        self._check(lib().rgbd_cvorb_debug_level(self._h, b, level, 0, None, None, 0, C.byref(n)), "cvorb_debug_level")
        out["n_fast"] = n.value
        xys = np.zeros((cap, 3), np.int32)
        hr = np.zeros(cap, np.float32)
        self._check(lib().rgbd_cvorb_debug_level(self._h, b, level, 1, _ptr(xys), None, cap, C.byref(n)), "cvorb_debug_level")
        out["s1"] = xys[:n.value].copy()
        self._check(lib().rgbd_cvorb_debug_level(self._h, b, level, 2, None, _ptr(hr), cap, C.byref(n)), "cvorb_debug_level")
        out["h1"] = hr[:n.value].copy()
        self._check(lib().rgbd_cvorb_debug_level(self._h, b, level, 3, _ptr(xys), _ptr(hr), cap, C.byref(n)), "cvorb_debug_level")
        out["s2"], out["h2"] = xys[:n.value].copy(), hr[:n.value].copy()
        return out

    # --- plain FAST (rgbd_create_fast contexts)
    def fast_debug_corners(self, b: int):
        """Frame b of the last batch: (the corners cv::FAST found, counted past cand_cap; the stored ones [m, 3] int32
        (x, y, score) in raster order, before retainBest)."""
        nc, n = C.c_int32(0), C.c_int32(0)
        self._check(lib().rgbd_fast_debug_corners(self._h, b, C.byref(nc), None, 0, C.byref(n)), "fast_debug_corners")
        xys = np.zeros((max(n.value, 1), 3), np.int32)
        self._check(lib().rgbd_fast_debug_corners(self._h, b, C.byref(nc), _ptr(xys), len(xys), C.byref(n)), "fast_debug_corners")
        return nc.value, xys[:n.value].copy()

    def fast_retain_best(self, resp: np.ndarray, n_points: int, depth_limit: int = -1) -> np.ndarray:
        """The device retainBest(n_points) of k_fast_select on up to 65536 responses: the kept original indices in order."""
        resp = np.ascontiguousarray(resp, dtype=np.float32)
        order = np.zeros(max(len(resp), 1), np.int32)
        m = C.c_int32(0)
        self._check(lib().rgbd_fast_retain_best(self._h, _ptr(resp), len(resp), n_points, depth_limit, _ptr(order), C.byref(m)),
                    "fast_retain_best")
        return order[:m.value].copy()

    # --- SVO + BRIEF (rgbd_create_svo contexts; the BRIEF table also on adaptive, GFTT and (FAST, BRIEF) contexts)
    def set_brief_pattern(self, pairs: np.ndarray):
        pairs = np.ascontiguousarray(pairs, dtype=np.int8).reshape(256, 4)
        self._check(lib().rgbd_svo_set_brief_pattern(self._h, _ptr(pairs)), "set_brief_pattern")

    def brief_pattern(self) -> np.ndarray:
        out = np.zeros((256, 4), np.int8)
        self._check(lib().rgbd_svo_get_brief_pattern(self._h, _ptr(out)), "brief_pattern")
        return out

    def svo_debug_level(self, b: int, level: int):
        w, h = self.W, self.H
        for _ in range(level):   # halfSample: floor halving per level
            w, h = w // 2, h // 2
        out = np.zeros((h, w), np.uint8)
        self._check(lib().rgbd_svo_debug_level(self._h, b, level, _ptr(out)), "svo_debug_level")
        return out

    def svo_debug_grid(self, b: int, cap=16384):
        xyl = np.zeros((cap, 3), np.int32)
        resp = np.zeros(cap, np.float32)
        n = C.c_int32(0)
        self._check(lib().rgbd_svo_debug_grid(self._h, b, _ptr(xyl), _ptr(resp), cap, C.byref(n)), "svo_debug_grid")
        return xyl[:n.value].copy(), resp[:n.value].copy()

    def svo_retain_best(self, resp: np.ndarray, n_points: int, depth_limit: int = -1) -> np.ndarray:
        resp = np.ascontiguousarray(resp, dtype=np.float32)
        order = np.zeros(max(len(resp), 1), np.int32)
        m = C.c_int32(0)
        self._check(lib().rgbd_svo_retain_best(self._h, _ptr(resp), len(resp), n_points, depth_limit, _ptr(order),
                                                               C.byref(m)),
                    "svo_retain_best")
        return order[:m.value].copy()

    def debug_level(self, b: int, level: int, w: int, h: int):
        out = np.zeros((h, w), np.uint8)
        self._check(lib().rgbd_debug_level(self._h, b, level, _ptr(out)), "debug_level")
        return out

    def debug_blurred(self, b: int, level: int, w: int, h: int):
        out = np.zeros((h, w), np.uint8)
        self._check(lib().rgbd_debug_blurred(self._h, b, level, _ptr(out)), "debug_blurred")
        return out

    def debug_candidates(self, b: int, level: int, cap=200000):
        out = np.zeros((cap, 3), np.int32)
        n = C.c_int32(0)
        self._check(lib().rgbd_debug_candidates(self._h, b, level, _ptr(out), cap, C.byref(n)), "debug_candidates")
        return out[:n.value].copy()

    def debug_selected(self, b: int, level: int, cap=8192):
        out = np.zeros((cap, 3), np.int32)
        n = C.c_int32(0)
        self._check(lib().rgbd_debug_selected(self._h, b, level, _ptr(out), cap, C.byref(n)), "debug_selected")
        return out[:n.value].copy()

    def debug_dist_path(self, b: int, level: int) -> int:
        """0 per-key state, 1 pyramid path, 2 pyramid path abandoned, 3 pyramid path skipped (rgbd_hip.h)."""
        v = C.c_int32(-1)
        self._check(lib().rgbd_debug_dist_path(self._h, b, level, C.byref(v)), "debug_dist_path")
        return v.value

    # --- matching
    def knn2(self, dq: np.ndarray, dt: np.ndarray):
        dq = np.ascontiguousarray(dq, np.uint8)
        dt = np.ascontiguousarray(dt, np.uint8)
        out = np.zeros((max(len(dq), 1), 4), np.int32)
        self._check(lib().rgbd_knn2(self._h, _ptr(dq), len(dq), _ptr(dt), len(dt), _ptr(out)), "knn2")
        return out[:len(dq)]

    def match(self, dq, dt, outlier_q, zq, zt, nnratio=0.9, discard_outliers=True):
        dq = np.ascontiguousarray(dq, np.uint8)
        dt = np.ascontiguousarray(dt, np.uint8)
        outlier_q = np.ascontiguousarray(outlier_q, np.uint8)
        zq = np.ascontiguousarray(zq, np.float32)
        zt = np.ascontiguousarray(zt, np.float32)
        out = np.zeros(max(len(dq), 1), DMATCH_DTYPE)
        m = C.c_int32(0)
        self._check(lib().rgbd_match(self._h, _ptr(dq), len(dq), _ptr(dt), len(dt), _ptr(outlier_q), _ptr(zq),
                                     _ptr(zt), nnratio, int(discard_outliers), _ptr(out), len(out), C.byref(m)),
                    "match")
        return out[:m.value].copy()

    # --- projection-guided matching (Matcher::projectionMatch, Features/Matcher.cpp:35-104)
    def image_bounds(self) -> Bounds:
        """Frame::computeImageBounds (Core/Frame.cpp:283-315) for this context's camera and image size."""
        b = Bounds()
        self._check(lib().rgbd_image_bounds(self._h, C.byref(b)), "image_bounds")
        return b

    @staticmethod
    def _projection_args(xyz1, desc1, outlier1, Tcw1, kps_un2, xyz2, desc2, Tcw2, bounds):
        xyz1 = np.ascontiguousarray(xyz1, np.float32).reshape(-1, 3)
        desc1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32)
        kun2 = np.ascontiguousarray(kps_un2, KEYPOINT_DTYPE)
        xyz2 = np.ascontiguousarray(xyz2, np.float32).reshape(-1, 3)
        desc2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
        if len(desc1) != len(xyz1) or len(xyz2) != len(kun2) or len(desc2) != len(kun2):
            raise ValueError("projection match: xyz / desc / keypoint lengths differ")
        if outlier1 is not None:
            outlier1 = np.ascontiguousarray(outlier1, np.uint8)
            if len(outlier1) != len(xyz1):
                raise ValueError("projection match: outlier1 length")
        T1 = np.ascontiguousarray(Tcw1, np.float32).reshape(16)
        T2 = np.ascontiguousarray(Tcw2, np.float32).reshape(16)
        if bounds is not None and not isinstance(bounds, Bounds):
            bounds = Bounds(*[float(v) for v in bounds])
        keep = (xyz1, desc1, outlier1, T1, kun2, xyz2, desc2, T2, bounds)
        args = [_ptr(xyz1), _ptr(desc1), _ptr(outlier1) if outlier1 is not None else None, len(xyz1), _ptr(T1), _ptr(kun2),
                _ptr(xyz2), _ptr(desc2), len(kun2), _ptr(T2), C.byref(bounds) if bounds is not None else None]
        return args, keep

    def projection_match(self, xyz1, desc1, outlier1, Tcw1, kps_un2, xyz2, desc2, Tcw2, th=5.0, bounds=None, cap=None):
        """Matcher::projectionMatch(F1, F2, matches, th) (rgbd_projection_match): F1 = (mvKeys3Dc, descriptors,
        mvbOutlier or None, Tcw), F2 = (mvKeysUn, mvKeys3Dc, descriptors, Tcw); bounds None = image_bounds().
        Matches in query order as DMATCH_DTYPE (imgIdx -1)."""
        args, keep = self._projection_args(xyz1, desc1, outlier1, Tcw1, kps_un2, xyz2, desc2, Tcw2, bounds)
        cap = len(keep[0]) if cap is None else int(cap)
        out = np.zeros(max(cap, 1), DMATCH_DTYPE)
        m = C.c_int32(0)
        self._check(lib().rgbd_projection_match(self._h, *args, float(th), _ptr(out), cap, C.byref(m)), "projection_match")
        return out[:m.value].copy()

    def projection_match_batch(self, qframe, tframe, poses, th=5.0, outlier=None):
        """rgbd_projection_match_batch over the frames of the last extract_batch: pairs (qframe[p], tframe[p])
        (qframe < 0 skips a pair), poses (B, 4, 4) Tcw, outlier (B, kp_cap) u8 or None.  A list of P match arrays."""
        qf = np.ascontiguousarray(qframe, np.int32)
        tf = np.ascontiguousarray(tframe, np.int32)
        if len(qf) != len(tf):
            raise ValueError("projection_match_batch: qframe and tframe lengths differ")
        P, K = len(qf), self.kp_cap
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
        if outlier is not None:
            outlier = np.ascontiguousarray(outlier, np.uint8)
            if outlier.shape != (len(poses), K):
                raise ValueError("projection_match_batch: outlier must be (B, kp_cap)")
        out = np.zeros((max(P, 1), K), DMATCH_DTYPE)
        counts = np.zeros(max(P, 1), np.int32)
        self._check(lib().rgbd_projection_match_batch(self._h, P, _ptr(qf), _ptr(tf), _ptr(poses),
                                                      _ptr(outlier) if outlier is not None else None, float(th),
                                                      _ptr(out), _ptr(counts)), "projection_match_batch")
        return [out[p, :counts[p]].copy() for p in range(P)]

    def debug_projection(self, xyz1, desc1, outlier1, Tcw1, kps_un2, xyz2, desc2, Tcw2, th=5.0, bounds=None, cand_cap=64):
        """The geometry of projection_match on its own (rgbd_debug_projection): dict(uv_bits (n1, 2) u32,
        status (n1,), cand = list of candidate index arrays in visiting order before the z and taken filters,
        cand_count (n1,))."""
        args, keep = self._projection_args(xyz1, desc1, outlier1, Tcw1, kps_un2, xyz2, desc2, Tcw2, bounds)
        n1 = len(keep[0])
        uv = np.zeros((max(n1, 1), 2), np.uint32)
        status = np.zeros(max(n1, 1), np.int32)
        cand = np.zeros((max(n1, 1), max(cand_cap, 1)), np.int32)
        cnt = np.zeros(max(n1, 1), np.int32)
        self._check(lib().rgbd_debug_projection(self._h, *args, float(th), _ptr(uv), _ptr(status), _ptr(cand), int(cand_cap),
                                                _ptr(cnt)), "debug_projection")
        return dict(uv_bits=uv[:n1].copy(), status=status[:n1].copy(), cand_count=cnt[:n1].copy(),
                    cand=[cand[i, :min(cnt[i], cand_cap)].copy() for i in range(n1)])

    # --- solvers
    def ransac_se3(self, xyz1, xyz2, matches, prm: RansacParams, r: Rng, st: Sticky, flags2=None):
        xyz1 = np.ascontiguousarray(xyz1, np.float32)
        xyz2 = np.ascontiguousarray(xyz2, np.float32)
        matches = np.ascontiguousarray(matches, DMATCH_DTYPE)
        m = len(matches)
        T = np.zeros(16, np.float32)
        inl = np.zeros(max(m, 1), DMATCH_DTYPE)
        n_in, ok = C.c_int32(0), C.c_int32(0)
        rm = C.c_float(0)
        self._check(lib().rgbd_ransac_se3(self._h, _ptr(xyz1), len(xyz1), _ptr(xyz2), len(xyz2),
                                          _ptr(matches) if m else None, m, C.byref(prm), C.byref(r), C.byref(st),
                                          int(flags2 is not None), _ptr(flags2) if flags2 is not None else None,
                                          _ptr(T), _ptr(inl), C.byref(n_in), C.byref(rm), C.byref(ok)), "ransac_se3")
        return bool(ok.value), T.reshape(4, 4), inl[:n_in.value].copy(), float(rm.value)

    def track_batch(self, d_bgr: int, d_depth: int, B: int, nnratio: float, prm: RansacParams, r: Rng,
                    st: Sticky, pose0=None):
        poses = np.zeros((B, 16), np.float32)
        poses[0] = (np.eye(4, dtype=np.float32) if pose0 is None else np.asarray(pose0, np.float32)).reshape(16)
        status = np.zeros(B, np.int32)
        ninl = np.zeros(B, np.int32)
        self._check(lib().rgbd_track_batch(self._h, C.c_void_p(d_bgr), C.c_void_p(d_depth), B, nnratio,
                                           C.byref(prm), C.byref(r), C.byref(st), _ptr(poses), _ptr(status),
                                           _ptr(ninl)), "track_batch")
        return poses.reshape(B, 4, 4), status, ninl

    def track_batch_kf(self, d_bgr: int, d_depth: int, B: int, nnratio: float, prm: RansacParams, r: Rng,
                       st: Sticky, ts: TrackState, pose0=None):
        """Tracking::track over a chunk (rgbd_track_batch_kf): poses (track()'s returns), status, inliers,
        relative poses (mRelativeFramePoses) and keyframe flags; ts carries the state on.  A continuing
        chunk (ts.valid) starts with the previous chunk's last two frames: pose0 is then the pose of
        its frame 1 (the previous chunk's last output), and rows 0-1 of the outputs are not tracked."""
        poses = np.zeros((B, 16), np.float32)
        p0 = (np.eye(4, dtype=np.float32) if pose0 is None else np.asarray(pose0, np.float32)).reshape(16)
        if ts.valid:
            poses[1] = p0
        else:
            poses[0] = p0
        status = np.zeros(B, np.int32)
        ninl = np.zeros(B, np.int32)
        rel = np.zeros((B, 16), np.float32)
        kf = np.zeros(B, np.int32)
        self._check(lib().rgbd_track_batch_kf(self._h, C.c_void_p(d_bgr), C.c_void_p(d_depth), B, nnratio,
                                              C.byref(prm), C.byref(r), C.byref(st), C.byref(ts), _ptr(poses),
                                              _ptr(status), _ptr(ninl), _ptr(rel), _ptr(kf)), "track_batch_kf")
        return poses.reshape(B, 4, 4), status, ninl, rel.reshape(B, 4, 4), kf

    def track_state(self) -> TrackState:
        """A zeroed TrackState whose flag buffers fit this context (kp_cap bytes each)."""
        return track_state(self.kp_cap)

    def track_lanes(self, d_bgr: int, d_depth: int, B: int, nnratio: float, prm: RansacParams, L: int, rngs, stickies,
                    pose0=None, lane_first=None):
        """rgbd_track_lanes: the RansacSE3 chain over L lanes of one batch, all advanced together on the
        device.  lane_first (L + 1 frame indices; default: rgbd-slam_amd/dist.py's shard_range split) ->
        per-lane chains, stitched into one trajectory like the multi-GPU chunks.  Returns (poses [B, 4, 4]
        stitched, status [B], n_inliers [B], lane-major raw poses [(B + L - 1), 4, 4])."""
        from .dist import stitch
        if lane_first is None:
            base, rem = divmod(B, L)
            st = [l * base + min(l, rem) for l in range(L + 1)]
            lane_first = [0] + [st[l] - 1 for l in range(1, L)] + [B - 1]
        lf = np.ascontiguousarray(lane_first, np.int32)
        if len(rngs) != L or len(stickies) != L or len(lf) != L + 1:
            raise ValueError("track_lanes: L rngs, L stickies and L + 1 lane_first entries")
        R = (Rng * L)(*rngs)
        S = (Sticky * L)(*stickies)
        n = B + L - 1
        poses = np.zeros((n, 16), np.float32)
        for l in range(L):
            poses[lf[l] + l] = np.eye(4, dtype=np.float32).reshape(16)
        if pose0 is not None:
            poses[0] = np.asarray(pose0, np.float32).reshape(16)
        status, ninl = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._check(lib().rgbd_track_lanes(self._h, C.c_void_p(d_bgr), C.c_void_p(d_depth), B, nnratio, C.byref(prm), L,
                                           _ptr(lf), C.cast(R, C.c_void_p), C.cast(S, C.c_void_p), _ptr(poses),
                                           _ptr(status), _ptr(ninl)), "track_lanes")
        for l in range(L):   # the caller's objects carry the lanes' RNG / sticky state on
            C.memmove(C.byref(rngs[l]), C.byref(R[l]), C.sizeof(Rng))
            C.memmove(C.byref(stickies[l]), C.byref(S[l]), C.sizeof(Sticky))
        raw = poses.reshape(n, 4, 4)
        chunks = [raw[lf[l] + l:lf[l + 1] + l + 1] for l in range(L)]
        st_all = np.concatenate([status[lf[0]:lf[1] + 1]] + [status[lf[l] + l + 1:lf[l + 1] + l + 1] for l in range(1, L)])
        ni_all = np.concatenate([ninl[lf[0]:lf[1] + 1]] + [ninl[lf[l] + l + 1:lf[l + 1] + l + 1] for l in range(1, L)])
        p0 = raw[0] if pose0 is not None else np.eye(4, dtype=np.float32)
        return stitch(chunks, p0), st_all, ni_all, raw

    def debug_sort_matches(self, dist, depth_limit: int = -1) -> np.ndarray:
        """The device's std::sort(vUsedMatches) order of integer distances (rgbd_debug_sort_matches)."""
        d = np.ascontiguousarray(dist, np.float32)
        order = np.zeros(max(len(d), 1), np.int32)
        self._check(lib().rgbd_debug_sort_matches(self._h, _ptr(d), len(d), int(depth_limit), _ptr(order)),
                    "debug_sort_matches")
        return order[:len(d)].copy()

    def debug_fast_rank16(self, flags):
        """k_fast's 16-lane emission rank on its own (rgbd_debug_fast_rank16): flags (rows, 64) 0/1 ->
        (slots (rows, 64) with 0xffffffff where clear, counts (64,)); row r of a 16-lane cell starts at 1000 r."""
        f = np.ascontiguousarray(flags, np.uint8)
        rows = f.shape[0]
        slots = np.zeros((rows, 64), np.uint32)
        counts = np.zeros(64, np.uint32)
        self._check(lib().rgbd_debug_fast_rank16(self._h, _ptr(f), rows, _ptr(slots), _ptr(counts)), "debug_fast_rank16")
        return slots, counts

    def debug_rotation_ops(self, x, num, den, theta):
        """The Jacobi rotations' short sqrt / division sequences on their own (rgbd_debug_rotation_ops):
        (sqrt(x), num / den, sign(theta) / (|theta| + sqrt(theta^2 + 1))) as computed on the device, x >= 1 finite,
        |den| in [1, 2^1000), num / den normal, |num| >= 2^-969 unless den == 1 (include/rgbd_hip.h)."""
        arrs = [np.ascontiguousarray(a, np.float64) for a in (x, num, den, theta)]
        n = len(arrs[0])
        assert n >= 1 and all(len(a) == n for a in arrs)
        sq, q, t = np.zeros(n), np.zeros(n), np.zeros(n)
        self._check(lib().rgbd_debug_rotation_ops(self._h, *[_ptr(a) for a in arrs], n, _ptr(sq), _ptr(q), _ptr(t)),
                    "debug_rotation_ops")
        return sq, q, t

    # --- motion-only bundle adjustment (PnPSolver::compute, Solver/PnPSolver.cpp:31-150)
    @staticmethod
    def _pnp_solver_edges(Xw, obs, K4, Tcw_in):
        Xw = np.ascontiguousarray(Xw, np.float32).reshape(-1, 3)
        obs = np.ascontiguousarray(obs, np.float32).reshape(-1, 2)
        if len(Xw) != len(obs):
            raise ValueError("pnp_solver: Xw and obs lengths differ")
        return Xw, obs, np.ascontiguousarray(K4, np.float32).reshape(4), np.ascontiguousarray(Tcw_in, np.float32).reshape(16)

    def pnp_solver(self, Xw, obs, K4, Tcw_in, prm: PnpSolverParams | None = None):
        """rgbd_pnp_solver: dict(ok, pose (4, 4) f32, mask (M,) u8 [1 = outlier], n_inliers); ok False (M < 3)
        leaves the rest None.  prm None = the reference's values (NULL)."""
        Xw, obs, K4, T = self._pnp_solver_edges(Xw, obs, K4, Tcw_in)
        M = len(Xw)
        pose = np.zeros(16, np.float32)
        mask = np.zeros(max(M, 1), np.uint8)
        ni, ok = C.c_int32(0), C.c_int32(0)
        self._check(lib().rgbd_pnp_solver(self._h, _ptr(Xw), _ptr(obs), M, _ptr(K4), _ptr(T),
                                          C.byref(prm) if prm is not None else None, _ptr(pose), _ptr(mask),
                                          C.byref(ni), C.byref(ok)), "pnp_solver")
        if not ok.value:
            return dict(ok=False, pose=None, mask=None, n_inliers=None)
        return dict(ok=True, pose=pose.reshape(4, 4), mask=mask[:M].copy(), n_inliers=ni.value)

    def pnp_solver_batch(self, problems, K4, prm: PnpSolverParams | None = None):
        """rgbd_pnp_solver_batch over problems = [(Xw, obs, Tcw_in), ...]: a list of pnp_solver's dicts."""
        P = len(problems)
        K4 = np.ascontiguousarray(K4, np.float32).reshape(4)
        xs = [np.ascontiguousarray(p[0], np.float32).reshape(-1, 3) for p in problems]
        os_ = [np.ascontiguousarray(p[1], np.float32).reshape(-1, 2) for p in problems]
        if any(len(a) != len(b) for a, b in zip(xs, os_)):
            raise ValueError("pnp_solver_batch: Xw and obs lengths differ")
        counts = np.array([len(a) for a in xs], np.int32)
        Xw = np.concatenate(xs + [np.zeros((0, 3), np.float32)])
        obs = np.concatenate(os_ + [np.zeros((0, 2), np.float32)])
        Tin = np.ascontiguousarray(np.stack([np.asarray(p[2], np.float32).reshape(16) for p in problems])
                                   if P else np.zeros((0, 16)), np.float32)
        pose = np.zeros((max(P, 1), 16), np.float32)
        masks = np.zeros(max(int(counts.sum()), 1), np.uint8)
        ni = np.zeros(max(P, 1), np.int32)
        ok = np.zeros(max(P, 1), np.int32)
        self._check(lib().rgbd_pnp_solver_batch(self._h, P, _ptr(counts), _ptr(Xw), _ptr(obs), _ptr(K4), _ptr(Tin),
                                                C.byref(prm) if prm is not None else None, _ptr(pose), _ptr(masks),
                                                _ptr(ni), _ptr(ok)), "pnp_solver_batch")
        out, off = [], 0
        for p in range(P):
            if ok[p]:
                out.append(dict(ok=True, pose=pose[p].reshape(4, 4).copy(), mask=masks[off:off + counts[p]].copy(),
                                n_inliers=int(ni[p])))
            else:
                out.append(dict(ok=False, pose=None, mask=None, n_inliers=None))
            off += int(counts[p])
        return out

    def pnp_solver_frames(self, qframe, tframe, poses, matches, as_written=False, prm: PnpSolverParams | None = None):
        """rgbd_pnp_solver_frames over the frames of the last extract_batch: matches = projection_match_batch's
        list of P match arrays (DMATCH_DTYPE), poses (B, 4, 4) Tcw.  A list of pnp_solver's dicts, the masks by
        match position."""
        qf = np.ascontiguousarray(qframe, np.int32)
        tf = np.ascontiguousarray(tframe, np.int32)
        P, K = len(qf), self.kp_cap
        if len(tf) != P or len(matches) != P:
            raise ValueError("pnp_solver_frames: qframe, tframe and matches lengths differ")
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
        rows = np.zeros((max(P, 1), K), DMATCH_DTYPE)
        counts = np.zeros(max(P, 1), np.int32)
        for p, m in enumerate(matches):
            if len(m) > K:
                raise ValueError("pnp_solver_frames: more matches than kp_cap")
            rows[p, :len(m)] = m
            counts[p] = len(m)
        pose = np.zeros((max(P, 1), 16), np.float32)
        masks = np.zeros((max(P, 1), K), np.uint8)
        ni = np.zeros(max(P, 1), np.int32)
        ok = np.zeros(max(P, 1), np.int32)
        self._check(lib().rgbd_pnp_solver_frames(self._h, P, _ptr(qf), _ptr(tf), _ptr(poses), _ptr(rows), _ptr(counts),
                                                 int(bool(as_written)), C.byref(prm) if prm is not None else None,
                                                 _ptr(pose), _ptr(masks), _ptr(ni), _ptr(ok)), "pnp_solver_frames")
        return [dict(ok=True, pose=pose[p].reshape(4, 4).copy(), mask=masks[p, :counts[p]].copy(), n_inliers=int(ni[p]))
                if ok[p] else dict(ok=False, pose=None, mask=None, n_inliers=None) for p in range(P)]

    def debug_pnp_solver(self, Xw, obs, K4, Tcw_in, prm: PnpSolverParams | None = None):
        """rgbd_debug_pnp_solver: pnp_solver's dict plus rounds_run and, per round, est (R, 7) f64 [q xyzw, t],
        iters, trials, lam, nu (R,), chi2 (R, M) f64 and level (R, M) u8 (zeros for the rounds not run)."""
        Xw, obs, K4, T = self._pnp_solver_edges(Xw, obs, K4, Tcw_in)
        M = len(Xw)
        R = prm.rounds if prm is not None else 4
        if R < 1:
            raise ValueError("debug_pnp_solver: rounds must be >= 1")
        pose = np.zeros(16, np.float32)
        mask = np.zeros(max(M, 1), np.uint8)
        ni, ok, rr = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        est = np.zeros((R, 7), np.float64)
        iters, trials = np.zeros(R, np.int32), np.zeros(R, np.int32)
        lam, nu = np.zeros(R, np.float64), np.zeros(R, np.float64)
        chi2 = np.zeros((R, max(M, 1)), np.float64)
        level = np.zeros((R, max(M, 1)), np.uint8)
        self._check(lib().rgbd_debug_pnp_solver(self._h, _ptr(Xw), _ptr(obs), M, _ptr(K4), _ptr(T),
                                                C.byref(prm) if prm is not None else None, _ptr(pose), _ptr(mask),
                                                C.byref(ni), C.byref(ok), C.byref(rr), _ptr(est), _ptr(iters), _ptr(trials),
                                                _ptr(lam), _ptr(nu), _ptr(chi2), _ptr(level)), "debug_pnp_solver")
        # the device rows are M long
        chi2 = chi2.reshape(-1)[:R * M].reshape(R, M) if M else chi2[:, :0]
        level = level.reshape(-1)[:R * M].reshape(R, M) if M else level[:, :0]
        out = dict(ok=bool(ok.value), rounds_run=rr.value, est=est, iters=iters, trials=trials, lam=lam, nu=nu,
                   chi2=chi2.copy(), level=level.copy(), pose=None, mask=None, n_inliers=None)
        if ok.value:
            out.update(pose=pose.reshape(4, 4), mask=mask[:M].copy(), n_inliers=ni.value)
        return out

    # --- Umeyama RANSAC (Ransac::compute, Solver/Ransac.cpp:46-181)
    @staticmethod
    def _um_result(T, inl, ni, it, ok, flags2, rng):
        return dict(ok=bool(ok), T=np.array(T, np.float32).reshape(4, 4), inliers=inl[:ni].copy(), n_inliers=int(ni),
                    iterations=int(it), flags2=flags2, rng=rng)

    def ransac_umeyama(self, xyz1, xyz2, matches, prm: UmeyamaParams, rng: Rng, flags2=None, debug=False):
        """rgbd_ransac_umeyama: dict(ok, T (4, 4) f32 [x1 = T x2], inliers (DMATCH_DTYPE), n_inliers, iterations,
        flags2, rng).  rng is advanced in place; flags2 (F2's mvbOutlier, zeros when None) is updated in place.
        debug: rgbd_debug_ransac_umeyama, adding hyp_pos (iterations, used_pairs), hyp_count, hyp_sneg, best_count
        and accepts (n, 3) [iteration, count, new bound]."""
        xyz1 = np.ascontiguousarray(xyz1, np.float32).reshape(-1, 3)
        xyz2 = np.ascontiguousarray(xyz2, np.float32).reshape(-1, 3)
        m = np.ascontiguousarray(matches, DMATCH_DTYPE)
        M = len(m)
        if flags2 is None:
            flags2 = np.zeros(max(len(xyz2), 1), np.uint8)
        if flags2.dtype != np.uint8 or not flags2.flags.c_contiguous or len(flags2) < len(xyz2):
            raise ValueError("ransac_umeyama: flags2 must be a contiguous u8 array of F2's length")
        T = np.zeros(16, np.float32)
        inl = np.zeros(max(M, 1), DMATCH_DTYPE)
        ni, it, ok = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        head = (self._h, _ptr(xyz1), len(xyz1), _ptr(xyz2), len(xyz2), _ptr(m), M, C.byref(prm), C.byref(rng), _ptr(flags2),
                _ptr(T), _ptr(inl), C.byref(ni), C.byref(it), C.byref(ok))
        if not debug:
            self._check(lib().rgbd_ransac_umeyama(*head), "ransac_umeyama")
            return self._um_result(T, inl, ni.value, it.value, ok.value, flags2, rng)
        cap = 31294 + 256   # iters(0.05), the largest count the limits allow, and a round
        n = max(prm.used_pairs, 1)
        pos = np.zeros((cap, n), np.int32)
        cnt = np.zeros(cap, np.int32)
        sneg = np.zeros(cap, np.uint8)
        acc = np.zeros((4097, 3), np.int32)
        best, nacc = C.c_int32(0), C.c_int32(0)
        self._check(lib().rgbd_debug_ransac_umeyama(*head, cap, _ptr(pos), _ptr(cnt), _ptr(sneg), C.byref(best), 4097,
                                                    _ptr(acc), C.byref(nacc)), "debug_ransac_umeyama")
        out = self._um_result(T, inl, ni.value, it.value, ok.value, flags2, rng)
        out.update(hyp_pos=pos[:it.value].copy(), hyp_count=cnt[:it.value].copy(), hyp_sneg=sneg[:it.value].copy(),
                   best_count=best.value, accepts=acc[:nacc.value].copy())
        return out

    def ransac_umeyama_batch(self, problems, prm: UmeyamaParams, rngs):
        """rgbd_ransac_umeyama_batch over problems = [(xyz1, xyz2, matches, flags2 or None), ...] and one Rng per
        problem (advanced in place): a list of ransac_umeyama's dicts."""
        P = len(problems)
        if len(rngs) != P:
            raise ValueError("ransac_umeyama_batch: one Rng per problem")
        x1 = [np.ascontiguousarray(p[0], np.float32).reshape(-1, 3) for p in problems]
        x2 = [np.ascontiguousarray(p[1], np.float32).reshape(-1, 3) for p in problems]
        ms = [np.ascontiguousarray(p[2], DMATCH_DTYPE) for p in problems]
        fl = [np.zeros(len(b), np.uint8) if p[3] is None else np.ascontiguousarray(p[3], np.uint8) for p, b in zip(problems, x2)]
        n1 = np.array([len(a) for a in x1], np.int32)
        n2 = np.array([len(a) for a in x2], np.int32)
        counts = np.array([len(a) for a in ms], np.int32)
        X1 = np.concatenate(x1 + [np.zeros((1, 3), np.float32)])
        X2 = np.concatenate(x2 + [np.zeros((1, 3), np.float32)])
        Mm = np.concatenate(ms + [np.zeros(1, DMATCH_DTYPE)])
        Fl = np.concatenate(fl + [np.zeros(1, np.uint8)])
        R = (Rng * max(P, 1))(*rngs)
        T = np.zeros((max(P, 1), 16), np.float32)
        inl = np.zeros(len(Mm), DMATCH_DTYPE)
        ni, it, ok = (np.zeros(max(P, 1), np.int32) for _ in range(3))
        self._check(lib().rgbd_ransac_umeyama_batch(self._h, P, _ptr(X1), _ptr(n1), _ptr(X2), _ptr(n2), _ptr(Mm), _ptr(counts),
                                                    C.byref(prm), C.cast(R, _vp), _ptr(Fl), _ptr(T), _ptr(inl), _ptr(ni),
                                                    _ptr(it), _ptr(ok)), "ransac_umeyama_batch")
        out, om, o2 = [], 0, 0
        for p in range(P):
            C.memmove(C.byref(rngs[p]), C.byref(R[p]), C.sizeof(Rng))
            f = Fl[o2:o2 + n2[p]].copy()
            if problems[p][3] is not None:
                problems[p][3][:] = f
            out.append(self._um_result(T[p], inl[om:om + counts[p]], ni[p], it[p], ok[p], f, rngs[p]))
            om += int(counts[p])
            o2 += int(n2[p])
        return out

    def ransac_umeyama_frames(self, qframe, tframe, matches, prm: UmeyamaParams, rngs, flags2=None):
        """rgbd_ransac_umeyama_frames over the frames of the last extract_batch: matches = a list of P match arrays
        (DMATCH_DTYPE), one Rng per pair (advanced in place), flags2 (P, kp_cap) u8 or None (zeros).  A list of
        ransac_umeyama's dicts (flags2 = the pair's kp_cap-long row)."""
        qf = np.ascontiguousarray(qframe, np.int32)
        tf = np.ascontiguousarray(tframe, np.int32)
        P, K = len(qf), self.kp_cap
        if len(tf) != P or len(matches) != P or len(rngs) != P:
            raise ValueError("ransac_umeyama_frames: qframe, tframe, matches and rngs lengths differ")
        rows = np.zeros((max(P, 1), K), DMATCH_DTYPE)
        counts = np.zeros(max(P, 1), np.int32)
        for p, m in enumerate(matches):
            if len(m) > K:
                raise ValueError("ransac_umeyama_frames: more matches than kp_cap")
            rows[p, :len(m)] = m
            counts[p] = len(m)
        fl = np.zeros((max(P, 1), K), np.uint8) if flags2 is None else flags2
        if fl.dtype != np.uint8 or not fl.flags.c_contiguous or fl.shape != (max(P, 1), K):
            raise ValueError("ransac_umeyama_frames: flags2 must be (P, kp_cap) u8")
        R = (Rng * max(P, 1))(*rngs)
        T = np.zeros((max(P, 1), 16), np.float32)
        inl = np.zeros((max(P, 1), K), DMATCH_DTYPE)
        ni, it, ok = (np.zeros(max(P, 1), np.int32) for _ in range(3))
        self._check(lib().rgbd_ransac_umeyama_frames(self._h, P, _ptr(qf), _ptr(tf), _ptr(rows), _ptr(counts), C.byref(prm),
                                                     C.cast(R, _vp), _ptr(fl), _ptr(T), _ptr(inl), _ptr(ni), _ptr(it),
                                                     _ptr(ok)), "ransac_umeyama_frames")
        out = []
        for p in range(P):
            C.memmove(C.byref(rngs[p]), C.byref(R[p]), C.sizeof(Rng))
            out.append(self._um_result(T[p], inl[p], ni[p], it[p], ok[p], fl[p], rngs[p]))
        return out

    @staticmethod
    def ransac_umeyama_pose(T12, Tcw1):
        """rgbd_ransac_umeyama_pose: inv(T12) * Tcw1 (Solver/Ransac.cpp:53), host only."""
        a = np.ascontiguousarray(T12, np.float32).reshape(16)
        b = np.ascontiguousarray(Tcw1, np.float32).reshape(16)
        out = np.zeros(16, np.float32)
        lib().rgbd_ransac_umeyama_pose(_ptr(a), _ptr(b), _ptr(out))
        return out.reshape(4, 4)

    # --- bag of words and the loop database (DESIGN.md "Bag-of-words and loop detection definition")
    def voc_set(self, voc):
        """rgbd_voc_set from a vocabulary.Vocabulary (or any object with its array fields)."""
        parent = np.ascontiguousarray(voc.parent, np.int32)
        desc = np.ascontiguousarray(voc.descriptor, np.uint8)
        weight = np.ascontiguousarray(voc.weight, np.float64)
        leaf = np.ascontiguousarray(voc.is_leaf, np.uint8)
        word = np.ascontiguousarray(voc.word_id, np.int32)
        n = len(parent)
        if not (len(desc) == len(weight) == len(leaf) == len(word) == n) or desc.ndim != 2:
            raise ValueError("voc_set: the node arrays differ in length")
        self._check(lib().rgbd_voc_set(self._h, int(voc.k), int(voc.L), int(voc.weighting), int(voc.scoring), desc.shape[1], n,
                                       _ptr(parent), _ptr(desc), _ptr(weight), _ptr(leaf), _ptr(word)), "voc_set")

    def voc_clear(self):
        self._check(lib().rgbd_voc_clear(self._h), "voc_clear")

    @staticmethod
    def _bow_result(ids, vals, nw, fvn, fvi, nfv):
        return dict(ids=ids[:nw].copy(), vals=vals[:nw].copy(), fv_node=fvn[:nfv].copy(), fv_idx=fvi[:nfv].copy())

    def bow_transform(self, desc, levelsup: int = 4):
        """rgbd_bow_transform: dict(ids u32 ascending, vals f64, fv_node, fv_idx) of one frame's descriptors."""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n, m = len(desc), max(len(desc), 1)
        ids, vals = np.zeros(m, np.uint32), np.zeros(m, np.float64)
        fvn, fvi = np.zeros(m, np.int32), np.zeros(m, np.int32)
        nw, nfv = C.c_int32(0), C.c_int32(0)
        self._check(lib().rgbd_bow_transform(self._h, _ptr(desc), n, levelsup, _ptr(ids), _ptr(vals), C.byref(nw), _ptr(fvn),
                                             _ptr(fvi), C.byref(nfv)), "bow_transform")
        return self._bow_result(ids, vals, nw.value, fvn, fvi, nfv.value)

    def bow_transform_batch(self, descs, levelsup: int = 4):
        """rgbd_bow_transform_batch over a list of descriptor arrays: a list of bow_transform's dicts."""
        descs = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in descs]
        P = len(descs)
        counts = np.array([len(d) for d in descs] + [0], np.int32)
        D = np.ascontiguousarray(np.concatenate(descs + [np.zeros((1, 32), np.uint8)]))
        m = len(D)
        ids, vals = np.zeros(m, np.uint32), np.zeros(m, np.float64)
        fvn, fvi = np.zeros(m, np.int32), np.zeros(m, np.int32)
        nw, nfv = np.zeros(P + 1, np.int32), np.zeros(P + 1, np.int32)
        self._check(lib().rgbd_bow_transform_batch(self._h, P, _ptr(D), _ptr(counts), levelsup, _ptr(ids), _ptr(vals), _ptr(nw),
                                                   _ptr(fvn), _ptr(fvi), _ptr(nfv)), "bow_transform_batch")
        out, o = [], 0
        for p in range(P):
            out.append(self._bow_result(ids[o:], vals[o:], nw[p], fvn[o:], fvi[o:], nfv[p]))
            o += int(counts[p])
        return out

    def bow_transform_frames(self, frames, levelsup: int = 4):
        """rgbd_bow_transform_frames over frames of the last extract_batch: a list of bow_transform's dicts."""
        fr = np.ascontiguousarray(frames, np.int32)
        P, K = len(fr), self.kp_cap
        m = max(P, 1) * K
        ids, vals = np.zeros(m, np.uint32), np.zeros(m, np.float64)
        fvn, fvi = np.zeros(m, np.int32), np.zeros(m, np.int32)
        nw, nfv = np.zeros(max(P, 1), np.int32), np.zeros(max(P, 1), np.int32)
        self._check(lib().rgbd_bow_transform_frames(self._h, P, _ptr(fr), levelsup, _ptr(ids), _ptr(vals), _ptr(nw), _ptr(fvn),
                                                    _ptr(fvi), _ptr(nfv)), "bow_transform_frames")
        return [self._bow_result(ids[p * K:], vals[p * K:], nw[p], fvn[p * K:], fvi[p * K:], nfv[p]) for p in range(P)]

    def debug_bow_words(self, desc, levelsup: int = 4):
        """rgbd_debug_bow_words: dict(word, weight, node, path (n, 10) u8 with 255 below the leaf)."""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n, m = len(desc), max(len(desc), 1)
        word, node = np.zeros(m, np.int32), np.zeros(m, np.int32)
        weight, path = np.zeros(m, np.float64), np.zeros((m, 10), np.uint8)
        self._check(lib().rgbd_debug_bow_words(self._h, _ptr(desc), n, levelsup, _ptr(word), _ptr(weight), _ptr(node),
                                               _ptr(path)), "debug_bow_words")
        return dict(word=word[:n], weight=weight[:n], node=node[:n], path=path[:n])

    def bow_score(self, a, b) -> float:
        """rgbd_bow_score: L1Scoring::score(a, b) of two (ids, vals) vectors."""
        ia, va = np.ascontiguousarray(a[0], np.uint32), np.ascontiguousarray(a[1], np.float64)
        ib, vb = np.ascontiguousarray(b[0], np.uint32), np.ascontiguousarray(b[1], np.float64)
        s = C.c_double(0)
        self._check(lib().rgbd_bow_score(self._h, _ptr(ia), _ptr(va), len(ia), _ptr(ib), _ptr(vb), len(ib), C.byref(s)),
                    "bow_score")
        return s.value

    def loopdb_add(self, ids, vals) -> int:
        ids, vals = np.ascontiguousarray(ids, np.uint32), np.ascontiguousarray(vals, np.float64)
        e = C.c_int32(0)
        self._check(lib().rgbd_loopdb_add(self._h, _ptr(ids), _ptr(vals), len(ids), C.byref(e)), "loopdb_add")
        return e.value

    def loopdb_query(self, ids, vals, query_first: bool = True):
        """rgbd_loopdb_query: (score f64, n_shared, min_shared) per database entry."""
        ids, vals = np.ascontiguousarray(ids, np.uint32), np.ascontiguousarray(vals, np.float64)
        cap = max(lib().rgbd_loopdb_size(self._h), 1)
        score, ns, mw = np.zeros(cap, np.float64), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        n = C.c_int32(0)
        self._check(lib().rgbd_loopdb_query(self._h, _ptr(ids), _ptr(vals), len(ids), int(query_first), cap, _ptr(score),
                                            _ptr(ns), _ptr(mw), C.byref(n)), "loopdb_query")
        return score[:n.value], ns[:n.value], mw[:n.value]

    def loopdb_clear(self):
        self._check(lib().rgbd_loopdb_clear(self._h), "loopdb_clear")

    def pnp_ransac_batch(self, problems, K4, prm: PnpParams | None = None):
        """solvePnPRansac on each (p3 [n,3], p2 [n,2]) of `problems`; one pass for all of them.
        Returns a list of dicts: ok, R (3x3 f64), t (3 f64), mask (bool[n]), n_inliers, iters."""
        prm = prm or pnp_params(min_matches=0)
        P = len(problems)
        counts = np.array([len(p3) for p3, _ in problems], np.int32)
        n = int(counts.sum())
        p3 = np.ascontiguousarray(np.concatenate([np.asarray(a, np.float32).reshape(-1, 3) for a, _ in problems])
                                  if n else np.zeros((1, 3), np.float32), np.float32)
        p2 = np.ascontiguousarray(np.concatenate([np.asarray(b, np.float32).reshape(-1, 2) for _, b in problems])
                                  if n else np.zeros((1, 2), np.float32), np.float32)
        K4 = np.ascontiguousarray(K4, np.float32)
        R, t = np.zeros((max(P, 1), 9)), np.zeros((max(P, 1), 3))
        masks = np.zeros(max(n, 1), np.uint8)
        ninl, iters, ok = (np.zeros(max(P, 1), np.int32) for _ in range(3))
        self._check(lib().rgbd_pnp_ransac_batch(self._h, P, _ptr(counts), _ptr(p3), _ptr(p2), _ptr(K4),
                                                C.byref(prm), _ptr(R), _ptr(t), _ptr(masks), _ptr(ninl), _ptr(iters),
                                                _ptr(ok)), "pnp_ransac_batch")
        out, off = [], 0
        for i in range(P):
            c = int(counts[i])
            out.append(dict(ok=bool(ok[i]), R=R[i].reshape(3, 3).copy(), t=t[i].copy(),
                            mask=masks[off:off + c].astype(bool), n_inliers=int(ninl[i]), iters=int(iters[i])))
            off += c
        return out

    def pnp_ransac(self, p3, p2, K4, prm: PnpParams | None = None):
        return self.pnp_ransac_batch([(p3, p2)], K4, prm)[0]

    def debug_pnp_chunks(self):
        """rgbd_debug_pnp_chunks: (k0, k1), the iterations per problem of the next solve's two device chunks."""
        k0, k1 = C.c_int32(), C.c_int32()
        self._check(lib().rgbd_debug_pnp_chunks(self._h, C.byref(k0), C.byref(k1)), "debug_pnp_chunks")
        return k0.value, k1.value

    def pnp_track_batch(self, d_bgr: int, d_depth: int, B: int, nnratio: float, prm: PnpParams | None = None,
                        pose0=None):
        prm = prm or pnp_params()
        poses = np.zeros((B, 16), np.float32)
        poses[0] = (np.eye(4, dtype=np.float32) if pose0 is None else np.asarray(pose0, np.float32)).reshape(16)
        status, ninl, nm = (np.zeros(B, np.int32) for _ in range(3))
        self._check(lib().rgbd_pnp_track_batch(self._h, C.c_void_p(d_bgr), C.c_void_p(d_depth), B, nnratio,
                                               C.byref(prm), _ptr(poses), _ptr(status), _ptr(ninl), _ptr(nm)),
                    "pnp_track_batch")
        return poses.reshape(B, 4, 4), status, ninl, nm

    def pnp_track_submit(self, d_bgr: int, d_depth: int, B: int, nnratio: float, prm: PnpParams | None = None):
        """Enqueue one extract + match + PnPRansac step (rgbd_pnp_track_submit); at most three outstanding."""
        prm = prm or pnp_params()
        self._pending.append(B)
        try:
            self._check(lib().rgbd_pnp_track_submit(self._h, C.c_void_p(d_bgr), C.c_void_p(d_depth), B, nnratio,
                                                    C.byref(prm)), "pnp_track_submit")
        except Exception:
            self._pending.pop()
            raise

    def pnp_track_collect(self, pose0=None):
        """Results of the oldest outstanding submission: (poses, status, n_inliers, n_matches)."""
        if not self._pending:
            raise RgbdError("pnp_track_collect: nothing submitted")
        B = self._pending.pop(0)
        poses = np.zeros((B, 16), np.float32)
        poses[0] = (np.eye(4, dtype=np.float32) if pose0 is None else np.asarray(pose0, np.float32)).reshape(16)
        status, ninl, nm = (np.zeros(B, np.int32) for _ in range(3))
        self._check(lib().rgbd_pnp_track_collect(self._h, _ptr(poses), _ptr(status), _ptr(ninl), _ptr(nm)),
                    "pnp_track_collect")
        return poses.reshape(B, 4, 4), status, ninl, nm

    def keyframe_cloud(self, bgr, depth, prm: CloudParams | None = None):
        """Tracking::createKeyFrame's dense cloud of one frame (host buffers): rgbd_point array."""
        prm = prm or cloud_params()
        bgr = np.ascontiguousarray(bgr, np.uint8)
        depth = np.ascontiguousarray(depth, np.uint16)
        cap = ((depth.shape[0] + prm.stride - 1) // prm.stride) * ((depth.shape[1] + prm.stride - 1) // prm.stride)
        out = np.zeros(cap, POINT_DTYPE)
        n = C.c_int32(0)
        self._check(lib().rgbd_keyframe_cloud(self._h, _ptr(bgr), _ptr(depth), C.byref(prm), _ptr(out), cap,
                                              C.byref(n)), "keyframe_cloud")
        return out[:n.value].copy()

    def keyframe_cloud_f32(self, bgr, depth_f32, prm: CloudParams | None = None):
        """The same cloud from Frame::mImDepth (f32, already scaled by 1/factor), as Frame::createCloud reads it."""
        prm = prm or cloud_params()
        bgr = np.ascontiguousarray(bgr, np.uint8)
        depth = np.ascontiguousarray(depth_f32, np.float32)
        cap = ((depth.shape[0] + prm.stride - 1) // prm.stride) * ((depth.shape[1] + prm.stride - 1) // prm.stride)
        out = np.zeros(cap, POINT_DTYPE)
        n = C.c_int32(0)
        self._check(lib().rgbd_keyframe_cloud_f32(self._h, _ptr(bgr), _ptr(depth), C.byref(prm), _ptr(out), cap,
                                                  C.byref(n)), "keyframe_cloud_f32")
        return out[:n.value].copy()

    def keyframe_cloud_batch(self, d_bgr: int, d_depth: int, B: int, frames, prm: CloudParams | None = None,
                             W: int = 640, H: int = 480):
        """Clouds of the listed frames of a device batch: list of rgbd_point arrays."""
        prm = prm or cloud_params()
        frames = np.ascontiguousarray(frames, np.int32)
        cap = ((H + prm.stride - 1) // prm.stride) * ((W + prm.stride - 1) // prm.stride)
        out = np.zeros((max(len(frames), 1), cap), POINT_DTYPE)
        counts = np.zeros(max(len(frames), 1), np.int32)
        self._check(lib().rgbd_keyframe_cloud_batch(self._h, C.c_void_p(d_bgr), C.c_void_p(d_depth), B, _ptr(frames),
                                                    len(frames), C.byref(prm), _ptr(out), cap, _ptr(counts)),
                    "keyframe_cloud_batch")
        return [out[k, :counts[k]].copy() for k in range(len(frames))]

    def gicp(self, src, tgt, guess, prm: GicpParams | None = None):
        """GICP align: (converged, T 4x4 f32, iterations)."""
        prm = prm or gicp_params()
        src = np.ascontiguousarray(src, np.float32).reshape(-1, 3)
        tgt = np.ascontiguousarray(tgt, np.float32).reshape(-1, 3)
        guess = np.ascontiguousarray(guess, np.float32).reshape(16)
        T = np.zeros(16, np.float32)
        cv, it = C.c_int32(0), C.c_int32(0)
        self._check(lib().rgbd_gicp(self._h, _ptr(src), _ptr(tgt), len(src), _ptr(guess), C.byref(prm), _ptr(T),
                                    C.byref(cv), C.byref(it)), "gicp")
        return bool(cv.value), T.reshape(4, 4), it.value

    def gicp_compute(self, src, tgt, guess, prm: GicpParams | None = None):
        """Gicp::compute: (ok, T 4x4 f32)."""
        prm = prm or gicp_params()
        src = np.ascontiguousarray(src, np.float32).reshape(-1, 3)
        tgt = np.ascontiguousarray(tgt, np.float32).reshape(-1, 3)
        guess = np.ascontiguousarray(guess, np.float32).reshape(16)
        T = np.zeros(16, np.float32)
        ok = C.c_int32(0)
        self._check(lib().rgbd_gicp_compute(self._h, _ptr(src), _ptr(tgt), len(src), _ptr(guess), C.byref(prm),
                                            _ptr(T), C.byref(ok)), "gicp_compute")
        return bool(ok.value), T.reshape(4, 4)

    def debug_gicp_cov(self, pts, k: int = 20, eps: float = 1e-3) -> np.ndarray:
        """The covariance stage of gicp() on its own (rgbd_debug_gicp_cov): (M, 3, 3) f64, one matrix per point."""
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
        cov = np.zeros((max(len(pts), 1), 9))
        self._check(lib().rgbd_debug_gicp_cov(self._h, _ptr(pts), len(pts), int(k), float(eps), _ptr(cov)),
                    "debug_gicp_cov")
        return cov[:len(pts)].reshape(-1, 3, 3)

    def set_tracking_gicp(self, prm: GicpParams | None):
        self._check(lib().rgbd_set_tracking_gicp(self._h, C.byref(prm) if prm is not None else None),
                    "set_tracking_gicp")

    # --- measurement
    def set_timing(self, on: bool):
        self._check(lib().rgbd_set_timing(self._h, int(on)), "set_timing")

    def set_timing_filter(self, kernel: str | None):
        self._check(lib().rgbd_set_timing_filter(self._h, kernel.encode() if kernel else None), "set_timing_filter")

    def reset_timing(self):
        self._check(lib().rgbd_reset_timing(self._h), "reset_timing")

    def timings(self):
        out = {}
        for i in range(lib().rgbd_timing_count(self._h)):
            name, ms, n = C.c_char_p(), C.c_double(), C.c_int64()
            self._check(lib().rgbd_timing_entry(self._h, i, C.byref(name), C.byref(ms), C.byref(n)), "timing")
            out[name.value.decode()] = (ms.value, n.value)
        return out

    def synchronize(self):
        self._check(lib().rgbd_synchronize(self._h), "synchronize")

    def set_stream(self, stream: int):
        """Launch on a caller's HIP stream (a torch.cuda.Stream's .cuda_stream); 0 = the context's own."""
        self._check(lib().rgbd_set_stream(self._h, C.c_void_p(stream)), "set_stream")


class OccupancyMap:
    """The coloured occupancy map (rgbd_occmap_*): OctomapDrawer's ColorOcTree as a device-resident voxel table on
    `ctx`'s stream.  Leaves only; the definition is DESIGN.md "Occupancy map definition" (parity with liboctomap is
    unpinned)."""

    def __init__(self, ctx: Context, prm: OccmapParams | None = None):
        self.ctx = ctx   # the context must outlive the map
        self.prm = prm or occmap_params()
        h = C.c_void_p()
        st = lib().rgbd_occmap_create(ctx._h, C.byref(self.prm), C.byref(h))
        self._h = h
        if st != 0:
            raise RgbdError(f"occmap_create: {lib().rgbd_last_error(ctx._h).decode()} (status {st})")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            if self.ctx._h.value:
                lib().rgbd_occmap_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st, what):
        if st != 0:
            raise RgbdError(f"{what}: {lib().rgbd_last_error(self.ctx._h).decode()} (status {st})")

    @staticmethod
    def _pose(Twc34, origin):
        T = np.ascontiguousarray(Twc34, np.float32)
        o = np.ascontiguousarray(origin, np.float32)
        if T.size != 12 or o.size != 3:
            raise ValueError("occmap: Twc34 is 3x4 and origin has 3 entries")
        return T, o

    def insert(self, pts, Twc34, origin, maxrange: float = -1.0):
        """One scan: rgbd_point array in the camera frame, the f32 [R' | Ow] and the sensor origin (occmap.sensor_pose).
        A scan that does not fit leaves the map as it was and raises (status 3)."""
        pts = np.ascontiguousarray(pts, POINT_DTYPE)
        T, o = self._pose(Twc34, origin)
        self._check(lib().rgbd_occmap_insert(self._h, _ptr(pts), len(pts), _ptr(T), _ptr(o), float(maxrange)), "occmap_insert")

    def insert_batch(self, clouds, Twc34s, origins, maxrange: float = -1.0) -> int:
        """The scans of a list of clouds queued in one call; returns how many were applied (all, unless one did not fit:
        that one and the scans after it are left out and nothing is raised)."""
        n = len(clouds)
        if n == 0:
            return 0
        cap = max(max(len(c) for c in clouds), 1)
        pts = np.zeros((n, cap), POINT_DTYPE)
        counts = np.zeros(n, np.int32)
        for k, c in enumerate(clouds):
            pts[k, :len(c)] = c
            counts[k] = len(c)
        T = np.ascontiguousarray(Twc34s, np.float32)
        o = np.ascontiguousarray(origins, np.float32)
        if T.size != 12 * n or o.size != 3 * n:
            raise ValueError("occmap: one 3x4 pose and one origin per cloud")
        applied = C.c_int32(0)
        st = lib().rgbd_occmap_insert_batch(self._h, _ptr(pts), _ptr(counts), cap, n, _ptr(T), _ptr(o), float(maxrange),
                                            C.byref(applied))
        if st != 3:   # RGBD_ERR_CAPACITY is the count
            self._check(st, "occmap_insert_batch")
        return applied.value

    def clear(self):
        self._check(lib().rgbd_occmap_clear(self._h), "occmap_clear")

    def __len__(self):
        n = C.c_int64(0)
        self._check(lib().rgbd_occmap_size(self._h, C.byref(n)), "occmap_size")
        return n.value

    def leaves(self, min_prob: float | None = None):
        """(keys (n, 3) u16, logodds (n,) f32, rgb (n, 3) u8) of the leaves with occupancy >= min_prob (None: all),
        ascending by (kx << 32) | (ky << 16) | kz."""
        lo = np.float32(-np.inf) if min_prob is None else occmap_logodds(min_prob)
        n = C.c_int64(0)
        cap = max(len(self), 1)
        keys, v, rgb = np.zeros((cap, 3), np.uint16), np.zeros(cap, np.float32), np.zeros((cap, 3), np.uint8)
        self._check(lib().rgbd_occmap_leaves(self._h, C.c_float(lo), _ptr(keys), _ptr(v), _ptr(rgb), cap, C.byref(n)),
                    "occmap_leaves")
        return keys[:n.value].copy(), v[:n.value].copy(), rgb[:n.value].copy()
