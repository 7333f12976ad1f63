"""Host-side mirror of the reference's front-end classes over the HIP C ABI (include/vsg_orb.h).

`ORBextractor` mirrors VS_GRAPHS::ORBextractor (orb_slam3/include/ORBextractor.h:42-119):
same constructor arguments, `__call__` = operator() returning (monoIndex, keypoints, descriptors),
the scale-table getters and `image_pyramid` (mvImagePyramid).  `ORBmatcher` mirrors the Hamming
searches of VS_GRAPHS::ORBmatcher (orb_slam3/include/ORBmatcher.h:34-99) on flattened arrays.

There is no CPU fallback: importing works anywhere, but constructing an extractor or calling a
matcher without libvsg_orb.so and a HIP device raises.
"""
import ctypes as C
from pathlib import Path

import numpy as np

import os

_PKG = Path(__file__).resolve().parent
# VSG_LIB=<path> loads an experimental build instead of the in-tree library (A/B scripts under tools/): the in-tree
# file is never overwritten, so later runs cannot silently pick up a variant
LIB_PATH = Path(os.environ["VSG_LIB"]) if os.environ.get("VSG_LIB") else _PKG / "libvsg_orb.so"

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28

VSG_OK = 0
ERRORS = {-1: "VSG_ERR_EMPTY_IMAGE", -2: "VSG_ERR_CAPACITY", -3: "VSG_ERR_UNSUPPORTED", -4: "VSG_ERR_NO_DEVICE",
          -5: "VSG_ERR_HIP", -6: "VSG_ERR_INVALID", -7: "VSG_ERR_BUSY"}

_u8p = C.POINTER(C.c_uint8)
_i32p = C.POINTER(C.c_int32)
_u32p = C.POINTER(C.c_uint32)
_f32p = C.POINTER(C.c_float)
_u16p = C.POINTER(C.c_uint16)

EXPORTS = [
    "vsg_last_error", "vsg_device_count", "vsg_orb_create", "vsg_orb_destroy", "vsg_orb_get_tables",
    "vsg_orb_set_blur_taps", "vsg_orb_capacity", "vsg_orb_extract", "vsg_orb_extract_batch",
    "vsg_orb_extract_batch_device", "vsg_orb_level_size", "vsg_orb_copy_pyramid_level",
    "vsg_orb_copy_blurred_level", "vsg_orb_copy_candidates", "vsg_orb_copy_selected", "vsg_orb_enable_timing",
    "vsg_orb_get_timing", "vsg_orb_set_serialize", "vsg_hamming_pairs", "vsg_hamming_block_best2", "vsg_hamming_block_best2_device",
    "vsg_search_by_bow_kf_f", "vsg_search_by_bow_kf_kf", "vsg_search_by_projection_last",
    "vsg_search_by_projection_local", "vsg_search_for_initialization", "vsg_search_window", "vsg_grid_build",
    "vsg_grid_destroy", "vsg_grid_query", "vsg_stereo_matches", "vsg_orb_set_gray_coeffs",
    "vsg_orb_extract_batch_device_color", "vsg_orb_extract_batch_color", "vsg_vocab_load", "vsg_vocab_destroy",
    "vsg_vocab_info", "vsg_bow_transform", "vsg_distinctive_descriptors", "vsg_debug_device_sort",
    "vsg_search_for_triangulation", "vsg_search_by_bow_kf_f_stereo",
    # round 2: threads / staging, async host pipeline, device-resident frames, routine-level searches
    "vsg_thread_release", "vsg_thread_arena_growths", "vsg_debug_call_profile", "vsg_orb_time_stats", "vsg_host_register", "vsg_host_unregister", "vsg_host_alloc", "vsg_host_free", "vsg_orb_slots",
    "vsg_orb_submit_batch", "vsg_orb_wait", "vsg_orb_copy_pyramid", "vsg_frame_create", "vsg_frame_destroy",
    "vsg_frame_upload", "vsg_frame_from_extractor", "vsg_frame_size", "vsg_frame_copy_grid",
    "vsg_frame_features_in_area", "vsg_frame_search_by_projection", "vsg_frame_search_by_projection_last",
    "vsg_frame_search_by_projection_sim3", "vsg_frame_search_by_projection_kf", "vsg_frame_search_by_sim3",
    "vsg_frame_fuse", "vsg_frame_fuse_sim3", "vsg_fuse_decide", "vsg_frame_search_for_initialization",
    "vsg_frame_search_by_bow_kf_f", "vsg_frame_search_by_bow_kf_kf", "vsg_frame_bow_transform", "vsg_frame_stereo_bow_search",
    "vsg_frame_search_for_triangulation",
    "vsg_frame_stereo_matches",
    "vsg_shard_last_error", "vsg_shard_record_bytes", "vsg_shard_record_desc_offset", "vsg_shard_frame_owner",
    "vsg_shard_stream_owner", "vsg_shard_unique_id", "vsg_shard_create", "vsg_shard_destroy", "vsg_shard_all_gather",
    "vsg_shard_record", "vsg_shard_world", "vsg_shard_send_recv_boundary", "vsg_shard_boundary_record",
    "vsg_copy_d2d_async",
    # round 4
    "vsg_orb_set_pyramid_tiling", "vsg_shard_rank", "vsg_camera_image_bounds", "vsg_frame_from_extractor_undistort",
    "vsg_orb_extract_to_frame",
    # RGB-D frames: Tracking::GrabImageRGBD's depth conversion + Frame::ComputeStereoFromRGBD
    "vsg_orb_extract_to_frame_rgbd", "vsg_depth_map_scale", "vsg_rgbd_depth_batch_device",
    # round 5
    "vsg_host_kind", "vsg_orb_set_direct_registered",
    # TemplatedVocabulary::score and the device-resident KeyFrameDatabase
    "vsg_vocab_score", "vsg_kfdb_create", "vsg_kfdb_destroy", "vsg_kfdb_add", "vsg_kfdb_erase", "vsg_kfdb_clear",
    "vsg_kfdb_clear_map", "vsg_kfdb_set_map", "vsg_kfdb_set_covisibility", "vsg_kfdb_detect_relocalization_candidates",
    "vsg_kfdb_detect_n_best_candidates",
    # resident map points: Frame::isInFrustum and Tracking::SearchLocalPoints
    "vsg_mappoints_create", "vsg_mappoints_destroy", "vsg_mappoints_capacity", "vsg_mappoints_update",
    "vsg_mappoints_read", "vsg_frame_is_in_frustum", "vsg_frame_search_local_points",
    # the motion-model and relocalisation projection searches on resident map points
    "vsg_frame_search_last_frame", "vsg_frame_search_keyframe_points",
    # Fuse x2 and the Sim3 projection search on resident map points
    "vsg_frame_fuse_points", "vsg_frame_fuse_points_sim3", "vsg_frame_search_sim3_points",
    # SearchForTriangulation with the epipolar test on the device (its test hook, vsg_debug_epipolar_pairs of
    # include/vsg_orb_debug_epipolar.h, is bound below but is no part of the two headers this list mirrors)
    "vsg_frame_search_for_triangulation_epipolar",
    # ComputeDistinctiveDescriptors and UpdateNormalAndDepth of resident map points from their observation lists
    "vsg_mappoints_refresh_from_observations",
    # Optimizer::PoseOptimization on a resident frame and resident map points
    "vsg_frame_pose_optimization", "vsg_frame_pose_optimization_resume",
    # Tracking::TrackWithMotionModel: search, ordered walk and PoseOptimization in one enqueue and one wait
    "vsg_frame_track_with_motion_model",
    # Tracking::TrackLocalMap: frustum, search, ordered walk, PoseOptimization and the statistics in one enqueue and one wait
    "vsg_frame_track_local_map",
    # LocalMapping::CreateNewMapPoints on resident keyframes: triangulate, gate, write the new points into the store
    "vsg_frame_set_stereo_points", "vsg_frame_triangulate_matches", "vsg_frame_create_new_map_points",
    # Sim3Solver on resident map points: every RANSAC hypothesis in one call, and the host-side set-up of the solver
    "vsg_mappoints_sim3_ransac", "vsg_sim3_ransac_iterations", "vsg_sim3_draw_samples",
    # Optimizer::OptimizeSim3 on two resident keyframes and resident map points
    "vsg_frame_optimize_sim3",
    # the visual part of Optimizer::LocalBundleAdjustment on resident keyframes and resident map points (its test hook,
    # vsg_debug_local_ba_trial_slots of include/vsg_orb_debug_local_ba.h, is bound below but is no part of the two headers
    # this list mirrors)
    "vsg_mappoints_local_bundle_adjustment",
    # Optimizer::LocalBundleAdjustment with its planes and rooms behind the visual part
    "vsg_mappoints_local_bundle_adjustment_sgraph",
    # the visual part of Optimizer::BundleAdjustment behind GlobalBundleAdjustemnt on resident keyframes and resident map
    # points (its test hooks, vsg_debug_ba_reduced_solve and vsg_debug_ba_solver_geometry of
    # include/vsg_orb_debug_global_ba.h, are bound below but are no part of the two headers this list mirrors)
    "vsg_mappoints_global_bundle_adjustment",
    # Optimizer::OptimizeEssentialGraph (the pose graph of loop closing) and the Sim3 point correction it shares with
    # LoopClosing::CorrectLoop, on resident map points
    "vsg_mappoints_optimize_essential_graph", "vsg_mappoints_correct_sim3",
    # TwoViewReconstruction::Reconstruct (the monocular initialisation) on two resident frames or on caller arrays, the
    # reference's default parameters and the host-side draw of the minimal sets
    "vsg_frame_two_view_reconstruct", "vsg_two_view_reconstruct", "vsg_two_view_default_params", "vsg_two_view_draw_sets",
    # MLPnPsolver on a resident frame and resident map points: one iterate() call with every hypothesis side by side, and
    # the host-side set-up of the solver
    "vsg_frame_mlpnp_ransac", "vsg_mlpnp_ransac_parameters", "vsg_mlpnp_draw_sets",
    # test hook: the launch forms of the last enqueue
    "vsg_debug_last_launch_forms",
    # test hook: the query state of one keyframe of the resident KeyFrameDatabase
    "vsg_debug_kfdb_state",
    # test hook: the chain calls' ordered walk (k_track_walk) alone, on lists the caller wrote
    "vsg_debug_track_walk",
    # k_fast_cells' launch form: automatic / general
    "vsg_orb_set_fast_form",
]

# include/vsg_orb_debug.h vsg_launch_forms, field for field
LAUNCH_FORM_FIELDS = ("latency_chain", "pyramid_tiling", "fast_cells_per_wg", "fast_tile_pitch", "cand_segmented",
                      "fused_blur", "octree_kernel", "octree_hist_big", "octree_label_bytes", "octree_lead", "self_slots",
                      "orient_mirror", "cus", "total_cells", "nframes", "fast_specialised")
# vsg_launch_forms.octree_kernel (VSG_OCT_*)
OCT_BLUR_MEMBATCH, OCT_BLUR_MEMBATCH_FUSED, OCT_FEW_MEMBATCH, OCT_FEW_MEMBATCH_FUSED, OCT_STANDALONE = 1, 2, 3, 4, 5


class _LaunchForms(C.Structure):
    _fields_ = [(n, C.c_int) for n in LAUNCH_FORM_FIELDS]


class FramePose(C.Structure):
    """include/vsg_orb.h vsg_frame_pose: the camera of one Frame as Frame::isInFrustum uses it (mRcw row-major, mtcw, mOw,
    Pinhole::mvParameters, mbf, mfLogScaleFactor, mnScaleLevels)."""
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3), ("fx", C.c_float),
                ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("mbf", C.c_float),
                ("log_scale_factor", C.c_float), ("n_levels", C.c_int32)]

    @classmethod
    def make(cls, Rcw, tcw, Ow, fx, fy, cx, cy, mbf, log_scale_factor, n_levels):
        p = cls()
        p.Rcw[:] = [float(v) for v in np.asarray(Rcw, np.float32).reshape(9)]
        p.tcw[:] = [float(v) for v in np.asarray(tcw, np.float32).reshape(3)]
        p.Ow[:] = [float(v) for v in np.asarray(Ow, np.float32).reshape(3)]
        p.fx, p.fy, p.cx, p.cy, p.mbf = float(fx), float(fy), float(cx), float(cy), float(mbf)
        p.log_scale_factor, p.n_levels = float(log_scale_factor), int(n_levels)
        return p


class TriangulationParams(C.Structure):
    """include/vsg_orb.h vsg_triangulation_params: the two cameras of LocalMapping::CreateNewMapPoints (kf1 =
    mpCurrentKeyFrame, kf2 = pKF2), ratioFactor, mbInertial, mbFarPoints / mThFarPoints and kf2_first =
    std::less<KeyFrame *>()(pKF2, mpCurrentKeyFrame)."""
    _fields_ = [("kf1", FramePose), ("kf2", FramePose), ("ratio_factor", C.c_float), ("th_far_points", C.c_float),
                ("inertial", C.c_int32), ("far_points", C.c_int32), ("kf2_first", C.c_int32)]

    @classmethod
    def make(cls, kf1, kf2, ratio_factor, inertial=False, far_points=False, th_far_points=0.0, kf2_first=False):
        p = cls()
        p.kf1, p.kf2 = kf1, kf2
        p.ratio_factor, p.th_far_points = float(ratio_factor), float(th_far_points)
        p.inertial, p.far_points, p.kf2_first = int(bool(inertial)), int(bool(far_points)), int(bool(kf2_first))
        return p


# vsg_frame_triangulate_matches / vsg_frame_create_new_map_points: reason and source codes (VSG_TRI_* of include/vsg_orb.h)
TRI_REASONS = ("accepted", "low_parallax", "w_zero", "stereo_depth", "z1", "z2", "reproj1", "reproj2", "dist_zero", "far",
               "scale_ratio", "no_free_slot")
TRI_NO_MATCH = 255
TRI_FROM_TRIANGULATE, TRI_FROM_STEREO1, TRI_FROM_STEREO2 = 0, 1, 2


class PoseSE3(C.Structure):
    """include/vsg_orb.h vsg_pose_se3: Tcw.unit_quaternion() as x y z w, Tcw.translation()."""
    _fields_ = [("q", C.c_float * 4), ("t", C.c_float * 3)]


class PoseResult(C.Structure):
    """include/vsg_orb.h vsg_pose_result."""
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("n_initial", C.c_int32), ("n_bad", C.c_int32),
                ("rounds_run", C.c_int32), ("held", C.c_int32)]


class TrackResult(C.Structure):
    """include/vsg_orb.h vsg_track_result."""
    _fields_ = [("pose", PoseResult)] + [(k, C.c_int32) for k in (
        "n_search", "wide", "n_matches_searched", "optimized", "n_matches", "n_matches_map", "direction", "pad")]


class TrackLocalResult(C.Structure):
    """include/vsg_orb.h vsg_track_local_result."""
    _fields_ = [("pose", PoseResult)] + [(k, C.c_int32) for k in (
        "n_to_match", "n_matches_searched", "n_matches_inliers", "walk_rounds")]


class Sim3Result(C.Structure):
    """include/vsg_orb.h vsg_sim3_result: mBestRotation (row-major), mBestTranslation, mBestScale, mBestT12, bConverge,
    bNoMore, mnBestInliers, the chosen hypothesis and mnIterations."""
    _fields_ = [("R12", C.c_float * 9), ("t12", C.c_float * 3), ("s12", C.c_float), ("T12", C.c_float * 16),
                ("converged", C.c_int32), ("no_more", C.c_int32), ("n_inliers", C.c_int32), ("best_hypothesis", C.c_int32),
                ("iterations", C.c_int32)]


class Sim3d(C.Structure):
    """include/vsg_orb.h vsg_sim3d: g2o::Sim3, r as x y z w (taken as it is, not normalised), t, s."""
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("s", C.c_double)]

    @classmethod
    def make(cls, q, t, s):
        o = cls()
        o.q[:] = [float(v) for v in np.asarray(q, np.float64).reshape(4)]
        o.t[:] = [float(v) for v in np.asarray(t, np.float64).reshape(3)]
        o.s = float(s)
        return o


class Sim3OptResult(C.Structure):
    """include/vsg_orb.h vsg_sim3_opt_result: g2oS12 on return, nCorrespondences, nBad, nIn, nInKF2, nOutKF2,
    nMoreIterations and whether g2oS12 was updated (Optimizer.cc:3526)."""
    _fields_ = [("S12", Sim3d), ("n_correspondences", C.c_int32), ("n_bad", C.c_int32), ("n_in", C.c_int32),
                ("n_in_kf2", C.c_int32), ("n_out_kf2", C.c_int32), ("more_iterations", C.c_int32), ("updated", C.c_int32)]


class PoseSE3d(C.Structure):
    """include/vsg_orb.h vsg_pose_se3d: a g2o::SE3Quat, the rotation as x y z w."""
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3)]


class BaCamera(C.Structure):
    """include/vsg_orb.h vsg_ba_camera: a keyframe's fx, fy, cx, cy, mbf."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float)]


LOCAL_BA_RESULT_INTS = ("ran", "n_opt_kf", "n_fixed_kf", "n_points", "n_edges", "n_mono", "n_stereo", "n_erase",
                        "iterations_run", "trials_run", "stop_reason")
LOCAL_BA_RESULT_DOUBLES = ("lambda", "chi2_initial", "chi2_final")
# vsg_local_ba_result.stop_reason
LOCAL_BA_STOP_REASONS = ("iterations_done", "terminate", "n_bad", "stop_flag")


class LocalBaResult(C.Structure):
    """include/vsg_orb.h vsg_local_ba_result."""
    _fields_ = [(k, C.c_int32) for k in LOCAL_BA_RESULT_INTS] + [(k, C.c_double) for k in LOCAL_BA_RESULT_DOUBLES]


SGRAPH_LOCAL_BA_RESULT_INTS = ("n_planes_active", "n_rooms_active", "n_plane_kf", "n_plane_point", "n_room_edges", "n_rows",
                               "n_erase_plane", "reserved")
SGRAPH_LOCAL_BA_MAX_ROWS = 768  # 6 optimised keyframes + 3 planes with an edge + 6 rooms


class SGraphLocalBaResult(C.Structure):
    """include/vsg_orb.h vsg_sgraph_local_ba_result: the local call's result, then the semantic counters."""
    _fields_ = [("local", LocalBaResult)] + [(k, C.c_int32) for k in SGRAPH_LOCAL_BA_RESULT_INTS]


GLOBAL_BA_RESULT_INTS = tuple(k for k in LOCAL_BA_RESULT_INTS if k != "n_erase")
GLOBAL_BA_RESULT_DOUBLES = LOCAL_BA_RESULT_DOUBLES


class GlobalBaResult(C.Structure):
    """include/vsg_orb.h vsg_global_ba_result: the local call's counters without n_erase."""
    _fields_ = [(k, C.c_int32) for k in GLOBAL_BA_RESULT_INTS] + [(k, C.c_double) for k in GLOBAL_BA_RESULT_DOUBLES]


ESSENTIAL_GRAPH_RESULT_INTS = ("ran", "n_opt_kf", "n_fixed_kf", "n_kf", "n_edges", "n_points", "iterations_run", "trials_run",
                               "stop_reason", "pad")
ESSENTIAL_GRAPH_RESULT_DOUBLES = LOCAL_BA_RESULT_DOUBLES
ESSENTIAL_GRAPH_MAX_OPT_KF = 438  # 7 rows each: 3066 <= 3072, the dense solve's tested range


class EssentialGraphResult(C.Structure):
    """include/vsg_orb.h vsg_essential_graph_result."""
    _fields_ = [(k, C.c_int32) for k in ESSENTIAL_GRAPH_RESULT_INTS] + [(k, C.c_double) for k in ESSENTIAL_GRAPH_RESULT_DOUBLES]


class TwoViewParams(C.Structure):
    """include/vsg_orb.h vsg_two_view_params: mSigma, the RH threshold of TwoViewReconstruction.cc:119, minParallax and
    minTriangulated (:116-127)."""
    _fields_ = [("sigma", C.c_float), ("rh_threshold", C.c_float), ("min_parallax", C.c_float), ("min_triangulated", C.c_int32)]


class TwoViewResult(C.Structure):
    """include/vsg_orb.h vsg_two_view_result."""
    _fields_ = [("ok", C.c_int32), ("reason", C.c_int32), ("model", C.c_int32), ("SH", C.c_float), ("SF", C.c_float),
                ("best_it_h", C.c_int32), ("best_it_f", C.c_int32), ("H21", C.c_float * 9), ("F21", C.c_float * 9),
                ("R21", C.c_float * 9), ("t21", C.c_float * 3), ("n_good", C.c_int32 * 8), ("parallax", C.c_float),
                ("n_inliers", C.c_int32)]


class MlpnpResult(C.Structure):
    """include/vsg_orb.h vsg_mlpnp_result: Tout (row-major), iterate's return value, bNoMore, nInliers, whether the return went
    through Refine() (hypothesis iterations - 1) or is the best at the loop's end, the best hypothesis, mnIterations on return,
    the correspondences and how often the best set was replaced."""
    _fields_ = [("Tcw", C.c_float * 16)] + [(k, C.c_int32) for k in (
        "found", "no_more", "n_inliers", "refined", "best_hypothesis", "iterations", "n_correspondences", "n_records")]


# vsg_two_view_result.reason / .model
TWO_VIEW_REASONS = ("ok", "no_score", "singular_values", "no_winner", "low_parallax")
TWO_VIEW_H, TWO_VIEW_F = 0, 1

# vsg_frame_optimize_sim3: state[i]
SIM3_OPT_STATES = ("no_edge", "inlier", "nulled_first_check", "nulled_second_check", "skipped_z_negative", "skipped_not_in_kf2")

_RANDOM_INT = C.CFUNCTYPE(C.c_int, C.c_int, C.c_int, C.c_void_p)


class VsgError(RuntimeError):
    def __init__(self, code, where, detail=""):
        self.code = code
        super().__init__(f"{where}: {ERRORS.get(code, code)} {detail}".strip())


_lib = None


def camera_image_bounds(cols, rows, K4, dist):
    """Frame::ComputeImageBounds (Frame.cc:924-955): (mnMinX, mnMinY, mnMaxX, mnMaxY); host arithmetic in the library."""
    L = load_library()
    K4, dist = np.ascontiguousarray(K4, np.float32), np.ascontiguousarray(dist, np.float32)
    out = np.zeros(4, np.float32)
    _check(L.vsg_camera_image_bounds(int(cols), int(rows), _p(K4, _f32p), _p(dist, _f32p), len(dist), _p(out, _f32p)),
           "vsg_camera_image_bounds")
    return tuple(float(v) for v in out)


def debug_device_sort(items, device=0):
    """Test hook: the device's std::sort replay (see include/vsg_orb.h) on uint64 items (key = upper 32 bits)."""
    L = load_library()
    a = np.ascontiguousarray(items, dtype=np.uint64).copy()
    L.vsg_debug_device_sort.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.c_int]
    _check(L.vsg_debug_device_sort(device, a.ctypes.data_as(C.POINTER(C.c_uint64)), len(a)), "vsg_debug_device_sort")
    return a


def _share_torch_hip_runtime():
    """PyTorch-ROCm ships its own libamdhip64; libvsg_orb.so links the system one under the same soname.  Whichever
    is loaded first serves both, and torch only finds its GPUs through its own copy -- so when torch is installed its
    copy is loaded here, by path and without importing torch, before libvsg_orb.so resolves the soname.  One HIP
    runtime per process then holds no matter whether `import torch` or this module comes first (streams and device
    pointers are handed between the two, bench.py)."""
    import importlib.util
    import os
    import sys
    if "torch" in sys.modules or os.environ.get("VSG_SYSTEM_HIP"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if not spec or not spec.origin:
        return
    cand = Path(spec.origin).parent / "lib" / "libamdhip64.so"
    if cand.exists():
        try:
            C.CDLL(str(cand), mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library():
    """dlopen libvsg_orb.so (built in-tree by visual_sgraphs_amd.build).  Fails loudly if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -m visual_sgraphs_amd.build` "
                           "(the ORB front-end has no CPU fallback)")
    _share_torch_hip_runtime()
    L = C.CDLL(str(LIB_PATH))
    L.vsg_last_error.restype = C.c_char_p
    L.vsg_orb_create.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.vsg_orb_destroy.argtypes = [C.c_void_p]
    L.vsg_orb_destroy.restype = None
    L.vsg_orb_get_tables.argtypes = [C.c_void_p, _f32p, _f32p, _f32p, _f32p, _i32p, _i32p]
    L.vsg_orb_set_blur_taps.argtypes = [C.c_void_p, _u16p]
    L.vsg_orb_capacity.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.vsg_orb_set_pyramid_tiling.argtypes = [C.c_void_p, C.c_int]
    L.vsg_orb_set_fast_form.argtypes = [C.c_void_p, C.c_int]
    L.vsg_orb_extract.argtypes = [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, _u8p,
                                  C.c_int, _i32p]
    L.vsg_orb_extract_batch.argtypes = [C.c_void_p, _u8p, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_void_p, _u8p, C.c_int, _i32p, _i32p]
    L.vsg_orb_extract_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                               C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                               C.c_void_p]
    L.vsg_orb_level_size.argtypes = [C.c_void_p, C.c_int, _i32p, _i32p]
    L.vsg_orb_copy_pyramid_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _u8p, C.c_int]
    L.vsg_orb_copy_blurred_level.argtypes = [C.c_void_p, C.c_int, C.c_int, _u8p, C.c_int]
    L.vsg_orb_copy_candidates.argtypes = [C.c_void_p, C.c_int, C.c_int, _u32p, C.c_int]
    L.vsg_orb_copy_selected.argtypes = [C.c_void_p, C.c_int, C.c_int, _u32p, C.c_int]
    L.vsg_orb_enable_timing.argtypes = [C.c_void_p, C.c_int]
    L.vsg_orb_get_timing.argtypes = [C.c_void_p, _f32p, C.c_int]
    L.vsg_orb_set_serialize.argtypes = [C.c_void_p, C.c_int]
    L.vsg_hamming_pairs.argtypes = [C.c_int, _u8p, C.c_int, _u8p, C.c_int, _i32p, _i32p, C.c_int, _i32p]
    L.vsg_hamming_block_best2.argtypes = [C.c_int, _u8p, C.c_int, _u8p, C.c_int, _i32p, _i32p, _i32p]
    L.vsg_hamming_block_best2_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                 C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]
    L.vsg_search_by_bow_kf_f.argtypes = [C.c_int, _u8p, _f32p, _u8p, C.c_int, _i32p, _i32p, _i32p, C.c_int,
                                         _u8p, _f32p, C.c_int, _i32p, _i32p, _i32p, C.c_int, C.c_float, C.c_int, _i32p]
    L.vsg_search_by_bow_kf_f_stereo.argtypes = [C.c_int, _u8p, _f32p, _u8p, C.c_int, _i32p, _i32p, _i32p, C.c_int,
                                                _u8p, _f32p, C.c_int, C.c_int, _i32p, _i32p, _i32p, C.c_int, C.c_float,
                                                C.c_int, _i32p]
    L.vsg_search_by_bow_kf_kf.argtypes = [C.c_int, _u8p, _f32p, _u8p, C.c_int, _i32p, _i32p, _i32p, C.c_int,
                                          _u8p, _f32p, _u8p, C.c_int, _i32p, _i32p, _i32p, C.c_int, C.c_float,
                                          C.c_int, _i32p]
    L.vsg_search_for_triangulation.argtypes = [C.c_int, _u8p, _f32p, _u8p, C.c_int, _i32p, _i32p, _i32p, C.c_int,
                                               _u8p, _f32p, _u8p, C.c_int, _i32p, _i32p, _i32p, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_int, _i32p]
    L.vsg_search_by_projection_last.argtypes = [C.c_int, _u8p, _f32p, _u8p, C.c_int, _i32p, _i32p, _u8p, _f32p, _u8p,
                                                C.c_int, C.c_int, C.c_int, _i32p]
    L.vsg_search_by_projection_local.argtypes = [C.c_int, _u8p, _u8p, C.c_int, _i32p, _i32p, _u8p, _i32p, _u8p,
                                                 C.c_int, C.c_float, _i32p]
    L.vsg_search_for_initialization.argtypes = [C.c_int, _u8p, _f32p, _i32p, C.c_int, _i32p, _i32p, _u8p, _f32p,
                                                C.c_int, C.c_float, C.c_int, _i32p]
    L.vsg_search_window.argtypes = [C.c_int, _u8p, _u8p, C.c_int, _i32p, _i32p, _u8p, _u8p, C.c_int, C.c_int, _i32p,
                                    _i32p, _i32p]
    L.vsg_stereo_matches.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, _u8p, C.c_int, C.c_void_p,
                                     _u8p, C.c_int, C.c_float, C.c_float, _f32p, _f32p]
    L.vsg_orb_set_gray_coeffs.argtypes = [C.c_void_p, _i32p, C.c_int]
    L.vsg_orb_extract_batch_device_color.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t,
                                                     C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.vsg_orb_extract_batch_color.argtypes = [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int,
                                              C.c_int, C.c_int, C.c_int, C.c_void_p, _u8p, C.c_int, _i32p, _i32p]
    _f64p = C.POINTER(C.c_double)
    L.vsg_vocab_load.argtypes = [C.c_int, _u8p, C.c_size_t, C.POINTER(C.c_void_p)]
    L.vsg_vocab_destroy.argtypes = [C.c_void_p]
    L.vsg_vocab_destroy.restype = None
    L.vsg_vocab_info.argtypes = [C.c_void_p] + [_i32p] * 6
    L.vsg_bow_transform.argtypes = [C.c_void_p, _u8p, C.c_int, C.c_int, _i32p, _f64p, C.c_int, _i32p, _i32p, _i32p,
                                    _i32p, C.c_int, _i32p, _i32p, _i32p, _f64p]
    L.vsg_distinctive_descriptors.argtypes = [C.c_int, _u8p, _i32p, C.c_int, _i32p]
    L.vsg_grid_build.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                                 C.POINTER(C.c_void_p)]
    L.vsg_grid_destroy.argtypes = [C.c_void_p]
    L.vsg_grid_destroy.restype = None
    L.vsg_grid_query.argtypes = [C.c_void_p, _f32p, _f32p, _f32p, _i32p, _i32p, C.c_int, _i32p, _i32p, C.c_int]
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    L.vsg_thread_arena_growths.argtypes = [ci]
    L.vsg_orb_time_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), ci]
    L.vsg_host_register.argtypes = [vp, C.c_size_t]
    L.vsg_host_unregister.argtypes = [vp]
    L.vsg_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    L.vsg_host_free.argtypes = [vp]
    L.vsg_host_kind.argtypes = [vp, C.c_size_t]
    L.vsg_orb_set_direct_registered.argtypes = [vp, ci]
    L.vsg_orb_slots.argtypes = [vp]
    L.vsg_debug_last_launch_forms.argtypes = [vp, C.POINTER(_LaunchForms)]
    L.vsg_orb_submit_batch.argtypes = [vp, vp, ci, C.c_size_t, ci, ci, ci, ci, ci, vp, vp, ci]
    L.vsg_orb_wait.argtypes = [vp, ci, _i32p, _i32p]
    L.vsg_orb_copy_pyramid.argtypes = [vp, ci, _u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.vsg_frame_create.argtypes = [ci, ci, C.POINTER(vp)]
    L.vsg_frame_destroy.argtypes = [vp]
    L.vsg_frame_destroy.restype = None
    L.vsg_frame_upload.argtypes = [vp, vp, _u8p, _f32p, ci, ci, cf, cf, cf, cf]
    L.vsg_frame_from_extractor.argtypes = [vp, vp, ci, vp, ci, cf, cf, cf, cf]
    L.vsg_frame_from_extractor_undistort.argtypes = [vp, vp, ci, vp, ci, _f32p, _f32p, ci, cf, cf, cf, cf, vp]
    L.vsg_camera_image_bounds.argtypes = [ci, ci, _f32p, _f32p, ci, _f32p]
    L.vsg_orb_extract_to_frame.argtypes = [vp, _u8p, ci, ci, ci, ci, ci, vp, _u8p, ci, _i32p, vp, _f32p, _f32p, ci, cf, cf,
                                           cf, cf, vp]
    L.vsg_orb_extract_to_frame_rgbd.argtypes = [vp, _u8p, ci, ci, ci, ci, ci, vp, _u8p, ci, _i32p, vp, _f32p, _f32p, ci,
                                                cf, cf, cf, cf, vp, vp, ci, C.c_size_t, ci, ci, cf, cf, _f32p, _f32p]
    L.vsg_depth_map_scale.argtypes = [cf]
    L.vsg_depth_map_scale.restype = cf
    L.vsg_rgbd_depth_batch_device.argtypes = [ci, vp, ci, ci, C.c_size_t, C.c_size_t, ci, ci, cf, cf, _f32p, _f32p, ci,
                                              vp, vp, ci, vp, vp, vp]
    L.vsg_frame_size.argtypes = [vp]
    L.vsg_frame_copy_grid.argtypes = [vp, ci, _i32p, _i32p]
    L.vsg_frame_features_in_area.argtypes = [vp, _f32p, _f32p, _f32p, _i32p, _i32p, ci, ci, _i32p, _i32p, ci]
    L.vsg_frame_search_by_projection.argtypes = [vp, ci, _u8p, _u8p, _u8p, _f32p, _f32p, _f32p, _i32p, _f32p, _u8p,
                                                 _f32p, _f32p, _i32p, _f32p, cf, cf, _f32p, ci, _i32p, _i32p, _u8p,
                                                 _i32p]
    L.vsg_frame_search_by_projection_last.argtypes = [vp, ci, _u8p, _u8p, _f32p, _f32p, _f32p, _f32p, _f32p, _i32p,
                                                      _f32p, cf, ci, _f32p, ci, ci, _u8p, _i32p]
    L.vsg_frame_search_by_projection_sim3.argtypes = [vp, ci, _u8p, _f32p, _f32p, _f32p, _i32p, cf, _i32p]
    L.vsg_frame_search_by_projection_kf.argtypes = [vp, ci, _u8p, _f32p, _f32p, _f32p, _i32p, _f32p, ci, ci, _u8p,
                                                    _i32p]
    L.vsg_frame_search_by_sim3.argtypes = [vp, vp, ci, _i32p, _u8p, _f32p, _f32p, _f32p, _i32p, ci, _i32p, _u8p, _f32p,
                                           _f32p, _f32p, _i32p, _i32p]
    L.vsg_frame_fuse.argtypes = [vp, ci, _u8p, _f32p, _f32p, _f32p, _f32p, _i32p, ci, _f32p, ci, _i32p, _i32p]
    L.vsg_frame_fuse_sim3.argtypes = [vp, ci, _u8p, _f32p, _f32p, _f32p, _i32p, _i32p, _i32p]
    L.vsg_fuse_decide.argtypes = [ci, _i32p, _i32p, _i32p, ci, _i32p, ci, _i32p, _u8p, ci, _i32p, _i32p]
    L.vsg_frame_search_for_initialization.argtypes = [vp, vp, _f32p, _f32p, ci, cf, ci, _i32p]
    L.vsg_frame_search_by_bow_kf_f.argtypes = [vp, _u8p, _i32p, _i32p, _i32p, ci, vp, _i32p, _i32p, _i32p, ci, cf, ci,
                                               _i32p]
    L.vsg_frame_search_by_bow_kf_kf.argtypes = [vp, _u8p, _i32p, _i32p, _i32p, ci, vp, _u8p, _i32p, _i32p, _i32p, ci,
                                                cf, ci, _i32p]
    L.vsg_frame_search_for_triangulation.argtypes = [vp, _u8p, _i32p, _i32p, _i32p, ci, vp, _u8p, _i32p, _i32p, _i32p,
                                                     ci, vp, vp, ci, _i32p]
    L.vsg_frame_search_for_triangulation_epipolar.argtypes = [vp, _u8p, _i32p, _i32p, _i32p, ci, vp, _u8p, _i32p, _i32p,
                                                              _i32p, ci, _f32p, _f32p, _f32p, _f32p, ci, ci, ci, ci, _i32p]
    L.vsg_debug_epipolar_pairs.argtypes = [vp, vp, ci, _i32p, _i32p, _f32p, _f32p, _f32p, _f32p, ci, ci, ci, _u8p]
    L.vsg_frame_bow_transform.argtypes = [vp, vp, ci, _i32p, _f64p, ci, _i32p, _i32p, _i32p, _i32p, ci, _i32p, _i32p,
                                          _i32p, _f64p]
    L.vsg_frame_stereo_matches.argtypes = [vp, ci, vp, ci, vp, vp, cf, cf, _f32p, _f32p]
    L.vsg_frame_stereo_bow_search.argtypes = [vp, ci, vp, ci, vp, vp, cf, cf, _f32p, _f32p, _i32p, vp, ci, _i32p, _f64p, ci,
                                              _i32p, _i32p, _i32p, _i32p, ci, _i32p, vp, _u8p, cf, ci, _i32p, _i32p]
    L.vsg_shard_last_error.restype = C.c_char_p
    L.vsg_shard_record_bytes.restype = C.c_size_t
    L.vsg_shard_record_bytes.argtypes = [ci]
    L.vsg_shard_record_desc_offset.restype = C.c_size_t
    L.vsg_shard_record_desc_offset.argtypes = [ci]
    L.vsg_shard_frame_owner.argtypes = [ci, ci]
    L.vsg_shard_stream_owner.argtypes = [ci, ci, ci, ci]
    L.vsg_shard_unique_id.argtypes = [_u8p]
    L.vsg_shard_create.argtypes = [ci, ci, ci, _u8p, ci, ci, C.POINTER(vp)]
    L.vsg_shard_destroy.argtypes = [vp]
    L.vsg_shard_destroy.restype = None
    L.vsg_shard_all_gather.argtypes = [vp, vp, vp, vp, ci, ci, vp]
    L.vsg_shard_record.argtypes = [vp, ci, ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.vsg_shard_world.argtypes = [vp]
    L.vsg_shard_rank.argtypes = [vp]
    L.vsg_shard_send_recv_boundary.argtypes = [vp, vp, vp, vp, ci, ci, vp]
    L.vsg_shard_boundary_record.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.vsg_copy_d2d_async.argtypes = [ci, vp, vp, C.c_size_t, vp]
    u64, i32 = C.c_uint64, C.c_int32
    _u64p = C.POINTER(C.c_uint64)
    L.vsg_vocab_score.argtypes = [vp, _i32p, _f64p, ci, _i32p, _i32p, _f64p, ci, _f64p]
    L.vsg_mappoints_create.argtypes = [ci, ci, C.POINTER(vp)]
    L.vsg_mappoints_destroy.argtypes = [vp]
    L.vsg_mappoints_destroy.restype = None
    L.vsg_mappoints_capacity.argtypes = [vp]
    L.vsg_mappoints_update.argtypes = [vp, ci, _i32p, _f32p, _f32p, _f32p, _f32p, _u8p, _u8p]
    L.vsg_mappoints_read.argtypes = [vp, ci, _i32p, _f32p, _f32p, _f32p, _f32p, _u8p, _u8p]
    L.vsg_mappoints_refresh_from_observations.argtypes = [vp, ci, _i32p, _i32p, _i32p, _i32p, _u8p, _i32p, ci, C.POINTER(vp),
                                                          _f32p, _f32p, ci, ci, _i32p, _f32p, _f32p, _f32p]
    L.vsg_frame_is_in_frustum.argtypes = [vp, vp, ci, _i32p, C.POINTER(FramePose), cf, _u8p, _f32p, _f32p, _f32p, _f32p,
                                          _i32p, _f32p]
    L.vsg_frame_search_local_points.argtypes = [vp, vp, ci, _i32p, _u8p, C.POINTER(FramePose), cf, cf, cf, ci, cf, _f32p,
                                                ci, _u8p, _i32p, _u8p, _f32p, _f32p, C.POINTER(ci)]
    L.vsg_frame_search_last_frame.argtypes = [vp, vp, vp, _i32p, C.POINTER(FramePose), C.POINTER(FramePose), cf, ci, cf,
                                              _f32p, ci, ci, _u8p, _i32p, C.POINTER(ci), _u8p, _f32p, _f32p, _f32p]
    L.vsg_frame_search_keyframe_points.argtypes = [vp, vp, ci, _i32p, _u8p, C.POINTER(FramePose), cf, ci, _f32p, ci, ci,
                                                   _f32p, _u8p, _i32p, _u8p, _f32p, _f32p, _i32p]
    L.vsg_frame_fuse_points.argtypes = [vp, vp, ci, _i32p, _u8p, C.POINTER(FramePose), cf, _f32p, _f32p, ci, _i32p, _i32p,
                                        _u8p, _f32p, _f32p, _f32p, _i32p]
    L.vsg_frame_fuse_points_sim3.argtypes = [vp, vp, ci, _i32p, _u8p, C.POINTER(FramePose), cf, _f32p, ci, _i32p, _i32p,
                                             _u8p, _f32p, _f32p, _i32p]
    L.vsg_frame_search_sim3_points.argtypes = [vp, vp, ci, _i32p, _u8p, C.POINTER(FramePose), cf, cf, _f32p, ci, _i32p,
                                               _u8p, _f32p, _f32p, _i32p]
    L.vsg_frame_pose_optimization.argtypes = [vp, vp, _i32p, C.POINTER(PoseSE3), cf, cf, cf, cf, cf, _f32p, ci, ci, _u8p,
                                              _f32p, C.POINTER(PoseResult)]
    L.vsg_frame_pose_optimization_resume.argtypes = [vp, _u8p, _u8p, _f32p, C.POINTER(PoseResult)]
    L.vsg_frame_track_with_motion_model.argtypes = [vp, vp, vp, _i32p, C.POINTER(FramePose), C.POINTER(FramePose), cf, ci,
                                                    cf, _f32p, ci, ci, C.POINTER(PoseSE3), _f32p, ci, _i32p, _i32p, _u8p,
                                                    _f32p, C.POINTER(TrackResult)]
    L.vsg_frame_track_local_map.argtypes = [vp, vp, ci, _i32p, _u8p, C.POINTER(FramePose), cf, cf, cf, ci, cf, _f32p, ci,
                                            _i32p, C.POINTER(PoseSE3), _f32p, ci, ci, ci, _i32p, _i32p, _u8p, _f32p, _u8p,
                                            _f32p, _f32p, C.POINTER(TrackLocalResult)]
    tri_tail = [C.POINTER(TriangulationParams), _f32p, _f32p, _f32p, _f32p, ci, vp, _i32p, ci]
    tri_outs = [_u8p, _u8p, _f32p, _i32p, _i32p]
    L.vsg_frame_set_stereo_points.argtypes = [vp, _f32p, _f32p]
    L.vsg_frame_triangulate_matches.argtypes = [vp, vp, _i32p] + tri_tail + tri_outs
    L.vsg_frame_create_new_map_points.argtypes = [vp, _u8p, _i32p, _i32p, _i32p, ci, vp, _u8p, _i32p, _i32p, _i32p, ci, _f32p,
                                                  _f32p, ci, ci, ci] + tri_tail + [_i32p] + tri_outs
    L.vsg_mappoints_sim3_ransac.argtypes = [vp, vp, ci, _i32p, _i32p, _f32p, _f32p, C.POINTER(FramePose), C.POINTER(FramePose),
                                            ci, ci, ci, _i32p, _u8p, C.POINTER(Sim3Result), _i32p, _f32p]
    L.vsg_sim3_ransac_iterations.argtypes = [C.c_double, ci, ci, ci]
    L.vsg_frame_optimize_sim3.argtypes = [vp, vp, vp, vp, _i32p, _i32p, _i32p, _i32p, C.POINTER(FramePose), C.POINTER(FramePose),
                                          _f32p, _f32p, ci, C.POINTER(Sim3d), cf, ci, ci, _u8p, _f64p, C.POINTER(Sim3OptResult)]
    L.vsg_sim3_draw_samples.argtypes = [ci, ci, _RANDOM_INT, vp, _i32p]
    tv_tail = [_i32p, _f32p, C.POINTER(TwoViewParams), ci, _i32p, C.POINTER(TwoViewResult), _u8p, _f32p, _u8p, _u8p, _f32p, _f32p]
    L.vsg_frame_two_view_reconstruct.argtypes = [vp, vp] + tv_tail
    L.vsg_two_view_reconstruct.argtypes = [ci, _f32p, ci, _f32p, ci] + tv_tail
    L.vsg_two_view_default_params.argtypes = [C.POINTER(TwoViewParams)]
    L.vsg_two_view_default_params.restype = None
    L.vsg_two_view_draw_sets.argtypes = [ci, ci, _RANDOM_INT, vp, _i32p]
    L.vsg_frame_mlpnp_ransac.argtypes = [vp, vp, _i32p, cf, cf, cf, cf, _f32p, ci, cf, ci, ci, ci, ci, ci, _i32p, _u8p,
                                         C.POINTER(MlpnpResult), _i32p, _f64p]
    L.vsg_mlpnp_ransac_parameters.argtypes = [C.c_double, ci, ci, ci, cf, ci, _i32p, _i32p]
    L.vsg_mlpnp_draw_sets.argtypes = [ci, ci, _RANDOM_INT, vp, _i32p]
    L.vsg_mappoints_local_bundle_adjustment.argtypes = [vp, ci, _i32p, _i32p, _i32p, _i32p, ci, C.POINTER(vp), C.POINTER(PoseSE3),
                                                        _u8p, C.POINTER(BaCamera), _f32p, ci, ci, _u8p, C.POINTER(PoseSE3d),
                                                        _f32p, _u8p, _f64p, C.POINTER(LocalBaResult)]
    L.vsg_mappoints_local_bundle_adjustment_sgraph.argtypes = L.vsg_mappoints_local_bundle_adjustment.argtypes[:-1] + [
        ci, _f64p, _i32p, _i32p, _f64p, _f64p, _f64p, _f64p, ci, _f64p, _i32p, _i32p, _f64p, _f64p, _u8p, _f64p, _f64p,
        C.POINTER(SGraphLocalBaResult)]
    L.vsg_debug_local_ba_trial_slots.argtypes = [ci]
    L.vsg_mappoints_global_bundle_adjustment.argtypes = [vp, ci, _i32p, _i32p, _i32p, _i32p, ci, C.POINTER(vp), C.POINTER(PoseSE3),
                                                         _u8p, C.POINTER(BaCamera), _f32p, ci, ci, ci, ci, _u8p,
                                                         C.POINTER(PoseSE3d), _f32p, _u8p, _f64p, C.POINTER(GlobalBaResult)]
    L.vsg_mappoints_optimize_essential_graph.argtypes = [vp, ci, C.POINTER(Sim3d), C.POINTER(Sim3d), _u8p, _u8p, ci, _i32p, _i32p,
                                                         _u8p, ci, ci, ci, _i32p, _i32p, C.POINTER(Sim3d), _f32p, _f64p,
                                                         C.POINTER(EssentialGraphResult)]
    L.vsg_mappoints_correct_sim3.argtypes = [vp, ci, _i32p, _i32p, ci, C.POINTER(Sim3d), C.POINTER(Sim3d), _f32p]
    L.vsg_debug_ba_reduced_solve.argtypes = [ci, _f64p, _f64p, _f64p, _i32p]
    L.vsg_debug_ba_solver_geometry.argtypes = [_i32p, _i32p]
    L.vsg_kfdb_create.argtypes = [vp, C.POINTER(vp)]
    L.vsg_kfdb_destroy.argtypes = [vp]
    L.vsg_kfdb_destroy.restype = None
    L.vsg_kfdb_add.argtypes = [vp, u64, i32, _i32p, _f64p, ci]
    L.vsg_kfdb_erase.argtypes = [vp, u64]
    L.vsg_kfdb_clear.argtypes = [vp]
    L.vsg_kfdb_clear_map.argtypes = [vp, i32]
    L.vsg_kfdb_set_map.argtypes = [vp, _u64p, _i32p, ci]
    L.vsg_kfdb_set_covisibility.argtypes = [vp, _u64p, _i32p, _u64p, ci]
    L.vsg_kfdb_detect_relocalization_candidates.argtypes = [vp, u64, _i32p, _f64p, ci, i32, _u64p, ci, _i32p]
    L.vsg_kfdb_detect_n_best_candidates.argtypes = [vp, u64, _i32p, _f64p, ci, _u64p, ci, i32, _i32p, ci, ci, _u64p,
                                                    _i32p, _u64p, _i32p]
    L.vsg_debug_kfdb_state.argtypes = [vp, u64, _u64p, _i32p, _f32p]
    L.vsg_debug_track_walk.argtypes = [ci, ci, ci, ci, _u32p, _i32p, _i32p, ci, _u8p, _u8p, _u8p, _f32p, _f32p, _i32p, _i32p,
                                       _u8p, ci, ci, ci, cf, _i32p, _u8p, _i32p, _u8p, _i32p, _i32p, _i32p]
    _lib = L
    return L


def optimize_essential_graph(L, store_handle, kf_Scw, kf_non_corrected, kf_has_non_corrected, kf_fixed, edge_i, edge_j, edge_loop,
                             fix_scale, slots=(), point_ref=(), iterations=20):
    """Optimizer::OptimizeEssentialGraph, first overload (Optimizer.cc:2456-2734; vsg_mappoints_optimize_essential_graph).
    kf_Scw (K, 8) float64 = vScw per keyframe in ascending mnId (q x y z w, t, s): CorrectedSim3 where present, else
    (GetPose(), 1); kf_non_corrected (K, 8) with kf_has_non_corrected (K) = NonCorrectedSim3; kf_fixed (K) != 0 for the map's
    initial keyframe.  Edge e joins vertex 0 = edge_i[e] and vertex 1 = edge_j[e]; edge_loop[e] != 0 for a loop-connection
    edge.  slots / point_ref: the map points to correct and nIDr as a keyframe index; store_handle None with no points runs
    the pose graph alone.  Returns dict(kf_Scw (K, 8), world_pos (n, 3) float32, chi2 per edge and the fields of
    vsg_essential_graph_result).  At most 438 keyframes that are not fixed and have an edge (a dense solve)."""
    S = np.ascontiguousarray(kf_Scw, np.float64).reshape(-1, 8)
    K = S.shape[0]
    N = np.ascontiguousarray(kf_non_corrected, np.float64).reshape(-1, 8)
    has, fx = _u8(kf_has_non_corrected), _u8(kf_fixed)
    ei, ej, el = _i32(edge_i), _i32(edge_j), _u8(edge_loop)
    E, n = int(np.asarray(edge_i).size), int(np.asarray(slots).size)
    sl, ref = _i32(slots), _i32(point_ref)
    if N.shape[0] != K or has.size != K or fx.size != K or np.asarray(edge_j).size != E or np.asarray(edge_loop).size != E or \
            np.asarray(point_ref).size != n:
        raise ValueError("the keyframe, edge or point arrays differ in length")
    out = {"kf_Scw": np.zeros((max(K, 1), 8), np.float64), "world_pos": np.zeros((max(n, 1), 3), np.float32),
           "chi2": np.zeros(max(E, 1), np.float64)}
    res = EssentialGraphResult()
    f64p = C.POINTER(C.c_double)
    _check(L.vsg_mappoints_optimize_essential_graph(
        store_handle, K, C.cast(_p(S, f64p), C.POINTER(Sim3d)), C.cast(_p(N, f64p), C.POINTER(Sim3d)), _p(has, _u8p), _p(fx, _u8p),
        E, _p(ei, _i32p), _p(ej, _i32p), _p(el, _u8p), int(bool(fix_scale)), int(iterations), n, _p(sl, _i32p), _p(ref, _i32p),
        C.cast(_p(out["kf_Scw"], f64p), C.POINTER(Sim3d)), _p(out["world_pos"], _f32p), _p(out["chi2"], f64p), C.byref(res)),
        "vsg_mappoints_optimize_essential_graph")
    got = {"kf_Scw": out["kf_Scw"][:K], "world_pos": out["world_pos"][:n], "chi2": out["chi2"][:E]}
    got.update({k: int(getattr(res, k)) for k in ESSENTIAL_GRAPH_RESULT_INTS if k != "pad"})
    got.update({k: float(getattr(res, k)) for k in ESSENTIAL_GRAPH_RESULT_DOUBLES})
    return got


def _check(rc, where):
    if rc < 0:
        raise VsgError(rc, where, load_library().vsg_last_error().decode(errors="replace"))
    return rc


def device_count():
    return load_library().vsg_device_count()


def _p(a, t):
    return a.ctypes.data_as(t)


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a if a.size else np.zeros(1, np.int32)


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a if a.size else np.zeros(1, np.float32)


class ORBextractor:
    """VS_GRAPHS::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST) on one MI355X."""

    STAGES = ("pyramid", "fast", "octree", "blur", "slots", "orient_desc", "total")

    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device=0, max_batch=1):
        self._L = load_library()
        self._h = C.c_void_p()
        _check(self._L.vsg_orb_create(int(nfeatures), float(scaleFactor), int(nlevels), int(iniThFAST), int(minThFAST),
                                      int(device), int(max_batch), C.byref(self._h)), "vsg_orb_create")
        self.nfeatures, self.nlevels, self.scaleFactor = int(nfeatures), int(nlevels), float(np.float32(scaleFactor))
        self.device, self.max_batch = int(device), int(max_batch)
        self._shape = None

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.vsg_orb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # ---- getters (ORBextractor.h:63-91)
    def _tables(self):
        n = self.nlevels
        out = [np.zeros(n, np.float32) for _ in range(4)] + [np.zeros(n, np.int32), np.zeros(16, np.int32)]
        self._L.vsg_orb_get_tables(self._h, _p(out[0], _f32p), _p(out[1], _f32p), _p(out[2], _f32p), _p(out[3], _f32p),
                                   _p(out[4], _i32p), _p(out[5], _i32p))
        return out

    def GetLevels(self):
        return self.nlevels

    def GetScaleFactor(self):
        return self.scaleFactor

    def GetScaleFactors(self):
        return self._tables()[0]

    def GetInverseScaleFactors(self):
        return self._tables()[1]

    def GetScaleSigmaSquares(self):
        return self._tables()[2]

    def GetInverseScaleSigmaSquares(self):
        return self._tables()[3]

    def features_per_level(self):
        return self._tables()[4]

    def umax(self):
        return self._tables()[5]

    def set_blur_taps(self, taps):
        t = np.ascontiguousarray(taps, dtype=np.uint16)
        assert t.shape == (7,)
        _check(self._L.vsg_orb_set_blur_taps(self._h, _p(t, _u16p)), "vsg_orb_set_blur_taps")

    def set_pyramid_tiling(self, which):
        """ComputePyramid's launch form: -1 automatic (default), 0 / 1 / 2 the fused tilings (32 / 36 / 16 px), 3 one launch
        per level."""
        _check(self._L.vsg_orb_set_pyramid_tiling(self._h, int(which)), "vsg_orb_set_pyramid_tiling")

    def set_fast_form(self, which):
        """k_fast_cells' launch form: -1 automatic (default), 0 the general form (every geometry)."""
        _check(self._L.vsg_orb_set_fast_form(self._h, int(which)), "vsg_orb_set_fast_form")

    def set_direct_registered(self, on=True):
        """Opt in to in-place device access of hipHostRegister-ed caller memory (`pin()`); by default such memory is staged
        like pageable memory and only vsg_host_alloc / hipHostMalloc memory (`PinnedArray`) is touched in place."""
        _check(self._L.vsg_orb_set_direct_registered(self._h, int(on)), "vsg_orb_set_direct_registered")

    def capacity(self, rows, cols):
        return _check(self._L.vsg_orb_capacity(self._h, int(rows), int(cols)), "vsg_orb_capacity")

    # ---- operator() (ORBextractor.h:59-61).  mask is ignored, like the reference (ORBextractor.h:58).
    def __call__(self, image, mask=None, vLappingArea=(0, 0)):
        """Returns (monoIndex, keypoints[KP_DTYPE], descriptors[n,32] uint8); monoIndex == -1 for an empty image."""
        if image is None or image.size == 0:
            return -1, np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)
        img = np.asarray(image)
        assert img.dtype == np.uint8 and img.ndim == 2, "CV_8UC1 expected (ORBextractor.cc:1091)"
        if img.strides[1] != 1:
            img = np.ascontiguousarray(img)
        rows, cols = img.shape
        cap = self.capacity(rows, cols)
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int32(0)
        mono = self._L.vsg_orb_extract(self._h, _p(img, _u8p), rows, cols, img.strides[0], int(vLappingArea[0]),
                                       int(vLappingArea[1]), kps.ctypes.data_as(C.c_void_p), _p(desc, _u8p), cap,
                                       C.byref(n))
        _check(mono, "vsg_orb_extract")
        self._shape = (rows, cols)
        return mono, kps[:n.value].copy(), desc[:n.value].copy()

    def extract_batch(self, images, vLappingArea=(0, 0)):
        """images: [B,H,W] uint8.  Returns list of (monoIndex, keypoints, descriptors)."""
        imgs = np.ascontiguousarray(images, dtype=np.uint8)
        assert imgs.ndim == 3 and imgs.shape[0] <= self.max_batch
        B, rows, cols = imgs.shape
        cap = self.capacity(rows, cols)
        kps = np.zeros((B, cap), KP_DTYPE)
        desc = np.zeros((B, cap, 32), np.uint8)
        n = np.zeros(B, np.int32)
        mono = np.zeros(B, np.int32)
        _check(self._L.vsg_orb_extract_batch(self._h, _p(imgs, _u8p), B, imgs.strides[0], rows, cols, imgs.strides[1],
                                             int(vLappingArea[0]), int(vLappingArea[1]),
                                             kps.ctypes.data_as(C.c_void_p), _p(desc, _u8p), cap, _p(n, _i32p),
                                             _p(mono, _i32p)), "vsg_orb_extract_batch")
        self._shape = (rows, cols)
        return [(int(mono[i]), kps[i, :n[i]].copy(), desc[i, :n[i]].copy()) for i in range(B)]

    # ---- asynchronous host pipeline (vsg_orb_submit_batch / vsg_orb_wait)
    def slots(self):
        return self._L.vsg_orb_slots(self._h)

    def debug_launch_forms(self):
        """Test hook: the launch forms the last enqueue of this handle took (include/vsg_orb_debug.h), as a dict."""
        f = _LaunchForms()
        _check(self._L.vsg_debug_last_launch_forms(self._h, C.byref(f)), "vsg_debug_last_launch_forms")
        return {n: int(getattr(f, n)) for n in LAUNCH_FORM_FIELDS}

    def submit_batch(self, images, kps_out, desc_out, vLappingArea=(0, 0)):
        """images [B,H,W] uint8 (pinned via `pin()` => DMA straight from it), kps_out [B,cap] KP_DTYPE, desc_out
        [B,cap,32] uint8 (pinned => the device writes them directly).  Returns a ticket for wait()."""
        assert images.dtype == np.uint8 and images.ndim == 3 and images.strides[2] == 1
        B, rows, cols = images.shape
        cap = kps_out.shape[1]
        assert kps_out.dtype == KP_DTYPE and kps_out.flags.c_contiguous and desc_out.flags.c_contiguous
        t = _check(self._L.vsg_orb_submit_batch(self._h, C.c_void_p(images.ctypes.data), B, images.strides[0], rows, cols,
                                                images.strides[1], int(vLappingArea[0]), int(vLappingArea[1]),
                                                C.c_void_p(kps_out.ctypes.data), C.c_void_p(desc_out.ctypes.data), cap),
                   "vsg_orb_submit_batch")
        self._shape = (rows, cols)
        self._inflight = getattr(self, "_inflight", {})
        self._inflight[t] = (B, images, kps_out, desc_out)  # keep the buffers alive until the wait
        return t

    def wait(self, ticket):
        """Blocks until the batch of `ticket` is complete.  Returns (n[B], monoIndex[B])."""
        B = self._inflight[ticket][0]
        n, mono = np.zeros(B, np.int32), np.zeros(B, np.int32)
        _check(self._L.vsg_orb_wait(self._h, int(ticket), _p(n, _i32p), _p(mono, _i32p)), "vsg_orb_wait")
        del self._inflight[ticket]
        return n, mono

    def copy_pyramid(self, frame=0):
        """mvImagePyramid of one frame in ONE D2H: list of bordered levels ((h+38) x (w+38) uint8 views)."""
        offs = (C.c_size_t * self.nlevels)()
        need = _check(self._L.vsg_orb_copy_pyramid(self._h, frame, None, 0, offs), "vsg_orb_copy_pyramid")
        buf = np.zeros(need, np.uint8)
        _check(self._L.vsg_orb_copy_pyramid(self._h, frame, _p(buf, _u8p), need, offs), "vsg_orb_copy_pyramid")
        out = []
        for l in range(self.nlevels):
            w, h = self.level_size(l)
            out.append(buf[offs[l]:offs[l] + (w + 38) * (h + 38)].reshape(h + 38, w + 38))
        return out

    def extract_batch_device(self, d_gray, nframes, frame_stride, rows, cols, stride, d_kps, d_desc, d_counts, capacity,
                             vLappingArea=(0, 0), stream=None):
        """Raw device-pointer entry (ints / torch .data_ptr()); asynchronous on `stream`."""
        _check(self._L.vsg_orb_extract_batch_device(self._h, C.c_void_p(d_gray), int(nframes), int(frame_stride),
                                                    int(rows), int(cols), int(stride), int(vLappingArea[0]),
                                                    int(vLappingArea[1]), C.c_void_p(d_kps), C.c_void_p(d_desc),
                                                    C.c_void_p(d_counts), int(capacity),
                                                    C.c_void_p(stream) if stream else None),
               "vsg_orb_extract_batch_device")
        self._shape = (rows, cols)

    def set_gray_coeffs(self, coeffs, shift):
        c = np.ascontiguousarray(coeffs, dtype=np.int32)
        _check(self._L.vsg_orb_set_gray_coeffs(self._h, _p(c, _i32p), int(shift)), "vsg_orb_set_gray_coeffs")

    def extract_batch_color(self, images, rgb_order=True, vLappingArea=(0, 0)):
        """images: [B,H,W,3|4] uint8 colour frames (Tracking::mbRGB = rgb_order).  Returns [(mono, kps, desc)]."""
        imgs = np.ascontiguousarray(images, dtype=np.uint8)
        assert imgs.ndim == 4 and imgs.shape[3] in (3, 4) and imgs.shape[0] <= self.max_batch
        B, rows, cols, ch = imgs.shape
        cap = self.capacity(rows, cols)
        kps = np.zeros((B, cap), KP_DTYPE)
        desc = np.zeros((B, cap, 32), np.uint8)
        n, mono = np.zeros(B, np.int32), np.zeros(B, np.int32)
        _check(self._L.vsg_orb_extract_batch_color(self._h, _p(imgs, _u8p), ch, int(rgb_order), B, imgs.strides[0],
                                                   rows, cols, imgs.strides[1], int(vLappingArea[0]),
                                                   int(vLappingArea[1]), kps.ctypes.data_as(C.c_void_p),
                                                   _p(desc, _u8p), cap, _p(n, _i32p), _p(mono, _i32p)),
               "vsg_orb_extract_batch_color")
        self._shape = (rows, cols)
        return [(int(mono[i]), kps[i, :n[i]].copy(), desc[i, :n[i]].copy()) for i in range(B)]

    def extract_batch_device_color(self, d_img, channels, rgb_order, nframes, frame_stride, rows, cols, stride, d_kps,
                                   d_desc, d_counts, capacity, vLappingArea=(0, 0), stream=None):
        """Interleaved 8-bit RGB(A)/BGR(A) frames on the device: cvtColor fused into the level-0 staging."""
        _check(self._L.vsg_orb_extract_batch_device_color(
            self._h, C.c_void_p(d_img), int(channels), int(rgb_order), int(nframes), int(frame_stride), int(rows),
            int(cols), int(stride), int(vLappingArea[0]), int(vLappingArea[1]), C.c_void_p(d_kps), C.c_void_p(d_desc),
            C.c_void_p(d_counts), int(capacity), C.c_void_p(stream) if stream else None),
            "vsg_orb_extract_batch_device_color")
        self._shape = (rows, cols)

    # ---- mvImagePyramid and stage read-back
    def level_size(self, level):
        w, h = C.c_int32(), C.c_int32()
        _check(self._L.vsg_orb_level_size(self._h, level, C.byref(w), C.byref(h)), "vsg_orb_level_size")
        return w.value, h.value

    def image_pyramid(self, level, frame=0, with_border=False):
        w, h = self.level_size(level)
        if with_border:
            w, h = w + 38, h + 38
        out = np.zeros((h, w), np.uint8)
        _check(self._L.vsg_orb_copy_pyramid_level(self._h, frame, level, int(with_border), _p(out, _u8p), w),
               "vsg_orb_copy_pyramid_level")
        return out

    def blurred_level(self, level, frame=0):
        w, h = self.level_size(level)
        out = np.zeros((h, w), np.uint8)
        _check(self._L.vsg_orb_copy_blurred_level(self._h, frame, level, _p(out, _u8p), w), "vsg_orb_copy_blurred_level")
        return out

    @staticmethod
    def _unpack(p):
        return (p & 0xFFF).astype(np.int32), ((p >> 12) & 0xFFF).astype(np.int32), (p >> 24).astype(np.int32)

    def candidates(self, level, frame=0):
        cap = 1 << 18
        buf = np.zeros(cap, np.uint32)
        n = _check(self._L.vsg_orb_copy_candidates(self._h, frame, level, _p(buf, _u32p), cap), "vsg_orb_copy_candidates")
        return self._unpack(buf[:n])

    def selected(self, level, frame=0):
        cap = 1 << 16
        buf = np.zeros(cap, np.uint32)
        n = _check(self._L.vsg_orb_copy_selected(self._h, frame, level, _p(buf, _u32p), cap), "vsg_orb_copy_selected")
        return self._unpack(buf[:n])

    def time_stats(self, reset=False):
        """REGISTER_TIMES analogue: (calls, mean_ms, std_ms) of the blocking operator() calls so far."""
        m, sd = C.c_double(), C.c_double()
        n = _check(self._L.vsg_orb_time_stats(self._h, C.byref(m), C.byref(sd), int(reset)), "vsg_orb_time_stats")
        return n, m.value, sd.value

    def set_serialize(self, on=True):
        _check(self._L.vsg_orb_set_serialize(self._h, int(on)), "vsg_orb_set_serialize")

    def enable_timing(self, on=True):
        _check(self._L.vsg_orb_enable_timing(self._h, int(on)), "vsg_orb_enable_timing")

    def timing_ms(self):
        out = np.zeros(len(self.STAGES), np.float32)
        self._L.vsg_orb_get_timing(self._h, _p(out, _f32p), len(out))
        return dict(zip(self.STAGES, out.tolist()))


class ORBmatcher:
    """VS_GRAPHS::ORBmatcher(nnratio=0.6, checkOri=true) on flattened arrays (ORBmatcher.h:37)."""

    TH_HIGH = 100
    TH_LOW = 50
    HISTO_LENGTH = 30

    def __init__(self, nnratio=0.6, checkOri=True, device=0):
        self._L = load_library()
        self.mfNNratio = float(np.float32(nnratio))
        self.mbCheckOrientation = bool(checkOri)
        self.device = int(device)

    @staticmethod
    def DescriptorDistance(a, b, device=0):
        """ORBmatcher::DescriptorDistance (ORBmatcher.cc:2047-2063).  One pair is eight popcounts: host arithmetic
        (a kernel launch would cost four orders of magnitude more); [n,32] arrays go row-wise through the device."""
        if np.ndim(a) == 1:
            x = np.bitwise_xor(_u8(a), _u8(b))
            return int(np.unpackbits(x).sum())
        a2, b2 = np.atleast_2d(_u8(a)), np.atleast_2d(_u8(b))
        n = len(a2)
        idx = np.arange(n, dtype=np.int32)
        out = np.zeros(n, np.int32)
        _check(load_library().vsg_hamming_pairs(device, _p(a2, _u8p), n, _p(b2, _u8p), len(b2), _p(idx, _i32p),
                                                _p(idx, _i32p), n, _p(out, _i32p)), "vsg_hamming_pairs")
        return out

    def hamming_pairs(self, a, b, ia, ib):
        a, b, ia, ib = _u8(a), _u8(b), _i32(ia), _i32(ib)
        n = 0 if len(a) == 0 or len(b) == 0 else len(ia)
        out = np.zeros(n, np.int32)
        if n:
            _check(self._L.vsg_hamming_pairs(self.device, _p(a, _u8p), len(a), _p(b, _u8p), len(b), _p(ia, _i32p),
                                             _p(ib, _i32p), n, _p(out, _i32p)), "vsg_hamming_pairs")
        return out

    def block_best2(self, a, b):
        a, b = _u8(a).reshape(-1, 32), _u8(b).reshape(-1, 32)
        best, second, arg = (np.zeros(len(a), np.int32) for _ in range(3))
        if len(a):
            bb = b if len(b) else np.zeros((1, 32), np.uint8)
            _check(self._L.vsg_hamming_block_best2(self.device, _p(a, _u8p), len(a), _p(bb, _u8p), len(b),
                                                   _p(best, _i32p), _p(second, _i32p), _p(arg, _i32p)),
                   "vsg_hamming_block_best2")
        return best, second, arg

    def SearchByBoW_KF_F(self, kf_desc, kf_angle, kf_valid, kf_fv, f_desc, f_angle, f_fv, f_nleft=-1):
        """SearchByBoW(KeyFrame*, Frame&, ...).  fv = (node_ids, offsets, indices); f_nleft = F.Nleft (fisheye
        stereo: right-camera features start there).  Returns (nmatches, matchF)."""
        kd, fd = _u8(kf_desc).reshape(-1, 32), _u8(f_desc).reshape(-1, 32)
        ka, fa, kv = _f32(kf_angle), _f32(f_angle), _u8(kf_valid)
        kn, ko, ki = (_i32(x) for x in kf_fv)
        fn, fo, fi = (_i32(x) for x in f_fv)
        out = np.full(max(len(fd), 1), -1, np.int32)
        n = _check(self._L.vsg_search_by_bow_kf_f_stereo(
            self.device, _p(kd, _u8p), _p(ka, _f32p), _p(kv, _u8p), len(kd), _p(kn, _i32p), _p(ko, _i32p),
            _p(ki, _i32p), len(kf_fv[0]), _p(fd, _u8p), _p(fa, _f32p), len(fd), int(f_nleft), _p(fn, _i32p),
            _p(fo, _i32p), _p(fi, _i32p), len(f_fv[0]), self.mfNNratio, int(self.mbCheckOrientation),
            _p(out, _i32p)), "vsg_search_by_bow_kf_f_stereo")
        return n, out[:len(fd)]

    def SearchByBoW_KF_KF(self, d1, a1, v1, fv1, d2, a2, v2, fv2):
        d1, d2 = _u8(d1).reshape(-1, 32), _u8(d2).reshape(-1, 32)
        a1, a2, v1, v2 = _f32(a1), _f32(a2), _u8(v1), _u8(v2)
        n1, o1, i1 = (_i32(x) for x in fv1)
        n2, o2, i2 = (_i32(x) for x in fv2)
        out = np.full(max(len(d1), 1), -1, np.int32)
        n = _check(self._L.vsg_search_by_bow_kf_kf(self.device, _p(d1, _u8p), _p(a1, _f32p), _p(v1, _u8p), len(d1),
                                                   _p(n1, _i32p), _p(o1, _i32p), _p(i1, _i32p), len(fv1[0]),
                                                   _p(d2, _u8p), _p(a2, _f32p), _p(v2, _u8p), len(d2), _p(n2, _i32p),
                                                   _p(o2, _i32p), _p(i2, _i32p), len(fv2[0]), self.mfNNratio,
                                                   int(self.mbCheckOrientation), _p(out, _i32p)),
                   "vsg_search_by_bow_kf_kf")
        return n, out[:len(d1)]

    def SearchForTriangulation(self, d1, a1, eligible1, fv1, d2, a2, eligible2, fv2, pair_ok=None, pair_off=None):
        """ORBmatcher::SearchForTriangulation (ORBmatcher.cc:902-1146) on flattened views; pair_ok / pair_off carry
        the adaptor-evaluated geometric predicate per pair of every shared node (see include/vsg_orb.h).
        Returns (nmatches, matches12)."""
        d1, d2 = _u8(d1).reshape(-1, 32), _u8(d2).reshape(-1, 32)
        a1, a2, e1, e2 = _f32(a1), _f32(a2), _u8(eligible1), _u8(eligible2)
        n1, o1, i1 = (_i32(x) for x in fv1)
        n2, o2, i2 = (_i32(x) for x in fv2)
        ok = np.ascontiguousarray(pair_ok, np.uint32) if pair_ok is not None else None
        po = _i32(pair_off) if pair_ok is not None else None
        out = np.full(max(len(d1), 1), -1, np.int32)
        n = _check(self._L.vsg_search_for_triangulation(
            self.device, _p(d1, _u8p), _p(a1, _f32p), _p(e1, _u8p), len(d1), _p(n1, _i32p), _p(o1, _i32p),
            _p(i1, _i32p), len(fv1[0]), _p(d2, _u8p), _p(a2, _f32p), _p(e2, _u8p), len(d2), _p(n2, _i32p),
            _p(o2, _i32p), _p(i2, _i32p), len(fv2[0]), ok.ctypes.data if ok is not None else None,
            po.ctypes.data if po is not None else None, int(self.mbCheckOrientation), _p(out, _i32p)),
            "vsg_search_for_triangulation")
        return n, out[:len(d1)]

    def SearchByProjection_Last(self, q_desc, q_angle, q_blocks, cand_off, cand_idx, t_desc, t_angle, t_blocked,
                                th_high=TH_HIGH):
        qd, td = _u8(q_desc).reshape(-1, 32), _u8(t_desc).reshape(-1, 32)
        qa, ta, qb = _f32(q_angle), _f32(t_angle), _u8(q_blocks)
        co, ci = _i32(cand_off), _i32(cand_idx)
        tb = _u8(t_blocked).copy()
        tm = np.full(max(len(td), 1), -1, np.int32)
        n = _check(self._L.vsg_search_by_projection_last(self.device, _p(qd, _u8p), _p(qa, _f32p), _p(qb, _u8p),
                                                         len(qd), _p(co, _i32p), _p(ci, _i32p), _p(td, _u8p),
                                                         _p(ta, _f32p), _p(tb, _u8p), len(td), int(th_high),
                                                         int(self.mbCheckOrientation), _p(tm, _i32p)),
                   "vsg_search_by_projection_last")
        return n, tm[:len(td)], tb

    def SearchByProjection_Local(self, q_desc, q_blocks, cand_off, cand_idx, t_desc, t_octave, t_blocked):
        qd, td = _u8(q_desc).reshape(-1, 32), _u8(t_desc).reshape(-1, 32)
        qb, to = _u8(q_blocks), _i32(t_octave)
        co, ci = _i32(cand_off), _i32(cand_idx)
        tb = _u8(t_blocked).copy()
        tm = np.full(max(len(td), 1), -1, np.int32)
        n = _check(self._L.vsg_search_by_projection_local(self.device, _p(qd, _u8p), _p(qb, _u8p), len(qd),
                                                          _p(co, _i32p), _p(ci, _i32p), _p(td, _u8p), _p(to, _i32p),
                                                          _p(tb, _u8p), len(td), self.mfNNratio, _p(tm, _i32p)),
                   "vsg_search_by_projection_local")
        return n, tm[:len(td)], tb

    def SearchForInitialization(self, d1, a1, oct1, cand_off, cand_idx, d2, a2):
        d1, d2 = _u8(d1).reshape(-1, 32), _u8(d2).reshape(-1, 32)
        a1, a2, o1 = _f32(a1), _f32(a2), _i32(oct1)
        co, ci = _i32(cand_off), _i32(cand_idx)
        out = np.full(max(len(d1), 1), -1, np.int32)
        n = _check(self._L.vsg_search_for_initialization(self.device, _p(d1, _u8p), _p(a1, _f32p), _p(o1, _i32p),
                                                         len(d1), _p(co, _i32p), _p(ci, _i32p), _p(d2, _u8p),
                                                         _p(a2, _f32p), len(d2), self.mfNNratio,
                                                         int(self.mbCheckOrientation), _p(out, _i32p)),
                   "vsg_search_for_initialization")
        return n, out[:len(d1)]


class FrameGrid:
    """Frame::AssignFeaturesToGrid + GetFeaturesInArea on the device (Frame.cc:521-553, 802-880)."""

    def __init__(self, kps, min_x, min_y, max_x, max_y, device=0):
        self._L = load_library()
        self._kps = np.ascontiguousarray(kps, dtype=KP_DTYPE)
        self._h = C.c_void_p()
        _check(self._L.vsg_grid_build(int(device), self._kps.ctypes.data_as(C.c_void_p), len(self._kps), float(min_x),
                                      float(min_y), float(max_x), float(max_y), C.byref(self._h)), "vsg_grid_build")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.vsg_grid_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def GetFeaturesInArea(self, x, y, r, minLevel=None, maxLevel=None):
        """Batched query.  Returns (cand_off[nq+1], cand_idx) in the reference's candidate order."""
        x, y, r = _f32(np.atleast_1d(x)), _f32(np.atleast_1d(y)), _f32(np.atleast_1d(r))
        nq = len(x)
        lo = _i32(np.atleast_1d(minLevel)) if minLevel is not None else None
        hi = _i32(np.atleast_1d(maxLevel)) if maxLevel is not None else None
        off = np.zeros(nq + 1, np.int32)
        cap = max(1, 64 * nq)
        while True:
            idx = np.zeros(cap, np.int32)
            total = _check(self._L.vsg_grid_query(self._h, _p(x, _f32p), _p(y, _f32p), _p(r, _f32p),
                                                  _p(lo, _i32p) if lo is not None else None,
                                                  _p(hi, _i32p) if hi is not None else None, nq, _p(off, _i32p),
                                                  _p(idx, _i32p), cap), "vsg_grid_query")
            if total <= cap:
                return off, idx[:total]
            cap = total


def search_window(q_desc, q_blocks, cand_off, cand_idx, t_desc, t_blocked, th_high, device=0):
    """vsg_search_window.  Returns (nmatches, q_best_idx, q_best_dist, train_match, train_blocked)."""
    qd, td = _u8(q_desc).reshape(-1, 32), _u8(t_desc).reshape(-1, 32)
    co, ci = _i32(cand_off), _i32(cand_idx)
    qb = _u8(q_blocks) if q_blocks is not None else None
    tb = _u8(t_blocked).copy() if t_blocked is not None else None
    qi, qdist = np.zeros(max(len(qd), 1), np.int32), np.zeros(max(len(qd), 1), np.int32)
    tm = np.full(max(len(td), 1), -1, np.int32)
    n = _check(load_library().vsg_search_window(int(device), _p(qd, _u8p), _p(qb, _u8p) if qb is not None else None,
                                                len(qd), _p(co, _i32p), _p(ci, _i32p), _p(td, _u8p),
                                                _p(tb, _u8p) if tb is not None else None, len(td), int(th_high),
                                                _p(qi, _i32p), _p(qdist, _i32p), _p(tm, _i32p)), "vsg_search_window")
    return n, qi[:len(qd)], qdist[:len(qd)], tm[:len(td)], tb


def ComputeStereoMatches(ex_left, frame_l, ex_right, frame_r, kps_l, desc_l, kps_r, desc_r, mb, mbf):
    """Frame::ComputeStereoMatches (Frame.cc:957-1127).  Returns (mvuRight, mvDepth)."""
    kl, kr = np.ascontiguousarray(kps_l, KP_DTYPE), np.ascontiguousarray(kps_r, KP_DTYPE)
    dl, dr = _u8(desc_l).reshape(-1, 32), _u8(desc_r).reshape(-1, 32)
    ur, dep = np.zeros(max(len(kl), 1), np.float32), np.zeros(max(len(kl), 1), np.float32)
    _check(load_library().vsg_stereo_matches(ex_left.handle, int(frame_l), ex_right.handle, int(frame_r),
                                             kl.ctypes.data_as(C.c_void_p), _p(dl, _u8p), len(kl),
                                             kr.ctypes.data_as(C.c_void_p), _p(dr, _u8p), len(kr), float(mb), float(mbf),
                                             _p(ur, _f32p), _p(dep, _f32p)), "vsg_stereo_matches")
    return ur[:len(kl)], dep[:len(kl)]


class ORBVocabulary:
    """DBoW2 ORBVocabulary on the device: loadFromBinFile image + transform (TemplatedVocabulary.h)."""

    def __init__(self, blob, device=0):
        self._L = load_library()
        b = np.frombuffer(blob, dtype=np.uint8).copy()
        self._h = C.c_void_p()
        _check(self._L.vsg_vocab_load(int(device), _p(b, _u8p), len(b), C.byref(self._h)), "vsg_vocab_load")
        v = [C.c_int32() for _ in range(6)]
        self._L.vsg_vocab_info(self._h, *[C.byref(x) for x in v])
        self.k, self.L, self.scoring, self.weighting, self.nnodes, self.nwords = [x.value for x in v]

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.vsg_vocab_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def transform(self, desc, levelsup=4):
        """Returns dict(bow_ids, bow_vals, fv=(node_ids, offsets, indices), word, node, weight)."""
        d = _u8(desc).reshape(-1, 32)
        n = len(d)
        cap = n + 1
        bi, bv = np.zeros(cap, np.int32), np.zeros(cap, np.float64)
        fn, fo, fi = np.zeros(cap, np.int32), np.zeros(cap + 1, np.int32), np.zeros(cap, np.int32)
        w_of, n_of, wt = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
        nb, nf = C.c_int32(), C.c_int32()
        f64p = C.POINTER(C.c_double)
        _check(self._L.vsg_bow_transform(self._h, _p(d, _u8p), n, int(levelsup), _p(bi, _i32p), _p(bv, f64p), cap,
                                         C.byref(nb), _p(fn, _i32p), _p(fo, _i32p), _p(fi, _i32p), cap, C.byref(nf),
                                         _p(w_of, _i32p), _p(n_of, _i32p), _p(wt, f64p)), "vsg_bow_transform")
        return dict(bow_ids=bi[:nb.value].copy(), bow_vals=bv[:nb.value].copy(),
                    fv=(fn[:nf.value].copy(), fo[:nf.value + 1].copy(), fi[:fo[nf.value]].copy()),
                    word=w_of[:n].copy(), node=n_of[:n].copy(), weight=wt[:n].copy())


    def score(self, a, b):
        """TemplatedVocabulary::score(a, b) (TemplatedVocabulary.h:1214-1219): a and b are BowVectors as (ids, vals)
        pairs or transform() dicts.  KL scoring raises VSG_ERR_UNSUPPORTED."""
        return float(self.score_many(a, [b])[0])

    def score_many(self, a, bs):
        """score(a, b) for every BowVector b of `bs`: float64 array, bit-identical to the reference's doubles."""
        qi, qv = _bow_arrays(a)
        vs = [_bow_arrays(b) for b in bs]
        off = np.zeros(len(vs) + 1, np.int32)
        off[1:] = np.cumsum([len(i) for i, _ in vs]) if vs else []
        ids = np.concatenate([i for i, _ in vs] + [np.zeros(1, np.int32)]).astype(np.int32)
        vals = np.concatenate([v for _, v in vs] + [np.zeros(1, np.float64)]).astype(np.float64)
        out = np.zeros(max(len(vs), 1), np.float64)
        f64p = C.POINTER(C.c_double)
        _check(self._L.vsg_vocab_score(self._h, _p(qi, _i32p), _p(qv, f64p), len(qi) if qi.size else 0, _p(off, _i32p),
                                       _p(ids, _i32p), _p(vals, f64p), len(vs), _p(out, f64p)), "vsg_vocab_score")
        return out[:len(vs)]


def _bow_arrays(b):
    """(ids int32, vals float64) of a BowVector given as a transform() dict or an (ids, vals) pair; the arrays have at
    least one element (n is passed separately)."""
    if isinstance(b, dict):
        b = (b["bow_ids"], b["bow_vals"])
    ids = np.ascontiguousarray(b[0], dtype=np.int32).reshape(-1)
    vals = np.ascontiguousarray(b[1], dtype=np.float64).reshape(-1)
    if len(ids) != len(vals):
        raise ValueError("BowVector ids and values differ in length")
    return ids, vals


class KeyFrameDatabase:
    """VS_GRAPHS::KeyFrameDatabase (orb_slam3/include/KeyFrameDatabase.h) resident on the device (vsg_kfdb_*).

    Keyframes are the caller's integer ids (KeyFrame::mnId), maps integer ids (KeyFrame::GetMap()).  BowVectors are
    (ids, vals) pairs or ORBVocabulary.transform() dicts.  The caller mirrors what the reference reads from KeyFrame:
    the map (add / set_map) and GetBestCovisibilityKeyFrames(10) (set_covisibility)."""

    def __init__(self, voc):
        self._L = load_library()
        self._voc = voc  # the vocabulary outlives the database
        self._h = C.c_void_p()
        self._seen = set()  # every keyframe id given to the database (bounds the candidates of a query)
        _check(self._L.vsg_kfdb_create(voc._h, C.byref(self._h)), "vsg_kfdb_create")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.vsg_kfdb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, kf_id, bow, map_id=0):
        i, v = _bow_arrays(bow)
        self._seen.add(int(kf_id))
        _check(self._L.vsg_kfdb_add(self._h, int(kf_id), int(map_id), _p(i, _i32p), _p(v, C.POINTER(C.c_double)), len(i)),
               "vsg_kfdb_add")

    def erase(self, kf_id):
        _check(self._L.vsg_kfdb_erase(self._h, int(kf_id)), "vsg_kfdb_erase")

    def clear(self):
        _check(self._L.vsg_kfdb_clear(self._h), "vsg_kfdb_clear")

    def clearMap(self, map_id):
        _check(self._L.vsg_kfdb_clear_map(self._h, int(map_id)), "vsg_kfdb_clear_map")

    def set_map(self, kf_ids, map_ids):
        k = np.ascontiguousarray(kf_ids, dtype=np.uint64).reshape(-1)
        m = np.ascontiguousarray(map_ids, dtype=np.int32).reshape(-1)
        assert len(k) == len(m)
        self._seen.update(int(x) for x in k)
        if len(k):
            _check(self._L.vsg_kfdb_set_map(self._h, _p(k, C.POINTER(C.c_uint64)), _p(m, _i32p), len(k)), "vsg_kfdb_set_map")

    def set_covisibility(self, neighbours):
        """neighbours: {kf_id: [neighbour ids in GetBestCovisibilityKeyFrames order]} (the first 10 are used)."""
        if not neighbours:
            return
        ids = np.array(list(neighbours.keys()), dtype=np.uint64)
        lists = [list(neighbours[int(k)]) for k in ids]
        off = np.zeros(len(ids) + 1, np.int32)
        off[1:] = np.cumsum([len(x) for x in lists])
        nb = np.array([x for l in lists for x in l] + [0], dtype=np.uint64)
        self._seen.update(int(x) for x in ids)
        self._seen.update(int(x) for l in lists for x in l[:10])
        u64p = C.POINTER(C.c_uint64)
        _check(self._L.vsg_kfdb_set_covisibility(self._h, _p(ids, u64p), _p(off, _i32p), _p(nb, u64p), len(ids)),
               "vsg_kfdb_set_covisibility")

    def DetectRelocalizationCandidates(self, query_id, bow, map_id):
        """KeyFrameDatabase::DetectRelocalizationCandidates(F, pMap): list of keyframe ids, in the reference's order."""
        i, v = _bow_arrays(bow)
        u64p = C.POINTER(C.c_uint64)
        # a query updates the keyframes' query state, so it cannot be repeated with a larger buffer: room for every
        # keyframe id the database has seen
        cap = max(len(self._seen), 1)
        out, n = np.zeros(cap, np.uint64), C.c_int32()
        _check(self._L.vsg_kfdb_detect_relocalization_candidates(self._h, int(query_id), _p(i, _i32p),
                                                                 _p(v, C.POINTER(C.c_double)), len(i), int(map_id),
                                                                 _p(out, u64p), cap, C.byref(n)),
               "vsg_kfdb_detect_relocalization_candidates")
        return [int(x) for x in out[:n.value]]

    def DetectNBestCandidates(self, query_kf_id, bow, connected_ids, map_id, nNumCandidates, bad_map_ids=()):
        """KeyFrameDatabase::DetectNBestCandidates(pKF, vpLoopCand, vpMergeCand, nNumCandidates): (loop, merge) id lists."""
        i, v = _bow_arrays(bow)
        u64p = C.POINTER(C.c_uint64)
        conn = np.array(list(connected_ids) + [0], dtype=np.uint64)
        bad = np.array(list(bad_map_ids) + [0], dtype=np.int32)
        nn = int(nNumCandidates)
        lo, me = np.zeros(max(nn, 1), np.uint64), np.zeros(max(nn, 1), np.uint64)
        nl, nm = C.c_int32(), C.c_int32()
        _check(self._L.vsg_kfdb_detect_n_best_candidates(self._h, int(query_kf_id), _p(i, _i32p),
                                                         _p(v, C.POINTER(C.c_double)), len(i), _p(conn, u64p),
                                                         len(conn) - 1, int(map_id), _p(bad, _i32p), len(bad) - 1, nn,
                                                         _p(lo, u64p), C.byref(nl), _p(me, u64p), C.byref(nm)),
               "vsg_kfdb_detect_n_best_candidates")
        return [int(x) for x in lo[:nl.value]], [int(x) for x in me[:nm.value]]

    def debug_state(self, kf_id):
        """Test hook (include/vsg_orb_debug.h): the six query-state members of keyframe `kf_id` as the device holds
        them: (mnRelocQuery, mnRelocWords, mRelocScore, mnPlaceRecognitionQuery, mnPlaceRecognitionWords,
        mPlaceRecognitionScore), the scores as np.float32.  An id the database never saw raises VSG_ERR_INVALID."""
        q, w, s = (C.c_uint64 * 2)(), (C.c_int32 * 2)(), (C.c_float * 2)()
        _check(self._L.vsg_debug_kfdb_state(self._h, int(kf_id), q, w, s), "vsg_debug_kfdb_state")
        sc = np.frombuffer(s, np.float32)
        return int(q[0]), int(w[0]), sc[0], int(q[1]), int(w[1]), sc[1]


REFRESH_DESC, REFRESH_NORMAL = 1, 2  # include/vsg_orb.h VSG_REFRESH_*


class MapPoints:
    """The local map's MapPoints resident on the device (include/vsg_orb.h: vsg_mappoints): per slot GetWorldPos(),
    GetNormal(), the members mfMinDistance / mfMaxDistance (unscaled: PredictScale divides mfMaxDistance itself),
    GetDescriptor(), Observations() > 0.  Slots are the caller's own index of a MapPoint."""

    def __init__(self, capacity, device=0):
        self._L = load_library()
        self._h = C.c_void_p()
        self.device = int(device)
        _check(self._L.vsg_mappoints_create(self.device, int(capacity), C.byref(self._h)), "vsg_mappoints_create")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.vsg_mappoints_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def capacity(self):
        return self._L.vsg_mappoints_capacity(self._h)

    def update(self, slots, world_pos=None, normal=None, min_dist=None, max_dist=None, desc=None, observed=None):
        """Scatter update of len(slots) slots; a field left None keeps what the slots hold; a slot listed twice takes its
        last entry."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        n = len(sl)

        def f(a, conv, t, width):
            if a is None:
                return None, None
            if np.asarray(a).size != n * width:
                raise ValueError("field length does not match the slot list")
            a = conv(a)
            return a, _p(a, t)
        keep = [f(world_pos, _f32, _f32p, 3), f(normal, _f32, _f32p, 3), f(min_dist, _f32, _f32p, 1),
                f(max_dist, _f32, _f32p, 1), f(desc, _u8, _u8p, 32), f(observed, _u8, _u8p, 1)]
        _check(self._L.vsg_mappoints_update(self._h, n, _p(_i32(sl), _i32p), *[k[1] for k in keep]),
               "vsg_mappoints_update")

    def read(self, slots):
        """dict of the fields of the listed slots (test / debug)."""
        sl = _i32(slots)
        n = len(np.asarray(slots))
        out = {"world_pos": np.zeros((max(n, 1), 3), np.float32), "normal": np.zeros((max(n, 1), 3), np.float32),
               "min_dist": np.zeros(max(n, 1), np.float32), "max_dist": np.zeros(max(n, 1), np.float32),
               "desc": np.zeros((max(n, 1), 32), np.uint8), "observed": np.zeros(max(n, 1), np.uint8)}
        _check(self._L.vsg_mappoints_read(self._h, n, _p(sl, _i32p), _p(out["world_pos"], _f32p), _p(out["normal"], _f32p),
                                          _p(out["min_dist"], _f32p), _p(out["max_dist"], _f32p), _p(out["desc"], _u8p),
                                          _p(out["observed"], _u8p)), "vsg_mappoints_read")
        return {k: v[:n] for k, v in out.items()}

    def refresh(self, slots, obs_off, obs_kf, obs_idx, ref_pos, keyframes, kf_Ow, scale_factors, obs_bad=None,
                what=REFRESH_DESC | REFRESH_NORMAL):
        """MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth of len(slots) points from their
        observation lists (vsg_mappoints_refresh_from_observations): point i has the observations
        [obs_off[i], obs_off[i + 1]) of obs_kf (index into `keyframes`, a list of orb.Frame), obs_idx (leftIndex) and
        obs_bad (pKF->isBad(), None: none); ref_pos[i] = where mpRefKF's observation sits in that list; kf_Ow =
        GetCameraCenter() per keyframe.  Returns dict(best, normal, min_dist, max_dist): best = the chosen observation's
        position in the point's list (-1: descriptor kept), the others = what the slots hold after the call."""
        n, nobs = int(np.asarray(slots).size), int(np.asarray(obs_kf).size)
        sl, off, kf, idx, ref = _i32(slots), _i32(obs_off), _i32(obs_kf), _i32(obs_idx), _i32(ref_pos)
        if np.asarray(obs_off).size != n + 1 or np.asarray(obs_idx).size != nobs or np.asarray(ref_pos).size != n:
            raise ValueError("observation arrays do not match the slot list")
        if nobs < int(off[-1]):
            raise ValueError("obs_off runs past the observation arrays")
        bad = _u8(obs_bad) if obs_bad is not None else None
        if bad is not None and bad.size != nobs:
            raise ValueError("obs_bad does not match the observation arrays")
        ow, sf = _f32(kf_Ow).reshape(-1), _f32(scale_factors)
        if np.asarray(kf_Ow).size != 3 * len(keyframes):
            raise ValueError("kf_Ow needs 3 floats per keyframe")
        handles = (C.c_void_p * max(len(keyframes), 1))(*[f.handle for f in keyframes])
        out = {"best": np.full(max(n, 1), -1, np.int32), "normal": np.zeros((max(n, 1), 3), np.float32),
               "min_dist": np.zeros(max(n, 1), np.float32), "max_dist": np.zeros(max(n, 1), np.float32)}
        _check(self._L.vsg_mappoints_refresh_from_observations(
            self._h, n, _p(sl, _i32p), _p(off, _i32p), _p(kf, _i32p), _p(idx, _i32p),
            _p(bad, _u8p) if bad is not None and nobs else None, _p(ref, _i32p), len(keyframes), handles, _p(ow, _f32p),
            _p(sf, _f32p), int(np.asarray(scale_factors).size), int(what),
            _p(out["best"], _i32p), _p(out["normal"], _f32p), _p(out["min_dist"], _f32p), _p(out["max_dist"], _f32p)),
            "vsg_mappoints_refresh_from_observations")
        return {k: v[:n] for k, v in out.items()}


    def _ba_begin(self, slots, obs_off, obs_kf, obs_idx, keyframes, kf_Tcw, kf_fixed, kf_cam, inv_level_sigma2, iterations, stop_flag):
        """What the three bundle adjustments share of a call, validated: n, K, the number of listed observations, the C
        arguments from the store's handle to `iterations`, the stop flag's pointer, the pointers of the outs kf_Tcw and
        world_pos, and the dict of those two outs and chi2 per observation (each call adds its own)."""
        n, K = int(np.asarray(slots).size), len(keyframes)
        sl, off, kf, idx = _i32(slots), _i32(obs_off), _i32(obs_kf), _i32(obs_idx)
        if np.asarray(obs_off).size != n + 1 or np.asarray(obs_idx).size != np.asarray(obs_kf).size:
            raise ValueError("observation arrays do not match the slot list")
        nobs = int(off[n]) if n else 0
        if int(np.asarray(obs_kf).size) < nobs:
            raise ValueError("obs_off runs past the observation arrays")
        T, fx, cam = _f32(kf_Tcw).reshape(-1), _u8(kf_fixed), _f32(kf_cam).reshape(-1)
        if np.asarray(kf_Tcw).size != 7 * K or np.asarray(kf_fixed).size != K or np.asarray(kf_cam).size != 5 * K:
            raise ValueError("kf_Tcw needs 7 floats, kf_fixed one byte and kf_cam 5 floats per keyframe")
        sig = _f32(inv_level_sigma2)
        handles = (C.c_void_p * max(K, 1))(*[f.handle for f in keyframes])
        out = {"kf_Tcw": np.zeros((max(K, 1), 7), np.float64), "world_pos": np.zeros((max(n, 1), 3), np.float32),
               "chi2": np.zeros(max(nobs, 1), np.float64)}
        head = (self._h, n, _p(sl, _i32p), _p(off, _i32p), _p(kf, _i32p), _p(idx, _i32p), K, handles,
                C.cast(_p(T, _f32p), C.POINTER(PoseSE3)), _p(fx, _u8p), C.cast(_p(cam, _f32p), C.POINTER(BaCamera)), _p(sig, _f32p),
                int(np.asarray(inv_level_sigma2).size), int(iterations))
        outs = (C.cast(_p(out["kf_Tcw"], C.POINTER(C.c_double)), C.POINTER(PoseSE3d)), _p(out["world_pos"], _f32p))
        return n, K, nobs, head, None if stop_flag is None else _p(stop_flag, _u8p), outs, out

    def _ba_finish(self, out, lens, res, ints, doubles, slots, kf_Tcw, restore=()):
        """The result dict of a bundle adjustment: out's arrays cut to `lens`, then res's fields.  A call that did not run
        wrote no pose and no position: those outs are the inputs, and so are the `restore` ones."""
        if not res.ran:
            K, n = lens["kf_Tcw"], lens["world_pos"]
            out["kf_Tcw"][:K] = np.asarray(kf_Tcw, np.float32).reshape(K, 7) if K else 0
            out["world_pos"][:n] = self.read(slots)["world_pos"] if n else 0
            for k, v in restore:
                out[k][:lens[k]] = v[:lens[k]]
        got = {k: out[k][:lens[k]] for k in lens}
        got.update({k: int(getattr(res, k)) for k in ints})
        got.update({k: float(getattr(res, k)) for k in doubles})
        return got

    def LocalBundleAdjustment(self, slots, obs_off, obs_kf, obs_idx, keyframes, kf_Tcw, kf_fixed, kf_cam, inv_level_sigma2,
                              iterations=10, stop_flag=None, trial_slots=0):
        """The visual part of Optimizer::LocalBundleAdjustment (vsg_mappoints_local_bundle_adjustment): point i = slot
        slots[i] with the observations [obs_off[i], obs_off[i + 1]) of obs_kf (index into `keyframes`, a list of resident
        orb.Frame in ascending mnId: the local keyframes AND the fixed ones) and obs_idx (leftIndex), as refresh() takes
        them.  kf_Tcw = (K, 7) floats q (x y z w), t; kf_fixed[k] != 0 for lFixedCameras and the map's initial keyframe;
        kf_cam = (K, 5) fx fy cx cy mbf; inv_level_sigma2 = mvInvLevelSigma2.  stop_flag = None or a uint8 array of one
        element (pbStopFlag).  trial_slots: the test hook's trial slots enqueued ahead (0 = the library's default); the
        result does not depend on it.  Returns dict(kf_Tcw (K, 7) float64, world_pos (n, 3) float32 -- also written into
        the slots -- erase and chi2 per observation, and the fields of vsg_local_ba_result).  Follow with
        refresh(what=REFRESH_NORMAL)."""
        n, K, nobs, head, flag, outs, out = self._ba_begin(slots, obs_off, obs_kf, obs_idx, keyframes, kf_Tcw, kf_fixed, kf_cam,
                                                           inv_level_sigma2, iterations, stop_flag)
        out["erase"] = np.zeros(max(nobs, 1), np.uint8)
        res = LocalBaResult()
        if trial_slots:
            _check(self._L.vsg_debug_local_ba_trial_slots(int(trial_slots)), "vsg_debug_local_ba_trial_slots")
        try:
            _check(self._L.vsg_mappoints_local_bundle_adjustment(
                *head, flag, *outs, _p(out["erase"], _u8p), _p(out["chi2"], C.POINTER(C.c_double)), C.byref(res)),
                "vsg_mappoints_local_bundle_adjustment")
        finally:
            if trial_slots:
                self._L.vsg_debug_local_ba_trial_slots(0)
        return self._ba_finish(out, {"kf_Tcw": K, "world_pos": n, "erase": nobs, "chi2": nobs}, res, LOCAL_BA_RESULT_INTS,
                               LOCAL_BA_RESULT_DOUBLES, slots, kf_Tcw)

    def LocalBundleAdjustmentSGraph(self, slots, obs_off, obs_kf, obs_idx, keyframes, kf_Tcw, kf_fixed, kf_cam, inv_level_sigma2,
                                    plane_eq=(), pl_obs_off=(0,), pl_obs_kf=(), pl_obs_local=(), pl_obs_G=(), w_plane_kf=(),
                                    w_plane_point=(), room_center=(), room_n_walls=(), room_wall=(), iterations=10, stop_flag=None):
        """Optimizer::LocalBundleAdjustment with its planes and rooms (vsg_mappoints_local_bundle_adjustment_sgraph).  The
        first arguments are LocalBundleAdjustment's.  plane_eq = (n_planes, 4) doubles; plane i has the observations
        [pl_obs_off[i], pl_obs_off[i + 1]) of pl_obs_kf (index into `keyframes`), each with pl_obs_local (4), pl_obs_G (4, 4)
        and the two weights confidence * information_gain (0 = that edge is not added).  room_center = (n_rooms, 3),
        room_n_walls = 2 or 4 per room, room_wall = (n_rooms, 4) indices into the planes.  Returns LocalBundleAdjustment's
        dict plus plane_eq (n_planes, 4), room_center (n_rooms, 3), erase_plane, chi2_plane_kf and chi2_plane_point per plane
        observation, and the fields of vsg_sgraph_local_ba_result."""
        f64 = lambda a, per: (lambda v: v if v.size else np.zeros(per, np.float64))(np.ascontiguousarray(a, np.float64).reshape(-1))
        n, K, nobs, head, flag, outs, out = self._ba_begin(slots, obs_off, obs_kf, obs_idx, keyframes, kf_Tcw, kf_fixed, kf_cam,
                                                           inv_level_sigma2, iterations, stop_flag)
        eq, poff, pkf = f64(plane_eq, 4), _i32(pl_obs_off), _i32(pl_obs_kf)
        n_planes, n_rooms = int(np.asarray(plane_eq).size) // 4, int(np.asarray(room_center).size) // 3
        if np.asarray(pl_obs_off).size != n_planes + 1:
            raise ValueError("pl_obs_off needs n_planes + 1 entries")
        npo = int(poff[n_planes])
        loc, G, wk, wp = f64(pl_obs_local, 4), f64(pl_obs_G, 16), f64(w_plane_kf, 1), f64(w_plane_point, 1)
        if min(np.asarray(pl_obs_kf).size, loc.size // 4, G.size // 16, np.asarray(w_plane_kf).size, np.asarray(w_plane_point).size) < npo:
            raise ValueError("pl_obs_off runs past the plane observation arrays")
        rc_, rn, rw = f64(room_center, 3), _i32(room_n_walls), _i32(np.asarray(room_wall, np.int32).reshape(-1))
        if np.asarray(room_n_walls).size != n_rooms or np.asarray(room_wall).size != 4 * n_rooms:
            raise ValueError("room_n_walls needs one entry and room_wall four per room")
        dp = C.POINTER(C.c_double)
        out.update({"erase": np.zeros(max(nobs, 1), np.uint8),
                    "plane_eq": np.zeros((max(n_planes, 1), 4), np.float64), "room_center": np.zeros((max(n_rooms, 1), 3), np.float64),
                    "erase_plane": np.zeros(max(npo, 1), np.uint8), "chi2_plane_kf": np.full(max(npo, 1), np.nan),
                    "chi2_plane_point": np.full(max(npo, 1), np.nan)})
        res = SGraphLocalBaResult()
        _check(self._L.vsg_mappoints_local_bundle_adjustment_sgraph(
            *head, flag, *outs, _p(out["erase"], _u8p), _p(out["chi2"], dp),
            n_planes, _p(eq, dp), _p(poff, _i32p), _p(pkf, _i32p), _p(loc, dp), _p(G, dp), _p(wk, dp), _p(wp, dp),
            n_rooms, _p(rc_, dp), _p(rn, _i32p), _p(rw, _i32p), _p(out["plane_eq"], dp), _p(out["room_center"], dp),
            _p(out["erase_plane"], _u8p), _p(out["chi2_plane_kf"], dp), _p(out["chi2_plane_point"], dp), C.byref(res)),
            "vsg_mappoints_local_bundle_adjustment_sgraph")
        lens = {"kf_Tcw": K, "world_pos": n, "erase": nobs, "chi2": nobs, "plane_eq": n_planes, "room_center": n_rooms,
                "erase_plane": npo, "chi2_plane_kf": npo, "chi2_plane_point": npo}
        got = self._ba_finish(out, lens, res.local, LOCAL_BA_RESULT_INTS, LOCAL_BA_RESULT_DOUBLES, slots, kf_Tcw,
                              restore=(("plane_eq", eq.reshape(-1, 4)), ("room_center", rc_.reshape(-1, 3))))
        got.update({k: int(getattr(res, k)) for k in SGRAPH_LOCAL_BA_RESULT_INTS if k != "reserved"})
        return got

    def GlobalBundleAdjustment(self, slots, obs_off, obs_kf, obs_idx, keyframes, kf_Tcw, kf_fixed, kf_cam, inv_level_sigma2,
                               iterations=10, robust=False, write_store=False, stop_flag=None):
        """The visual part of Optimizer::BundleAdjustment as GlobalBundleAdjustemnt calls it
        (vsg_mappoints_global_bundle_adjustment).  The arguments are LocalBundleAdjustment's with `keyframes` = every
        keyframe of the map in ascending mnId and kf_fixed[k] != 0 for the map's initial keyframe alone.  robust = bRobust
        (Huber with sqrt(5.99) / sqrt(7.815)); iterations = nIterations (20 and robust at CreateInitialMapMonocular, 10 and
        not robust at RunGlobalBundleAdjustment); write_store = the case nLoopKF == the origin keyframe: the positions are
        written into the slots (follow with refresh(what=REFRESH_NORMAL)); otherwise the store is untouched and the
        positions come back in world_pos alone (mPosGBA).  Returns dict(kf_Tcw (K, 7) float64, world_pos (n, 3) float32,
        included (n) uint8 -- 0 for a point with an empty list --, chi2 per observation, and the fields of
        vsg_global_ba_result)."""
        n, K, nobs, head, flag, outs, out = self._ba_begin(slots, obs_off, obs_kf, obs_idx, keyframes, kf_Tcw, kf_fixed, kf_cam,
                                                           inv_level_sigma2, iterations, stop_flag)
        out["included"] = np.zeros(max(n, 1), np.uint8)
        res = GlobalBaResult()
        _check(self._L.vsg_mappoints_global_bundle_adjustment(
            *head, int(bool(robust)), int(bool(write_store)), flag, *outs, _p(out["included"], _u8p),
            _p(out["chi2"], C.POINTER(C.c_double)), C.byref(res)), "vsg_mappoints_global_bundle_adjustment")
        return self._ba_finish(out, {"kf_Tcw": K, "world_pos": n, "included": n, "chi2": nobs}, res, GLOBAL_BA_RESULT_INTS,
                               GLOBAL_BA_RESULT_DOUBLES, slots, kf_Tcw)

    def OptimizeEssentialGraph(self, kf_Scw, kf_non_corrected, kf_has_non_corrected, kf_fixed, edge_i, edge_j, edge_loop,
                               fix_scale, slots=(), point_ref=(), iterations=20):
        """Optimizer::OptimizeEssentialGraph, first overload (vsg_mappoints_optimize_essential_graph): see
        optimize_essential_graph, which this calls with the store's handle."""
        return optimize_essential_graph(self._L, self._h, kf_Scw, kf_non_corrected, kf_has_non_corrected, kf_fixed, edge_i, edge_j,
                                        edge_loop, fix_scale, slots, point_ref, iterations)

    def CorrectSim3(self, slots, point_ref, S_from, S_to_inverse):
        """The point correction of LoopClosing::CorrectLoop (LoopClosing.cc:1060-1064) and Optimizer.cc:2723-2728
        (vsg_mappoints_correct_sim3): slot slots[i] becomes float(S_to_inverse[r].map(S_from[r].map(double(pos)))) with
        r = point_ref[i]; S_from / S_to_inverse are (R, 8) float64 (q x y z w, t, s).  Follow with
        refresh(what=REFRESH_NORMAL).  Returns the new positions, (n, 3) float32."""
        n = int(np.asarray(slots).size)
        sl, ref = _i32(slots), _i32(point_ref)
        a, b = np.ascontiguousarray(S_from, np.float64).reshape(-1, 8), np.ascontiguousarray(S_to_inverse, np.float64).reshape(-1, 8)
        if np.asarray(point_ref).size != n or a.shape != b.shape:
            raise ValueError("slots / point_ref or S_from / S_to_inverse differ in length")
        out = np.zeros((max(n, 1), 3), np.float32)
        f64p = C.POINTER(C.c_double)
        _check(self._L.vsg_mappoints_correct_sim3(self._h, n, _p(sl, _i32p), _p(ref, _i32p), a.shape[0],
                                                  C.cast(_p(a, f64p), C.POINTER(Sim3d)), C.cast(_p(b, f64p), C.POINTER(Sim3d)),
                                                  _p(out, _f32p)), "vsg_mappoints_correct_sim3")
        return out[:n]

    def Sim3Ransac(self, slots1, slots2, max_err1, max_err2, kf1, kf2, samples, min_inliers, fix_scale=False, other=None,
                   per_hypothesis=False):
        """Sim3Solver on resident map points (vsg_mappoints_sim3_ransac): correspondence i = slot slots1[i] of this store
        against slot slots2[i] of `other` (None: this store); max_err1 / 2 = sim3_max_err(...); kf1 / kf2 = FramePose;
        samples = n_hyp x 3 correspondence indices (sim3_draw_samples).  Returns dict(inlier, R12, t12, s12, T12, converged,
        no_more, n_inliers, best_hypothesis, iterations) and, with per_hypothesis, hyp_inliers and hyp_T12."""
        s1, s2, e1, e2 = _i32(slots1), _i32(slots2), _f32(max_err1), _f32(max_err2)
        n = int(np.asarray(slots1).size)
        if any(int(np.asarray(a).size) != n for a in (slots2, max_err1, max_err2)):
            raise ValueError("the correspondence arrays differ in length")
        sm = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 3)
        nh = len(sm)
        inlier, res = np.zeros(max(n, 1), np.uint8), Sim3Result()
        hc = np.zeros(max(nh, 1), np.int32) if per_hypothesis else None
        hT = np.zeros((max(nh, 1), 4, 4), np.float32) if per_hypothesis else None
        _check(self._L.vsg_mappoints_sim3_ransac(
            self._h, (other or self).handle, n, _p(s1, _i32p), _p(s2, _i32p), _p(e1, _f32p), _p(e2, _f32p), C.byref(kf1),
            C.byref(kf2), int(bool(fix_scale)), int(min_inliers), nh, _p(_i32(sm), _i32p), _p(inlier, _u8p), C.byref(res),
            _p(hc, _i32p) if per_hypothesis else None, _p(hT, _f32p) if per_hypothesis else None), "vsg_mappoints_sim3_ransac")
        out = dict(inlier=inlier[:n].astype(bool), R12=np.array(res.R12, np.float32).reshape(3, 3), t12=np.array(res.t12, np.float32),
                   s12=np.float32(res.s12), T12=np.array(res.T12, np.float32).reshape(4, 4), converged=bool(res.converged),
                   no_more=bool(res.no_more), n_inliers=int(res.n_inliers), best_hypothesis=int(res.best_hypothesis),
                   iterations=int(res.iterations), result=res)
        if per_hypothesis:
            out.update(hyp_inliers=hc[:nh], hyp_T12=hT[:nh])
        return out


def debug_ba_solver_geometry():
    """include/vsg_orb_debug_global_ba.h vsg_debug_ba_solver_geometry -> (columns per panel, rows per tile)."""
    panel, tile = C.c_int32(0), C.c_int32(0)
    _check(load_library().vsg_debug_ba_solver_geometry(C.byref(panel), C.byref(tile)), "vsg_debug_ba_solver_geometry")
    return int(panel.value), int(tile.value)


def debug_ba_reduced_solve(M, b):
    """include/vsg_orb_debug_global_ba.h vsg_debug_ba_reduced_solve: the global call's reduced solve on the lower triangle
    of M (n, n) float64 and b (n) on the current device -> (ok, x)."""
    M, b = np.ascontiguousarray(M, np.float64), np.ascontiguousarray(b, np.float64)
    n = int(b.size)
    if M.shape != (n, n):
        raise ValueError("M must be (n, n) for b of n")
    x, ok = np.zeros(max(n, 1), np.float64), C.c_int32(-1)
    dp = C.POINTER(C.c_double)
    _check(load_library().vsg_debug_ba_reduced_solve(n, _p(M, dp), _p(b, dp), _p(x, dp), C.byref(ok)), "vsg_debug_ba_reduced_solve")
    return int(ok.value), x[:n]


WALK_SENTINEL_I32, WALK_SENTINEL_U8 = 0x55555555, 0x55  # what debug_track_walk's outputs hold before the call
# vsg_debug_track_walk's arguments by position (tests replace single ones)
WALK_ARGS = ("form", "nq", "nf", "n_ent", "ent", "off", "cnt", "cap", "q_valid", "observed", "blocked_in", "q_angle", "t_angle",
             "q_slot", "slots_in", "slot_observed", "n_slots", "check_orientation", "min_matches", "nnratio", "train_match",
             "train_blocked", "feat_slots", "feat_observed", "edge_feat", "edge_slot", "status")


def debug_track_walk_args(case, cap=None, min_matches=0, slot_observed=None):
    """The argument list of vsg_debug_track_walk (in the order of WALK_ARGS) for one case dictionary of tests/walk_cases.py,
    the outputs as arrays filled with sentinels, and the input arrays the pointers point into (keep them while calling).
    As the host build of the walk (tests/_walkcore) takes a case: q_valid and the rotation filter belong to one form each."""
    c = case
    nq, nf, local = int(c["nq"]), int(c["nf"]), int(c["form"]) == 1
    keep = []

    def ptr(a, dtype, t):  # None stays NULL, an empty array gets an address
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype)
        keep.append(a if a.size else np.zeros(1, dtype))
        return _p(keep[-1], t)

    i32 = lambda: np.full(max(nf, 1), WALK_SENTINEL_I32, np.int32)
    u8 = lambda: np.full(max(nf, 1), WALK_SENTINEL_U8, np.uint8)
    tm, tb, fs, fo, ef, es = i32(), u8(), i32(), u8(), i32(), i32()
    status = np.full(36, WALK_SENTINEL_I32, np.int32)
    out = dict(tm=tm[:max(nf, 0)], tb=tb[:max(nf, 0)], feat_slots=fs[:max(nf, 0)], feat_observed=fo[:max(nf, 0)],
               edges_feat=ef[:max(nf, 0)], edges_slot=es[:max(nf, 0)], status=status)
    args = [int(c["form"]), nq, nf, int(c["n_ent"]), ptr(c["ent"], np.uint32, _u32p), ptr(c["off"], np.int32, _i32p),
            ptr(c["cnt"], np.int32, _i32p), 0x7FFFFFFF if cap is None else int(cap),
            ptr(c["q_valid"] if local else None, np.uint8, _u8p), ptr(c["observed"], np.uint8, _u8p),
            ptr(c["blocked"], np.uint8, _u8p), ptr(c["q_angle"], np.float32, _f32p), ptr(c["t_angle"], np.float32, _f32p),
            ptr(c["q_slot"], np.int32, _i32p), ptr(c["slots_in"], np.int32, _i32p), ptr(slot_observed, np.uint8, _u8p),
            0 if slot_observed is None else int(np.asarray(slot_observed).size), 0 if local else int(c["check"]),
            int(min_matches), float(c["nnratio"]), _p(tm, _i32p), _p(tb, _u8p), _p(fs, _i32p), _p(fo, _u8p), _p(ef, _i32p),
            _p(es, _i32p), _p(status, _i32p)]
    return args, out, keep


def debug_track_walk(case, cap=None, min_matches=0, slot_observed=None):
    """include/vsg_orb_debug.h vsg_debug_track_walk: k_track_walk alone on one case dictionary of tests/walk_cases.py
    (form, nq, nf, n_ent, ent, off, cnt, q_valid, observed, blocked, q_angle, t_angle, q_slot, slots_in, check, nnratio; an
    absent array is None).  cap: the overflow area's entries (None: no bound, as the host build of the walk takes it);
    slot_observed: the store's observed flags per slot, or None.  Every output starts as a sentinel (WALK_SENTINEL_*), so an
    entry the kernel did not write shows: tm, tb, feat_slots, feat_observed and the raw edge arrays `edges_feat` /
    `edges_slot` have nf entries, edge_feat / edge_slot are their first n_edges.  A refused call raises VsgError with the
    outputs as they are after it in its `outputs`."""
    args, out, keep = debug_track_walk_args(case, cap, min_matches, slot_observed)
    rc = load_library().vsg_debug_track_walk(*args)
    del keep
    if rc < 0:
        e = VsgError(rc, "vsg_debug_track_walk", load_library().vsg_last_error().decode(errors="replace"))
        e.outputs = out
        raise e
    status = out["status"]
    flags = int(status[2])
    n_edges = int(status[1]) if not flags & 1 else 0
    out.update(nmatches=int(status[0]), n_edges=n_edges, flags=flags, rounds=int(status[3]), overflow_sum=int(status[4]),
               bins=status[5:35].copy(), edge_feat=out["edges_feat"][:n_edges].copy(),
               edge_slot=out["edges_slot"][:n_edges].copy())
    return out


def sim3_max_err(level_sigma2, octave):
    """mvnMaxError of Sim3Solver (Sim3Solver.cc:96-97) as the comparison sees it: 9.210 * sigmaSquare, a double, truncated by
    the std::vector<size_t> it is stored in, as a float."""
    t = 9.210 * np.asarray(level_sigma2, np.float32)[np.asarray(octave, np.int64)].astype(np.float64)
    return np.floor(t).astype(np.float32)


def sim3_ransac_iterations(probability, min_inliers, max_iterations, n):
    """Sim3Solver::SetRansacParameters: mRansacMaxIts for n correspondences (host only)."""
    return _check(load_library().vsg_sim3_ransac_iterations(float(probability), int(min_inliers), int(max_iterations), int(n)),
                  "vsg_sim3_ransac_iterations")


def sim3_draw_samples(n, n_hyp, random_int=None):
    """The minimal sets of Sim3Solver::iterate (:242-256) for n_hyp hypotheses over n correspondences: n_hyp x 3 int32.
    random_int(lo, hi) stands for DUtils::Random::RandomInt; None: its formula over the C library's rand() (host only)."""
    out = np.zeros((max(int(n_hyp), 1), 3), np.int32)
    cb = _RANDOM_INT(lambda lo, hi, _ctx: int(random_int(lo, hi))) if random_int is not None else _RANDOM_INT()
    _check(load_library().vsg_sim3_draw_samples(int(n), int(n_hyp), cb, None, _p(out, _i32p)), "vsg_sim3_draw_samples")
    return out[:int(n_hyp)]


def two_view_draw_sets(n, n_iter, random_int=None):
    """mvSets of TwoViewReconstruction::Reconstruct (:82-97) for n_iter iterations over n matches: n_iter x 8 int32.
    random_int(lo, hi) stands for DUtils::Random::RandomInt; None: its formula over the C library's rand() (host only;
    SeedRandOnce(0) stays with the caller)."""
    out = np.zeros((max(int(n_iter), 1), 8), np.int32)
    cb = _RANDOM_INT(lambda lo, hi, _ctx: int(random_int(lo, hi))) if random_int is not None else _RANDOM_INT()
    _check(load_library().vsg_two_view_draw_sets(int(n), int(n_iter), cb, None, _p(out, _i32p)), "vsg_two_view_draw_sets")
    return out[:int(n_iter)]


def mlpnp_ransac_parameters(n, probability=0.99, min_inliers=10, max_iterations=300, min_set=6, epsilon=0.5):
    """MLPnPsolver::SetRansacParameters for n correspondences (the defaults are Tracking.cc:3736's): (mRansacMinInliers,
    mRansacMaxIts) as the solver holds them afterwards (host only)."""
    out = np.zeros(2, np.int32)
    _check(load_library().vsg_mlpnp_ransac_parameters(float(probability), int(min_inliers), int(max_iterations), int(min_set),
                                                      float(epsilon), int(n), _p(out[:1], _i32p), _p(out[1:], _i32p)),
           "vsg_mlpnp_ransac_parameters")
    return int(out[0]), int(out[1])


def mlpnp_draw_sets(n, n_hyp, random_int=None):
    """The minimal sets of MLPnPsolver::iterate (:125-145) for n_hyp hypotheses over n correspondences: n_hyp x 6 int32.
    random_int(lo, hi) stands for DUtils::Random::RandomInt; None: its formula over the C library's rand() (host only)."""
    out = np.zeros((max(int(n_hyp), 1), 6), np.int32)
    cb = _RANDOM_INT(lambda lo, hi, _ctx: int(random_int(lo, hi))) if random_int is not None else _RANDOM_INT()
    _check(load_library().vsg_mlpnp_draw_sets(int(n), int(n_hyp), cb, None, _p(out, _i32p)), "vsg_mlpnp_draw_sets")
    return out[:int(n_hyp)]


class TwoViewReconstruction:
    """TwoViewReconstruction(k, sigma, iterations) (TwoViewReconstruction.cc:31-38) with Reconstruct on the device: every
    homography and fundamental-matrix hypothesis, the selection, the motion hypotheses and CheckRT in one enqueue and one wait
    (vsg_frame_two_view_reconstruct / vsg_two_view_reconstruct)."""

    def __init__(self, K, sigma=1.0, iterations=200, device=0):
        self._L = load_library()
        self.K = np.ascontiguousarray(K, np.float32).reshape(3, 3)
        self.params = TwoViewParams()
        self._L.vsg_two_view_default_params(C.byref(self.params))
        self.params.sigma = float(sigma)
        self.iterations, self.device = int(iterations), int(device)

    def Reconstruct(self, keys1, keys2, matches12, sets=None, random_int=None, x3d=None, per_hypothesis=False):
        """keys1 / keys2: two resident Frames, or two [n, 2] arrays of undistorted keypoint coordinates.  matches12 =
        vMatches12.  sets: n_iter x 8 indices into the compacted matches (None: drawn as the reference draws them, through
        random_int).  x3d: the caller's vP3D [n1, 3] (None: zeros) -- left as it is unless the call succeeds from F.  Returns
        dict(ok, reason, model, R21, t21, x3d, triangulated, SH, SF, best_it_h, best_it_f, H21, F21, n_good, parallax,
        n_inliers) and, with per_hypothesis, inlier_h, inlier_f, score_h, score_f."""
        m12 = _i32(matches12)
        resident = isinstance(keys1, Frame)
        n_matches = int((np.asarray(matches12) >= 0).sum())
        if sets is None:
            sets = two_view_draw_sets(n_matches, self.iterations, random_int)
        st = np.ascontiguousarray(sets, np.int32).reshape(-1, 8)
        n1 = keys1.N if resident else len(np.asarray(keys1).reshape(-1, 2))
        if int(np.asarray(matches12).size) != n1:
            raise ValueError("matches12 has not one entry per keypoint of the first frame")
        tri, res = np.zeros(max(n1, 1), np.uint8), TwoViewResult()
        pts = np.zeros((max(n1, 1), 3), np.float32) if x3d is None else np.ascontiguousarray(x3d, np.float32).reshape(-1, 3).copy()
        if len(pts) < n1:
            raise ValueError("x3d is shorter than the first frame")
        opt = [None] * 4
        if per_hypothesis:
            opt = [np.zeros(max(n_matches, 1), np.uint8), np.zeros(max(n_matches, 1), np.uint8),
                   np.zeros(max(len(st), 1), np.float32), np.zeros(max(len(st), 1), np.float32)]
        tail = (_p(m12, _i32p), _p(self.K, _f32p), C.byref(self.params), len(st), _p(_i32(st), _i32p), C.byref(res),
                _p(tri, _u8p), _p(pts, _f32p), *[None if a is None else _p(a, _u8p if a.dtype == np.uint8 else _f32p) for a in opt])
        if resident:
            _check(self._L.vsg_frame_two_view_reconstruct(keys1.handle, keys2.handle, *tail), "vsg_frame_two_view_reconstruct")
        else:
            a, b = _f32(np.asarray(keys1).reshape(-1, 2)), _f32(np.asarray(keys2).reshape(-1, 2))
            _check(self._L.vsg_two_view_reconstruct(self.device, _p(a, _f32p), n1, _p(b, _f32p), len(np.asarray(keys2).reshape(-1, 2)),
                                                    *tail), "vsg_two_view_reconstruct")
        out = dict(ok=bool(res.ok), reason=int(res.reason), model=int(res.model), R21=np.array(res.R21, np.float32).reshape(3, 3),
                   t21=np.array(res.t21, np.float32), x3d=pts[:n1], triangulated=tri[:n1].astype(bool), SH=np.float32(res.SH),
                   SF=np.float32(res.SF), best_it_h=int(res.best_it_h), best_it_f=int(res.best_it_f),
                   H21=np.array(res.H21, np.float32).reshape(3, 3), F21=np.array(res.F21, np.float32).reshape(3, 3),
                   n_good=np.array(res.n_good, np.int32), parallax=np.float32(res.parallax), n_inliers=int(res.n_inliers), result=res)
        if per_hypothesis:
            out.update(inlier_h=opt[0][:n_matches].astype(bool), inlier_f=opt[1][:n_matches].astype(bool), score_h=opt[2][:len(st)],
                       score_f=opt[3][:len(st)])
        return out


def ComputeDistinctiveDescriptors(desc, off, device=0):
    """MapPoint::ComputeDistinctiveDescriptors for many map points: returns the chosen row index per group."""
    d, o = _u8(desc).reshape(-1, 32), _i32(off)
    if len(d) == 0:
        d = np.zeros((1, 32), np.uint8)
    best = np.zeros(max(len(o) - 1, 1), np.int32)
    _check(load_library().vsg_distinctive_descriptors(int(device), _p(d, _u8p), _p(o, _i32p), len(o) - 1,
                                                      _p(best, _i32p)), "vsg_distinctive_descriptors")
    return best[:len(o) - 1]


HOST_KINDS = {0: "pageable", 1: "vsg_host_alloc", 2: "hipHostMalloc", 3: "registered"}


def host_kind(array):
    """How the library classifies the whole memory range of a (contiguous) numpy array: one of HOST_KINDS' values."""
    a = np.asarray(array)
    return HOST_KINDS[_check(load_library().vsg_host_kind(C.c_void_p(a.ctypes.data), max(a.nbytes, 1)), "vsg_host_kind")]


def pin(array):
    """hipHostRegister a numpy array (vsg_host_register).  Registered heap memory is only touched in place by handles
    that opted in (ORBextractor.set_direct_registered); prefer PinnedArray."""
    a = np.ascontiguousarray(array)
    _check(load_library().vsg_host_register(C.c_void_p(a.ctypes.data), a.nbytes), "vsg_host_register")
    return a


def unpin(array):
    _check(load_library().vsg_host_unregister(C.c_void_p(array.ctypes.data)), "vsg_host_unregister")


def _host_free(ptr):
    lib = _lib
    if lib is not None and ptr:
        lib.vsg_host_free(C.c_void_p(ptr))


class PinnedArray:
    """A numpy array over hipHostMalloc memory (vsg_host_alloc): pinned without a user-pointer mapping of heap pages
    underneath; the device reads / writes it in place.  `.a` is the array.  The memory lives as long as this object OR any
    numpy view derived from `.a` (the views hold the buffer object whose finalizer frees the allocation), so dropping the
    PinnedArray while a view is still in use -- or in flight -- is safe.  free() releases this object's own references;
    the allocation itself goes when the last view does."""

    class _Buf:  # owns the allocation; exposes it through the buffer protocol via a ctypes array
        def __init__(self, nbytes):
            import weakref
            p = C.c_void_p()
            _check(load_library().vsg_host_alloc(C.c_size_t(nbytes), C.byref(p)), "vsg_host_alloc")
            self.ptr = p.value
            self.raw = (C.c_uint8 * nbytes).from_address(self.ptr)
            # the ctypes array is what numpy keeps alive (ndarray.base chain): its death frees the memory
            self._fin = weakref.finalize(self.raw, _host_free, self.ptr)

    def __init__(self, shape, dtype=np.uint8):
        dt = np.dtype(dtype)
        count = int(np.prod(shape))
        n = max(count * dt.itemsize, 1)
        buf = PinnedArray._Buf(n)
        self._ptr = buf.ptr
        self._fin = buf._fin
        self.a = np.frombuffer(buf.raw, dtype=dt, count=count).reshape(shape)

    @property
    def ptr(self):
        return self._ptr

    def free(self):
        """Drop this object's array.  The pinned memory is released as soon as no numpy view of it is left -- it is NOT
        returned to the runtime here if a slice, a reshape or an exception traceback still holds one: use
        release() where the pinned footprint has to be bounded."""
        self.a = None

    @property
    def alive(self):
        """True while the hipHostMalloc block behind this object is still allocated (this object or a view holds it)."""
        return self._fin.alive

    def release(self):
        """free() + a check that the allocation really went: raises if a view of the array is still referenced
        somewhere (the memory then stays pinned until that view dies)."""
        self.a = None
        import gc
        if self._fin.alive:
            gc.collect()
        if self._fin.alive:
            raise RuntimeError("PinnedArray.release(): a numpy view of the array is still alive; the block stays pinned until "
                               "it is dropped")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def copy_d2d_async(dst, src, nbytes, stream, device=0):
    """Device-to-device copy of raw pointers (ints) on `stream` through the library's own HIP runtime."""
    _check(load_library().vsg_copy_d2d_async(int(device), C.c_void_p(dst), C.c_void_p(src), int(nbytes),
                                            C.c_void_p(stream) if stream else None), "vsg_copy_d2d_async")


def thread_arena_growths(device=0):
    return load_library().vsg_thread_arena_growths(int(device))


def _opt(a, t, conv):
    return (None, None) if a is None else (lambda x: (x, _p(x, t)))(conv(a))


VSG_DEPTH_U16, VSG_DEPTH_F32 = 0, 1


def depth_map_scale(yaml_value):
    """Tracking's mDepthMapFactor from RGBD.DepthMapFactor (Tracking.cc:638-642): 1 when |yaml| < 1e-5, else 1.0f / yaml."""
    return load_library().vsg_depth_map_scale(float(np.float32(yaml_value)))


def _depth_type(dtype):
    """VSG_DEPTH_* of a numpy / torch element type; anything else is passed as -1 (the library answers
    VSG_ERR_UNSUPPORTED)."""
    name = str(dtype).replace("torch.", "")
    return {"uint16": VSG_DEPTH_U16, "float32": VSG_DEPTH_F32}.get(name, -1)


def _depth_view(depth):
    """(pointer, VSG_DEPTH_*, rows, cols, row stride in bytes, owner) of a depth plane without copying it: the library
    classifies the memory itself (pinned memory is read in place).  None -> a NULL plane."""
    if depth is None:
        return 0, VSG_DEPTH_U16, 0, 0, 0, None
    if hasattr(depth, "data_ptr"):  # torch tensor: host memory only (pinned or not)
        if depth.device.type != "cpu":
            raise ValueError(f"depth must be in host memory, not on {depth.device} (device planes: rgbd_depth_batch_device)")
        if depth.dim() != 2 or depth.stride(1) != 1:
            raise ValueError("depth must be a 2-D tensor with contiguous rows")
        return depth.data_ptr(), _depth_type(depth.dtype), depth.shape[0], depth.shape[1], \
            depth.stride(0) * depth.element_size(), depth
    a = np.asarray(depth)
    if a.ndim != 2 or a.strides[1] != a.itemsize or a.strides[0] < 0:
        a = np.ascontiguousarray(a)
    return a.ctypes.data, _depth_type(a.dtype), a.shape[0], a.shape[1], a.strides[0], a


def rgbd_depth_batch_device(d_depth, depth_type, nframes, frame_stride, depth_stride, rows, cols, depth_scale, mbf, K4,
                            dist, d_kps, d_counts, capacity, d_u_right, d_depth_out, stream=None, device=0):
    """vsg_rgbd_depth_batch_device on raw device pointers (ints / torch .data_ptr()): mvuRight / mvDepth
    [nframes][capacity] of the records vsg_orb_extract_batch_device wrote; asynchronous on `stream`."""
    k4 = _f32(np.asarray(K4))
    d = _f32(np.asarray(dist)) if dist is not None else None
    _check(load_library().vsg_rgbd_depth_batch_device(
        int(device), C.c_void_p(d_depth), int(depth_type), int(nframes), int(frame_stride), int(depth_stride), int(rows),
        int(cols), float(depth_scale), float(mbf), _p(k4, _f32p), _p(d, _f32p) if d is not None else None,
        len(d) if d is not None else 0, C.c_void_p(d_kps), C.c_void_p(d_counts), int(capacity), C.c_void_p(d_u_right),
        C.c_void_p(d_depth_out), C.c_void_p(stream) if stream else None), "vsg_rgbd_depth_batch_device")


class Frame:
    """What the searches read of a VS_GRAPHS::Frame / KeyFrame, resident on the device (include/vsg_orb.h: vsg_frame):
    mvKeysUn (or mvKeys || mvKeysRight with Nleft), mDescriptors, mvuRight, mGrid / mGridRight (Frame.h:280-290)."""

    def __init__(self, capacity, device=0):
        self._L = load_library()
        self._h = C.c_void_p()
        self.device = int(device)
        _check(self._L.vsg_frame_create(self.device, int(capacity), C.byref(self._h)), "vsg_frame_create")
        self.kps = np.zeros(0, KP_DTYPE)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.vsg_frame_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def N(self):
        return self._L.vsg_frame_size(self._h)

    def upload(self, kps, desc, bounds, u_right=None, nleft=-1):
        """bounds = (mnMinX, mnMinY, mnMaxX, mnMaxY)."""
        k = np.ascontiguousarray(kps, dtype=KP_DTYPE)
        d = _u8(desc).reshape(-1, 32)
        assert len(k) == len(d)
        ur = _f32(u_right) if u_right is not None else None
        _check(self._L.vsg_frame_upload(self._h, k.ctypes.data_as(C.c_void_p), _p(d, _u8p) if len(d) else None,
                                        _p(ur, _f32p) if ur is not None else None, len(k), int(nleft),
                                        *[float(b) for b in bounds]), "vsg_frame_upload")
        self.kps, self.nleft = k, int(nleft)
        return self

    def from_extractor(self, ex, index, kps, bounds, n=None):
        """Device-to-device from frame `index` of the extractor's last call; kps = the records that call returned
        (n: only the first n of them)."""
        k = np.ascontiguousarray(kps, dtype=KP_DTYPE)[:n]
        _check(self._L.vsg_frame_from_extractor(self._h, ex.handle, int(index), k.ctypes.data_as(C.c_void_p), len(k),
                                                *[float(b) for b in bounds]), "vsg_frame_from_extractor")
        self.kps, self.nleft = k, -1
        return self

    def from_extractor_undistort(self, ex, index, kps, K4, dist, bounds, n=None):
        """The same for a distorted pinhole camera: Frame::UndistortKeyPoints (Frame.cc:891-921) on the device inside the
        grid launch.  self.kps = mvKeysUn afterwards."""
        k = np.ascontiguousarray(kps, dtype=KP_DTYPE)[:n]
        K4, dist = _f32(np.asarray(K4)), _f32(np.asarray(dist))
        un = np.zeros(len(k), KP_DTYPE)
        _check(self._L.vsg_frame_from_extractor_undistort(
            self._h, ex.handle, int(index), k.ctypes.data_as(C.c_void_p), len(k), _p(K4, _f32p), _p(dist, _f32p), len(dist),
            *[float(b) for b in bounds], un.ctypes.data_as(C.c_void_p)), "vsg_frame_from_extractor_undistort")
        self.kps, self.nleft = un, -1
        return self

    def extract_into(self, ex, image, bounds, K4=None, dist=None, vLappingArea=(0, 0)):
        """Frame::Frame front end in one call and one wait: operator() -> UndistortKeyPoints -> AssignFeaturesToGrid
        (vsg_orb_extract_to_frame).  Returns (monoIndex, mvKeys, descriptors); self.kps = mvKeysUn."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        rows, cols = img.shape
        cap = ex.capacity(rows, cols)
        kps, desc, un = np.zeros(cap, KP_DTYPE), np.zeros((cap, 32), np.uint8), np.zeros(cap, KP_DTYPE)
        n = C.c_int32(0)
        k4 = _f32(np.asarray(K4)) if K4 is not None else None
        d = _f32(np.asarray(dist)) if dist is not None else None
        mono = _check(self._L.vsg_orb_extract_to_frame(
            ex.handle, _p(img, _u8p), rows, cols, img.strides[0], int(vLappingArea[0]), int(vLappingArea[1]),
            kps.ctypes.data_as(C.c_void_p), _p(desc, _u8p), cap, C.byref(n), self._h, _p(k4, _f32p) if k4 is not None else None,
            _p(d, _f32p) if d is not None else None, len(d) if d is not None else 0, *[float(b) for b in bounds],
            un.ctypes.data_as(C.c_void_p)), "vsg_orb_extract_to_frame")
        self.kps, self.nleft = un[:n.value].copy(), -1
        return mono, kps[:n.value].copy(), desc[:n.value].copy()

    def extract_into_rgbd(self, ex, image, depth, bounds, K4, dist, depth_scale, mbf, vLappingArea=(0, 0)):
        """RGB-D Frame front end in one call and one wait (vsg_orb_extract_to_frame_rgbd): operator() ->
        UndistortKeyPoints -> GrabImageRGBD's depth conversion + ComputeStereoFromRGBD -> AssignFeaturesToGrid.
        depth: [rows, cols] uint16 or float32 (numpy -- pageable or a PinnedArray's .a -- or a CPU torch tensor; row
        strides may be padded); depth_scale = mDepthMapFactor (depth_map_scale); K4 / dist may be None (no distortion).
        Returns (monoIndex, mvKeys, descriptors, mvuRight, mvDepth); self.kps = mvKeysUn."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        rows, cols = img.shape
        ptr, dtype, drows, dcols, dstride, keep = _depth_view(depth)
        cap = ex.capacity(rows, cols)
        kps, desc, un = np.zeros(cap, KP_DTYPE), np.zeros((cap, 32), np.uint8), np.zeros(cap, KP_DTYPE)
        ur, dep = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
        n = C.c_int32(0)
        k4 = _f32(np.asarray(K4)) if K4 is not None else None
        d = _f32(np.asarray(dist)) if dist is not None else None
        mono = _check(self._L.vsg_orb_extract_to_frame_rgbd(
            ex.handle, _p(img, _u8p), rows, cols, img.strides[0], int(vLappingArea[0]), int(vLappingArea[1]),
            kps.ctypes.data_as(C.c_void_p), _p(desc, _u8p), cap, C.byref(n), self._h, _p(k4, _f32p) if k4 is not None else None,
            _p(d, _f32p) if d is not None else None, len(d) if d is not None else 0, *[float(b) for b in bounds],
            un.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), dtype, dstride, drows, dcols, float(depth_scale), float(mbf),
            _p(ur, _f32p), _p(dep, _f32p)), "vsg_orb_extract_to_frame_rgbd")
        del keep
        k = n.value
        self.kps, self.nleft = un[:k].copy(), -1
        return mono, kps[:k].copy(), desc[:k].copy(), ur[:k].copy(), dep[:k].copy()

    def grid(self, right=False):
        cs, en = np.zeros(64 * 48 + 1, np.int32), np.zeros(max(self.N, 1), np.int32)
        ne = _check(self._L.vsg_frame_copy_grid(self._h, int(right), _p(cs, _i32p), _p(en, _i32p)), "vsg_frame_copy_grid")
        return cs, en[:ne]

    def GetFeaturesInArea(self, x, y, r, minLevel=None, maxLevel=None, bRight=False):
        x, y, r = _f32(np.atleast_1d(x)), _f32(np.atleast_1d(y)), _f32(np.atleast_1d(r))
        nq = len(x)
        lo = _i32(np.atleast_1d(minLevel)) if minLevel is not None else None
        hi = _i32(np.atleast_1d(maxLevel)) if maxLevel is not None else None
        off = np.zeros(nq + 1, np.int32)
        cap = max(1, 64 * nq)
        while True:
            idx = np.zeros(cap, np.int32)
            total = _check(self._L.vsg_frame_features_in_area(
                self._h, _p(x, _f32p), _p(y, _f32p), _p(r, _f32p), _p(lo, _i32p) if lo is not None else None,
                _p(hi, _i32p) if hi is not None else None, int(bRight), nq, _p(off, _i32p), _p(idx, _i32p), cap),
                "vsg_frame_features_in_area")
            if total <= cap:
                return off, idx[:total]
            cap = total

    # ---- ORBmatcher::SearchByProjection(Frame &F, vpMapPoints, th, ...)  (ORBmatcher.cc:42-216)
    def SearchByProjection(self, mp, th, nnratio, scale_factors, train_blocked, left_to_right=None, right_to_left=None):
        """mp: dict of per-map-point arrays (desc, observed, in_view, proj_x, proj_y, proj_xr, scale_level, view_cos
        and, for Nleft != -1, in_view_r, proj_x_r, proj_y_r, scale_level_r, view_cos_r).
        Returns (nmatches, train_match, train_blocked)."""
        d = _u8(mp["desc"]).reshape(-1, 32)
        n = len(d)
        obs, inv = _u8(mp["observed"]), _u8(mp["in_view"])
        px, py, lvl, vc = _f32(mp["proj_x"]), _f32(mp["proj_y"]), _i32(mp["scale_level"]), _f32(mp["view_cos"])
        pxr = _f32(mp["proj_xr"]) if mp.get("proj_xr") is not None else None
        R = {}
        for key, conv, t in (("in_view_r", _u8, _u8p), ("proj_x_r", _f32, _f32p), ("proj_y_r", _f32, _f32p),
                             ("scale_level_r", _i32, _i32p), ("view_cos_r", _f32, _f32p)):
            R[key] = conv(mp[key]) if mp.get(key) is not None else None
        sf = _f32(scale_factors)
        ltr = _i32(left_to_right) if left_to_right is not None else None
        rtl = _i32(right_to_left) if right_to_left is not None else None
        tb = _u8(train_blocked).copy()
        tm = np.full(max(len(tb), 1), -1, np.int32)

        def o(a, t):
            return _p(a, t) if a is not None else None
        nm = _check(self._L.vsg_frame_search_by_projection(
            self._h, n, _p(d, _u8p), _p(obs, _u8p), _p(inv, _u8p), _p(px, _f32p), _p(py, _f32p), o(pxr, _f32p),
            _p(lvl, _i32p), _p(vc, _f32p), o(R["in_view_r"], _u8p), o(R["proj_x_r"], _f32p), o(R["proj_y_r"], _f32p),
            o(R["scale_level_r"], _i32p), o(R["view_cos_r"], _f32p), float(th), float(np.float32(nnratio)), _p(sf, _f32p),
            len(scale_factors), o(ltr, _i32p), o(rtl, _i32p), _p(tb, _u8p), _p(tm, _i32p)),
            "vsg_frame_search_by_projection")
        return nm, tm[:len(tb)], tb

    # ---- the entries on resident map points (MapPoints): what they share on this side
    @staticmethod
    def _resident_points(slots, skip, fields, n=None, of="the slots"):
        """slots (None: slots 0 .. n-1), skip flags of the same length (or None), and one output array of max(n, 1) entries
        per dtype of `fields`.  Returns (n, slots pointer, skip pointer, the outputs' pointers in that order, trimmed) with
        trimmed() = the outputs cut to n."""
        sl = np.ascontiguousarray(slots, dtype=np.int32) if slots is not None else None
        n = len(sl) if sl is not None else int(n)
        sk = _u8(skip) if skip is not None else None
        if sk is not None and len(sk) != n:
            raise ValueError(f"skip length does not match {of}")
        outs = [np.zeros(max(n, 1), dt) for dt in fields]
        ptr = {np.uint8: _u8p, np.int32: _i32p, np.float32: _f32p}
        return (n, _p(_i32(sl), _i32p) if sl is not None else None, _p(sk, _u8p) if sk is not None and n else None,
                [_p(a, ptr[dt]) for a, dt in zip(outs, fields)], lambda: tuple(a[:n] for a in outs))

    # ---- Frame::isInFrustum (Frame.cc:656-719) on resident map points
    def isInFrustum(self, mp, pose, n=None, slots=None, viewing_cos_limit=0.5):
        """mp: MapPoints, pose: FramePose.  Map point i = slot slots[i] (None: slots 0 .. n-1, n defaulting to the store's
        capacity).  Returns a dict: in_view, proj_x, proj_y, proj_xr, depth, scale_level, view_cos."""
        u8, f32, i32 = np.uint8, np.float32, np.int32
        n, slp, _, o, trimmed = self._resident_points(slots, None, (u8, f32, f32, f32, f32, i32, f32),
                                                      mp.capacity if n is None else n)
        _check(self._L.vsg_frame_is_in_frustum(self._h, mp.handle, n, slp, C.byref(pose),
                                               float(np.float32(viewing_cos_limit)), *o), "vsg_frame_is_in_frustum")
        return dict(zip(("in_view", "proj_x", "proj_y", "proj_xr", "depth", "scale_level", "view_cos"), trimmed()))

    # ---- Tracking::SearchLocalPoints (Tracking.cc:3423-3495): isInFrustum + SearchByProjection(F, vpMapPoints)
    def SearchLocalPoints(self, mp, pose, th, nnratio, scale_factors, train_blocked, n=None, slots=None, skip=None,
                          viewing_cos_limit=0.5, far_points=False, th_far_points=0.0):
        """skip[i] != 0: mnLastFrameSeen == mnId or isBad() (never projected).  Returns (nmatches, train_match,
        train_blocked, in_view, proj_x, proj_y, n_to_match)."""
        n, slp, skp, o, trimmed = self._resident_points(slots, skip, (np.uint8, np.float32, np.float32),
                                                        mp.capacity if n is None else n, "the map points")
        sf = _f32(scale_factors)
        tb = _u8(train_blocked).copy()
        tm = np.full(max(len(tb), 1), -1, np.int32)
        ntm = C.c_int(0)
        nm = _check(self._L.vsg_frame_search_local_points(
            self._h, mp.handle, n, slp, skp, C.byref(pose), float(np.float32(viewing_cos_limit)), float(th),
            float(np.float32(nnratio)), int(bool(far_points)), float(np.float32(th_far_points)), _p(sf, _f32p),
            len(scale_factors), _p(tb, _u8p), _p(tm, _i32p), *o, C.byref(ntm)), "vsg_frame_search_local_points")
        return (nm, tm[:len(tb)], tb, *trimmed(), ntm.value)

    # ---- Optimizer::PoseOptimization(pFrame) on resident map points  (Optimizer.cc:1063-1452)
    @staticmethod
    def _pose_result(ret, res, outlier, chi2):
        return dict(ret=ret, q=np.array(res.q[:], np.float64), t=np.array(res.t[:], np.float64), n_initial=res.n_initial,
                    n_bad=res.n_bad, rounds_run=res.rounds_run, held=res.held, outlier=outlier, chi2=chi2)

    def pose_optimization(self, mp, feat_slots, q, t, camera, inv_level_sigma2, outlier, hold_round=-1, chi2=None):
        """feat_slots[i] = slot of mvpMapPoints[i] (< 0: none), one per feature; q (x y z w), t = pFrame->GetPose();
        camera = (fx, fy, cx, cy, mbf); outlier = mvbOutlier, updated IN A COPY for the features with a slot; chi2 (an
        optional float array of the same length) likewise.  hold_round = 2 stops after round 2's optimize() (held = 1: run
        the plane step on q / t, then pose_optimization_resume).  Returns a dict: ret, q, t (float64), n_initial, n_bad,
        rounds_run, held, outlier, chi2."""
        if len(feat_slots) != len(self.kps):
            raise ValueError("feat_slots length does not match the frame's features")
        sl, sig = _i32(feat_slots), _f32(inv_level_sigma2)
        out = _u8(outlier).copy()
        if len(out) != len(self.kps):
            raise ValueError("outlier length does not match the frame's features")
        out = out if out.size else np.zeros(1, np.uint8)
        c2 = np.zeros(max(len(self.kps), 1), np.float32) if chi2 is None else _f32(chi2).copy()
        pose, res = PoseSE3(), PoseResult()
        pose.q[:] = [float(v) for v in np.asarray(q, np.float32).reshape(4)]
        pose.t[:] = [float(v) for v in np.asarray(t, np.float32).reshape(3)]
        ret = _check(self._L.vsg_frame_pose_optimization(
            self._h, mp.handle, _p(sl, _i32p), C.byref(pose), *[float(np.float32(c)) for c in camera], _p(sig, _f32p),
            len(inv_level_sigma2), int(hold_round), _p(out, _u8p), _p(c2, _f32p), C.byref(res)),
            "vsg_frame_pose_optimization")
        return self._pose_result(ret, res, out[:len(self.kps)], c2[:len(self.kps)])

    def mlpnp_ransac(self, mp, slots, camera, level_sigma2, sets, min_inliers, max_its, first=0, n_iterations=5, th2=5.991,
                     per_hypothesis=False):
        """MLPnPsolver::iterate(n_iterations, ...) entered at mnIterations == first (vsg_frame_mlpnp_ransac): slots[i] = slot of
        vpMapPointMatches[i] in mp (< 0: none), one per feature; camera = (fx, fy, cx, cy); level_sigma2 = mvLevelSigma2;
        sets = n_hyp x 6 correspondence indices (mlpnp_draw_sets); min_inliers / max_its from mlpnp_ransac_parameters.  A
        resumed call passes first = the `iterations` of the call before.  Returns a dict: found, no_more, n_inliers, refined,
        best_hypothesis, iterations, n_correspondences, n_records, Tcw (4 x 4 float32), inlier (bool per feature), result
        (the raw MlpnpResult) and, with per_hypothesis, hyp_inliers and hyp_T (n_hyp x 3 x 4 float64)."""
        if len(slots) != len(self.kps):
            raise ValueError("slots length does not match the frame's features")
        sl, sig = _i32(slots), _f32(level_sigma2)
        sm = np.ascontiguousarray(sets, np.int32).reshape(-1, 6)
        nh = len(sm)
        inl = np.zeros(max(len(self.kps), 1), np.uint8)
        hc, hT = np.zeros(max(nh, 1), np.int32), np.zeros((max(nh, 1), 3, 4), np.float64)
        res = MlpnpResult()
        _check(self._L.vsg_frame_mlpnp_ransac(
            self._h, mp.handle, _p(sl, _i32p), *[float(np.float32(c)) for c in camera], _p(sig, _f32p), len(sig), float(th2),
            int(min_inliers), int(max_its), int(first), int(n_iterations), nh, _p(sm, _i32p), _p(inl, _u8p), C.byref(res),
            _p(hc, _i32p) if per_hypothesis else None, _p(hT, C.POINTER(C.c_double)) if per_hypothesis else None), "vsg_frame_mlpnp_ransac")
        out = dict(found=bool(res.found), no_more=bool(res.no_more), n_inliers=res.n_inliers, refined=bool(res.refined),
                   best_hypothesis=res.best_hypothesis, iterations=res.iterations, n_correspondences=res.n_correspondences,
                   n_records=res.n_records, Tcw=np.array(res.Tcw[:], np.float32).reshape(4, 4),
                   inlier=inl[:len(self.kps)].astype(bool), result=res)
        if per_hypothesis:
            out.update(hyp_inliers=hc[:nh], hyp_T=hT[:nh])
        return out

    def pose_optimization_resume(self, outlier, removed=None, chi2=None):
        """Round 2's classification and round 3 of a held pose_optimization.  removed[i] != 0: the plane step set
        mvpMapPoints[i] = NULL.  outlier / chi2 = the arrays the held call returned."""
        out = _u8(outlier).copy()
        out = out if out.size else np.zeros(1, np.uint8)
        c2 = np.zeros(max(len(self.kps), 1), np.float32) if chi2 is None else _f32(chi2).copy()
        rem = None if removed is None else _u8(removed)
        if rem is not None and len(rem) != len(self.kps):
            raise ValueError("removed length does not match the frame's features")
        res = PoseResult()
        ret = _check(self._L.vsg_frame_pose_optimization_resume(
            self._h, _p(rem, _u8p) if rem is not None else None, _p(out, _u8p), _p(c2, _f32p), C.byref(res)),
            "vsg_frame_pose_optimization_resume")
        return self._pose_result(ret, res, out[:len(self.kps)], c2[:len(self.kps)])

    # ---- Tracking::TrackWithMotionModel (Tracking.cc:2945-3005) on resident map points: search, ordered walk and
    # PoseOptimization in one enqueue and one wait
    @staticmethod
    def _se3(q, t):
        pose = PoseSE3()
        pose.q[:] = [float(v) for v in np.asarray(q, np.float32).reshape(4)]
        pose.t[:] = [float(v) for v in np.asarray(t, np.float32).reshape(3)]
        return pose

    def TrackWithMotionModel(self, last, mp, last_slots, cur_pose, last_pose, mb, mono, th, scale_factors, q, t,
                             inv_level_sigma2, outlier, check_orientation=True, hold_round=-1, chi2=None):
        """self = mCurrentFrame, last = the resident LastFrame; the arguments of SearchLastFrame and pose_optimization (the
        camera is cur_pose's).  outlier / chi2 are updated IN A COPY.  Returns a dict: ret, feat_slots (one per feature,
        after the discard), train_match, outlier, chi2, q, t, n_initial, n_bad, rounds_run, held, n_search, wide,
        n_matches_searched, optimized, n_matches, n_matches_map, direction."""
        if last_slots is not None and len(last_slots) != len(last.kps):
            raise ValueError("last_slots length does not match the last frame's features")
        n = len(self.kps)
        _, slp, _, _, _ = self._resident_points(last_slots, None, (), len(last.kps))
        sf, sig = _f32(scale_factors), _f32(inv_level_sigma2)
        if len(sf) != len(sig):
            raise ValueError("inv_level_sigma2 length does not match the scale factors")
        out = np.zeros(max(n, 1), np.uint8)
        out[:n] = _u8(outlier)
        c2 = np.zeros(max(n, 1), np.float32)
        if chi2 is not None:
            c2[:n] = _f32(chi2)
        fs, tm = np.full(max(n, 1), -1, np.int32), np.full(max(n, 1), -1, np.int32)
        res = TrackResult()
        ret = _check(self._L.vsg_frame_track_with_motion_model(
            self._h, last.handle, mp.handle, slp, C.byref(cur_pose), C.byref(last_pose), float(np.float32(mb)), int(bool(mono)), float(th), _p(sf, _f32p), len(sf),
            int(bool(check_orientation)), C.byref(self._se3(q, t)), _p(sig, _f32p), int(hold_round), _p(fs, _i32p),
            _p(tm, _i32p), _p(out, _u8p), _p(c2, _f32p), C.byref(res)), "vsg_frame_track_with_motion_model")
        d = self._pose_result(ret, res.pose, out[:n], c2[:n])
        d.update(feat_slots=fs[:n], train_match=tm[:n])
        d.update({k: int(getattr(res, k)) for k, _ in TrackResult._fields_[1:-1]})
        return d

    # ---- Tracking::TrackLocalMap (Tracking.cc:3019-3131) on resident map points: frustum, search, ordered walk,
    # PoseOptimization and the statistics loop in one enqueue and one wait
    def TrackLocalMap(self, mp, pose, th, nnratio, scale_factors, feat_slots, q, t, inv_level_sigma2, outlier, n=None,
                      slots=None, skip=None, viewing_cos_limit=0.5, far_points=False, th_far_points=0.0, hold_round=-1,
                      only_tracking=False, drop_outliers=False, chi2=None):
        """The arguments of SearchLocalPoints and pose_optimization (the camera is pose's); feat_slots[i] = the slot of
        mvpMapPoints[i] on entry (< 0: none), e.g. TrackWithMotionModel's feat_slots.  outlier / chi2 are updated IN A COPY.
        Returns a dict: ret (= n_matches_inliers), feat_slots (after the walk and the drop), train_match, outlier, chi2,
        in_view, proj_x, proj_y, q, t, n_initial, n_bad, rounds_run, held, n_to_match, n_matches_searched,
        n_matches_inliers, walk_rounds."""
        nf = len(self.kps)
        if len(feat_slots) != nf:
            raise ValueError("feat_slots length does not match the frame's features")
        n, slp, skp, o, trimmed = self._resident_points(slots, skip, (np.uint8, np.float32, np.float32),
                                                        mp.capacity if n is None else n, "the map points")
        sf, sig = _f32(scale_factors), _f32(inv_level_sigma2)
        if len(sf) != len(sig):
            raise ValueError("inv_level_sigma2 length does not match the scale factors")
        fin = np.full(max(nf, 1), -1, np.int32)
        fin[:nf] = _i32(feat_slots)
        out = np.zeros(max(nf, 1), np.uint8)
        out[:nf] = _u8(outlier)
        c2 = np.zeros(max(nf, 1), np.float32)
        if chi2 is not None:
            c2[:nf] = _f32(chi2)
        fs, tm = np.full(max(nf, 1), -1, np.int32), np.full(max(nf, 1), -1, np.int32)
        res = TrackLocalResult()
        ret = _check(self._L.vsg_frame_track_local_map(
            self._h, mp.handle, n, slp, skp, C.byref(pose), float(np.float32(viewing_cos_limit)), float(th),
            float(np.float32(nnratio)), int(bool(far_points)), float(np.float32(th_far_points)), _p(sf, _f32p), len(sf),
            _p(fin, _i32p), C.byref(self._se3(q, t)), _p(sig, _f32p), int(hold_round), int(bool(only_tracking)),
            int(bool(drop_outliers)), _p(fs, _i32p), _p(tm, _i32p), _p(out, _u8p), _p(c2, _f32p), *o, C.byref(res)),
            "vsg_frame_track_local_map")
        d = self._pose_result(ret, res.pose, out[:nf], c2[:nf])
        d.update(feat_slots=fs[:nf], train_match=tm[:nf])
        d.update(zip(("in_view", "proj_x", "proj_y"), trimmed()))
        d.update({k: int(getattr(res, k)) for k, _ in TrackLocalResult._fields_[1:]})
        return d

    # ---- Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale, ...) on resident map points
    # (Optimizer.cc:3261-3529); self is pKF1
    def OptimizeSim3(self, kf2, mp1, mp2, slots1, slots2, idx2, level2, pose1, pose2, inv_level_sigma2_1,
                     inv_level_sigma2_2, S12, th2, fix_scale, all_points=False, chi2=None):
        """slots1[i] / slots2[i] = slot of vpMapPoints1[i] in mp1 / of vpMatches1[i] in mp2 (< 0: missing or bad), one per
        feature of this keyframe; idx2[i] = the match's index in kf2 or < 0; level2[i] = its mnTrackScaleLevel (read when
        idx2[i] < 0); pose1 / pose2: FramePose (Rcw, tcw, fx, fy, cx, cy are read); S12 = (q x y z w, t, s), taken as it is.
        chi2 (an optional float64 array of shape (n, 2)) is updated IN A COPY for the pairs with an edge.  Returns a dict:
        ret (nIn, or 0), S12 = (q, t, s) float64, S12_bytes, updated, n_correspondences, n_bad, n_in, n_in_kf2, n_out_kf2,
        more_iterations, state (uint8 per feature, SIM3_OPT_STATES), chi2.  The caller nulls vpMatches1[i] where state[i]
        is 2 or 3 and zero-fills mAcumHessian."""
        n = len(self.kps)
        arrs = [_i32(a) for a in (slots1, slots2, idx2, level2)]
        if any(len(a) != n for a in arrs):
            raise ValueError("slots1 / slots2 / idx2 / level2 length does not match the keyframe's features")
        if len(inv_level_sigma2_1) != len(inv_level_sigma2_2):
            raise ValueError("the two sigma tables differ in length")
        arrs = [a if a.size else np.zeros(1, np.int32) for a in arrs]
        sig1, sig2 = _f32(inv_level_sigma2_1), _f32(inv_level_sigma2_2)
        state = np.zeros(max(n, 1), np.uint8)
        c2 = np.zeros(2 * max(n, 1), np.float64) if chi2 is None else np.ascontiguousarray(chi2, np.float64).reshape(-1).copy()
        if c2.size < 2 * n:
            raise ValueError("chi2 needs two entries per feature")
        s12, res = Sim3d.make(*S12), Sim3OptResult()
        ret = _check(self._L.vsg_frame_optimize_sim3(
            self._h, kf2.handle, mp1.handle, mp2.handle, *[_p(a, _i32p) for a in arrs], C.byref(pose1), C.byref(pose2),
            _p(sig1, _f32p), _p(sig2, _f32p), len(sig1), C.byref(s12), float(np.float32(th2)), int(bool(fix_scale)),
            int(bool(all_points)), _p(state, _u8p), _p(c2, C.POINTER(C.c_double)), C.byref(res)), "vsg_frame_optimize_sim3")
        out = dict(ret=ret, S12=(np.array(res.S12.q[:], np.float64), np.array(res.S12.t[:], np.float64), float(res.S12.s)),
                   S12_bytes=bytes(res.S12), input_bytes=bytes(s12), state=state[:n], chi2=c2[:2 * n].reshape(n, 2))
        out.update({k: int(getattr(res, k)) for k, _ in Sim3OptResult._fields_[1:]})
        return out

    # ---- SearchByProjection(CurrentFrame, LastFrame, th, bMono) on resident map points  (ORBmatcher.cc:1667-1878)
    def SearchLastFrame(self, last, mp, last_slots, cur_pose, last_pose, mb, mono, th, scale_factors, train_blocked,
                        check_orientation=True):
        """last: the resident LastFrame; last_slots[i] = slot of its feature i's map point (< 0: none, or an outlier).
        Returns (nmatches, train_match, train_blocked, direction, projected, u, v, ur); train_match[i2] = index of the
        last-frame feature, the last four per last-frame feature."""
        if last_slots is not None and len(last_slots) != len(last.kps):
            raise ValueError("last_slots length does not match the last frame's features")
        _, slp, _, o, trimmed = self._resident_points(last_slots, None, (np.uint8, np.float32, np.float32, np.float32),
                                                      len(last.kps))
        sf = _f32(scale_factors)
        tb = _u8(train_blocked).copy()
        tm = np.full(max(len(tb), 1), -1, np.int32)
        direction = C.c_int(0)
        nm = _check(self._L.vsg_frame_search_last_frame(
            self._h, last.handle, mp.handle, slp, C.byref(cur_pose), C.byref(last_pose), float(np.float32(mb)),
            int(bool(mono)), float(th), _p(sf, _f32p), len(scale_factors), int(bool(check_orientation)), _p(tb, _u8p),
            _p(tm, _i32p), C.byref(direction), *o), "vsg_frame_search_last_frame")
        return (nm, tm[:len(tb)], tb, direction.value, *trimmed())

    # ---- SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) on resident map points  (ORBmatcher.cc:1880-2000)
    def SearchKeyFramePoints(self, mp, slots, pose, th, orb_dist, scale_factors, occupied, kf_angle=None, skip=None,
                             check_orientation=True):
        """slots[i] = slot of the KeyFrame's i-th map point, kf_angle[i] = pKF->mvKeysUn[i].angle, skip[i] != 0 = isBad() or
        in sAlreadyFound.  Returns (nmatches, train_match, occupied, projected, u, v, predicted_level); train_match[i2] =
        query index."""
        n, slp, skp, o, trimmed = self._resident_points(slots, skip, (np.uint8, np.float32, np.float32, np.int32))
        ka = _f32(kf_angle) if kf_angle is not None else None
        if ka is not None and len(ka) != n:
            raise ValueError("kf_angle length does not match the slots")
        sf = _f32(scale_factors)
        oc = _u8(occupied).copy()
        tm = np.full(max(len(oc), 1), -1, np.int32)
        nm = _check(self._L.vsg_frame_search_keyframe_points(
            self._h, mp.handle, n, slp, skp, C.byref(pose), float(th), int(orb_dist), _p(sf, _f32p), len(scale_factors),
            int(bool(check_orientation)), _p(ka, _f32p) if ka is not None and n else None, _p(oc, _u8p), _p(tm, _i32p), *o),
            "vsg_frame_search_keyframe_points")
        return (nm, tm[:len(oc)], oc, *trimmed())

    # ---- Fuse x2 and SearchByProjection(pKF, Scw, ...) on resident map points  (ORBmatcher.cc:1148-1446, :430-528)
    def FusePoints(self, mp, slots, pose, th, scale_factors, inv_level_sigma2, skip=None):
        """Fuse(pKF, vpMapPoints, th, false) with self = pKF: slots[i] = slot of vpMapPoints[i], skip[i] != 0 = NULL, isBad()
        or IsInKeyFrame(pKF), pose = pKF's.  Returns (nFused, best_idx, best_dist, projected, u, v, ur, predicted_level),
        every array per query."""
        u8, f32, i32 = np.uint8, np.float32, np.int32
        n, slp, skp, o, trimmed = self._resident_points(slots, skip, (i32, i32, u8, f32, f32, f32, i32))
        sf, s2 = _f32(scale_factors), _f32(inv_level_sigma2)
        if len(s2) != len(sf):
            raise ValueError("inv_level_sigma2 length does not match the scale factors")
        nf = _check(self._L.vsg_frame_fuse_points(self._h, mp.handle, n, slp, skp, C.byref(pose), float(th), _p(sf, _f32p),
                                                  _p(s2, _f32p), len(sf), *o), "vsg_frame_fuse_points")
        return (nf, *trimmed())

    def FusePoints_Sim3(self, mp, slots, pose, th, scale_factors, skip=None):
        """Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) with self = pKF and pose = the decomposed Scw.  Returns (nFused,
        best_idx, best_dist, projected, u, v, predicted_level)."""
        u8, f32, i32 = np.uint8, np.float32, np.int32
        n, slp, skp, o, trimmed = self._resident_points(slots, skip, (i32, i32, u8, f32, f32, i32))
        sf = _f32(scale_factors)
        nf = _check(self._L.vsg_frame_fuse_points_sim3(self._h, mp.handle, n, slp, skp, C.byref(pose), float(th),
                                                       _p(sf, _f32p), len(sf), *o), "vsg_frame_fuse_points_sim3")
        return (nf, *trimmed())

    def SearchSim3Points(self, mp, slots, pose, th, ratio_hamming, scale_factors, matched, skip=None):
        """SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) with self = pKF and pose = the decomposed
        Scw; matched[i] != -1 = vpMatched[i] is set.  Returns (nmatches, matched, projected, u, v, predicted_level); a new
        entry of matched holds the query index."""
        n, slp, skp, o, trimmed = self._resident_points(slots, skip, (np.uint8, np.float32, np.float32, np.int32))
        sf = _f32(scale_factors)
        if len(matched) != self.N:
            raise ValueError("matched length does not match the KeyFrame's features")
        m = np.full(max(len(matched), 1), -1, np.int32)
        m[:len(matched)] = matched
        nm = _check(self._L.vsg_frame_search_sim3_points(
            self._h, mp.handle, n, slp, skp, C.byref(pose), float(th), float(np.float32(ratio_hamming)), _p(sf, _f32p),
            len(sf), _p(m, _i32p), *o), "vsg_frame_search_sim3_points")
        return (nm, m[:len(matched)], *trimmed())

    # ---- SearchByProjection(CurrentFrame, LastFrame, th, bMono)  (ORBmatcher.cc:1667-1878)
    def SearchByProjection_Last(self, desc, observed, u, v, ur, last_octave, last_angle, th, direction, scale_factors,
                                check_orientation, train_blocked, u_r=None, v_r=None):
        d = _u8(desc).reshape(-1, 32)
        obs = _u8(observed)
        uu, vv, oc, an = _f32(u), _f32(v), _i32(last_octave), _f32(last_angle)
        ur_ = _f32(ur) if ur is not None else None
        ur2, vr2 = (_f32(u_r), _f32(v_r)) if u_r is not None else (None, None)
        sf = _f32(scale_factors)
        tb = _u8(train_blocked).copy()
        tm = np.full(max(len(tb), 1), -1, np.int32)
        nm = _check(self._L.vsg_frame_search_by_projection_last(
            self._h, len(d), _p(d, _u8p), _p(obs, _u8p), _p(uu, _f32p), _p(vv, _f32p),
            _p(ur_, _f32p) if ur_ is not None else None, _p(ur2, _f32p) if ur2 is not None else None,
            _p(vr2, _f32p) if vr2 is not None else None, _p(oc, _i32p), _p(an, _f32p), float(th), int(direction),
            _p(sf, _f32p), len(scale_factors), int(check_orientation), _p(tb, _u8p), _p(tm, _i32p)),
            "vsg_frame_search_by_projection_last")
        return nm, tm[:len(tb)], tb

    # ---- SearchByProjection(KeyFrame*, Sim3, vpPoints, vpMatched, th, ratioHamming)  (ORBmatcher.cc:430-641)
    def SearchByProjection_Sim3(self, desc, u, v, radius, predicted_level, ratio_hamming, matched):
        d = _u8(desc).reshape(-1, 32)
        m = _i32(matched).copy()
        nm = _check(self._L.vsg_frame_search_by_projection_sim3(
            self._h, len(d), _p(d, _u8p), _p(_f32(u), _f32p), _p(_f32(v), _f32p), _p(_f32(radius), _f32p),
            _p(_i32(predicted_level), _i32p), float(np.float32(ratio_hamming)), _p(m, _i32p)),
            "vsg_frame_search_by_projection_sim3")
        return nm, m[:len(matched)]

    # ---- SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)  (ORBmatcher.cc:1880-2000)
    def SearchByProjection_KF(self, desc, u, v, radius, predicted_level, kf_angle, orb_dist, check_orientation, occupied):
        d = _u8(desc).reshape(-1, 32)
        oc = _u8(occupied).copy()
        tm = np.full(max(len(oc), 1), -1, np.int32)
        nm = _check(self._L.vsg_frame_search_by_projection_kf(
            self._h, len(d), _p(d, _u8p), _p(_f32(u), _f32p), _p(_f32(v), _f32p), _p(_f32(radius), _f32p),
            _p(_i32(predicted_level), _i32p), _p(_f32(kf_angle), _f32p), int(orb_dist), int(check_orientation),
            _p(oc, _u8p), _p(tm, _i32p)), "vsg_frame_search_by_projection_kf")
        return nm, tm[:len(occupied)], oc

    # ---- Fuse x2 (ORBmatcher.cc:1148-1446): the search part
    def Fuse(self, desc, u, v, ur, radius, predicted_level, inv_level_sigma2, right=False):
        d = _u8(desc).reshape(-1, 32)
        bi, bd = np.zeros(max(len(d), 1), np.int32), np.zeros(max(len(d), 1), np.int32)
        s2 = _f32(inv_level_sigma2)
        nf = _check(self._L.vsg_frame_fuse(self._h, len(d), _p(d, _u8p), _p(_f32(u), _f32p), _p(_f32(v), _f32p),
                                           _p(_f32(ur), _f32p), _p(_f32(radius), _f32p),
                                           _p(_i32(predicted_level), _i32p), int(right), _p(s2, _f32p),
                                           len(inv_level_sigma2), _p(bi, _i32p), _p(bd, _i32p)), "vsg_frame_fuse")
        return nf, bi[:len(d)], bd[:len(d)]

    def Fuse_Sim3(self, desc, u, v, radius, predicted_level):
        d = _u8(desc).reshape(-1, 32)
        bi, bd = np.zeros(max(len(d), 1), np.int32), np.zeros(max(len(d), 1), np.int32)
        nf = _check(self._L.vsg_frame_fuse_sim3(self._h, len(d), _p(d, _u8p), _p(_f32(u), _f32p), _p(_f32(v), _f32p),
                                                _p(_f32(radius), _f32p), _p(_i32(predicted_level), _i32p),
                                                _p(bi, _i32p), _p(bd, _i32p)), "vsg_frame_fuse_sim3")
        return nf, bi[:len(d)], bd[:len(d)]

    def SearchForInitialization(self, f2, prev_x, prev_y, window_size, nnratio, check_orientation):
        """self = F1, f2 = F2 (both resident)."""
        out = np.full(max(self.N, 1), -1, np.int32)
        nm = _check(self._L.vsg_frame_search_for_initialization(
            self._h, f2.handle, _p(_f32(prev_x), _f32p), _p(_f32(prev_y), _f32p), int(window_size),
            float(np.float32(nnratio)), int(check_orientation), _p(out, _i32p)), "vsg_frame_search_for_initialization")
        return nm, out[:self.N]

    def SearchByBoW_KF_F(self, kf_valid, kf_fv, f, f_fv, nnratio, check_orientation):
        """self = KeyFrame, f = Frame (both resident).  kf_fv = f_fv = None: the FeatureVectors both frames keep resident
        since their ComputeBoW are joined on the device.  Returns (nmatches, matchF)."""
        kv = _u8(kf_valid)
        out = np.full(max(f.N, 1), -1, np.int32)
        if kf_fv is None and f_fv is None:
            nm = _check(self._L.vsg_frame_search_by_bow_kf_f(
                self._h, _p(kv, _u8p), None, None, None, 0, f.handle, None, None, None, 0, float(np.float32(nnratio)),
                int(check_orientation), _p(out, _i32p)), "vsg_frame_search_by_bow_kf_f")
            return nm, out[:f.N]
        kn, ko, ki = (_i32(x) for x in kf_fv)
        fn, fo, fi = (_i32(x) for x in f_fv)
        nm = _check(self._L.vsg_frame_search_by_bow_kf_f(
            self._h, _p(kv, _u8p), _p(kn, _i32p), _p(ko, _i32p), _p(ki, _i32p), len(kf_fv[0]), f.handle, _p(fn, _i32p),
            _p(fo, _i32p), _p(fi, _i32p), len(f_fv[0]), float(np.float32(nnratio)), int(check_orientation),
            _p(out, _i32p)), "vsg_frame_search_by_bow_kf_f")
        return nm, out[:f.N]

    def SearchByBoW_KF_KF(self, valid1, fv1, kf2, valid2, fv2, nnratio, check_orientation):
        v1, v2 = _u8(valid1), _u8(valid2)
        out = np.full(max(self.N, 1), -1, np.int32)
        if fv1 is None and fv2 is None:  # both FeatureVectors resident
            nm = _check(self._L.vsg_frame_search_by_bow_kf_kf(
                self._h, _p(v1, _u8p), None, None, None, 0, kf2.handle, _p(v2, _u8p), None, None, None, 0,
                float(np.float32(nnratio)), int(check_orientation), _p(out, _i32p)), "vsg_frame_search_by_bow_kf_kf")
            return nm, out[:self.N]
        n1, o1, i1 = (_i32(x) for x in fv1)
        n2, o2, i2 = (_i32(x) for x in fv2)
        nm = _check(self._L.vsg_frame_search_by_bow_kf_kf(
            self._h, _p(v1, _u8p), _p(n1, _i32p), _p(o1, _i32p), _p(i1, _i32p), len(fv1[0]), kf2.handle, _p(v2, _u8p),
            _p(n2, _i32p), _p(o2, _i32p), _p(i2, _i32p), len(fv2[0]), float(np.float32(nnratio)),
            int(check_orientation), _p(out, _i32p)), "vsg_frame_search_by_bow_kf_kf")
        return nm, out[:self.N]

    def SearchForTriangulation(self, eligible1, fv1, kf2, eligible2, fv2, check_orientation, pair_ok=None, pair_off=None):
        """ORBmatcher::SearchForTriangulation (ORBmatcher.cc:902-1146), self = pKF1, kf2 = pKF2, both resident."""
        e1, e2 = _u8(eligible1), _u8(eligible2)
        n1, o1, i1 = (_i32(x) for x in fv1)
        n2, o2, i2 = (_i32(x) for x in fv2)
        ok = np.ascontiguousarray(pair_ok, np.uint32) if pair_ok is not None else None
        po = _i32(pair_off) if pair_ok is not None else None
        out = np.full(max(self.N, 1), -1, np.int32)
        nm = _check(self._L.vsg_frame_search_for_triangulation(
            self._h, _p(e1, _u8p), _p(n1, _i32p), _p(o1, _i32p), _p(i1, _i32p), len(fv1[0]), kf2.handle, _p(e2, _u8p),
            _p(n2, _i32p), _p(o2, _i32p), _p(i2, _i32p), len(fv2[0]), ok.ctypes.data if ok is not None else None,
            po.ctypes.data if po is not None else None, int(check_orientation), _p(out, _i32p)),
            "vsg_frame_search_for_triangulation")
        return nm, out[:self.N]

    def SearchForTriangulationEpipolar(self, no_mp1, kf2, no_mp2, F12, ep, scale_factors2, level_sigma2_2, only_stereo,
                                       coarse, check_orientation, fv1=None, fv2=None):
        """ORBmatcher::SearchForTriangulation (ORBmatcher.cc:902-1146), self = pKF1, kf2 = pKF2, both resident, with the
        epipole gate and Pinhole::epipolarConstrain evaluated on the device (vsg_frame_search_for_triangulation_epipolar).
        no_mpX[i] = !pKFX->GetMapPoint(i); F12 = the 3 x 3 fundamental matrix (row-major), ep = the epipole in kf2;
        scale_factors2 / level_sigma2_2 = pKF2's mvScaleFactors / mvLevelSigma2.  fv1 = fv2 = None: the FeatureVectors both
        frames keep resident since their ComputeBoW are joined on the device.  Returns (nmatches, matches12)."""
        m1, m2 = _u8(no_mp1), _u8(no_mp2)
        F, e = _f32(np.asarray(F12).reshape(9)), _f32(np.asarray(ep).reshape(2))
        sf, s2 = _f32(scale_factors2), _f32(level_sigma2_2)
        assert len(sf) == len(s2)
        if (fv1 is None) != (fv2 is None):
            raise ValueError("fv1 and fv2: both or neither")
        a1 = a2 = (None, None, None)
        keep = []
        if fv1 is not None:
            keep = [_i32(x) for x in fv1] + [_i32(x) for x in fv2]
            a1, a2 = tuple(_p(x, _i32p) for x in keep[:3]), tuple(_p(x, _i32p) for x in keep[3:])
        out = np.full(max(self.N, 1), -1, np.int32)
        nm = _check(self._L.vsg_frame_search_for_triangulation_epipolar(
            self._h, _p(m1, _u8p), *a1, len(fv1[0]) if fv1 is not None else 0, kf2.handle, _p(m2, _u8p), *a2,
            len(fv2[0]) if fv2 is not None else 0, _p(F, _f32p), _p(e, _f32p), _p(sf, _f32p), _p(s2, _f32p), len(sf),
            int(bool(only_stereo)), int(bool(coarse)), int(bool(check_orientation)), _p(out, _i32p)),
            "vsg_frame_search_for_triangulation_epipolar")
        return nm, out[:self.N]

    def SetStereoPoints(self, xyz_c, cos_parallax):
        """vsg_frame_set_stereo_points: per feature x3Dc of KeyFrame::UnprojectStereo (KeyFrame.cc:887-894) and
        cos(2 * atan2(mb / 2, mvDepth[i])) (LocalMapping.cc:569), computed by the caller; once per keyframe, dropped by
        the next upload."""
        x, c = _f32(np.asarray(xyz_c).reshape(-1)), _f32(cos_parallax)
        assert len(x) >= 3 * self.N and len(c) >= self.N
        _check(self._L.vsg_frame_set_stereo_points(self._h, _p(x, _f32p), _p(c, _f32p)), "vsg_frame_set_stereo_points")
        return self

    def _tri_args(self, params, tables, mp, free_slots):
        sf1, s1, sf2, s2 = (_f32(t) for t in tables)
        assert len(sf1) == len(s1) == len(sf2) == len(s2)
        fs = _i32(free_slots if free_slots is not None else [])
        n_free = 0 if free_slots is None else len(free_slots)
        n = max(self.N, 1)
        out = dict(reason=np.zeros(n, np.uint8), source=np.zeros(n, np.uint8), x3d=np.zeros((n, 3), np.float32),
                   new_slot=np.zeros(n, np.int32))
        created = C.c_int32(0)
        tail = [C.byref(params), _p(sf1, _f32p), _p(s1, _f32p), _p(sf2, _f32p), _p(s2, _f32p), len(sf1),
                mp.handle if mp is not None else None, _p(fs, _i32p), n_free]
        outs = [_p(out["reason"], _u8p), _p(out["source"], _u8p), _p(out["x3d"], _f32p), _p(out["new_slot"], _i32p),
                C.byref(created)]
        return tail, outs, out, created, (sf1, s1, sf2, s2, fs)

    def TriangulateMatches(self, kf2, matches12, params, scale_factors1, level_sigma2_1, scale_factors2, level_sigma2_2,
                           mp=None, free_slots=None):
        """The loop over one neighbour's matches of LocalMapping::CreateNewMapPoints (LocalMapping.cc:475-708), self =
        mpCurrentKeyFrame, kf2 = pKF2, for a match list the caller holds (vsg_frame_triangulate_matches).  mp = a
        MapPoints store the accepted pairs are written into, in ascending idx1 into free_slots (None: geometry only).
        Returns dict(reason, source, x3d, new_slot, n_created)."""
        m = _i32(matches12)
        assert len(m) >= self.N
        tail, outs, out, created, keep = self._tri_args(params, (scale_factors1, level_sigma2_1, scale_factors2,
                                                                 level_sigma2_2), mp, free_slots)
        _check(self._L.vsg_frame_triangulate_matches(self._h, kf2.handle, _p(m, _i32p), *tail, *outs),
               "vsg_frame_triangulate_matches")
        return dict({k: v[:self.N] for k, v in out.items()}, n_created=created.value)

    def CreateNewMapPoints(self, no_mp1, kf2, no_mp2, F12, ep, only_stereo, coarse, check_orientation, params,
                           scale_factors1, level_sigma2_1, scale_factors2, level_sigma2_2, mp=None, free_slots=None,
                           fv1=None, fv2=None):
        """One neighbour of LocalMapping::CreateNewMapPoints (LocalMapping.cc:456-708) in one enqueue and one wait
        (vsg_frame_create_new_map_points): SearchForTriangulationEpipolar's search, the rotation filter on the device, then
        TriangulateMatches on what is left.  Returns dict(nmatches, matches12, reason, source, x3d, new_slot, n_created)."""
        m1, m2 = _u8(no_mp1), _u8(no_mp2)
        F, e = _f32(np.asarray(F12).reshape(9)), _f32(np.asarray(ep).reshape(2))
        if (fv1 is None) != (fv2 is None):
            raise ValueError("fv1 and fv2: both or neither")
        a1 = a2 = (None, None, None)
        keep_fv = []
        if fv1 is not None:
            keep_fv = [_i32(x) for x in fv1] + [_i32(x) for x in fv2]
            a1, a2 = tuple(_p(x, _i32p) for x in keep_fv[:3]), tuple(_p(x, _i32p) for x in keep_fv[3:])
        tail, outs, out, created, keep = self._tri_args(params, (scale_factors1, level_sigma2_1, scale_factors2,
                                                                 level_sigma2_2), mp, free_slots)
        m12 = np.full(max(self.N, 1), -1, np.int32)
        nm = _check(self._L.vsg_frame_create_new_map_points(
            self._h, _p(m1, _u8p), *a1, len(fv1[0]) if fv1 is not None else 0, kf2.handle, _p(m2, _u8p), *a2,
            len(fv2[0]) if fv2 is not None else 0, _p(F, _f32p), _p(e, _f32p), int(bool(only_stereo)), int(bool(coarse)),
            int(bool(check_orientation)), *tail, _p(m12, _i32p), *outs), "vsg_frame_create_new_map_points")
        return dict({k: v[:self.N] for k, v in out.items()}, nmatches=nm, matches12=m12[:self.N], n_created=created.value)

    def ComputeBoW(self, voc, levelsup=4):
        """Frame::ComputeBoW on the resident descriptors; same dict as ORBVocabulary.transform."""
        n = self.N
        cap = n + 1
        bi, bv = np.zeros(cap, np.int32), np.zeros(cap, np.float64)
        fn, fo, fi = np.zeros(cap, np.int32), np.zeros(cap + 1, np.int32), np.zeros(cap, np.int32)
        w_of, n_of, wt = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
        nb, nf = C.c_int32(), C.c_int32()
        f64p = C.POINTER(C.c_double)
        _check(self._L.vsg_frame_bow_transform(voc._h, self._h, int(levelsup), _p(bi, _i32p), _p(bv, f64p), cap,
                                               C.byref(nb), _p(fn, _i32p), _p(fo, _i32p), _p(fi, _i32p), cap,
                                               C.byref(nf), _p(w_of, _i32p), _p(n_of, _i32p), _p(wt, f64p)),
               "vsg_frame_bow_transform")
        return dict(bow_ids=bi[:nb.value].copy(), bow_vals=bv[:nb.value].copy(),
                    fv=(fn[:nf.value].copy(), fo[:nf.value + 1].copy(), fi[:fo[nf.value]].copy()),
                    word=w_of[:n].copy(), node=n_of[:n].copy(), weight=wt[:n].copy())


def debug_epipolar_pairs(kf1, kf2, i1, i2, F12, ep, scale_factors2, level_sigma2_2, only_stereo, coarse):
    """Test hook (include/vsg_orb_debug_epipolar.h): the reason code the DEVICE predicate of SearchForTriangulationEpipolar gives
    each listed pair (feature i1[p] of kf1, i2[p] of kf2): 0 pass, 1 not stereo under only_stereo, 2 epipole gate,
    3 den == 0, 4 chi-square."""
    a, b = _i32(i1), _i32(i2)
    assert len(a) == len(b)
    F, e = _f32(np.asarray(F12).reshape(9)), _f32(np.asarray(ep).reshape(2))
    sf, s2 = _f32(scale_factors2), _f32(level_sigma2_2)
    out = np.zeros(max(len(a), 1), np.uint8)
    _check(load_library().vsg_debug_epipolar_pairs(
        kf1.handle, kf2.handle, len(a), _p(a, _i32p), _p(b, _i32p), _p(F, _f32p), _p(e, _f32p), _p(sf, _f32p), _p(s2, _f32p),
        len(sf), int(bool(only_stereo)), int(bool(coarse)), _p(out, _u8p)), "vsg_debug_epipolar_pairs")
    return out[:len(a)]


def SearchBySim3(kf1, kf2, q1, q2):
    """ORBmatcher::SearchBySim3 (ORBmatcher.cc:1448-1665) on two resident KeyFrames.  q1 / q2: dicts with idx, desc,
    u, v, radius, level of the points projected KF1 -> KF2 and KF2 -> KF1.  Returns (nFound, matches12)."""
    L = load_library()

    def unpack(q):
        d = _u8(q["desc"]).reshape(-1, 32)
        return (len(d), _i32(q["idx"]), d if len(d) else np.zeros((1, 32), np.uint8), _f32(q["u"]), _f32(q["v"]),
                _f32(q["radius"]), _i32(q["level"]))
    a, b = unpack(q1), unpack(q2)
    out = np.full(max(kf1.N, 1), -1, np.int32)
    nf = _check(L.vsg_frame_search_by_sim3(
        kf1.handle, kf2.handle, a[0], _p(a[1], _i32p), _p(a[2], _u8p), _p(a[3], _f32p), _p(a[4], _f32p), _p(a[5], _f32p),
        _p(a[6], _i32p), b[0], _p(b[1], _i32p), _p(b[2], _u8p), _p(b[3], _f32p), _p(b[4], _f32p), _p(b[5], _f32p),
        _p(b[6], _i32p), _p(out, _i32p)), "vsg_frame_search_by_sim3")
    return nf, out[:kf1.N]


def fuse_decide(query_mp, best_idx, best_dist, sim3_form, slot_mp, mp_obs, mp_bad):
    """The ordered replace-vs-add pass of Fuse (ORBmatcher.cc:1308-1327, :1429-1444) on flattened map-point ids.
    Returns (nFused, action, other_mp, slot_mp, mp_obs, mp_bad) -- the three state arrays are updated copies."""
    qm, bi, bd = _i32(query_mp), _i32(best_idx), _i32(best_dist)
    sm, ob, bad = _i32(slot_mp).copy(), _i32(mp_obs).copy(), _u8(mp_bad).copy()
    act, oth = np.zeros(max(len(qm), 1), np.int32), np.zeros(max(len(qm), 1), np.int32)
    nf = _check(load_library().vsg_fuse_decide(len(query_mp), _p(qm, _i32p), _p(bi, _i32p), _p(bd, _i32p),
                                               int(sim3_form), _p(sm, _i32p), len(slot_mp), _p(ob, _i32p),
                                               _p(bad, _u8p), len(mp_obs), _p(act, _i32p), _p(oth, _i32p)),
                "vsg_fuse_decide")
    return nf, act[:len(query_mp)], oth[:len(query_mp)], sm, ob, bad


def stereo_bow_search(ex_left, frame_l, ex_right, frame_r, fl, fr, mb, mbf, voc, levelsup=4, kf=None, kf_valid=None,
                      nnratio=0.7, check_orientation=True):
    """vsg_frame_stereo_bow_search: ComputeStereoMatches + ComputeBoW (+ SearchByBoW(kf, fl) when kf is given) of one stereo
    Frame in one enqueue and one wait.  Returns dict(u_right, depth, n_stereo, bow_ids, bow_vals, fv, n_match, match_f)."""
    L = load_library()
    n = fl.N
    cap = n + 1
    ur, dep = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
    bi, bv = np.zeros(cap, np.int32), np.zeros(cap, np.float64)
    fn, fo, fi = np.zeros(cap, np.int32), np.zeros(cap + 1, np.int32), np.zeros(cap, np.int32)
    match = np.full(cap, -1, np.int32)
    ns, nb, nf, nm = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    f64p = C.POINTER(C.c_double)
    kv = _u8(kf_valid) if kf is not None else None
    _check(L.vsg_frame_stereo_bow_search(
        ex_left.handle, int(frame_l), ex_right.handle, int(frame_r), fl.handle, fr.handle, float(mb), float(mbf), _p(ur, _f32p),
        _p(dep, _f32p), C.byref(ns), voc._h, int(levelsup), _p(bi, _i32p), _p(bv, f64p), cap, C.byref(nb), _p(fn, _i32p),
        _p(fo, _i32p), _p(fi, _i32p), cap, C.byref(nf), kf.handle if kf is not None else None,
        _p(kv, _u8p) if kf is not None else None, float(np.float32(nnratio)), int(check_orientation), _p(match, _i32p),
        C.byref(nm)), "vsg_frame_stereo_bow_search")
    return dict(u_right=ur[:n], depth=dep[:n], n_stereo=ns.value, bow_ids=bi[:nb.value].copy(), bow_vals=bv[:nb.value].copy(),
                fv=(fn[:nf.value].copy(), fo[:nf.value + 1].copy(), fi[:fo[nf.value]].copy()), n_match=nm.value,
                match_f=match[:n])


def ComputeStereoMatches_resident(ex_left, frame_l, ex_right, frame_r, fl, fr, mb, mbf):
    """Frame::ComputeStereoMatches on two resident feature sets (vsg_frame_stereo_matches)."""
    ur, dep = np.zeros(max(fl.N, 1), np.float32), np.zeros(max(fl.N, 1), np.float32)
    _check(load_library().vsg_frame_stereo_matches(ex_left.handle, int(frame_l), ex_right.handle, int(frame_r),
                                                   fl.handle, fr.handle, float(mb), float(mbf), _p(ur, _f32p),
                                                   _p(dep, _f32p)), "vsg_frame_stereo_matches")
    return ur[:fl.N], dep[:fl.N]
