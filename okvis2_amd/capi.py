"""ctypes binding of libokvfe.so (the C ABI declared in include/okvfe.h).

This is the product path used by bench.py and the GPU tests: every call goes through the C ABI
into the hand-written HIP kernels.  There is no Python or CPU implementation behind it -- if the
library is missing or no gfx950 device is present, loading / okvfe_create fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OKVFE_LIB") or os.path.join(_HERE, "libokvfe.so")  # OKVFE_LIB: A/B builds

OK = 0
ERR_INVALID_ARGUMENT, ERR_NO_DEVICE, ERR_OUT_OF_MEMORY, ERR_UNSUPPORTED, ERR_CAPACITY, ERR_DEVICE, \
    ERR_NOT_READY = 1, 2, 3, 4, 5, 6, 7
ABI_VERSION = 8
DIST_NONE, DIST_RADTAN, DIST_EQUIDISTANT, DIST_RADTAN8 = 0, 1, 2, 3
SCORE_HARRIS, SCORE_AGAST_9_16, SCORE_BRISK_SCALESPACE = 0, 1, 2
DESC_BYTES = 48

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
STEREO_MATCH_DTYPE = np.dtype([("k1", "<i4"), ("dist", "<i4"), ("initialisable", "<i4"),
                               ("pad", "<i4"), ("hp_W", "<f8", (4,))])
CAND_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("dist", "<i4")])
MOTION_MATCH_DTYPE = np.dtype([("k1", "<i4"), ("dist", "<i4"), ("initialisable", "<i4"),
                               ("accepted", "<i4"), ("cos_quality", "<f8"), ("hp_W", "<f8", (4,))])
COVERAGE_DTYPE = np.dtype([("n_keypoints", "<i4"), ("n_matched", "<i4"), ("detections_area", "<i4"),
                           ("matches_area", "<i4"), ("intersection_area", "<i4"), ("union_area", "<i4")])
OVERLAP_COUNTS_DTYPE = np.dtype([("n_keypoints", "<i4", (2,)), ("n_matched", "<i4", (2,)),
                                 ("intersection_area", "<i4", (2,)), ("union_area", "<i4", (2,))])
KPTRAD = 0.09  # Frontend.cpp:104
KEYFRAME_OVERLAP_THRESHOLD = 0.55  # keyframeInsertionOverlapThreshold_, Frontend.cpp:145


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("max_batch", C.c_int32), ("num_cameras", C.c_int32),
                ("uniformity_radius", C.c_float), ("octaves", C.c_int32),
                ("absolute_threshold", C.c_int32), ("max_keypoints", C.c_int32),
                ("rotation_invariant", C.c_int32), ("scale_invariant", C.c_int32),
                ("match_threshold", C.c_int32), ("max_candidates", C.c_int32),
                ("score_type", C.c_int32), ("box_scale", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fu", C.c_double), ("fv", C.c_double),
                ("cu", C.c_double), ("cv", C.c_double), ("distortion", C.c_int32),
                ("d", C.c_double * 4)]


class CameraExt(C.Structure):
    """okvfe_camera_ext (ABI 8): base.d = k1 k2 p1 p2, d_ext = k3 k4 k5 k6 of DIST_RADTAN8."""
    _fields_ = [("base", Camera), ("d_ext", C.c_double * 4)]


class Pose(C.Structure):
    _fields_ = [("C", C.c_double * 9), ("r", C.c_double * 3)]


class StereoPair(C.Structure):
    _fields_ = [("image0", C.c_int32), ("image1", C.c_int32), ("T_WC0", Pose), ("T_WC1", Pose),
                ("f0", C.c_double), ("f1", C.c_double)]


class PatternData(C.Structure):
    """okvfe_pattern: the extractor's sampling pattern as data (okvfe_get_pattern / okvfe_set_pattern)."""
    _fields_ = [("n_points", C.c_int32), ("px", C.c_float * 72), ("py", C.c_float * 72),
                ("sigma_half", C.c_float * 72), ("n_short", C.c_int32),
                ("short_i", C.c_uint8 * 384), ("short_j", C.c_uint8 * 384),
                ("n_long", C.c_int32), ("long_i", C.c_uint8 * 1100), ("long_j", C.c_uint8 * 1100),
                ("long_wdx", C.c_int32 * 1100), ("long_wdy", C.c_int32 * 1100), ("border", C.c_int32)]


class MapDevice(C.Structure):
    """okvfe_map_device: the pooled landmark set in device memory (all members device pointers)."""
    _fields_ = [("n_landmarks", C.c_int32), ("desc_begin", C.c_void_p), ("pool", C.c_void_p),
                ("projections", C.c_void_p), ("e0_W", C.c_void_p), ("r0_W", C.c_void_p)]


class DeviceOutputs(C.Structure):
    _fields_ = [("max_keypoints", C.c_int32), ("counts", C.c_void_p), ("keypoints", C.c_void_p),
                ("descriptors", C.c_void_p), ("backproj", C.c_void_p),
                ("backproj_valid", C.c_void_p), ("scores", C.c_void_p),
                ("detect_counts", C.c_void_p), ("candidate_counts", C.c_void_p),
                ("score_pitch", C.c_int32), ("score_strips", C.c_int32)]


EXPORTS = [
    "okvfe_create", "okvfe_destroy", "okvfe_last_error", "okvfe_abi_version",
    "okvfe_set_camera_maps", "okvfe_set_camera", "okvfe_build_awareness_maps",
    "okvfe_detect_describe", "okvfe_detect", "okvfe_detect_ahead", "okvfe_detect_describe_batch_device",
    "okvfe_get_device_outputs", "okvfe_score_column", "okvfe_set_heavy_kernel_chaining", "okvfe_set_keep_score_map", "okvfe_set_internal_lanes", "okvfe_lanes_join", "okvfe_set_fp64_reduction", "okvfe_scale_index", "okvfe_download_image_result", "okvfe_harris_score_device", "okvfe_harris_byte_mover_device",
    "okvfe_match_stereo_batch_device", "okvfe_match_stereo", "okvfe_hamming_candidates",
    "okvfe_hamming_argmin", "okvfe_popcnt_xor", "okvfe_gather_block_bytes",
    "okvfe_pack_gather_block_device", "okvfe_match_stereo_blocks_device",
    "okvfe_profile_enable", "okvfe_profile_read", "okvfe_match_motion_stereo_blocks_device",
    "okvfe_detect_batch_device", "okvfe_describe_batch_device", "okvfe_camera_overlap", "okvfe_compute",
    "okvfe_match_motion_stereo", "okvfe_match_to_map",
    "okvfe_format_keypoint_lines", "okvfe_parse_keypoint_lines", "okvfe_fbrisk_mean",
    "okvfe_match_to_map_uninitialised", "okvfe_pack_gather_blocks_device",
    "okvfe_match_stereo_blocks_batch_device", "okvfe_check_capacity",
    "okvfe_detect_describe_batch_host", "okvfe_verify_place_match", "okvfe_fbrisk_transform",
    "okvfe_match_to_map_landmarks", "okvfe_bow_vector", "okvfe_bow_query_l1",
    "okvfe_get_pattern", "okvfe_set_pattern", "okvfe_pattern_kernel_class",
    "okvfe_match_to_map_blocks_device", "okvfe_match_to_map_uninitialised_blocks_device",
    "okvfe_verify_place_blocks_device",
    "okvfe_comm_unique_id", "okvfe_comm_create", "okvfe_comm_wrap", "okvfe_comm_destroy",
    "okvfe_comm_world", "okvfe_comm_rank", "okvfe_comm_last_error", "okvfe_gather_blocks",
    "okvfe_device_alloc", "okvfe_device_free", "okvfe_stream_create", "okvfe_stream_destroy",
    "okvfe_stream_synchronize", "okvfe_copy_to_device", "okvfe_copy_to_host", "okvfe_device_fill",
    "okvfe_set_camera_ext", "okvfe_build_awareness_maps_ext", "okvfe_camera_overlap_ext",
    "okvfe_match_motion_stereo_ext",
    "okvfe_keyframe_coverage_blocks_device", "okvfe_keyframe_coverage", "okvfe_keyframe_decision",
    "okvfe_landmark_table_check_device", "okvfe_match_to_map_table_blocks_device",
    "okvfe_match_to_map_table_uninitialised_blocks_device",
    "okvfe_ransac3d2d_consensus_blocks_device", "okvfe_remove_outliers_blocks_device",
    "okvfe_match_motion_stereo_blocks_batch_device",
    "okvfe_place_landmark_set", "okvfe_place_claims_blocks_device", "okvfe_place_consensus_blocks_device",
    "okvfe_place_hessian_blocks_device", "okvfe_place_refine_blocks_device",
    "okvfe_vocabulary_check", "okvfe_bow_vectors_blocks_device", "okvfe_place_query_blocks_device",
    "okvfe_bow_database_add_blocks_device", "okvfe_bow_database_check_device",
    "okvfe_stereo_insert_blocks_device",
    "okvfe_ransac2d2d_consensus_blocks_device",
    "okvfe_overlap_pairs_blocks_device", "okvfe_overlap_fraction", "okvfe_motion_frame_order",
    "okvfe_tracking_quality",
    "okvfe_imu_propagation", "okvfe_imu_propagation_blocks_device",
    "okvfe_p3p_hypothesis", "okvfe_ransac3d2d_hypotheses_blocks_device", "okvfe_place_hypotheses_blocks_device",
    "okvfe_twopt_rotation_hypothesis", "okvfe_fivept_hypothesis", "okvfe_ransac2d2d_hypotheses_blocks_device",
]
# exported for the tests and deliberately not declared in include/okvfe.h (EXPORTS is exactly what the header declares)
TEST_HOOKS = [
    "okvfe_test_set_map_table_workspace_limit", "okvfe_test_ransac_chunk_records", "okvfe_test_ransac_ring_records",
    "okvfe_test_ransac2d2d_chunk_records", "okvfe_test_ransac2d2d_ring_records", "okvfe_test_ransac2d2d_id_slot",
    "okvfe_test_place_hessian_chunk_terms", "okvfe_test_context_sizes",
]

STAGES = ["harris", "nms", "sort", "select", "map", "describe", "compact", "match"]

_LIB = None


class LandmarkTable(C.Structure):
    _fields_ = [("n_landmarks", C.c_int32), ("n_observations", C.c_int32), ("n_poses", C.c_int32),
                ("hp_W", C.c_void_p), ("quality", C.c_void_p), ("obs_begin", C.c_void_p),
                ("obs_pose", C.c_void_p), ("obs_desc", C.c_void_p), ("obs_backproj", C.c_void_p),
                ("poses", C.c_void_p)]


class LandmarkPool(C.Structure):
    _fields_ = [("status", C.c_void_p), ("n_desc", C.c_void_p), ("obs_rows", C.c_void_p),
                ("projection", C.c_void_p), ("e_W", C.c_void_p), ("r_W", C.c_void_p)]


class LandmarkTableDevice(C.Structure):
    """okvfe_landmark_table_device: the landmark table in device memory (every pointer a device pointer)."""
    _fields_ = LandmarkTable._fields_


class LandmarkPoolDevice(C.Structure):
    """okvfe_landmark_pool_device: per-frame pooling results, device arrays n_frames x L (any member may be None)."""
    _fields_ = LandmarkPool._fields_


class StereoInsertDevice(C.Structure):
    """okvfe_stereo_insert_device: device pointers; action and lm are optional (None)."""
    _fields_ = [("action", C.c_void_p), ("lm", C.c_void_p), ("landmark_out", C.c_void_p), ("counts", C.c_void_p)]


STEREO_MAX_PAIRS = 16
STEREO_REINIT, STEREO_CREATE, STEREO_OBS0, STEREO_OBS1 = 1, 2, 4, 8


class RansacResultDevice(C.Structure):
    """okvfe_ransac_result_device: device pointers; the last four are optional (None)."""
    _fields_ = [("n_correspondences", C.c_void_p), ("best_hypothesis", C.c_void_p), ("n_inliers", C.c_void_p),
                ("accepted", C.c_void_p), ("hyp_inliers", C.c_void_p), ("state", C.c_void_p),
                ("distance", C.c_void_p), ("landmark_out", C.c_void_p)]


class RansacHypothesesDevice(C.Structure):
    """okvfe_ransac_hypotheses_device: device pointers; the last three are optional (None)."""
    _fields_ = [("hypotheses", C.c_void_p), ("hyp_valid", C.c_void_p), ("n_correspondences", C.c_void_p),
                ("samples", C.c_void_p), ("n_solutions", C.c_void_p)]


class Ransac2d2dResultDevice(C.Structure):
    """okvfe_ransac2d2d_result_device: device pointers; the last six are optional (None)."""
    _fields_ = [(n, C.c_void_p) for n in (
        "n_correspondences", "rot_best", "rot_inliers", "rel_best", "rel_inliers", "branch", "removed",
        "total_inliers", "rotation_only", "success",
        "rot_hyp_inliers", "rel_hyp_inliers", "match1", "state", "distance", "landmark1_out")]


class Ransac2d2dHypothesesDevice(C.Structure):
    """okvfe_ransac2d2d_hypotheses_device: device pointers; the last four are optional (None)."""
    _fields_ = [(n, C.c_void_p) for n in (
        "rot_hyp", "rot_valid", "rel_hyp", "rel_valid", "n_correspondences", "rot_samples", "rel_samples", "rel_n_roots")]


class PlaceSetDevice(C.Structure):
    """okvfe_place_set_device: the old frame's landmark set, hp a device pointer (L x 4 doubles)."""
    _fields_ = [("n_landmarks", C.c_int32), ("hp", C.c_void_p)]


class PlaceClaimsDevice(C.Structure):
    """okvfe_place_claims_device: device pointers, all required."""
    _fields_ = [("n_matches", C.c_void_p), ("n_points", C.c_void_p), ("n_correspondences", C.c_void_p),
                ("gate", C.c_void_p), ("match_landmark", C.c_void_p)]


class PlaceHessianDevice(C.Structure):
    """okvfe_place_hessian_device: device pointers; residual and jacobian_minimal are optional (None)."""
    _fields_ = [("H", C.c_void_p), ("n_terms", C.c_void_p), ("n_singular", C.c_void_p), ("residual", C.c_void_p),
                ("jacobian_minimal", C.c_void_p)]


class PlaceRefineDevice(C.Structure):
    """okvfe_place_refine_device: device pointers; all but poses and status are optional (None)."""
    _fields_ = [(k, C.c_void_p) for k in ("poses", "status", "n_iterations", "n_accepted", "n_terms", "cost", "start_poses",
                                          "H", "n_singular")]


class ImuParams(C.Structure):
    """okvfe_imu_params"""
    _fields_ = [(k, C.c_double) for k in ("a_max", "g_max", "sigma_g_c", "sigma_a_c", "sigma_gw_c", "sigma_aw_c", "g")]


class ImuResultDevice(C.Structure):
    """okvfe_imu_result_device: device pointers (host pointers for okvfe_imu_propagation); the last four are optional
    (None)."""
    _fields_ = [("pose", C.c_void_p), ("speed_and_bias", C.c_void_p), ("n_propagated", C.c_void_p),
                ("status", C.c_void_p), ("n_out_of_range", C.c_void_p), ("jacobian", C.c_void_p),
                ("covariance", C.c_void_p), ("T_WC", C.c_void_p), ("gravity_C", C.c_void_p)]


IMU_SAMPLE_DOUBLES, IMU_STATE_DOUBLES = 8, 18
IMU_STATUS_FRONT_AFTER_START, IMU_STATUS_EMPTY = 1, 2


class VocabularyDevice(C.Structure):
    """okvfe_vocabulary_device: the DBoW2 vocabulary tree; device pointers (host pointers for okvfe_vocabulary_check)."""
    _fields_ = [("n_nodes", C.c_int32), ("n_words", C.c_int32), ("weighting", C.c_int32), ("normalise_l1", C.c_int32),
                ("node_descriptors", C.c_void_p), ("child_begin", C.c_void_p), ("child_index", C.c_void_p),
                ("node_word", C.c_void_p), ("word_weight", C.c_void_p)]


class BowVectorsDevice(C.Structure):
    """okvfe_bow_vectors_device: BowVectors of a batch, device rows M x stride."""
    _fields_ = [("n_words", C.c_void_p), ("ids", C.c_void_p), ("values", C.c_void_p), ("stride", C.c_int32),
                ("n_vocabulary_words", C.c_int32)]


class BowDatabaseDevice(C.Structure):
    """okvfe_bow_database_device: device arrays in okvfe_bow_query_l1's layout; n_entries is a HOST field."""
    _fields_ = [("begin", C.c_void_p), ("ids", C.c_void_p), ("values", C.c_void_p), ("cap_entries", C.c_int32),
                ("cap_words", C.c_int32), ("n_entries", C.c_int32), ("overflow", C.c_void_p)]


class PlaceCandidatesDevice(C.Structure):
    """okvfe_place_candidates_device: device pointers; entry / score are M x cap rows."""
    _fields_ = [("n_listed", C.c_void_p), ("n_candidates", C.c_void_p), ("entry", C.c_void_p), ("score", C.c_void_p),
                ("cap", C.c_int32)]


class MotionClaimDevice(C.Structure):
    """okvfe_motion_claim_device: device pointers; matched1_out is optional (None)."""
    _fields_ = [("claimed", C.c_void_p), ("n_claimed", C.c_void_p), ("matched1_out", C.c_void_p)]


MOTION_CLAIM_MAX_KEYPOINTS = 12288  # K above it: claims are OKVFE_ERR_UNSUPPORTED

RANSAC_MAX_HYPOTHESES = 64  # OKVFE_RANSAC_MAX_HYPOTHESES
RANSAC_THRESHOLD = 16.0     # Frontend.cpp:2235
REMOVE_OUTLIERS_MAX_ERROR = 4.0  # Frontend.cpp:2185
RANSAC2D2D_THRESHOLD = 9.0  # Frontend.cpp:2312, 2329
RANSAC2D2D_MAX_KEYPOINTS = 4095  # K above it: okvfe_ransac2d2d_consensus_blocks_device is OKVFE_ERR_UNSUPPORTED
PLACE_CLAIMS_MAX_KEYPOINTS = 12288  # K above it: okvfe_place_claims_blocks_device is OKVFE_ERR_UNSUPPORTED
BOW_MAX_FEATURES = 8192  # n_cams x K above it: okvfe_bow_vectors_blocks_device is OKVFE_ERR_UNSUPPORTED
PLACE_MIN_SCORE = 0.4    # Frontend.cpp:802
PLACE_VERDICTS = ("gate", "too_few_correspondences", "rejected", "verified")  # okvfe_place_consensus_blocks_device


class OkvfeError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"okvfe status {status}: {message}")
        self.status = status


def lib():
    """Loads libokvfe.so; raises if it has not been built (no fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                f"{LIB_PATH} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
        # PyTorch-ROCm ships its own libamdhip64; whichever HIP runtime is loaded second finds no
        # GPU.  Importing torch first makes libokvfe.so bind to the runtime torch already loaded
        # (same soname), so device pointers and streams are shared.  Without torch installed the
        # system runtime under /opt/rocm is used.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.okvfe_last_error.restype = C.c_char_p
        L.okvfe_last_error.argtypes = [C.c_void_p]
        L.okvfe_popcnt_xor.restype = C.c_uint32
        L.okvfe_gather_block_bytes.restype = C.c_size_t
        L.okvfe_gather_block_bytes.argtypes = [C.c_void_p]
        L.okvfe_destroy.argtypes = [C.c_void_p]
        L.okvfe_destroy.restype = None
        L.okvfe_comm_last_error.restype = C.c_char_p
        L.okvfe_comm_destroy.argtypes = [C.c_void_p]
        L.okvfe_comm_destroy.restype = None
        L.okvfe_gather_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.okvfe_comm_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        V = C.c_void_p
        L.okvfe_match_to_map_table_uninitialised_blocks_device.restype = C.c_int32
        L.okvfe_match_to_map_table_uninitialised_blocks_device.argtypes = [
            V, V, V, V, C.c_int32, V, V, C.c_int32, V, V, V, V, V, V, V, V]
        L.okvfe_ransac3d2d_consensus_blocks_device.restype = C.c_int32
        L.okvfe_ransac3d2d_consensus_blocks_device.argtypes = [
            V, V, V, C.c_int32, C.c_int32, V, V, V, V, V, C.c_int32, C.c_double, C.c_int32, V, V]
        L.okvfe_ransac2d2d_consensus_blocks_device.restype = C.c_int32
        L.okvfe_ransac2d2d_consensus_blocks_device.argtypes = [
            V, V, C.c_int32, V, C.c_int32, C.c_int32, V, V, C.c_int32, V, V, V, V, C.c_int32, V, V, V, V, C.c_int32,
            C.c_double, C.c_int32, V, V]
        L.okvfe_ransac2d2d_hypotheses_blocks_device.restype = C.c_int32
        L.okvfe_ransac2d2d_hypotheses_blocks_device.argtypes = [
            V, V, C.c_int32, V, C.c_int32, C.c_int32, V, V, C.c_int32, V, V, V, V, C.c_int32, V, C.c_uint64, C.c_int32,
            V, V]
        L.okvfe_twopt_rotation_hypothesis.restype = C.c_int32
        L.okvfe_twopt_rotation_hypothesis.argtypes = [V, V, V, V]
        L.okvfe_fivept_hypothesis.restype = C.c_int32
        L.okvfe_fivept_hypothesis.argtypes = [V, V, V, V, C.c_int32, V, V, V]
        L.okvfe_stereo_insert_blocks_device.restype = C.c_int32
        L.okvfe_stereo_insert_blocks_device.argtypes = [
            V, V, V, V, C.c_int32, C.c_int32, C.c_int32, C.c_int32, V, C.c_int32, V, V, V, V, V, V, V]
        L.okvfe_remove_outliers_blocks_device.restype = C.c_int32
        L.okvfe_remove_outliers_blocks_device.argtypes = [V, V, V, C.c_int32, V, V, C.c_double, V, V, V, V]
        L.okvfe_match_motion_stereo_blocks_batch_device.restype = C.c_int32
        L.okvfe_match_motion_stereo_blocks_batch_device.argtypes = [
            V, V, C.c_int32, V, C.c_int32, C.c_int32, V, V, V, V, V, V, V, V, V, V]
        L.okvfe_place_landmark_set.restype = C.c_int32
        L.okvfe_place_landmark_set.argtypes = [C.c_int32, V, V, V, V, V, C.c_int32, V, V, V, C.c_int32, V, C.c_int32, V, V]
        L.okvfe_place_claims_blocks_device.restype = C.c_int32
        L.okvfe_place_claims_blocks_device.argtypes = [V, V, V, C.c_int32, C.c_int32, V, V, C.c_int32, V, V]
        L.okvfe_place_consensus_blocks_device.restype = C.c_int32
        L.okvfe_place_consensus_blocks_device.argtypes = [
            V, V, V, C.c_int32, C.c_int32, V, V, V, V, V, V, C.c_int32, C.c_double, C.c_int32, V, V, V]
        L.okvfe_p3p_hypothesis.restype = C.c_int32
        L.okvfe_p3p_hypothesis.argtypes = [V, V, C.c_double, V, C.c_int32, V, V, V]
        L.okvfe_ransac3d2d_hypotheses_blocks_device.restype = C.c_int32
        L.okvfe_ransac3d2d_hypotheses_blocks_device.argtypes = [
            V, V, V, C.c_int32, C.c_int32, V, V, V, V, C.c_uint64, C.c_int32, V, V]
        L.okvfe_place_hypotheses_blocks_device.restype = C.c_int32
        L.okvfe_place_hypotheses_blocks_device.argtypes = [
            V, V, V, C.c_int32, C.c_int32, V, V, V, V, V, C.c_uint64, C.c_int32, V, V]
        L.okvfe_place_hessian_blocks_device.restype = C.c_int32
        L.okvfe_place_hessian_blocks_device.argtypes = [V, V, V, C.c_int32, C.c_int32, V, V, V, V, V, V, V, V]
        L.okvfe_vocabulary_check.restype = C.c_int32
        L.okvfe_vocabulary_check.argtypes = [V]
        L.okvfe_bow_vectors_blocks_device.restype = C.c_int32
        L.okvfe_bow_vectors_blocks_device.argtypes = [V, V, V, C.c_int32, C.c_int32, V, V, V]
        L.okvfe_place_query_blocks_device.restype = C.c_int32
        L.okvfe_place_query_blocks_device.argtypes = [V, V, V, C.c_int32, C.c_double, V, V, V, V]
        L.okvfe_bow_database_add_blocks_device.restype = C.c_int32
        L.okvfe_bow_database_add_blocks_device.argtypes = [V, V, V, C.c_int32, V, C.c_int32, V]
        L.okvfe_bow_database_check_device.restype = C.c_int32
        L.okvfe_bow_database_check_device.argtypes = [V, V, V]
        L.okvfe_overlap_pairs_blocks_device.restype = C.c_int32
        L.okvfe_overlap_pairs_blocks_device.argtypes = [
            V, V, C.c_int32, C.c_int32, C.c_int32, C.c_int32, V, V, V, C.c_int32, C.c_double, V, V, V]
        L.okvfe_overlap_fraction.restype = C.c_int32
        L.okvfe_overlap_fraction.argtypes = [V, C.c_int32, V]
        L.okvfe_motion_frame_order.restype = C.c_int32
        L.okvfe_motion_frame_order.argtypes = [V, V, C.c_int32, C.c_int32, V, V]
        L.okvfe_tracking_quality.restype = C.c_int32
        L.okvfe_tracking_quality.argtypes = [V, C.c_int32, C.c_int32, C.c_int32, C.c_double, V]
        L.okvfe_imu_propagation.restype = C.c_int32
        L.okvfe_imu_propagation.argtypes = [V, V, V, V, C.c_int32, C.c_int32, V, C.c_int32, V]
        L.okvfe_place_refine_blocks_device.restype = C.c_int32
        L.okvfe_place_refine_blocks_device.argtypes = [V, V, V, C.c_int32, C.c_int32, V, V, V, C.c_int32, V, V, V, V, V,
                                                       C.c_int32, V, V]
        L.okvfe_imu_propagation_blocks_device.restype = C.c_int32
        L.okvfe_imu_propagation_blocks_device.argtypes = [V, V, V, V, V, C.c_int32, C.c_int32, V, V, V]
        _LIB = L
    return _LIB


def _p(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return C.c_void_p(int(a))


STREAM_LEGACY_DEFAULT = 1  # OKVFE_STREAM_LEGACY_DEFAULT (= hipStreamLegacy)
COMM_ID_BYTES = 128


class Comm:
    """okvfe_comm: the RCCL communicator of the cross-camera gather, driven through the C ABI
    (okvfe_comm_create = ncclCommInitRank, okvfe_gather_blocks = ncclAllGather on the caller's
    stream).  Comm.local() is the world-1 communicator that never touches RCCL."""

    def __init__(self, handle, world, rank):
        self._h, self.world, self.rank = handle, world, rank

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        st = lib().okvfe_comm_unique_id(buf)
        if st != 0:
            raise OkvfeError(st, lib().okvfe_comm_last_error().decode())
        return bytes(buf)

    @classmethod
    def create(cls, comm_id, world: int, rank: int, device: int):
        h = C.c_void_p()
        idbuf = None
        if comm_id is not None:
            idbuf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(bytes(comm_id))
        st = lib().okvfe_comm_create(C.cast(idbuf, C.c_void_p) if idbuf is not None else None,
                                     int(world), int(rank), int(device), C.byref(h))
        if st != 0:
            raise OkvfeError(st, lib().okvfe_comm_last_error().decode())
        return cls(h, world, rank)

    @classmethod
    def local(cls):
        return cls.create(None, 1, 0, 0)

    def gather(self, send_ptr, recv_ptr, bytes_per_rank: int, stream=None):
        """raw stream handle: torch.cuda.Stream.cuda_stream (0 / None = the HIP null stream)"""
        raw = getattr(stream, "cuda_stream", stream)
        st = lib().okvfe_gather_blocks(self._h, _p(send_ptr), _p(recv_ptr), int(bytes_per_rank),
                                       C.c_void_p(int(raw)) if raw else None)
        if st != 0:
            raise OkvfeError(st, lib().okvfe_comm_last_error().decode())

    def close(self):
        if self._h:
            lib().okvfe_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass



def _s(stream):
    """Stream argument of the "_device" entry points: None = the context's own stream; a
    torch.cuda.Stream (anything with .cuda_stream) = that stream, torch's default stream (raw
    handle 0) becoming OKVFE_STREAM_LEGACY_DEFAULT; an int = a raw hipStream_t (0 = None)."""
    if stream is None:
        return None
    if hasattr(stream, "cuda_stream"):
        h = int(stream.cuda_stream)
        return C.c_void_p(h if h else STREAM_LEGACY_DEFAULT)
    return C.c_void_p(int(stream)) if int(stream) else None


def make_camera(cam):
    """okvfe_camera of a synth.Camera-like object; a CameraExt for DIST_RADTAN8 (8 coefficients),
    which the callers route to the _ext entry points."""
    c = Camera()
    c.width, c.height, c.fu, c.fv, c.cu, c.cv = cam.w, cam.h, cam.fu, cam.fv, cam.cu, cam.cv
    c.distortion = cam.dist_type
    for i in range(4):
        c.d[i] = cam.d[i]
    if cam.dist_type != DIST_RADTAN8:
        return c
    e = CameraExt()
    e.base = c
    for i in range(4):
        e.d_ext[i] = cam.d[4 + i]
    return e


def _camera_fn(name, *cams):
    """The entry point `name` or, when a camera is DIST_RADTAN8, its _ext form; and the structs."""
    structs = [make_camera(c) for c in cams]
    if not any(isinstance(s, CameraExt) for s in structs):
        return getattr(lib(), name), structs
    ext = [s if isinstance(s, CameraExt) else CameraExt(base=s) for s in structs]
    return getattr(lib(), name + "_ext"), ext


def make_pose(Cm, r) -> Pose:
    p = Pose()
    flat = np.asarray(Cm, dtype=np.float64).reshape(-1)
    for i in range(9):
        p.C[i] = float(flat[i])
    for i in range(3):
        p.r[i] = float(r[i])
    return p


def bow_vector(word_ids, word_weight, weighting=0, normalise_l1=True):
    """DBoW2 BowVector of a feature set from its word ids (okvfe_fbrisk_transform) and the
    vocabulary's word weights: (ascending word ids, values).  Host helper."""
    w = np.ascontiguousarray(word_ids, dtype=np.int32)
    ww = np.ascontiguousarray(word_weight, dtype=np.float64)
    ids = np.zeros(len(ww), dtype=np.int32)
    vals = np.zeros(len(ww), dtype=np.float64)
    n = C.c_int32()
    st = lib().okvfe_bow_vector(_p(w), len(w), _p(ww), len(ww), int(weighting), int(bool(normalise_l1)),
                                _p(ids), _p(vals), len(ww), C.byref(n))
    if st != OK:
        raise OkvfeError(st, "okvfe_bow_vector")
    return ids[:n.value].copy(), vals[:n.value].copy()


def vocabulary_check(node_desc, child_begin, child_index, node_word, word_weight, weighting=0, normalise_l1=True):
    """okvfe_vocabulary_check on host arrays: raises OkvfeError (the first offence named) unless the tree is a tree whose
    leaves carry words in range.  Host helper; call it once before the vocabulary is uploaded."""
    nd = np.ascontiguousarray(node_desc, dtype=np.uint8).reshape(-1, DESC_BYTES)
    cb = np.ascontiguousarray(child_begin, dtype=np.int32)
    ci = np.ascontiguousarray(child_index, dtype=np.int32)
    nw = np.ascontiguousarray(node_word, dtype=np.int32)
    ww = np.ascontiguousarray(word_weight, dtype=np.float64)
    if len(cb) != len(nd) + 1 or len(nw) != len(nd) or (len(cb) and cb[-1] > len(ci)):
        raise ValueError("vocabulary arrays: n_nodes descriptors and words, n_nodes + 1 child_begin, child_begin[-1] children")
    v = VocabularyDevice(len(nd), len(ww), int(weighting), int(bool(normalise_l1)), _p(nd), _p(cb),
                         _p(ci) if len(ci) else None, _p(nw), _p(ww))
    st = lib().okvfe_vocabulary_check(C.byref(v))
    if st != OK:
        raise OkvfeError(st, lib().okvfe_last_error(None).decode())


def place_landmark_set(n_kps, landmark_ids, landmarks, initialised, descriptors, eigen_tree=True):
    """okvfe_place_landmark_set: the landmark set of an old frame (Frontend.cpp:289-327) from its keypoints of all
    cameras, camera-major (n_kps per camera).  -> dict(ids [L] u64, hp [L, 4], desc_begin [L + 1] i32, pool [rows, 48])
    in ascending landmark id.  Host helper."""
    nk = np.ascontiguousarray(n_kps, dtype=np.int32)
    ids = np.ascontiguousarray(landmark_ids, dtype=np.uint64)
    hp = np.ascontiguousarray(landmarks, dtype=np.float64).reshape(-1, 4)
    ini = np.ascontiguousarray(initialised, dtype=np.uint8)
    desc = np.ascontiguousarray(descriptors, dtype=np.uint8).reshape(-1, 48)
    n = int(nk.sum())
    if not (len(ids) == len(hp) == len(ini) == len(desc) == n):
        raise ValueError("one id, landmark, flag and descriptor per keypoint")
    cap_l = cap_r = n
    out = dict(ids=np.zeros(cap_l, np.uint64), hp=np.zeros((cap_l, 4)), desc_begin=np.zeros(cap_l + 1, np.int32),
               pool=np.zeros((cap_r, 48), np.uint8))
    nl, nr = C.c_int32(0), C.c_int32(0)
    st = lib().okvfe_place_landmark_set(len(nk), _p(nk), _p(ids), _p(hp), _p(ini), _p(desc), 1 if eigen_tree else 0,
                                        _p(out["ids"]), _p(out["hp"]), _p(out["desc_begin"]), cap_l, _p(out["pool"]),
                                        cap_r, C.byref(nl), C.byref(nr))
    if st != 0:
        raise OkvfeError(st, "okvfe_place_landmark_set")
    L, R = nl.value, nr.value
    return dict(ids=out["ids"][:L], hp=out["hp"][:L], desc_begin=out["desc_begin"][:L + 1], pool=out["pool"][:R])


def p3p_hypothesis(points, bearings, sigma, T_SC, eigen_tree=True):
    """okvfe_p3p_hypothesis (host arithmetic, no context): points / bearings [4, 3] (rows 0 .. 2 are solved, row 3
    chooses among the solutions), sigma of the fourth, T_SC = (C, r) of their camera.
    -> (hypothesis [12] = row-major [R | t] of T_WS, valid, n_solutions)"""
    P = np.ascontiguousarray(points, dtype=np.float64).reshape(-1)
    f = np.ascontiguousarray(bearings, dtype=np.float64).reshape(-1)
    if len(P) != 12 or len(f) != 12:
        raise ValueError("four points and four bearings")
    pose = make_pose(*T_SC)
    H = np.zeros(12)
    valid, n_sol = C.c_uint8(0), C.c_int32(0)
    st = lib().okvfe_p3p_hypothesis(_p(P), _p(f), C.c_double(sigma), C.byref(pose), 1 if eigen_tree else 0, _p(H),
                                    C.byref(valid), C.byref(n_sol))
    if st != OK:
        raise OkvfeError(st, "okvfe_p3p_hypothesis")
    return H, int(valid.value), int(n_sol.value)


def twopt_rotation_hypothesis(b1, b2):
    """okvfe_twopt_rotation_hypothesis (host arithmetic, no context): b1 / b2 [2, 3] unit bearings of the older / current
    frame.  -> (M [9] row-major with b1 ~ M b2, valid)"""
    a = np.ascontiguousarray(b1, dtype=np.float64).reshape(-1)
    b = np.ascontiguousarray(b2, dtype=np.float64).reshape(-1)
    if len(a) != 6 or len(b) != 6:
        raise ValueError("two bearings per frame")
    M = np.zeros(9)
    valid = C.c_uint8(0)
    st = lib().okvfe_twopt_rotation_hypothesis(_p(a), _p(b), _p(M), C.byref(valid))
    if st != OK:
        raise OkvfeError(st, "okvfe_twopt_rotation_hypothesis")
    return M, int(valid.value)


def fivept_hypothesis(b1, b2, sigma1, sigma2, eigen_tree=True):
    """okvfe_fivept_hypothesis (host arithmetic, no context): b1 / b2 [8, 3] unit bearings of the older / current frame
    (rows 0 .. 4 are solved, rows 5 .. 7 choose among the candidates), sigma1 / sigma2 [3] of rows 5 .. 7.
    -> (hypothesis [12] = row-major [R | t], valid, n_roots)"""
    a = np.ascontiguousarray(b1, dtype=np.float64).reshape(-1)
    b = np.ascontiguousarray(b2, dtype=np.float64).reshape(-1)
    s1 = np.ascontiguousarray(sigma1, dtype=np.float64).reshape(-1)
    s2 = np.ascontiguousarray(sigma2, dtype=np.float64).reshape(-1)
    if len(a) != 24 or len(b) != 24 or len(s1) != 3 or len(s2) != 3:
        raise ValueError("eight bearings per frame and three sigmas per frame")
    H = np.zeros(12)
    valid, n_roots = C.c_uint8(0), C.c_int32(0)
    st = lib().okvfe_fivept_hypothesis(_p(a), _p(b), _p(s1), _p(s2), 1 if eigen_tree else 0, _p(H), C.byref(valid),
                                       C.byref(n_roots))
    if st != OK:
        raise OkvfeError(st, "okvfe_fivept_hypothesis")
    return H, int(valid.value), int(n_roots.value)


def keyframe_decision(current, others=None, overlap_threshold=KEYFRAME_OVERLAP_THRESHOLD):
    """okvfe_keyframe_decision (Frontend.cpp:1103, :1116-1166; host arithmetic, no context): current = the coverage
    records of the current multiframe's cameras, others = (n_others, n_cameras) records of the multiframes it is
    compared with.  Returns (need_keyframe, overlap).  The two early returns of :1060-1065 stay with the caller."""
    cur = np.ascontiguousarray(current, dtype=COVERAGE_DTYPE).reshape(-1)
    n_cam = len(cur)
    oth = np.zeros((0, max(n_cam, 1)), dtype=COVERAGE_DTYPE) if others is None else \
        np.ascontiguousarray(others, dtype=COVERAGE_DTYPE)
    if oth.size and (n_cam == 0 or oth.size % n_cam):
        raise ValueError("others: n_others x n_cameras records")
    n_oth = oth.size // n_cam if n_cam else 0
    need, overlap = C.c_int32(), C.c_double()
    st = lib().okvfe_keyframe_decision(_p(cur) if n_cam else None, n_cam, _p(oth) if n_oth else None, n_oth,
                                       C.c_float(overlap_threshold), C.byref(need), C.byref(overlap))
    if st != OK:
        raise OkvfeError(st, "okvfe_keyframe_decision")
    return bool(need.value), overlap.value


def overlap_fraction(counts):
    """okvfe_overlap_fraction (ViSlamBackend.cpp:2386-2389, :2410-2426; host arithmetic, no context): one double per
    OVERLAP_COUNTS_DTYPE record.  NaN (0 / 0) goes through as in the reference."""
    c = np.ascontiguousarray(counts, dtype=OVERLAP_COUNTS_DTYPE).reshape(-1)
    out = np.zeros(len(c), dtype=np.float64)
    st = lib().okvfe_overlap_fraction(_p(c) if len(c) else None, len(c), _p(out) if len(c) else None)
    if st != OK:
        raise OkvfeError(st, "okvfe_overlap_fraction: a negative count, or exactly one side without matched keypoints")
    return out


def make_imu_params(params) -> ImuParams:
    """okvfe_imu_params from a mapping (or an object) with a_max, g_max, sigma_g_c, sigma_a_c, sigma_gw_c, sigma_aw_c, g"""
    get = params.__getitem__ if hasattr(params, "__getitem__") else (lambda k: getattr(params, k))
    return ImuParams(*[float(get(k)) for k, _ in ImuParams._fields_])


def make_imu_result(pose_ptr, speed_and_bias_ptr, n_propagated_ptr, status_ptr, n_out_of_range_ptr, jacobian_ptr=None,
                    covariance_ptr=None, T_WC_ptr=None, gravity_C_ptr=None) -> ImuResultDevice:
    return ImuResultDevice(*[int(p) if p else None for p in (
        pose_ptr, speed_and_bias_ptr, n_propagated_ptr, status_ptr, n_out_of_range_ptr, jacobian_ptr, covariance_ptr,
        T_WC_ptr, gravity_C_ptr)])


def _imu_T_SC(T_SC_params):
    prm = np.ascontiguousarray(T_SC_params if T_SC_params is not None else np.zeros((0, 7)), dtype=np.float64).reshape(-1)
    if len(prm) % 7:
        raise ValueError("T_SC_params: seven doubles per camera")
    return prm, len(prm) // 7


def imu_propagation(params, samples, sample_begin, states, T_SC_params=None, eigen_tree=True, jacobian=True,
                    covariance=True):
    """okvfe_imu_propagation (ImuError::propagation, ImuError.cpp:557-779; the host loop, no context) over a batch in
    the layout of include/okvfe.h: samples [total, 8], sample_begin [n + 1] int32, states [n, 18].  Returns a dict of
    arrays with one record per multiframe; rows the call leaves alone hold NaN (-1 in the int32 outputs)."""
    smp = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1, IMU_SAMPLE_DOUBLES)
    beg = np.ascontiguousarray(sample_begin, dtype=np.int32).reshape(-1)
    sta = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, IMU_STATE_DOUBLES)
    n = len(sta)
    if len(beg) != n + 1 or (n and int(beg.max()) > len(smp)):
        raise ValueError("sample_begin: n_multiframes + 1 offsets within samples")
    prm, n_cams = _imu_T_SC(T_SC_params)
    out = dict(pose=np.full((n, 7), np.nan), speed_and_bias=np.full((n, 9), np.nan),
               n_propagated=np.full(n, -1, np.int32), status=np.full(n, -1, np.int32),
               n_out_of_range=np.full(n, -1, np.int32),
               jacobian=np.full((n, 225), np.nan) if jacobian or covariance else None,
               covariance=np.full((n, 225), np.nan) if covariance else None,
               T_WC=np.full((n, n_cams, 7), np.nan) if n_cams else None,
               gravity_C=np.full((n, n_cams, 3), np.nan, np.float32) if n_cams else None)
    # (an empty array has no address worth passing: the required outputs of an empty batch point at one spare record)
    spare = np.zeros(32)
    ptr = lambda a: None if a is None else (a.ctypes.data if a.size else spare.ctypes.data)
    res = make_imu_result(*[ptr(out[k]) for k, _ in ImuResultDevice._fields_])
    p = make_imu_params(params)
    st = lib().okvfe_imu_propagation(C.byref(p), _p(smp if len(smp) else spare), _p(beg), _p(sta if n else spare), n,
                                     n_cams, _p(prm) if n_cams else None, 1 if eigen_tree else 0, C.byref(res))
    if st != OK:
        raise OkvfeError(st, "okvfe_imu_propagation: bad argument")
    return out


def motion_frame_order(overlap, frame_ids, previous=-1):
    """okvfe_motion_frame_order (Frontend.cpp:1751-1767; host arithmetic, no context): the indices of the frames in
    the order of the motion-stereo sweep.  The entry at index `previous` (-1 = none) counts as overlap 1.0.  A NaN
    overlap is refused (std::sort is undefined there), as are duplicate ids."""
    ov = np.ascontiguousarray(overlap, dtype=np.float64).reshape(-1)
    ids = np.ascontiguousarray(frame_ids, dtype=np.uint64).reshape(-1)
    if len(ids) != len(ov):
        raise ValueError("frame_ids: one per overlap")
    n = len(ov)
    order = np.zeros(max(n, 1), dtype=np.int32)
    n_order = C.c_int32()
    st = lib().okvfe_motion_frame_order(_p(ov) if n else None, _p(ids) if n else None, n, int(previous), _p(order),
                                        C.byref(n_order))
    if st != OK:
        what = f"entry {n_order.value}: NaN overlap" if n_order.value >= 0 else "bad argument or duplicate frame ids"
        raise OkvfeError(st, "okvfe_motion_frame_order: " + what)
    return order[:n_order.value].copy()


def tracking_quality(coverage, width, height, kptrad):
    """okvfe_tracking_quality (ViSlamBackend.cpp:157-196; host arithmetic, no context): coverage = the records of a
    coverage call without an id set, one per camera, taken with the not-observed-elsewhere ids zeroed."""
    c = np.ascontiguousarray(coverage, dtype=COVERAGE_DTYPE).reshape(-1)
    q = C.c_double()
    st = lib().okvfe_tracking_quality(_p(c) if len(c) else None, len(c), int(width), int(height), C.c_double(kptrad),
                                      C.byref(q))
    if st != OK:
        raise OkvfeError(st, "okvfe_tracking_quality")
    return q.value


def set_heavy_kernel_chaining(mode: int):
    """okvfe_set_heavy_kernel_chaining: 0 off, 1 score kernels of all contexts in turn, 2 + describe."""
    st = lib().okvfe_set_heavy_kernel_chaining(int(mode))
    if st != OK:
        raise OkvfeError(st, "okvfe_set_heavy_kernel_chaining")


def popcnt_xor(a, b, n128=3) -> int:
    a = np.ascontiguousarray(a, dtype=np.uint8)
    b = np.ascontiguousarray(b, dtype=np.uint8)
    return int(lib().okvfe_popcnt_xor(_p(a), _p(b), int(n128)))


def scale_index(size) -> int:
    """Scale index (0..63) of the scale-invariant extractor for a keypoint diameter (host only)."""
    f = lib().okvfe_scale_index
    f.restype, f.argtypes = C.c_int32, [C.c_float]
    return int(f(float(size)))


def build_awareness_maps(cam):
    fn, (c,) = _camera_fn("okvfe_build_awareness_maps", cam)
    rays = np.zeros((cam.h, cam.w, 3), dtype=np.float32)
    jac = np.zeros((cam.h, cam.w, 6), dtype=np.float32)
    st = fn(C.byref(c), _p(rays), _p(jac))
    if st != OK:
        raise OkvfeError(st, lib().okvfe_last_error(None).decode())
    return rays, jac


def format_keypoint_lines(state_id, camera_idx, keypoints, descriptors) -> bytes:
    """Map-file text records (okvis::Component::save format)."""
    kps = np.ascontiguousarray(keypoints, dtype=KEYPOINT_DTYPE)
    desc = np.ascontiguousarray(descriptors, dtype=np.uint8)
    need = C.c_size_t()
    st = lib().okvfe_format_keypoint_lines(C.c_uint64(state_id), C.c_uint64(camera_idx), _p(kps),
                                           _p(desc), len(kps), None, C.c_size_t(0), C.byref(need))
    if st != OK:
        raise OkvfeError(st, "okvfe_format_keypoint_lines")
    buf = C.create_string_buffer(max(need.value, 1))
    st = lib().okvfe_format_keypoint_lines(C.c_uint64(state_id), C.c_uint64(camera_idx), _p(kps),
                                           _p(desc), len(kps), buf, C.c_size_t(need.value),
                                           C.byref(need))
    if st != OK:
        raise OkvfeError(st, "okvfe_format_keypoint_lines")
    return buf.raw[:need.value]


def parse_keypoint_lines(text: bytes, cap=4096):
    """Returns (state_id, camera_idx, keypoints, descriptors, bytes_consumed)."""
    kps = np.zeros(cap, dtype=KEYPOINT_DTYPE)
    desc = np.zeros((cap, DESC_BYTES), dtype=np.uint8)
    sid, cam, n, used = C.c_uint64(), C.c_uint64(), C.c_int32(), C.c_size_t()
    st = lib().okvfe_parse_keypoint_lines(text, C.c_size_t(len(text)), C.byref(sid), C.byref(cam),
                                          _p(kps), _p(desc), cap, C.byref(n), C.byref(used))
    if st != OK:
        raise OkvfeError(st, "okvfe_parse_keypoint_lines")
    return sid.value, cam.value, kps[:n.value].copy(), desc[:n.value].copy(), used.value


def fbrisk_mean(descriptors) -> np.ndarray:
    d = np.ascontiguousarray(descriptors, dtype=np.uint8).reshape(-1, DESC_BYTES)
    out = np.zeros(DESC_BYTES, dtype=np.uint8)
    st = lib().okvfe_fbrisk_mean(_p(d), len(d), _p(out))
    if st != OK:
        raise OkvfeError(st, "okvfe_fbrisk_mean")
    return out


def camera_overlap(cam, other, R_other_cam, want_mask=False):
    fn, (c, o) = _camera_fn("okvfe_camera_overlap", cam, other)
    R = (C.c_double * 9)(*[float(v) for v in np.asarray(R_other_cam).reshape(-1)])
    mask = np.zeros((cam.h, cam.w), dtype=np.uint8) if want_mask else None
    has = C.c_int32()
    st = fn(C.byref(c), C.byref(o), R, _p(mask), C.byref(has))
    if st != OK:
        raise OkvfeError(st, lib().okvfe_last_error(None).decode())
    return (bool(has.value), mask) if want_mask else bool(has.value)


class Frontend:
    """One okvfe context = the detector + extractor + matcher of one camera stream on one GPU.

    Mirrors the reference's per-camera objects (okvis_frontend/src/Frontend.cpp:2405-2413):
    constructor arguments are the brisk::ScaleSpaceFeatureDetector / BriskDescriptorExtractor
    ones plus image size and batch capacity.
    """

    def __init__(self, width, height, uniformity_radius, octaves, absolute_threshold,
                 max_keypoints, rotation_invariant=True, scale_invariant=False,
                 match_threshold=60, max_batch=1, num_cameras=1, device=0, max_candidates=0,
                 score_type=SCORE_HARRIS, box_scale=1.0):
        cfg = Config(ABI_VERSION, device, width, height, max_batch, num_cameras,
                     float(uniformity_radius), int(octaves), int(absolute_threshold),
                     int(max_keypoints), int(bool(rotation_invariant)), int(bool(scale_invariant)),
                     int(match_threshold), int(max_candidates), int(score_type), float(box_scale))
        self._h = C.c_void_p()
        # row capacity per image: a scale space (octaves > 0) has 2 * octaves layers and every layer
        # may deliver max_keypoints (okvfe_device_outputs.max_keypoints reports the same number)
        self.w, self.h, self.max_batch = width, height, max_batch
        self.max_keypoints = int(max_keypoints) * max(1, 2 * int(octaves))
        st = lib().okvfe_create(C.byref(cfg), C.byref(self._h))
        if st != OK:
            raise OkvfeError(st, lib().okvfe_last_error(None).decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().okvfe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != OK:
            raise OkvfeError(st, lib().okvfe_last_error(self._h).decode())

    # -- setup ----------------------------------------------------------------------------
    def set_camera(self, slot, cam):
        fn, (c,) = _camera_fn("okvfe_set_camera", cam)
        self._check(fn(self._h, int(slot), C.byref(c)))

    def set_camera_maps(self, slot, rays, jac, fu):
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        jac = np.ascontiguousarray(jac, dtype=np.float32)
        self._check(lib().okvfe_set_camera_maps(self._h, int(slot), _p(rays), _p(jac),
                                                C.c_float(fu)))

    # -- host-buffer API ------------------------------------------------------------------
    def detect(self, image):
        image = np.ascontiguousarray(image, dtype=np.uint8)
        cap = self.max_keypoints
        kps = np.zeros(cap, dtype=KEYPOINT_DTYPE)
        n = C.c_int32()
        self._check(lib().okvfe_detect(self._h, _p(image), C.c_size_t(image.strides[0]), _p(kps),
                                       cap, C.byref(n)))
        return kps[:n.value].copy()

    def detect_ahead(self, image, cam=-1, gravity=None):
        """okvfe_detect_ahead: detect() whose compute() on the same image is answered from the kept result."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        self._ahead_image = image  # the pairing is by pointer: keep the buffer alive for compute()
        cap = self.max_keypoints
        kps = np.zeros(cap, dtype=KEYPOINT_DTYPE)
        n = C.c_int32()
        g = None if gravity is None else (C.c_float * 3)(*[float(v) for v in gravity])
        self._check(lib().okvfe_detect_ahead(self._h, _p(image), C.c_size_t(image.strides[0]), int(cam), g,
                                             _p(kps), cap, C.byref(n)))
        return kps[:n.value].copy()

    def harris_byte_mover_device(self, images_ptr, n_images, stream=None):
        """Diagnostic: the fused score kernel's loads and stores without its arithmetic."""
        self._check(lib().okvfe_harris_byte_mover_device(self._h, _p(images_ptr), int(n_images), _s(stream)))

    def detect_describe(self, image, cam=-1, gravity=None):
        image = np.ascontiguousarray(image, dtype=np.uint8)
        cap = self.max_keypoints
        kps = np.zeros(cap, dtype=KEYPOINT_DTYPE)
        desc = np.zeros((cap, DESC_BYTES), dtype=np.uint8)
        bp = np.zeros((cap, 3), dtype=np.float64)
        bpv = np.zeros(cap, dtype=np.uint8)
        n = C.c_int32()
        g = None if gravity is None else (C.c_float * 3)(*[float(v) for v in gravity])
        self._check(lib().okvfe_detect_describe(self._h, _p(image), C.c_size_t(image.strides[0]),
                                                int(cam), g, _p(kps), _p(desc), _p(bp), _p(bpv),
                                                cap, C.byref(n)))
        k = n.value
        return kps[:k].copy(), desc[:k].copy(), bp[:k].copy(), bpv[:k].copy()

    def compute(self, image, keypoints, cam=-1, gravity=None):
        """cv::DescriptorExtractor::compute: describe the given keypoints (some may be removed)."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        kps = np.ascontiguousarray(keypoints, dtype=KEYPOINT_DTYPE).copy()
        n_in = len(kps)
        if n_in == 0:
            kps = np.zeros(1, dtype=KEYPOINT_DTYPE)
        desc = np.zeros((max(n_in, 1), DESC_BYTES), dtype=np.uint8)
        bp = np.zeros((max(n_in, 1), 3), dtype=np.float64)
        bpv = np.zeros(max(n_in, 1), dtype=np.uint8)
        n = C.c_int32()
        g = None if gravity is None else (C.c_float * 3)(*[float(v) for v in gravity])
        self._check(lib().okvfe_compute(self._h, _p(image), C.c_size_t(image.strides[0]), int(cam),
                                        g, _p(kps), n_in, _p(desc), _p(bp), _p(bpv), C.byref(n)))
        k = n.value
        return kps[:k].copy(), desc[:k].copy(), bp[:k].copy(), bpv[:k].copy()

    # -- device-resident API --------------------------------------------------------------
    def harris_score_device(self, images_ptr, n_images, scores_ptr, stream=None):
        self._check(lib().okvfe_harris_score_device(self._h, _p(images_ptr), int(n_images),
                                                    _p(scores_ptr), _s(stream)))

    def detect_batch_device(self, images_ptr, n_images, stream=None):
        self._check(lib().okvfe_detect_batch_device(self._h, _p(images_ptr), int(n_images),
                                                    _s(stream)))

    def describe_batch_device(self, images_ptr, n_images, cam_ids=None, gravity=None, stream=None):
        ids = None if cam_ids is None else np.ascontiguousarray(cam_ids, dtype=np.int32)
        g = None if gravity is None else np.ascontiguousarray(gravity, dtype=np.float32)
        self._check(lib().okvfe_describe_batch_device(self._h, _p(images_ptr), int(n_images),
                                                      _p(ids), _p(g), _s(stream)))

    def detect_describe_batch_device(self, images_ptr, n_images, cam_ids=None, gravity=None,
                                     stream=None):
        ids = None if cam_ids is None else np.ascontiguousarray(cam_ids, dtype=np.int32)
        g = None if gravity is None else np.ascontiguousarray(gravity, dtype=np.float32)
        self._check(lib().okvfe_detect_describe_batch_device(self._h, _p(images_ptr),
                                                             int(n_images), _p(ids), _p(g),
                                                             _s(stream)))

    def detect_describe_batch_host(self, images_host_ptr, n_images, cam_ids=None, gravity=None,
                                   stream=None):
        """images_host_ptr: address of n_images contiguous images in (preferably pinned) HOST
        memory; the copy overlaps the previous batch's kernels (okvfe_detect_describe_batch_host)."""
        ids = None if cam_ids is None else np.ascontiguousarray(cam_ids, dtype=np.int32)
        g = None if gravity is None else np.ascontiguousarray(gravity, dtype=np.float32)
        self._check(lib().okvfe_detect_describe_batch_host(self._h, _p(images_host_ptr),
                                                           int(n_images), _p(ids), _p(g),
                                                           _s(stream)))

    def set_keep_score_map(self, keep: bool = True):
        """okvfe_set_keep_score_map: single-scale Harris detection writes no score map by default
        (device_outputs().scores is then null); keep=True restores it for the following calls."""
        self._check(lib().okvfe_set_keep_score_map(self._h, int(bool(keep))))

    def set_internal_lanes(self, lanes: int = 0):
        """okvfe_set_internal_lanes: slices a batch call is cut into, each on a stream of the context's own
        (0 = automatic, 1 = off)."""
        self._check(lib().okvfe_set_internal_lanes(self._h, int(lanes)))

    def lanes_join(self, stream=None):
        """okvfe_lanes_join: `stream` (None: the context's own) waits for every pipelined lane (set_internal_lanes(-k))"""
        self._check(lib().okvfe_lanes_join(self._h, _s(stream)))

    def set_fp64_reduction(self, eigen_tree: bool = True):
        """okvfe_set_fp64_reduction: order of the 3-term FP64 sums of the gate chain -- Eigen's x0 + (x1 + x2)
        (default) or left to right; device-wide."""
        self._check(lib().okvfe_set_fp64_reduction(self._h, 1 if eigen_tree else 0))

    def device_outputs(self) -> DeviceOutputs:
        out = DeviceOutputs()
        self._check(lib().okvfe_get_device_outputs(self._h, C.byref(out)))
        return out

    def download(self, index):
        cap = self.max_keypoints
        kps = np.zeros(cap, dtype=KEYPOINT_DTYPE)
        desc = np.zeros((cap, DESC_BYTES), dtype=np.uint8)
        bp = np.zeros((cap, 3), dtype=np.float64)
        bpv = np.zeros(cap, dtype=np.uint8)
        n = C.c_int32()
        self._check(lib().okvfe_download_image_result(self._h, int(index), _p(kps), _p(desc),
                                                      _p(bp), _p(bpv), cap, C.byref(n)))
        k = n.value
        return kps[:k].copy(), desc[:k].copy(), bp[:k].copy(), bpv[:k].copy()

    def check_capacity(self, n_images):
        """Raises OkvfeError(ERR_CAPACITY) if an NMS candidate list of the last batch overflowed."""
        first = C.c_int32(-1)
        self._check(lib().okvfe_check_capacity(self._h, int(n_images), C.byref(first)))

    def match_stereo_batch_device(self, pairs, matches_ptr, stream=None):
        arr = pairs if isinstance(pairs, C.Array) else (StereoPair * len(pairs))(*pairs)
        self._check(lib().okvfe_match_stereo_batch_device(self._h, arr, len(pairs),
                                                          _p(matches_ptr), _s(stream)))

    # -- matching, host buffers -----------------------------------------------------------
    def match_stereo(self, desc0, kp0, bp0, bpv0, desc1, kp1, bp1, bpv1, T0, T1, f0, f1):
        n0, n1 = len(kp0), len(kp1)
        out = np.zeros(max(n0, 1), dtype=STEREO_MATCH_DTYPE)
        arrs = [np.ascontiguousarray(a) for a in (desc0, kp0, bp0, bpv0, desc1, kp1, bp1, bpv1)]
        P0, P1 = make_pose(*T0), make_pose(*T1)
        self._check(lib().okvfe_match_stereo(self._h, _p(arrs[0]), _p(arrs[1]), _p(arrs[2]),
                                             _p(arrs[3]), n0, _p(arrs[4]), _p(arrs[5]),
                                             _p(arrs[6]), _p(arrs[7]), n1, C.byref(P0),
                                             C.byref(P1), C.c_double(f0), C.c_double(f1),
                                             _p(out)))
        return out[:n0]

    def match_motion_stereo(self, cam, desc0, kp0, bp0, bpv0, skip0, desc1, kp1, bp1, bpv1, matched1,
                            T0, T1):
        n0, n1 = len(kp0), len(kp1)
        out = np.zeros(max(n0, 1), dtype=MOTION_MATCH_DTYPE)
        arrs = [None if a is None else np.ascontiguousarray(a)
                for a in (desc0, kp0, bp0, bpv0, skip0, desc1, kp1, bp1, bpv1, matched1)]
        fn, (c,) = _camera_fn("okvfe_match_motion_stereo", cam)
        P0, P1 = make_pose(*T0), make_pose(*T1)
        self._check(fn(
            self._h, C.byref(c), _p(arrs[0]), _p(arrs[1]), _p(arrs[2]), _p(arrs[3]), _p(arrs[4]), n0,
            _p(arrs[5]), _p(arrs[6]), _p(arrs[7]), _p(arrs[8]), _p(arrs[9]), n1, C.byref(P0),
            C.byref(P1), _p(out)))
        return out[:n0]

    def match_to_map(self, desc, kps, use, proj, desc_begin, pool, repr_thr):
        n, nl = len(kps), len(desc_begin) - 1
        bl = np.zeros(max(n, 1), dtype=np.int32)
        bd = np.zeros(max(n, 1), dtype=np.int32)
        arrs = [np.ascontiguousarray(a) for a in (desc, kps, np.asarray(use, dtype=np.uint8),
                                                 np.asarray(proj, dtype=np.float64),
                                                 np.asarray(desc_begin, dtype=np.int32),
                                                 np.asarray(pool, dtype=np.uint8))]
        self._check(lib().okvfe_match_to_map(self._h, _p(arrs[0]), _p(arrs[1]), _p(arrs[2]), n,
                                             _p(arrs[3]), _p(arrs[4]), nl, _p(arrs[5]),
                                             C.c_double(repr_thr), _p(bl), _p(bd)))
        return bl[:n], bd[:n]

    def match_to_map_uninitialised(self, desc, bp, use, previous, desc_begin, pool, e0_W, r0_W, T1,
                                   focal):
        n, nl = len(desc), len(desc_begin) - 1
        bl = np.zeros(max(n, 1), dtype=np.int32)
        bd = np.zeros(max(n, 1), dtype=np.int32)
        hp = np.zeros((max(n, 1), 4), dtype=np.float64)
        hs = np.zeros(max(n, 1), dtype=np.uint8)
        ctr = C.c_int32()
        arrs = [np.ascontiguousarray(desc, dtype=np.uint8), np.ascontiguousarray(bp, dtype=np.float64),
                np.ascontiguousarray(use, dtype=np.uint8), np.ascontiguousarray(previous, dtype=np.int32),
                np.ascontiguousarray(desc_begin, dtype=np.int32), np.ascontiguousarray(pool, dtype=np.uint8),
                np.ascontiguousarray(e0_W, dtype=np.float64), np.ascontiguousarray(r0_W, dtype=np.float64)]
        P1 = make_pose(*T1)
        self._check(lib().okvfe_match_to_map_uninitialised(
            self._h, _p(arrs[0]), _p(arrs[1]), _p(arrs[2]), _p(arrs[3]), n, _p(arrs[4]), nl,
            _p(arrs[5]), _p(arrs[6]), _p(arrs[7]), C.byref(P1), C.c_double(focal), _p(bl), _p(bd),
            _p(hp), _p(hs), C.byref(ctr)))
        return bl[:n], bd[:n], hp[:n], hs[:n], ctr.value

    def hamming_candidates(self, A, B, thr, cap=None):
        A = np.ascontiguousarray(A, dtype=np.uint8)
        B = np.ascontiguousarray(B, dtype=np.uint8)
        cap = len(A) * len(B) if cap is None else cap
        out = np.zeros(max(cap, 1), dtype=CAND_DTYPE)
        n = C.c_int32()
        st = lib().okvfe_hamming_candidates(self._h, _p(A), len(A), _p(B), len(B), int(thr),
                                            _p(out), int(cap), C.byref(n))
        if st == ERR_CAPACITY:
            return out[:cap].copy(), n.value
        self._check(st)
        return out[:n.value].copy(), n.value

    def hamming_argmin(self, A, B, thr):
        A = np.ascontiguousarray(A, dtype=np.uint8)
        B = np.ascontiguousarray(B, dtype=np.uint8)
        bj = np.zeros(max(len(A), 1), dtype=np.int32)
        bd = np.zeros(max(len(A), 1), dtype=np.uint32)
        self._check(lib().okvfe_hamming_argmin(self._h, _p(A), len(A), _p(B), len(B),
                                               C.c_uint32(int(thr)), _p(bj), _p(bd)))
        return bj[:len(A)], bd[:len(A)]

    def match_to_map_landmarks(self, cam, hp_W, quality, obs_begin, obs_pose, obs_desc, obs_bp, poses,
                               T_WC1, repr_threshold, exclusive, desc, kps, use):
        """Frontend::matchToMap from the raw landmark table (projection + view pooling + 3-D match on
        the device).  poses: list of (C, r).  Returns (best_landmark, best_dist, pool dict)."""
        hp = np.ascontiguousarray(hp_W, dtype=np.float64).reshape(-1, 4)
        q = np.ascontiguousarray(quality, dtype=np.float64)
        ob = np.ascontiguousarray(obs_begin, dtype=np.int32)
        op = np.ascontiguousarray(obs_pose, dtype=np.int32)
        od = np.ascontiguousarray(obs_desc, dtype=np.uint8).reshape(-1, DESC_BYTES)
        obp = np.ascontiguousarray(obs_bp, dtype=np.float64).reshape(-1, 3)
        P = (Pose * max(len(poses), 1))(*[make_pose(*p) for p in poses])
        nl = len(hp)
        t = LandmarkTable(nl, len(op), len(poses), _p(hp).value, _p(q).value, _p(ob).value,
                          _p(op).value if len(op) else None, _p(od).value if len(od) else None,
                          _p(obp).value if len(obp) else None, C.addressof(P))
        pool = {"status": np.zeros(max(nl, 1), np.int32), "n_desc": np.zeros(max(nl, 1), np.int32),
                "obs_rows": np.zeros((max(nl, 1), 3), np.int32), "projection": np.zeros((max(nl, 1), 2)),
                "e_W": np.zeros((max(nl, 1), 2, 3)), "r_W": np.zeros((max(nl, 1), 2, 3))}
        lp = LandmarkPool(*[_p(pool[k]).value for k in ("status", "n_desc", "obs_rows", "projection",
                                                         "e_W", "r_W")])
        d = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, DESC_BYTES)
        kk = np.ascontiguousarray(kps, dtype=KEYPOINT_DTYPE)
        u = np.ascontiguousarray(use, dtype=np.uint8)
        n = len(kk)
        lm = np.zeros(max(n, 1), dtype=np.int32)
        bd = np.zeros(max(n, 1), dtype=np.int32)
        T1 = make_pose(*T_WC1)
        self._check(lib().okvfe_match_to_map_landmarks(
            self._h, int(cam), C.byref(t), C.byref(T1), C.c_double(repr_threshold), int(bool(exclusive)),
            _p(d), _p(kk), _p(u), n, C.byref(lp), _p(lm), _p(bd)))
        return lm[:n], bd[:n], {k: v[:nl] for k, v in pool.items()}

    def verify_place_match(self, landmark_desc, desc_begin, frame_desc):
        """Frontend::verifyRecognisedPlace descriptor matching, all landmarks in one launch."""
        pool = np.ascontiguousarray(landmark_desc, dtype=np.uint8).reshape(-1, DESC_BYTES)
        db = np.ascontiguousarray(desc_begin, dtype=np.int32)
        fd = np.ascontiguousarray(frame_desc, dtype=np.uint8).reshape(-1, DESC_BYTES)
        n = len(db) - 1
        k_min = np.zeros(max(n, 1), dtype=np.int32)
        d_min = np.zeros(max(n, 1), dtype=np.uint32)
        self._check(lib().okvfe_verify_place_match(self._h, _p(pool), _p(db), n, _p(fd), len(fd),
                                                   _p(k_min), _p(d_min)))
        return k_min[:n], d_min[:n]

    def fbrisk_transform(self, desc, node_desc, child_begin, child_index, node_word):
        """DBoW2 vocabulary descent (FBrisk trait): word id and leaf node per descriptor."""
        d = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, DESC_BYTES)
        nd = np.ascontiguousarray(node_desc, dtype=np.uint8).reshape(-1, DESC_BYTES)
        cb = np.ascontiguousarray(child_begin, dtype=np.int32)
        ci = np.ascontiguousarray(child_index, dtype=np.int32)
        nw = np.ascontiguousarray(node_word, dtype=np.int32)
        words = np.zeros(max(len(d), 1), dtype=np.int32)
        leaves = np.zeros(max(len(d), 1), dtype=np.int32)
        self._check(lib().okvfe_fbrisk_transform(self._h, _p(d), len(d), _p(nd), len(nd), _p(cb), _p(ci),
                                                 _p(nw), _p(words), _p(leaves)))
        return words[:len(d)], leaves[:len(d)]

    def bow_query_l1(self, db_begin, db_ids, db_values, q_ids, q_values):
        """DBoW2 database query with L1 scoring against all entries: score per entry (-1 = no
        common word)."""
        b = np.ascontiguousarray(db_begin, dtype=np.int32)
        ids = np.ascontiguousarray(db_ids, dtype=np.int32)
        vals = np.ascontiguousarray(db_values, dtype=np.float64)
        qi = np.ascontiguousarray(q_ids, dtype=np.int32)
        qv = np.ascontiguousarray(q_values, dtype=np.float64)
        n = len(b) - 1
        scores = np.zeros(max(n, 1), dtype=np.float64)
        self._check(lib().okvfe_bow_query_l1(self._h, _p(b), _p(ids), _p(vals), n, _p(qi), _p(qv), len(qi),
                                             _p(scores)))
        return scores[:n]

    # -- stage profiling (HIP events on the launch stream) --------------------------------
    def profile_enable(self, on=True, stages=None):
        """on=True times every stage; stages=("harris", ...) only those (fewer event records)."""
        flag = int(bool(on))
        if on and stages:
            flag = 0
            for name in stages:
                flag |= 1 << (8 + list(STAGES).index(name))
        self._check(lib().okvfe_profile_enable(self._h, flag))

    def profile_read(self):
        ms = (C.c_double * len(STAGES))()
        n = (C.c_int32 * len(STAGES))()
        self._check(lib().okvfe_profile_read(self._h, ms, n))
        return {STAGES[i]: (ms[i], n[i]) for i in range(len(STAGES))}

    # -- sampling pattern as data ----------------------------------------------------------
    def get_pattern(self) -> PatternData:
        p = PatternData()
        self._check(lib().okvfe_get_pattern(self._h, C.byref(p)))
        return p

    def set_pattern(self, pattern: PatternData):
        self._check(lib().okvfe_set_pattern(self._h, C.byref(pattern)))

    def pattern_kernel_class(self) -> int:
        """0 / 1: the fast descriptor kernels (11 x 11 / 21 x 21 row slots); 2: the all-modes kernel (include/okvfe.h)"""
        return int(lib().okvfe_pattern_kernel_class(self._h))

    # -- device-resident, batched map matchers (frame f = gather block f) -----------------
    @staticmethod
    def make_map_device(n_landmarks, desc_begin_ptr, pool_ptr, projections_ptr=None, e0_ptr=None,
                        r0_ptr=None) -> MapDevice:
        m = MapDevice()
        m.n_landmarks = int(n_landmarks)
        m.desc_begin, m.pool = int(desc_begin_ptr), int(pool_ptr) if pool_ptr else None
        m.projections = int(projections_ptr) if projections_ptr else None
        m.e0_W = int(e0_ptr) if e0_ptr else None
        m.r0_W = int(r0_ptr) if r0_ptr else None
        return m

    def match_to_map_blocks_device(self, blocks_ptr, n_frames, use_ptr, map_dev, repr_thr, best_lm_ptr,
                                   best_d_ptr, stream=None):
        self._check(lib().okvfe_match_to_map_blocks_device(
            self._h, _p(blocks_ptr), int(n_frames), _p(use_ptr), C.byref(map_dev), C.c_double(repr_thr),
            _p(best_lm_ptr), _p(best_d_ptr), _s(stream)))

    def match_to_map_uninitialised_blocks_device(self, blocks_ptr, n_frames, use_ptr, previous_ptr, map_dev,
                                                 poses_T_WC1, focal, best_lm_ptr, best_d_ptr, hps_ptr,
                                                 hp_set_ptr, ctr_ptr, stream=None):
        P = (Pose * int(n_frames))(*[make_pose(*T) for T in poses_T_WC1])
        self._check(lib().okvfe_match_to_map_uninitialised_blocks_device(
            self._h, _p(blocks_ptr), int(n_frames), _p(use_ptr), _p(previous_ptr), C.byref(map_dev), P,
            C.c_double(focal), _p(best_lm_ptr), _p(best_d_ptr), _p(hps_ptr), _p(hp_set_ptr), _p(ctr_ptr),
            _s(stream)))

    # -- matchToMap from a device-resident landmark table, a batch of frames ---------------
    @staticmethod
    def make_landmark_table_device(n_landmarks, n_observations, n_poses, hp_ptr, quality_ptr, obs_begin_ptr,
                                   obs_pose_ptr, obs_desc_ptr, obs_backproj_ptr, poses_ptr) -> LandmarkTableDevice:
        """Device pointers (ints; 0 / None = NULL) of a table uploaded once per map change."""
        return LandmarkTableDevice(int(n_landmarks), int(n_observations), int(n_poses),
                                   *[int(p) if p else None for p in (hp_ptr, quality_ptr, obs_begin_ptr, obs_pose_ptr,
                                                                     obs_desc_ptr, obs_backproj_ptr, poses_ptr)])

    @staticmethod
    def make_landmark_pool_device(status_ptr=None, n_desc_ptr=None, obs_rows_ptr=None, projection_ptr=None,
                                  e_W_ptr=None, r_W_ptr=None) -> LandmarkPoolDevice:
        return LandmarkPoolDevice(*[int(p) if p else None for p in (status_ptr, n_desc_ptr, obs_rows_ptr,
                                                                    projection_ptr, e_W_ptr, r_W_ptr)])

    def landmark_table_check_device(self, table: LandmarkTableDevice, stream=None):
        """The structural checks of the table on the device; synchronises.  Raises OkvfeError naming the first bad row."""
        self._check(lib().okvfe_landmark_table_check_device(self._h, C.byref(table), _s(stream)))

    def match_to_map_table_blocks_device(self, table: LandmarkTableDevice, blocks_ptr, n_frames, cam_ids, poses_T_WC1,
                                         repr_thr, exclusive, use_ptr, pool_out, best_lm_ptr, best_d_ptr,
                                         stream=None):
        """okvfe_match_to_map_landmarks for n_frames gather blocks against one device-resident table.  cam_ids /
        poses_T_WC1: host sequences of n_frames camera slots / (C, r); pool_out: LandmarkPoolDevice or None."""
        n = int(n_frames)
        cams = np.ascontiguousarray(cam_ids, dtype=np.int32)
        if len(cams) != n or len(poses_T_WC1) != n:
            raise ValueError("cam_ids and poses_T_WC1: one per frame")
        P = (Pose * max(n, 1))(*[make_pose(*T) for T in poses_T_WC1])
        self._check(lib().okvfe_match_to_map_table_blocks_device(
            self._h, C.byref(table), _p(blocks_ptr), n, _p(cams) if n else _p(np.zeros(1, np.int32)), P,
            C.c_double(repr_thr), int(bool(exclusive)), _p(use_ptr), C.byref(pool_out) if pool_out is not None else None,
            _p(best_lm_ptr), _p(best_d_ptr), _s(stream)))

    def match_to_map_table_uninitialised_blocks_device(self, table: LandmarkTableDevice, pool: LandmarkPoolDevice,
                                                       blocks_ptr, n_frames, cam_ids, poses_T_WC1, exclusive, use_ptr,
                                                       previous_ptr, best_lm_ptr, best_d_ptr, hps_ptr, hp_set_ptr,
                                                       ctr_ptr, stream=None):
        """The second pass of matchToMap for n_frames gather blocks: every frame over the landmarks its first pass
        (match_to_map_table_blocks_device with `pool` as pool_out) left with status 2.  cam_ids / poses_T_WC1: host
        sequences of n_frames camera slots / (C, r), the poses as they are NOW; previous_ptr: device n_frames x K table
        rows or None."""
        n = int(n_frames)
        cams = np.ascontiguousarray(cam_ids, dtype=np.int32)
        if len(cams) != n or len(poses_T_WC1) != n:
            raise ValueError("cam_ids and poses_T_WC1: one per frame")
        P = (Pose * max(n, 1))(*[make_pose(*T) for T in poses_T_WC1])
        self._check(lib().okvfe_match_to_map_table_uninitialised_blocks_device(
            self._h, C.byref(table), C.byref(pool) if pool is not None else None, _p(blocks_ptr), n,
            _p(cams) if n else _p(np.zeros(1, np.int32)), P, int(bool(exclusive)), _p(use_ptr), _p(previous_ptr),
            _p(best_lm_ptr), _p(best_d_ptr), _p(hps_ptr), _p(hp_set_ptr), _p(ctr_ptr), _s(stream)))

    # -- between the two passes: RANSAC consensus and outlier removal ------------------------
    @staticmethod
    def make_ransac_result_device(n_correspondences_ptr, best_hypothesis_ptr, n_inliers_ptr, accepted_ptr,
                                  hyp_inliers_ptr=None, state_ptr=None, distance_ptr=None,
                                  landmark_out_ptr=None) -> RansacResultDevice:
        return RansacResultDevice(*[int(p) if p else None for p in (
            n_correspondences_ptr, best_hypothesis_ptr, n_inliers_ptr, accepted_ptr, hyp_inliers_ptr, state_ptr,
            distance_ptr, landmark_out_ptr)])

    def ransac3d2d_consensus_blocks_device(self, table: LandmarkTableDevice, blocks_ptr, n_multiframes, cam_ids,
                                           poses_T_SC, landmark_ptr, hypotheses_ptr, hyp_valid_ptr, n_hyp,
                                           result: RansacResultDevice, threshold=RANSAC_THRESHOLD,
                                           remove_outliers=True, stream=None):
        """The consensus step of runRansac3d2d for n_multiframes multiframes of len(cam_ids) gather blocks each.
        cam_ids / poses_T_SC: host sequences of the rig's camera slots / (C, r); hypotheses_ptr: device
        n_multiframes x n_hyp x 12 doubles ([R | t] = T_WS, row-major); hyp_valid_ptr: device bytes or None."""
        cams = np.ascontiguousarray(cam_ids, dtype=np.int32)
        n_cams = len(cams)
        if len(poses_T_SC) != n_cams:
            raise ValueError("cam_ids and poses_T_SC: one per camera")
        P = (Pose * max(n_cams, 1))(*[make_pose(*T) for T in poses_T_SC])
        self._check(lib().okvfe_ransac3d2d_consensus_blocks_device(
            self._h, C.byref(table), _p(blocks_ptr), int(n_multiframes), n_cams,
            _p(cams) if n_cams else _p(np.zeros(1, np.int32)), P, _p(landmark_ptr), _p(hypotheses_ptr),
            _p(hyp_valid_ptr), int(n_hyp), C.c_double(threshold), int(bool(remove_outliers)),
            C.byref(result) if result is not None else None, _s(stream)))

    # -- the hypotheses of the two consensus calls: sampler and P3P on the device --------------
    @staticmethod
    def make_ransac_hypotheses_device(hypotheses_ptr, hyp_valid_ptr, n_correspondences_ptr=None, samples_ptr=None,
                                      n_solutions_ptr=None) -> RansacHypothesesDevice:
        return RansacHypothesesDevice(*[int(p) if p else None for p in (
            hypotheses_ptr, hyp_valid_ptr, n_correspondences_ptr, samples_ptr, n_solutions_ptr)])

    def ransac3d2d_hypotheses_blocks_device(self, table: LandmarkTableDevice, blocks_ptr, n_multiframes, cam_ids,
                                            poses_T_SC, landmark_ptr, sample_keys_ptr, seed, n_hyp,
                                            result: RansacHypothesesDevice, stream=None):
        """n_hyp pose hypotheses per multiframe for ransac3d2d_consensus_blocks_device (the defined sampler and P3P of
        include/okvfe.h).  sample_keys_ptr: device n_multiframes uint64 or None (the multiframe's index);
        result.hypotheses / result.hyp_valid are that call's hypotheses_ptr / hyp_valid_ptr."""
        cams = np.ascontiguousarray(cam_ids, dtype=np.int32)
        n_cams = len(cams)
        if len(poses_T_SC) != n_cams:
            raise ValueError("cam_ids and poses_T_SC: one per camera")
        P = (Pose * max(n_cams, 1))(*[make_pose(*T) for T in poses_T_SC])
        self._check(lib().okvfe_ransac3d2d_hypotheses_blocks_device(
            self._h, C.byref(table) if table is not None else None, _p(blocks_ptr), int(n_multiframes), n_cams,
            _p(cams) if n_cams else _p(np.zeros(1, np.int32)), P, _p(landmark_ptr), _p(sample_keys_ptr),
            C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(n_hyp), C.byref(result) if result is not None else None,
            _s(stream)))

    def place_hypotheses_blocks_device(self, place_set: PlaceSetDevice, blocks_ptr, n_multiframes, cam_ids, poses_T_SC,
                                       match_landmark_ptr, gate_ptr, sample_keys_ptr, seed, n_hyp,
                                       result: RansacHypothesesDevice, stream=None):
        """The same for place_consensus_blocks_device; with gate_ptr[m] == 0 every hypothesis of multiframe m is
        invalid and nothing is solved."""
        cams = np.ascontiguousarray(cam_ids, dtype=np.int32)
        n_cams = len(cams)
        if len(poses_T_SC) != n_cams:
            raise ValueError("cam_ids and poses_T_SC: one per camera")
        P = (Pose * max(n_cams, 1))(*[make_pose(*T) for T in poses_T_SC])
        self._check(lib().okvfe_place_hypotheses_blocks_device(
            self._h, C.byref(place_set) if place_set is not None else None, _p(blocks_ptr), int(n_multiframes), n_cams,
            _p(cams) if n_cams else _p(np.zeros(1, np.int32)), P, _p(match_landmark_ptr), _p(gate_ptr),
            _p(sample_keys_ptr), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(n_hyp),
            C.byref(result) if result is not None else None, _s(stream)))

    def remove_outliers_blocks_device(self, table: LandmarkTableDevice, blocks_ptr, n_frames, cam_ids, poses_T_WC,
                                      landmark_ptr, landmark_out_ptr, kept_ptr, max_error=REMOVE_OUTLIERS_MAX_ERROR,
                                      stream=None):
        """Frontend::removeOutliers for n_frames gather blocks.  cam_ids / poses_T_WC: host sequences of n_frames camera
        slots / (C, r); landmark_out_ptr may be landmark_ptr; kept_ptr: device n_frames int32."""
        n = int(n_frames)
        cams = np.ascontiguousarray(cam_ids, dtype=np.int32)
        if len(cams) != n or len(poses_T_WC) != n:
            raise ValueError("cam_ids and poses_T_WC: one per frame")
        P = (Pose * max(n, 1))(*[make_pose(*T) for T in poses_T_WC])
        self._check(lib().okvfe_remove_outliers_blocks_device(
            self._h, C.byref(table), _p(blocks_ptr), n, _p(cams) if n else _p(np.zeros(1, np.int32)), P,
            C.c_double(max_error), _p(landmark_ptr), _p(landmark_out_ptr), _p(kept_ptr), _s(stream)))

    # -- before initialisation: the consensus of runRansac2d2d inside the motion-stereo sweep ----
    @staticmethod
    def make_ransac2d2d_result_device(n_correspondences_ptr, rot_best_ptr, rot_inliers_ptr, rel_best_ptr,
                                      rel_inliers_ptr, branch_ptr, removed_ptr, total_inliers_ptr, rotation_only_ptr,
                                      success_ptr, rot_hyp_inliers_ptr=None, rel_hyp_inliers_ptr=None, match1_ptr=None,
                                      state_ptr=None, distance_ptr=None,
                                      landmark1_out_ptr=None) -> Ransac2d2dResultDevice:
        return Ransac2d2dResultDevice(*[int(p) if p else None for p in (
            n_correspondences_ptr, rot_best_ptr, rot_inliers_ptr, rel_best_ptr, rel_inliers_ptr, branch_ptr, removed_ptr,
            total_inliers_ptr, rotation_only_ptr, success_ptr, rot_hyp_inliers_ptr, rel_hyp_inliers_ptr, match1_ptr,
            state_ptr, distance_ptr, landmark1_out_ptr)])

    def ransac2d2d_consensus_blocks_device(self, blocks0_ptr, n_multiframes0, blocks1_ptr, n_multiframes1, mf0, mf1,
                                           cam_ids, landmark0_ptr, landmark1_ptr, added_ptr, n_landmarks, rot_hyp_ptr,
                                           rot_valid_ptr, rel_hyp_ptr, rel_valid_ptr, n_hyp,
                                           result: Ransac2d2dResultDevice, threshold=RANSAC2D2D_THRESHOLD,
                                           remove_outliers=True, stream=None):
        """The consensus step of runRansac2d2d for the pairs (older multiframe mf0[p], current multiframe mf1[p]) of
        len(cam_ids) gather blocks each.  mf0 / mf1 / cam_ids: host sequences; rot_hyp_ptr / rel_hyp_ptr: device
        n_pairs x n_cams x n_hyp x 9 / x 12 doubles; the valid pointers: device bytes or None; added_ptr: device
        n_landmarks bytes or None."""
        a0 = np.ascontiguousarray(mf0, dtype=np.int32).reshape(-1)
        a1 = np.ascontiguousarray(mf1, dtype=np.int32).reshape(-1)
        if len(a0) != len(a1):
            raise ValueError("mf0 and mf1: one per pair")
        cams = np.ascontiguousarray(cam_ids, dtype=np.int32)
        one = np.zeros(1, np.int32)
        self._check(lib().okvfe_ransac2d2d_consensus_blocks_device(
            self._h, _p(blocks0_ptr), int(n_multiframes0), _p(blocks1_ptr), int(n_multiframes1), len(a0),
            _p(a0) if len(a0) else _p(one), _p(a1) if len(a1) else _p(one), len(cams),
            _p(cams) if len(cams) else _p(one), _p(landmark0_ptr), _p(landmark1_ptr), _p(added_ptr), int(n_landmarks),
            _p(rot_hyp_ptr), _p(rot_valid_ptr), _p(rel_hyp_ptr), _p(rel_valid_ptr), int(n_hyp), C.c_double(threshold),
            int(bool(remove_outliers)), C.byref(result) if result is not None else None, _s(stream)))

    @staticmethod
    def make_ransac2d2d_hypotheses_device(rot_hyp_ptr, rot_valid_ptr, rel_hyp_ptr, rel_valid_ptr,
                                          n_correspondences_ptr=None, rot_samples_ptr=None, rel_samples_ptr=None,
                                          rel_n_roots_ptr=None) -> Ransac2d2dHypothesesDevice:
        return Ransac2d2dHypothesesDevice(*[int(p) if p else None for p in (
            rot_hyp_ptr, rot_valid_ptr, rel_hyp_ptr, rel_valid_ptr, n_correspondences_ptr, rot_samples_ptr,
            rel_samples_ptr, rel_n_roots_ptr)])

    def ransac2d2d_hypotheses_blocks_device(self, blocks0_ptr, n_multiframes0, blocks1_ptr, n_multiframes1, mf0, mf1,
                                            cam_ids, landmark0_ptr, landmark1_ptr, added_ptr, n_landmarks,
                                            sample_keys_ptr, seed, n_hyp, result: Ransac2d2dHypothesesDevice,
                                            stream=None):
        """n_hyp hypotheses of both problems per (pair, camera) for ransac2d2d_consensus_blocks_device (the defined
        sampler, two-point and five-point solvers of include/okvfe.h).  The block, pair and id arguments are that
        call's; sample_keys_ptr: device n_pairs uint64 or None (the pair's index); result.rot_hyp / rot_valid /
        rel_hyp / rel_valid are that call's rot_hyp_ptr / rot_valid_ptr / rel_hyp_ptr / rel_valid_ptr."""
        a0 = np.ascontiguousarray(mf0, dtype=np.int32).reshape(-1)
        a1 = np.ascontiguousarray(mf1, dtype=np.int32).reshape(-1)
        if len(a0) != len(a1):
            raise ValueError("mf0 and mf1: one per pair")
        cams = np.ascontiguousarray(cam_ids, dtype=np.int32)
        one = np.zeros(1, np.int32)
        self._check(lib().okvfe_ransac2d2d_hypotheses_blocks_device(
            self._h, _p(blocks0_ptr), int(n_multiframes0), _p(blocks1_ptr), int(n_multiframes1), len(a0),
            _p(a0) if len(a0) else _p(one), _p(a1) if len(a1) else _p(one), len(cams),
            _p(cams) if len(cams) else _p(one), _p(landmark0_ptr), _p(landmark1_ptr), _p(added_ptr), int(n_landmarks),
            _p(sample_keys_ptr), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(n_hyp),
            C.byref(result) if result is not None else None, _s(stream)))

    # -- matchStereo's landmark bookkeeping, chained over the pairs of a rig ---------------------
    @staticmethod
    def make_stereo_insert_device(action_ptr, lm_ptr, landmark_out_ptr, counts_ptr) -> StereoInsertDevice:
        return StereoInsertDevice(*[int(p) if p else None for p in (action_ptr, lm_ptr, landmark_out_ptr, counts_ptr)])

    def stereo_insert_blocks_device(self, table: LandmarkTableDevice, initialised_ptr, blocks_ptr, block_stride_m,
                                    block_stride_c, n_multiframes, pairs, cam_ids, poses_T_WC, matches_ptr, landmark_ptr,
                                    as_keyframe_ptr, result: StereoInsertDevice, stream=None):
        """Frontend.cpp:2076-2141 for n_multiframes multiframes of len(cam_ids) cameras over the ordered camera `pairs`
        (host, n_pairs x 2).  poses_T_WC: host sequence of n_multiframes x n_cams (C, r), multiframe-major; matches_ptr:
        device n_pairs x n_multiframes x K rows of the stereo matcher; landmark_ptr: device int32, K per block;
        as_keyframe_ptr: device bytes or None; result.landmark_out may be landmark_ptr."""
        n = int(n_multiframes)
        cams = np.ascontiguousarray(cam_ids, dtype=np.int32)
        n_cams = len(cams)
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        if len(poses_T_WC) != n * n_cams:
            raise ValueError("poses_T_WC: one per (multiframe, camera)")
        P = (Pose * max(n * n_cams, 1))(*[make_pose(*T) for T in poses_T_WC])
        self._check(lib().okvfe_stereo_insert_blocks_device(
            self._h, C.byref(table) if table is not None else None, _p(initialised_ptr), _p(blocks_ptr),
            int(block_stride_m), int(block_stride_c), n, n_cams, _p(pr) if len(pr) else _p(np.zeros(2, np.int32)),
            len(pr), _p(cams) if n_cams else _p(np.zeros(1, np.int32)), P, _p(matches_ptr), _p(landmark_ptr),
            _p(as_keyframe_ptr), C.byref(result) if result is not None else None, _s(stream)))

    # -- loop closure: verifyRecognisedPlace after its descriptor matching ---------------------
    place_landmark_set = staticmethod(place_landmark_set)

    @staticmethod
    def make_place_set_device(n_landmarks, hp_ptr) -> PlaceSetDevice:
        return PlaceSetDevice(int(n_landmarks), int(hp_ptr) if hp_ptr else None)

    @staticmethod
    def make_place_claims_device(n_matches_ptr, n_points_ptr, n_correspondences_ptr, gate_ptr,
                                 match_landmark_ptr) -> PlaceClaimsDevice:
        return PlaceClaimsDevice(*[int(p) if p else None for p in (
            n_matches_ptr, n_points_ptr, n_correspondences_ptr, gate_ptr, match_landmark_ptr)])

    def place_claims_blocks_device(self, place_set: PlaceSetDevice, blocks_ptr, n_multiframes, n_cams, k_min_ptr,
                                   dist_min_ptr, min_inliers, result: PlaceClaimsDevice, stream=None):
        """The claims and count gates of verifyRecognisedPlace (Frontend.cpp:347-351, 359, 380) for n_multiframes
        multiframes of n_cams gather blocks, from the rows okvfe_verify_place_blocks_device wrote (blocks x L)."""
        self._check(lib().okvfe_place_claims_blocks_device(
            self._h, C.byref(place_set) if place_set is not None else None, _p(blocks_ptr), int(n_multiframes),
            int(n_cams), _p(k_min_ptr), _p(dist_min_ptr), int(min_inliers),
            C.byref(result) if result is not None else None, _s(stream)))

    def place_consensus_blocks_device(self, place_set: PlaceSetDevice, blocks_ptr, n_multiframes, cam_ids, poses_T_SC,
                                      match_landmark_ptr, gate_ptr, hypotheses_ptr, hyp_valid_ptr, n_hyp, min_inliers,
                                      result: RansacResultDevice, verdict_ptr, threshold=RANSAC_THRESHOLD, stream=None):
        """The consensus and verdict of verifyRecognisedPlace (Frontend.cpp:372-397).  verdict_ptr: device bytes per
        multiframe, an index into PLACE_VERDICTS; the other arguments as ransac3d2d_consensus_blocks_device."""
        cams = np.ascontiguousarray(cam_ids, dtype=np.int32)
        n_cams = len(cams)
        if len(poses_T_SC) != n_cams:
            raise ValueError("cam_ids and poses_T_SC: one per camera")
        P = (Pose * max(n_cams, 1))(*[make_pose(*T) for T in poses_T_SC])
        self._check(lib().okvfe_place_consensus_blocks_device(
            self._h, C.byref(place_set) if place_set is not None else None, _p(blocks_ptr), int(n_multiframes), n_cams,
            _p(cams) if n_cams else _p(np.zeros(1, np.int32)), P, _p(match_landmark_ptr), _p(gate_ptr),
            _p(hypotheses_ptr), _p(hyp_valid_ptr), int(n_hyp), C.c_double(threshold), int(min_inliers),
            C.byref(result) if result is not None else None, _p(verdict_ptr), _s(stream)))

    @staticmethod
    def make_place_hessian_device(H_ptr, n_terms_ptr, n_singular_ptr, residual_ptr=None,
                                  jacobian_minimal_ptr=None) -> PlaceHessianDevice:
        return PlaceHessianDevice(*[int(p) if p else None for p in (
            H_ptr, n_terms_ptr, n_singular_ptr, residual_ptr, jacobian_minimal_ptr)])

    def place_hessian_blocks_device(self, place_set: PlaceSetDevice, blocks_ptr, n_multiframes, cam_ids, T_SC_params,
                                    poses_ptr, match_landmark_ptr, state_ptr, verdict_ptr, result: PlaceHessianDevice,
                                    stream=None):
        """The Hessian H of verifyRecognisedPlace (Frontend.cpp:529-551) and the residual and minimal Jacobian of every
        inlier of the consensus.  T_SC_params: host, one (t[3], qx, qy, qz, qw) per camera; poses_ptr: device,
        n_multiframes x 7 doubles in the same layout; state_ptr: the consensus call's state rows; verdict_ptr: its
        verdict bytes, or None (every multiframe counts)."""
        cams = np.ascontiguousarray(cam_ids, dtype=np.int32)
        n_cams = len(cams)
        prm = np.ascontiguousarray(T_SC_params, dtype=np.float64).reshape(-1)
        if len(prm) != 7 * n_cams:
            raise ValueError("cam_ids and T_SC_params: seven doubles per camera")
        self._check(lib().okvfe_place_hessian_blocks_device(
            self._h, C.byref(place_set) if place_set is not None else None, _p(blocks_ptr), int(n_multiframes), n_cams,
            _p(cams) if n_cams else _p(np.zeros(1, np.int32)), _p(prm) if n_cams else _p(np.zeros(7)), _p(poses_ptr),
            _p(match_landmark_ptr), _p(state_ptr), _p(verdict_ptr), C.byref(result) if result is not None else None,
            _s(stream)))

    @staticmethod
    def make_place_refine_device(poses_ptr, status_ptr, n_iterations_ptr=None, n_accepted_ptr=None, n_terms_ptr=None,
                                 cost_ptr=None, start_poses_ptr=None, H_ptr=None, n_singular_ptr=None) -> PlaceRefineDevice:
        return PlaceRefineDevice(*[int(p) if p else None for p in (
            poses_ptr, status_ptr, n_iterations_ptr, n_accepted_ptr, n_terms_ptr, cost_ptr, start_poses_ptr, H_ptr,
            n_singular_ptr)])

    def place_refine_blocks_device(self, place_set: PlaceSetDevice, blocks_ptr, n_multiframes, cam_ids, T_SC_params,
                                   hypotheses_ptr, n_hyp, best_hypothesis_ptr, initial_poses_ptr, match_landmark_ptr,
                                   state_ptr, verdict_ptr, max_iterations, result: PlaceRefineDevice, stream=None):
        """The refinement of T_Sold_Snew of verifyRecognisedPlace (Frontend.cpp:399-527) as the defined algorithm of
        include/okvfe.h, and H at the pose out.  The start: initial_poses_ptr (device, n_multiframes x 7) where given,
        else hypothesis best_hypothesis_ptr[m] of hypotheses_ptr (device, n_multiframes x n_hyp x 12).  The other
        arguments are those of place_hessian_blocks_device.  Nothing waits for the device."""
        cams = np.ascontiguousarray(cam_ids, dtype=np.int32)
        n_cams = len(cams)
        prm = np.ascontiguousarray(T_SC_params, dtype=np.float64).reshape(-1)
        if len(prm) != 7 * n_cams:
            raise ValueError("cam_ids and T_SC_params: seven doubles per camera")
        self._check(lib().okvfe_place_refine_blocks_device(
            self._h, C.byref(place_set) if place_set is not None else None, _p(blocks_ptr), int(n_multiframes), n_cams,
            _p(cams) if n_cams else _p(np.zeros(1, np.int32)), _p(prm) if n_cams else _p(np.zeros(7)),
            _p(hypotheses_ptr), int(n_hyp), _p(best_hypothesis_ptr), _p(initial_poses_ptr), _p(match_landmark_ptr),
            _p(state_ptr), _p(verdict_ptr), int(max_iterations), C.byref(result) if result is not None else None,
            _s(stream)))

    # -- IMU propagation on device-resident batches -------------------------------------------
    def imu_propagation_blocks_device(self, params, samples_ptr, sample_begin_ptr, states_ptr, n_multiframes,
                                      T_SC_params, result: ImuResultDevice, stream=None):
        """ImuError::propagation (ImuError.cpp:557-779) for n_multiframes multiframes in one launch.  params: a mapping
        or an ImuParams; samples_ptr / sample_begin_ptr / states_ptr: device, the layout of include/okvfe.h;
        T_SC_params: host, one (t[3], qx, qy, qz, qw) per camera (None: no cameras); result: make_imu_result -- the
        form follows the optional outputs asked for."""
        p = params if isinstance(params, ImuParams) else make_imu_params(params)
        prm, n_cams = _imu_T_SC(T_SC_params)
        self._check(lib().okvfe_imu_propagation_blocks_device(
            self._h, C.byref(p), _p(samples_ptr), _p(sample_begin_ptr), _p(states_ptr), int(n_multiframes), n_cams,
            _p(prm) if n_cams else None, C.byref(result) if result is not None else None, _s(stream)))

    # -- place recognition: the DBoW2 query and database on device-resident batches -----------
    def bow_vectors_blocks_device(self, vocabulary: VocabularyDevice, blocks_ptr, n_multiframes, n_cams,
                                  vectors: BowVectorsDevice, word_ids_ptr=None, stream=None):
        """BowVectors of n_multiframes multiframes of n_cams gather blocks (Frontend.cpp:660-672 + DBoW2's transform) into
        the device rows of `vectors`; word_ids_ptr: None or device blocks x K int32."""
        self._check(lib().okvfe_bow_vectors_blocks_device(
            self._h, C.byref(vocabulary) if vocabulary is not None else None, _p(blocks_ptr), int(n_multiframes),
            int(n_cams), C.byref(vectors) if vectors is not None else None, _p(word_ids_ptr), _s(stream)))

    def place_query_blocks_device(self, database: BowDatabaseDevice, vectors: BowVectorsDevice, n_multiframes,
                                  result: PlaceCandidatesDevice, min_score=PLACE_MIN_SCORE, suppressible_ptr=None,
                                  scores_ptr=None, stream=None):
        """database.query and the estimator-free part of the walk (Frontend.cpp:761-802): per multiframe n_listed, the
        true n_candidates and the first result.cap candidates.  suppressible_ptr: None (all ones) or device n_entries
        bytes; scores_ptr: None or device M x n_entries doubles."""
        self._check(lib().okvfe_place_query_blocks_device(
            self._h, C.byref(database) if database is not None else None,
            C.byref(vectors) if vectors is not None else None, int(n_multiframes), C.c_double(min_score),
            _p(suppressible_ptr), _p(scores_ptr), C.byref(result) if result is not None else None, _s(stream)))

    def bow_database_add_blocks_device(self, database: BowDatabaseDevice, vectors: BowVectorsDevice, n_multiframes,
                                       add_index, stream=None):
        """database.add (Frontend.cpp:896-898) for the multiframes add_index (host ints, strictly ascending):
        database.n_entries (host) grows by len(add_index)."""
        idx = np.ascontiguousarray(add_index, dtype=np.int32).reshape(-1)
        self._check(lib().okvfe_bow_database_add_blocks_device(
            self._h, C.byref(database) if database is not None else None,
            C.byref(vectors) if vectors is not None else None, int(n_multiframes), _p(idx) if len(idx) else None,
            len(idx), _s(stream)))

    def bow_database_check_device(self, database: BowDatabaseDevice, stream=None):
        """Waits for the stream; raises OkvfeError(ERR_CAPACITY) if an add stored entries empty for want of room."""
        self._check(lib().okvfe_bow_database_check_device(
            self._h, C.byref(database) if database is not None else None, _s(stream)))

    @staticmethod
    def _test_ransac_chunk_records() -> int:
        """test hook (not part of include/okvfe.h): correspondences the consensus kernel scores at a time"""
        f = lib().okvfe_test_ransac_chunk_records
        f.restype = C.c_int32
        return int(f())

    @staticmethod
    def _test_place_hessian_chunk_terms() -> int:
        """test hook (not part of include/okvfe.h): terms the Hessian kernel evaluates at a time"""
        f = lib().okvfe_test_place_hessian_chunk_terms
        f.restype = C.c_int32
        return int(f())

    @staticmethod
    def _test_ransac2d2d_chunk_records() -> int:
        """test hook (not part of include/okvfe.h): correspondences the 2d2d consensus kernel scores at a time"""
        f = lib().okvfe_test_ransac2d2d_chunk_records
        f.restype = C.c_int32
        return int(f())

    @staticmethod
    def _test_ransac_ring_records() -> int:
        """test hook (not part of include/okvfe.h): records of the consensus kernel's LDS ring"""
        f = lib().okvfe_test_ransac_ring_records
        f.restype = C.c_int32
        return int(f())

    @staticmethod
    def _test_ransac2d2d_ring_records() -> int:
        """test hook (not part of include/okvfe.h): records of the 2d2d consensus kernel's LDS ring"""
        f = lib().okvfe_test_ransac2d2d_ring_records
        f.restype = C.c_int32
        return int(f())

    @staticmethod
    def _test_ransac2d2d_id_slot(landmark_id) -> int:
        """test hook (not part of include/okvfe.h): the home slot of a landmark id in the 2d2d consensus kernel's id
        table of RANSAC2D2D_MAX_KEYPOINTS + 1 slots"""
        f = lib().okvfe_test_ransac2d2d_id_slot
        f.argtypes = [C.c_int32]
        f.restype = C.c_int32
        return int(f(int(landmark_id)))

    def _test_set_map_table_workspace_limit(self, nbytes):
        """test hook (not part of include/okvfe.h): the workspace size above which the call above slices its frames"""
        f = lib().okvfe_test_set_map_table_workspace_limit
        f.argtypes = [C.c_void_p, C.c_uint64]
        self._check(f(self._h, int(nbytes)))

    def _test_context_sizes(self, stream=None) -> dict:
        """test hook (not part of include/okvfe.h), read-only: slot size and device address of the pair ring, size and
        address of `stream`'s entries in the two per-stream workspace lists (0 without one), the entries of each list"""
        f = lib().okvfe_test_context_sizes
        f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        out = (C.c_uint64 * 8)()
        self._check(f(self._h, _s(stream), out))
        keys = ("ring_slot_bytes", "ring_dev", "table_ws_bytes", "table_ws_dev", "perm_bytes", "perm_dev",
                "table_ws_entries", "perm_entries")
        return dict(zip(keys, (int(v) for v in out)))

    def verify_place_blocks_device(self, blocks_ptr, n_frames, map_dev, k_min_ptr, dist_min_ptr, stream=None):
        self._check(lib().okvfe_verify_place_blocks_device(
            self._h, _p(blocks_ptr), int(n_frames), C.byref(map_dev), _p(k_min_ptr), _p(dist_min_ptr),
            _s(stream)))

    # -- keyframe decision: coverage masks of doWeNeedANewKeyframe -------------------------
    def keyframe_coverage_blocks_device(self, blocks_ptr, n_frames, landmark_ids_ptr, coverage_ptr, id_set_ptr=None,
                                        n_id_set=0, kptrad=KPTRAD, stream=None):
        """landmark_ids_ptr: device u64 [n_frames][max_keypoints]; coverage_ptr: device COVERAGE_DTYPE [n_frames];
        id_set_ptr None: matched = id != 0, else id != 0 and among the n_id_set u64 at id_set_ptr (device)."""
        self._check(lib().okvfe_keyframe_coverage_blocks_device(
            self._h, _p(blocks_ptr), int(n_frames), _p(landmark_ids_ptr), _p(id_set_ptr), int(n_id_set),
            C.c_double(kptrad), _p(coverage_ptr), _s(stream)))

    def keyframe_coverage(self, keypoints, landmark_ids, id_set=None, kptrad=KPTRAD):
        """The B = 1 host seam: one image's keypoints and landmark ids in, its COVERAGE_DTYPE record out."""
        kps = np.ascontiguousarray(keypoints, dtype=KEYPOINT_DTYPE)
        ids = np.ascontiguousarray(landmark_ids, dtype=np.uint64)
        if len(ids) != len(kps):
            raise ValueError("landmark_ids: one per keypoint")
        s = None if id_set is None else np.ascontiguousarray(id_set, dtype=np.uint64).reshape(-1)
        if s is not None and len(s) == 0:
            s = np.zeros(1, dtype=np.uint64)  # the empty set, not "no set": a non-null pointer with n_id_set = 0
            n_set = 0
        else:
            n_set = 0 if s is None else len(s)
        out = np.zeros(1, dtype=COVERAGE_DTYPE)
        self._check(lib().okvfe_keyframe_coverage(self._h, _p(kps) if len(kps) else None, len(kps),
                                                  _p(ids) if len(ids) else None, _p(s), n_set,
                                                  C.c_double(kptrad), _p(out)))
        return out[0]

    def overlap_pairs_blocks_device(self, blocks_ptr, block_stride_m, block_stride_c, n_multiframes, n_cams,
                                    landmark_ids_ptr, pair_a, pair_b, counts_ptr, coverage_ptr=None, kptrad=KPTRAD,
                                    stream=None):
        """ViSlamBackend::overlapFraction up to its counts for len(pair_a) ordered multiframe pairs in one launch.
        The block of (m, c) is block m * block_stride_m + c * block_stride_c; landmark_ids_ptr: device u64, K per block
        at that block index; pair_a / pair_b: host int sequences; counts_ptr: device OVERLAP_COUNTS_DTYPE [n_pairs];
        coverage_ptr: None, or device COVERAGE_DTYPE [n_pairs][2][n_cams]."""
        a = np.ascontiguousarray(pair_a, dtype=np.int32).reshape(-1)
        b = np.ascontiguousarray(pair_b, dtype=np.int32).reshape(-1)
        if len(a) != len(b):
            raise ValueError("pair_a / pair_b: one multiframe index each per pair")
        n = len(a)
        self._check(lib().okvfe_overlap_pairs_blocks_device(
            self._h, _p(blocks_ptr), int(block_stride_m), int(block_stride_c), int(n_multiframes), int(n_cams),
            _p(landmark_ids_ptr), _p(a) if n else None, _p(b) if n else None, n, C.c_double(kptrad), _p(counts_ptr),
            _p(coverage_ptr), _s(stream)))

    # -- gather blocks --------------------------------------------------------------------
    def gather_block_bytes(self) -> int:
        return int(lib().okvfe_gather_block_bytes(self._h))

    def pack_gather_block_device(self, index, block_ptr, stream=None):
        self._check(lib().okvfe_pack_gather_block_device(self._h, int(index), _p(block_ptr),
                                                         _s(stream)))

    def pack_gather_blocks_device(self, first, n, blocks_ptr, stream=None):
        self._check(lib().okvfe_pack_gather_blocks_device(self._h, int(first), int(n),
                                                          _p(blocks_ptr), _s(stream)))

    def match_stereo_blocks_batch_device(self, blocks0_ptr, blocks1_ptr, n_frames, T0, T1, f0, f1,
                                         matches_ptr, stream=None):
        P0, P1 = make_pose(*T0), make_pose(*T1)
        self._check(lib().okvfe_match_stereo_blocks_batch_device(
            self._h, _p(blocks0_ptr), _p(blocks1_ptr), int(n_frames), C.byref(P0), C.byref(P1),
            C.c_double(f0), C.c_double(f1), _p(matches_ptr), _s(stream)))

    def match_motion_stereo_blocks_device(self, cam, block0_ptr, block1_ptr, skip0_ptr,
                                          matched1_ptr, T0, T1, matches_ptr, stream=None):
        P0, P1 = make_pose(*T0), make_pose(*T1)
        self._check(lib().okvfe_match_motion_stereo_blocks_device(
            self._h, int(cam), _p(block0_ptr), _p(block1_ptr), _p(skip0_ptr), _p(matched1_ptr),
            C.byref(P0), C.byref(P1), _p(matches_ptr), _s(stream)))

    def match_motion_stereo_blocks_batch_device(self, blocks0_ptr, n_blocks0, blocks1_ptr, n_blocks1, idx0, idx1,
                                                cam_ids, poses_T_WC0, poses_T_WC1, skip0_ptr, matched1_ptr,
                                                matches_ptr, claim=None, stream=None):
        """matchMotionStereo for len(cam_ids) (older block idx0[p], current block idx1[p], camera slot cam_ids[p])
        pairs in one launch.  idx0 / idx1: host int sequences or None (= pair p uses block p); poses: host sequences of
        (C, r), one per pair; skip0_ptr: device n_pairs x K (pair-major) or None; matched1_ptr: device n_blocks1 x K
        (by current block) or None; matches_ptr: device n_pairs x K MOTION_MATCH_DTYPE.  claim: None, or a dict of
        device pointers {"claimed": n_pairs x K uint8, "n_claimed": n_pairs int32, "matched1_out": n_blocks1 x K uint8
        or None (may be matched1_ptr)} -- the frame-data part of the insertion loop (Frontend.cpp:1915-1958)."""
        cams = np.ascontiguousarray(cam_ids, dtype=np.int32)
        n = len(cams)
        if len(poses_T_WC0) != n or len(poses_T_WC1) != n:
            raise ValueError("poses: one (C, r) per pair")
        i0 = None if idx0 is None else np.ascontiguousarray(idx0, dtype=np.int32)
        i1 = None if idx1 is None else np.ascontiguousarray(idx1, dtype=np.int32)
        if (i0 is not None and len(i0) != n) or (i1 is not None and len(i1) != n):
            raise ValueError("idx0 / idx1: one block index per pair")
        P0 = (Pose * max(n, 1))(*[make_pose(*T) for T in poses_T_WC0])
        P1 = (Pose * max(n, 1))(*[make_pose(*T) for T in poses_T_WC1])
        cd = None
        if claim is not None:
            cd = MotionClaimDevice(int(claim["claimed"] or 0) or None, int(claim["n_claimed"] or 0) or None,
                                   int(claim.get("matched1_out") or 0) or None)
        self._check(lib().okvfe_match_motion_stereo_blocks_batch_device(
            self._h, _p(blocks0_ptr), int(n_blocks0), _p(blocks1_ptr), int(n_blocks1), n,
            _p(i0) if n else None, _p(i1) if n else None, _p(cams) if n else None, P0, P1, _p(skip0_ptr),
            _p(matched1_ptr), _p(matches_ptr), C.byref(cd) if cd is not None else None, _s(stream)))

    def match_stereo_blocks_device(self, block0_ptr, block1_ptr, T0, T1, f0, f1, matches_ptr,
                                   stream=None):
        P0, P1 = make_pose(*T0), make_pose(*T1)
        self._check(lib().okvfe_match_stereo_blocks_device(self._h, _p(block0_ptr), _p(block1_ptr),
                                                           C.byref(P0), C.byref(P1),
                                                           C.c_double(f0), C.c_double(f1),
                                                           _p(matches_ptr), _s(stream)))
