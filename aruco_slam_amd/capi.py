"""ctypes binding of libaruco_slam_hip.so (include/aruco_slam_hip.h).

The product path is the hipcc/gfx950 build next to this file.  There is no CPU fallback: if the library
is missing, or no HIP device is usable, loading / `Context()` raises.  (The parity tests may point
ARUCO_SLAM_LIB at the CPU *emulation* build of the same sources under tests/hipemu — test
infrastructure used only by `-m "not gpu"` tests to exercise kernel logic in the GPU-less container.)
"""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "libaruco_slam_hip.so")

ASLAM_OK = 0
E_NAMES = {-1: "INVALID", -2: "NO_DEVICE", -3: "HIP", -4: "CAPACITY", -5: "STATE"}
MAP_RECORD_BYTES = 104
MARKER_MAX = 128
CAND_MAX = 2048
ID_TABLE_SIZE = 1024


class AslamInit(C.Structure):
    _fields_ = [
        ("Q_k", C.c_double), ("R_x", C.c_double), ("R_y", C.c_double), ("R_theta", C.c_double),
        ("kl", C.c_double), ("kr", C.c_double), ("b", C.c_double),
        ("marker_length", C.c_double),
        ("markers_dictionary", C.c_int),
        ("useful_distance_threshold", C.c_float),
        ("r2c_t", C.c_double * 3), ("r2c_q", C.c_double * 4),
        ("device_id", C.c_int),
        ("max_landmarks", C.c_int),
        ("max_rows", C.c_int), ("max_cols", C.c_int),
        ("max_batch", C.c_int),
        ("persistent_waves", C.c_int),
        ("max_updates_per_frame", C.c_int),
        ("cap_starts_per_frame", C.c_uint),
        ("cap_contours_per_frame", C.c_uint),
        ("cap_points_per_frame", C.c_uint),
        ("ekf_reserved_cus_per_xcd", C.c_int),
    ]


class DetectorParams(C.Structure):
    """mirror of aslam_detector_params (cv::aruco::DetectorParameters of OpenCV 3.2.0)"""
    _fields_ = [
        ("adaptiveThreshWinSizeMin", C.c_int), ("adaptiveThreshWinSizeMax", C.c_int), ("adaptiveThreshWinSizeStep", C.c_int),
        ("adaptiveThreshConstant", C.c_double),
        ("minMarkerPerimeterRate", C.c_double), ("maxMarkerPerimeterRate", C.c_double),
        ("polygonalApproxAccuracyRate", C.c_double),
        ("minCornerDistanceRate", C.c_double),
        ("minDistanceToBorder", C.c_int),
        ("minMarkerDistanceRate", C.c_double),
        ("doCornerRefinement", C.c_int),
        ("cornerRefinementWinSize", C.c_int), ("cornerRefinementMaxIterations", C.c_int),
        ("cornerRefinementMinAccuracy", C.c_double),
        ("markerBorderBits", C.c_int),
        ("perspectiveRemovePixelPerCell", C.c_int),
        ("perspectiveRemoveIgnoredMarginPerCell", C.c_double),
        ("maxErroneousBitsInBorderRate", C.c_double),
        ("minOtsuStdDev", C.c_double),
        ("errorCorrectionRate", C.c_double),
    ]


MAX_CAMERAS = 8
MAX_ROBOTS = 256


class Camera(C.Structure):
    """mirror of aslam_camera: one camera of a rig (K row-major, plumb-bob D, planar mount in base_link)"""
    _fields_ = [("K", C.c_double * 9), ("D", C.c_double * 5), ("nD", C.c_int), ("pad", C.c_int),
                ("mount_x", C.c_double), ("mount_y", C.c_double), ("mount_yaw", C.c_double)]

    @classmethod
    def make(cls, K, D=None, mount=(0.0, 0.0, 0.0)):
        c = cls()
        K = np.asarray(K, np.float64).reshape(9)
        D = np.zeros(0) if D is None else np.asarray(D, np.float64).reshape(-1)
        for i in range(9):
            c.K[i] = K[i]
        for i in range(min(D.size, 5)):
            c.D[i] = D[i]
        c.nD = int(D.size)
        c.mount_x, c.mount_y, c.mount_yaw = (float(v) for v in mount)
        return c


class PoseMsg(C.Structure):
    _fields_ = [("position", C.c_double * 3), ("orientation", C.c_double * 4), ("covariance", C.c_double * 36)]


class MarkerMsg(C.Structure):
    _fields_ = [("id", C.c_int), ("pad", C.c_int), ("scale", C.c_double * 3), ("color", C.c_float * 4), ("position", C.c_double * 3),
                ("orientation", C.c_double * 4), ("lifetime_sec", C.c_double)]


class RelocalizeParams(C.Structure):
    """mirror of aslam_relocalize_params"""
    _fields_ = [("tol_xy", C.c_double), ("tol_th", C.c_double), ("min_inliers", C.c_int)]


# mirror of aslam_relocalize_result: what Context.relocalize / fleet_relocalize return (sigma row-major 3 x 3)
RELOC_DTYPE = np.dtype([("status", "<i4"), ("n_candidates", "<i4"), ("n_inliers", "<i4"), ("runner_up", "<i4"), ("best", "<i4"),
                        ("pose", "<f8", (3,)), ("sigma", "<f8", (3, 3))], align=True)


class GateParams(C.Structure):
    """mirror of aslam_gate_params"""
    _fields_ = [("gate_d2", C.c_double), ("min_attempted", C.c_int), ("min_accept_percent", C.c_int), ("lost_after", C.c_int),
                ("pad", C.c_int)]


# mirrors of aslam_slot_health / aslam_track_health: what Context.get_slot_health / get_track_health / fleet_get_health return
SLOT_HEALTH_DTYPE = np.dtype([("attempted", "<i4"), ("accepted", "<i4"), ("rejected", "<i4"), ("ref_flagged", "<i4"), ("nis_sum", "<f8"),
                              ("d2_max", "<f8"), ("worst_id", "<i4"), ("pad", "<i4")], align=True)
TRACK_HEALTH_DTYPE = np.dtype([("frames", "<i4"), ("accepted_total", "<i4"), ("rejected_total", "<i4"), ("bad_streak", "<i4"),
                               ("lost", "<i4"), ("pad", "<i4", (3,))], align=True)


class ConfirmParams(C.Structure):
    """mirror of aslam_confirm_params"""
    _fields_ = [("min_sightings", C.c_int), ("max_gap", C.c_int)]


# mirror of aslam_slot_confirm: what Context.get_slot_confirm returns
SLOT_CONFIRM_DTYPE = np.dtype([("judged", "<i4"), ("tentative", "<i4"), ("withheld", "<i4"), ("promoted", "<i4"),
                               ("withheld_mask", "<u4", (4,))], align=True)


class PoseAmbiguityParams(C.Structure):
    """mirror of aslam_pose_ambiguity_params"""
    _fields_ = [("ratio", C.c_double), ("floor_px", C.c_double), ("min_dtheta", C.c_double), ("reject", C.c_int), ("pad", C.c_int)]


# mirrors of aslam_pose_ambiguity / aslam_slot_pose_ambiguity: what Context.get_slot_pose_ambiguity returns
POSE_AMBIGUITY_DTYPE = np.dtype([("rvec_alt", "<f8", (3,)), ("tvec_alt", "<f8", (3,)), ("xyth_alt", "<f8", (3,)), ("rms", "<f8"),
                                 ("rms_alt", "<f8"), ("dtheta", "<f8"), ("flags", "<i4"), ("iters", "<i4")], align=True)
SLOT_POSE_AMBIGUITY_DTYPE = np.dtype([("checked", "<i4"), ("ambiguous", "<i4"), ("rejected", "<i4"), ("pad", "<i4")], align=True)


class ObsCovarianceParams(C.Structure):
    """mirror of aslam_obs_covariance_params"""
    _fields_ = [("sigma_px", C.c_double), ("scale", C.c_double), ("floor_xy", C.c_double), ("floor_th", C.c_double),
                ("gate_norm", C.c_double), ("use_residual", C.c_int), ("pad", C.c_int)]


# mirrors of aslam_obs_covariance / aslam_slot_obs_covariance: what Context.get_slot_obs_covariance returns
OBS_COVARIANCE_DTYPE = np.dtype([("cov", "<f8", (3, 3)), ("sigma2", "<f8"), ("e2", "<f8"), ("r_ref", "<f8", (3,)), ("flags", "<i4"),
                                 ("pad", "<i4")], align=True)
SLOT_OBS_COVARIANCE_DTYPE = np.dtype([("checked", "<i4"), ("degenerate", "<i4"), ("gated", "<i4"), ("pad", "<i4")], align=True)


class AslamError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"aslam error {code} ({E_NAMES.get(code, '?')}): {msg}")
        self.code = code


_P = C.POINTER
_u8p, _ip, _fp, _dp, _llp = _P(C.c_uint8), _P(C.c_int), _P(C.c_float), _P(C.c_double), _P(C.c_longlong)
_up = _P(C.c_uint)

_SIGS = {
    "aslam_default_init": (None, [_P(AslamInit)]),
    "aslam_create": (C.c_int, [_P(AslamInit), _P(C.c_void_p)]),
    "aslam_destroy": (None, [C.c_void_p]),
    "aslam_last_error": (C.c_char_p, [C.c_void_p]),
    "aslam_set_camera": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int]),
    "aslam_get_pose_msg": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aslam_get_map_markers": (C.c_int, [C.c_void_p, C.c_int, _ip, C.c_void_p]),
    "aslam_get_detected_markers": (C.c_int, [C.c_void_p, C.c_int, _ip, C.c_void_p]),
    "aslam_export_map_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "aslam_export_wait": (C.c_int, [C.c_void_p, C.c_int]),
    "aslam_draw_detected_markers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t]),
    "aslam_load_map_txt": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, _ip, C.c_void_p]),
    "aslam_localize_begin": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp, _dp, _dp]),
    "aslam_localize_end": (C.c_int, [C.c_void_p]),
    "aslam_is_localizing": (C.c_int, [C.c_void_p, _ip]),
    "aslam_localize_begin_uncertain": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp, _dp, _dp, _dp]),
    "aslam_fleet_begin_uncertain": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, _ip, _dp, _dp, _dp, _dp]),
    "aslam_is_map_uncertain": (C.c_int, [C.c_void_p, _ip]),
    "aslam_fleet_get_cross": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp]),
    "aslam_landmarks_from_markers": (C.c_int, [C.c_int, C.c_void_p, _ip, _dp]),
    "aslam_fleet_begin": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, _ip, _dp, _dp, _dp]),
    "aslam_fleet_add_images": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp, _dp, _dp, _P(C.c_void_p), C.c_int, C.c_int, C.c_int, _P(C.c_size_t)]),
    "aslam_fleet_run_staged": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip, C.c_int]),
    "aslam_fleet_get_poses": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp, _dp]),
    "aslam_fleet_set_pose": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    "aslam_fleet_end": (C.c_int, [C.c_void_p]),
    "aslam_is_fleet": (C.c_int, [C.c_void_p, _ip]),
    "aslam_fleet_slam_begin": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "aslam_is_fleet_slam": (C.c_int, [C.c_void_p, _ip]),
    "aslam_fleet_get_state": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp, _dp]),
    "aslam_fleet_set_state": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _ip]),
    "aslam_fleet_get_landmark_ids": (C.c_int, [C.c_void_p, C.c_int, _ip, _ip]),
    "aslam_remove_landmarks": (C.c_int, [C.c_void_p, C.c_int, _ip, _ip]),
    "aslam_fleet_remove_landmarks": (C.c_int, [C.c_void_p, C.c_int, _ip, C.c_int, _ip, _ip]),
    "aslam_merge_map_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, _dp, _dp,
                                          _ip, _ip, _dp]),
    "aslam_fleet_merge_maps": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _ip, _ip, _dp, _dp, _ip, _ip, _dp]),
    "aslam_merge_scratch_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]),
    "aslam_default_relocalize_params": (None, [_P(RelocalizeParams)]),
    "aslam_relocalize": (C.c_int, [C.c_void_p, C.c_int, _P(RelocalizeParams), C.c_int, C.c_void_p]),
    "aslam_fleet_relocalize": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip, _P(RelocalizeParams), C.c_int, C.c_void_p]),
    "aslam_slam_relocalize": (C.c_int, [C.c_void_p, C.c_int, _P(RelocalizeParams), C.c_int, C.c_void_p]),
    "aslam_fleet_slam_relocalize": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip, _P(RelocalizeParams), C.c_int, C.c_void_p]),
    "aslam_default_gate_params": (None, [_P(GateParams)]),
    "aslam_set_innovation_gate": (C.c_int, [C.c_void_p, _P(GateParams)]),
    "aslam_get_innovation_gate": (C.c_int, [C.c_void_p, _ip, _P(GateParams)]),
    "aslam_set_slam_gate": (C.c_int, [C.c_void_p, _P(GateParams)]),
    "aslam_get_slam_gate": (C.c_int, [C.c_void_p, _ip, _P(GateParams)]),
    "aslam_set_slam_gate_windows": (C.c_int, [C.c_void_p, C.c_int]),
    "aslam_get_slam_gate_windows": (C.c_int, [C.c_void_p, _ip]),
    "aslam_default_confirm_params": (None, [_P(ConfirmParams)]),
    "aslam_set_landmark_confirmation": (C.c_int, [C.c_void_p, _P(ConfirmParams)]),
    "aslam_get_landmark_confirmation": (C.c_int, [C.c_void_p, _ip, _P(ConfirmParams)]),
    "aslam_get_slot_confirm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "aslam_get_tentative": (C.c_int, [C.c_void_p, C.c_int, _ip, _ip, _ip, _ip]),
    "aslam_fleet_get_tentative": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip, _ip, _ip, _ip]),
    "aslam_default_pose_ambiguity_params": (None, [_P(PoseAmbiguityParams)]),
    "aslam_set_pose_ambiguity": (C.c_int, [C.c_void_p, _P(PoseAmbiguityParams)]),
    "aslam_get_pose_ambiguity": (C.c_int, [C.c_void_p, _ip, _P(PoseAmbiguityParams)]),
    "aslam_get_slot_pose_ambiguity": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip, C.c_void_p, C.c_void_p]),
    "aslam_default_obs_covariance_params": (None, [_P(ObsCovarianceParams)]),
    "aslam_set_observation_covariance": (C.c_int, [C.c_void_p, _P(ObsCovarianceParams)]),
    "aslam_get_observation_covariance": (C.c_int, [C.c_void_p, _ip, _P(ObsCovarianceParams)]),
    "aslam_get_slot_obs_covariance": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip, C.c_void_p, C.c_void_p]),
    "aslam_set_consistent_innovations": (C.c_int, [C.c_void_p, C.c_int]),
    "aslam_get_consistent_innovations": (C.c_int, [C.c_void_p, _ip]),
    "aslam_set_consistent_windows": (C.c_int, [C.c_void_p, C.c_int]),
    "aslam_get_consistent_windows": (C.c_int, [C.c_void_p, _ip]),
    "aslam_set_gated_consistent_windows": (C.c_int, [C.c_void_p, C.c_int]),
    "aslam_get_gated_consistent_windows": (C.c_int, [C.c_void_p, _ip]),
    "aslam_get_slot_health": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "aslam_get_track_health": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aslam_fleet_get_health": (C.c_int, [C.c_void_p, C.c_int, _ip, C.c_void_p]),
    "aslam_save_state": (C.c_int, [C.c_void_p, C.c_char_p]),
    "aslam_load_state": (C.c_int, [C.c_void_p, C.c_char_p]),
    "aslam_stream_open": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "aslam_stream_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_double, C.c_double]),
    "aslam_stream_acquire": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "aslam_stream_commit": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double]),
    "aslam_stream_flush": (C.c_int, [C.c_void_p]),
    "aslam_default_detector_params": (None, [C.c_void_p]),
    "aslam_set_detector_params": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aslam_set_dictionary": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "aslam_set_dictionary_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "aslam_add_encoder": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double]),
    "aslam_add_image": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int, C.c_size_t]),
    "aslam_get_state": (C.c_int, [C.c_void_p, _ip, _dp, _dp]),
    "aslam_set_state": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _ip]),
    "aslam_get_detections": (C.c_int, [C.c_void_p, _ip, _ip, _fp, _dp, _dp]),
    "aslam_get_observations": (C.c_int, [C.c_void_p, _ip, _ip, _ip, _ip, _dp, _dp]),
    "aslam_get_landmark_ids": (C.c_int, [C.c_void_p, _ip, _ip]),
    "aslam_stage_frames": (C.c_int, [C.c_void_p, C.c_int, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t]),
    "aslam_stage_encoders": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp]),
    "aslam_run_staged": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "aslam_sync": (C.c_int, [C.c_void_p]),
    "aslam_get_slot_detections": (C.c_int, [C.c_void_p, C.c_int, _ip, _ip, _fp, _dp, _dp]),
    "aslam_get_slot_raw_observations": (C.c_int, [C.c_void_p, C.c_int, _ip, _ip, _ip, _dp, _dp]),
    "aslam_get_slot_ekf_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip]),
    "aslam_set_camera_rig": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "aslam_add_images": (C.c_int, [C.c_void_p, C.c_int, _P(C.c_void_p), C.c_int, C.c_int, C.c_int, _P(C.c_size_t)]),
    "aslam_run_staged_rig": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "aslam_get_rig_observations": (C.c_int, [C.c_void_p, _ip, _ip, _ip, _ip, _ip, _dp, _dp]),
    "aslam_get_rig_step_ekf_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip]),
    "aslam_detect_batch": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t,
                                     C.c_int, _ip, _ip, _fp, _dp, _dp]),
    "aslam_export_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "aslam_comm_get_unique_id": (C.c_int, [C.c_void_p]),
    "aslam_comm_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "aslam_comm_gather_maps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "aslam_comm_destroy": (C.c_int, [C.c_void_p]),
    "aslam_debug_get_nbr": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _u8p]),
    "aslam_debug_get_frame_counts": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint)]),
    "aslam_debug_get_contours": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_longlong, _ip, _ip, _ip, _ip, _llp]),
    "aslam_debug_get_candidates": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _ip, _fp, _ip, _ip]),
    "aslam_debug_inject_observations": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip, _ip, _dp, _dp]),
    "aslam_debug_inject_candidates": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip, _ip, _fp]),
    "aslam_debug_run_pose": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip]),
    "aslam_debug_run_pose_refined": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip]),
    "aslam_debug_run_identify": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "aslam_debug_get_identified": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip, _ip, _ip, _u8p, _llp]),
    "aslam_debug_inject_contours": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip, _ip, _ip, _ip]),
    "aslam_debug_inject_quads": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip, _ip, _ip, _ip]),
    "aslam_debug_run_quads": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "aslam_debug_run_contours": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "aslam_debug_get_nodes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip, _up, _up, _up, _ip]),
    "aslam_debug_get_write_tickets": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip, _up, _up, _up, _up]),
    "aslam_debug_get_link_todo": (C.c_int, [C.c_void_p, C.c_int, _ip]),
    "aslam_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "aslam_profile_reset": (C.c_int, [C.c_void_p]),
    "aslam_get_plan_stats": (C.c_int, [C.c_void_p, _llp]),
    "aslam_get_last_timing": (C.c_int, [C.c_void_p, _dp]),
    "aslam_profile_get": (C.c_int, [C.c_void_p, C.c_int, _P(C.c_char_p), _ip, _dp]),
    "aslam_synth_render": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, C.c_int, _ip, _dp, C.c_double, C.c_int,
                                     C.c_int, C.c_uint, C.c_int, _u8p]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)
_lib = None


def lib_path():
    return os.environ.get("ARUCO_SLAM_LIB", DEFAULT_LIB)


def load():
    """Load the shared library (once).  Raises if it is missing — there is no fallback implementation."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise OSError(f"{path} not found: build it with `make -C aruco_slam_amd/csrc` (hipcc, gfx950)")
        _share_hip_runtime(path)
        lib = C.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _share_hip_runtime(path):
    """One HIP runtime per process, whatever the import order.  The library needs `libamdhip64.so.7` (found in /opt/rocm by its
    RUNPATH); a PyTorch wheel bundles its own copy under the file name `libamdhip64.so`, which torch's libraries ask for by that
    name - so with the library loaded first, a later `import torch` would map a SECOND runtime and find no devices.  If torch is
    installed but not yet imported, its copy is mapped here first: the library then binds to it by soname, and torch finds its
    own file already loaded.  (torch imported first: nothing to do, the soname is already satisfied.)"""
    if os.path.basename(path) != "libaruco_slam_hip.so" or "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is not None and spec.origin:
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)


def _ptr(a, typ):
    return a.ctypes.data_as(typ) if a is not None else None


def default_init(**over):
    init = AslamInit()
    load().aslam_default_init(C.byref(init))
    for k, v in over.items():
        if k in ("r2c_t", "r2c_q"):
            for i, x in enumerate(v):
                getattr(init, k)[i] = x
        else:
            setattr(init, k, v)
    return init


def _marker_msgs(markers):
    """marker dicts (Context.load_map_txt / map_markers) -> MarkerMsg array"""
    arr = (MarkerMsg * max(len(markers), 1))()
    for a, m in zip(arr, markers):
        a.id = int(m["id"])
        for k in range(3):
            a.scale[k] = float(m["scale"][k]) if "scale" in m else 0.0
            a.position[k] = float(m["position"][k])
        for k in range(4):
            a.orientation[k] = float(m["orientation"][k])
    return arr


def landmarks_from_markers(markers):
    """MapLoader markers (dicts with id, position, orientation (x, y, z, w)) -> (ids, xyth n x 3): heading of each marker's +z axis"""
    n = len(markers)
    arr = _marker_msgs(markers)
    ids = np.zeros(max(n, 1), np.int32)
    xyth = np.zeros((max(n, 1), 3))
    lib = load()
    rc = lib.aslam_landmarks_from_markers(n, arr, _ptr(ids, _ip), _ptr(xyth, _dp))
    if rc != ASLAM_OK:
        raise AslamError(rc, lib.aslam_last_error(None).decode())
    return ids[:n].copy(), xyth[:n].copy()


def load_map_txt(path):
    """aslam_load_map_txt without a context: the marker dicts of a MapLoader map file"""
    lib = load()
    n = C.c_int(0)
    rc = lib.aslam_load_map_txt(None, str(path).encode(), 0, C.byref(n), None)
    if rc != ASLAM_OK:
        raise AslamError(rc, f"cannot read {path}")
    arr = (MarkerMsg * max(n.value, 1))()
    rc = lib.aslam_load_map_txt(None, str(path).encode(), n.value, C.byref(n), arr)
    if rc != ASLAM_OK:
        raise AslamError(rc, f"cannot read {path}")
    return [dict(id=a.id, scale=tuple(a.scale), color=tuple(a.color), position=np.array(a.position), orientation=np.array(a.orientation),
                 lifetime=a.lifetime_sec) for a in arr[:n.value]]


def known_map_from_txt(path):
    """a MapLoader map file -> (ids, xyth n x 3), the arguments of Context.localize_begin"""
    return landmarks_from_markers(load_map_txt(path))


class Context:
    """One filter fed by one camera stream (set_camera) or by a camera rig (set_camera_rig): thin RAII wrapper over aslam_ctx
    (mirrors the `ArucoSlam` class surface)."""

    def __init__(self, init=None, **over):
        self.lib = load()
        self.init = init if init is not None else default_init(**over)
        h = C.c_void_p()
        rc = self.lib.aslam_create(C.byref(self.init), C.byref(h))
        if rc != ASLAM_OK:
            raise AslamError(rc, "aslam_create failed (no usable HIP device, bad init, or out of memory)")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.aslam_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != ASLAM_OK:
            raise AslamError(rc, self.lib.aslam_last_error(self.h).decode())

    # -- reference class surface ---------------------------------------------------------------
    def set_camera(self, K, D=None):
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        D = np.zeros(0) if D is None else np.ascontiguousarray(D, dtype=np.float64).reshape(-1)
        self._ck(self.lib.aslam_set_camera(self.h, _ptr(K, _dp), _ptr(D, _dp) if D.size else None, int(D.size)))

    # -- what the node publishes / persistence --------------------------------------------------
    def pose_msg(self):
        m = PoseMsg()
        self._ck(self.lib.aslam_get_pose_msg(self.h, C.byref(m)))
        return np.array(m.position), np.array(m.orientation), np.array(m.covariance).reshape(6, 6)

    def _markers(self, fn):
        n = C.c_int(0)
        self._ck(fn(self.h, 0, C.byref(n), None))
        arr = (MarkerMsg * max(n.value, 1))()
        self._ck(fn(self.h, n.value, C.byref(n), arr))
        return [dict(id=a.id, scale=tuple(a.scale), color=tuple(a.color), position=np.array(a.position), orientation=np.array(a.orientation),
                     lifetime=a.lifetime_sec) for a in arr[:n.value]]

    def map_markers(self):
        return self._markers(self.lib.aslam_get_map_markers)

    def detected_markers(self):
        return self._markers(self.lib.aslam_get_detected_markers)

    def draw_detected_markers(self, bgr):
        """markered_img_ of getObservations (aruco_slam.cpp:318-319): returns a copy of the bgr8 frame with the last detections drawn"""
        out = np.ascontiguousarray(bgr, dtype=np.uint8).copy()
        assert out.ndim == 3 and out.shape[2] == 3
        self._ck(self.lib.aslam_draw_detected_markers(self.h, out.ctypes.data_as(C.c_void_p), out.shape[0], out.shape[1], out.strides[0]))
        return out

    def export_map_async(self, device_ptr, buffer):
        self._ck(self.lib.aslam_export_map_async(self.h, C.c_void_p(int(device_ptr)), int(buffer)))

    def export_wait(self, buffer):
        self._ck(self.lib.aslam_export_wait(self.h, int(buffer)))

    def load_map_txt(self, path):
        n = C.c_int(0)
        self._ck(self.lib.aslam_load_map_txt(self.h, str(path).encode(), 0, C.byref(n), None))
        arr = (MarkerMsg * max(n.value, 1))()
        self._ck(self.lib.aslam_load_map_txt(self.h, str(path).encode(), n.value, C.byref(n), arr))
        return [dict(id=a.id, scale=tuple(a.scale), color=tuple(a.color), position=np.array(a.position), orientation=np.array(a.orientation),
                     lifetime=a.lifetime_sec) for a in arr[:n.value]]

    # -- localization against a fixed, known marker map (include/aruco_slam_hip.h) ----------
    def localize_begin(self, ids, xyth, pose, pose_sigma):
        """freeze the map (ids, xyth: n x 3) and track the pose from `pose` with covariance `pose_sigma` (3 x 3)"""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        xyth = np.ascontiguousarray(xyth, dtype=np.float64).reshape(-1, 3)
        if xyth.shape[0] != ids.size:
            raise ValueError("one (x, y, theta) row per landmark id")
        pose = np.ascontiguousarray(pose, dtype=np.float64).reshape(3)
        ps = np.ascontiguousarray(pose_sigma, dtype=np.float64).reshape(9)
        self._ck(self.lib.aslam_localize_begin(self.h, int(ids.size), _ptr(ids, _ip), _ptr(xyth, _dp), _ptr(pose, _dp), _ptr(ps, _dp)))
    def localize_end(self):
        self._ck(self.lib.aslam_localize_end(self.h))
    def is_localizing(self):
        on = C.c_int(0)
        self._ck(self.lib.aslam_is_localizing(self.h, C.byref(on)))
        return bool(on.value)
    # -- localization on an uncertain map: Schmidt-Kalman steps (include/aruco_slam_hip.h) ----------------
    def localize_begin_uncertain(self, ids, xyth, map_sigmas, pose, pose_sigma):
        """localize_begin with one 3 x 3 covariance per landmark (n x 3 x 3 or n x 9, as a map merge returns them)"""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        xyth = np.ascontiguousarray(xyth, dtype=np.float64).reshape(-1, 3)
        ms = np.ascontiguousarray(map_sigmas, dtype=np.float64).reshape(-1, 9)
        if xyth.shape[0] != ids.size or ms.shape[0] != ids.size:
            raise ValueError("one (x, y, theta) row and one covariance per landmark id")
        pose = np.ascontiguousarray(pose, dtype=np.float64).reshape(3)
        ps = np.ascontiguousarray(pose_sigma, dtype=np.float64).reshape(9)
        self._ck(self.lib.aslam_localize_begin_uncertain(self.h, int(ids.size), _ptr(ids, _ip), _ptr(xyth, _dp), _ptr(ms, _dp),
                                                         _ptr(pose, _dp), _ptr(ps, _dp)))
    def fleet_begin_uncertain(self, cams, ids, xyth, map_sigmas, poses, pose_sigmas):
        """fleet_begin with one shared table of landmark covariances (n x 3 x 3 or n x 9)"""
        cams = [c if isinstance(c, Camera) else Camera.make(*c) for c in cams]
        arr = (Camera * max(len(cams), 1))(*cams)
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        xyth = np.ascontiguousarray(xyth, dtype=np.float64).reshape(-1, 3)
        ms = np.ascontiguousarray(map_sigmas, dtype=np.float64).reshape(-1, 9)
        if xyth.shape[0] != ids.size or ms.shape[0] != ids.size:
            raise ValueError("one (x, y, theta) row and one covariance per landmark id")
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        sig = np.ascontiguousarray(pose_sigmas, dtype=np.float64).reshape(-1, 9)
        self._ck(self.lib.aslam_fleet_begin_uncertain(self.h, len(cams), arr, int(ids.size), _ptr(ids, _ip), _ptr(xyth, _dp), _ptr(ms, _dp),
                                                      _ptr(poses, _dp), _ptr(sig, _dp)))
    def is_map_uncertain(self):
        on = C.c_int(0)
        self._ck(self.lib.aslam_is_map_uncertain(self.h, C.byref(on)))
        return bool(on.value)
    def fleet_get_cross(self, robot):
        """robot's Sigma_xl, 3 x 3L"""
        L = C.c_int()
        self._ck(self.lib.aslam_fleet_get_cross(self.h, int(robot), C.byref(L), None))
        cross = np.zeros((3, 3 * L.value))
        self._ck(self.lib.aslam_fleet_get_cross(self.h, int(robot), C.byref(L), _ptr(cross, _dp)))
        return cross
    # -- fleet localization: many robots, one camera each, on one frozen map ----------------------------
    def fleet_begin(self, cams, ids, xyth, poses, pose_sigmas):
        """cams: one Camera (or (K, D, mount) tuple) per robot; poses R x 3, pose_sigmas R x 3 x 3; map as localize_begin"""
        cams = [c if isinstance(c, Camera) else Camera.make(*c) for c in cams]
        arr = (Camera * max(len(cams), 1))(*cams)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        xyth = np.ascontiguousarray(xyth, dtype=np.float64).reshape(-1, 3)
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        sig = np.ascontiguousarray(pose_sigmas, dtype=np.float64).reshape(-1, 9)
        self._ck(self.lib.aslam_fleet_begin(self.h, len(cams), arr, int(ids.size), _ptr(ids, _ip), _ptr(xyth, _dp), _ptr(poses, _dp),
                                            _ptr(sig, _dp)))

    def fleet_add_images(self, robots, imgs, wl, wr, dt):
        """one synchronous call: imgs[i] (all of one size) is robot robots[i]'s frame, after its encoder sample (wl[i], wr[i], dt[i])"""
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in imgs]
        if any(im.shape != imgs[0].shape for im in imgs):
            raise ValueError("the images of a fleet call must all have the same size and channels")
        rows, cols = imgs[0].shape[:2]
        ch = 1 if imgs[0].ndim == 2 else imgs[0].shape[2]
        robots = np.ascontiguousarray(robots, dtype=np.int32)
        wl, wr, dt = (np.ascontiguousarray(v, dtype=np.float64) for v in (wl, wr, dt))
        ptrs = (C.c_void_p * len(imgs))(*[im.ctypes.data for im in imgs])
        steps = (C.c_size_t * len(imgs))(*[im.strides[0] for im in imgs])
        self._ck(self.lib.aslam_fleet_add_images(self.h, len(imgs), _ptr(robots, _ip), _ptr(wl, _dp), _ptr(wr, _dp), _ptr(dt, _dp), ptrs,
                                                 rows, cols, ch, steps))

    def fleet_run_staged(self, first, robot_of_slot, with_ekf=True):
        """staged slots first .. first + len(robot_of_slot) - 1; slot first + i is robot robot_of_slot[i]'s frame"""
        rs = np.ascontiguousarray(robot_of_slot, dtype=np.int32)
        self._ck(self.lib.aslam_fleet_run_staged(self.h, int(first), int(rs.size), _ptr(rs, _ip), int(with_ekf)))

    def fleet_get_poses(self):
        """(R x 3 poses, R x 3 x 3 Sigma_xx)"""
        n = C.c_int()
        self._ck(self.lib.aslam_fleet_get_poses(self.h, 0, C.byref(n), None, None))
        R = n.value
        poses = np.zeros((R, 3)); sig = np.zeros((R, 3, 3))
        self._ck(self.lib.aslam_fleet_get_poses(self.h, R, C.byref(n), _ptr(poses, _dp), _ptr(sig, _dp)))
        return poses, sig

    def fleet_set_pose(self, robot, pose, sigma):
        pose = np.ascontiguousarray(pose, dtype=np.float64).reshape(3)
        sig = np.ascontiguousarray(sigma, dtype=np.float64).reshape(9)
        self._ck(self.lib.aslam_fleet_set_pose(self.h, int(robot), _ptr(pose, _dp), _ptr(sig, _dp)))

    def fleet_end(self):
        self._ck(self.lib.aslam_fleet_end(self.h))

    def is_fleet(self):
        """robots of the active fleet, 0 outside fleet mode"""
        n = C.c_int()
        self._ck(self.lib.aslam_is_fleet(self.h, C.byref(n)))
        return n.value

    # -- fleet SLAM: many robots, one camera and one SLAM filter each -------------------------------------------
    def fleet_slam_begin(self, cams):
        """cams: one Camera (or (K, D, mount) tuple) per robot; every robot starts with an empty map, disarmed"""
        cams = [c if isinstance(c, Camera) else Camera.make(*c) for c in cams]
        arr = (Camera * max(len(cams), 1))(*cams)
        self._ck(self.lib.aslam_fleet_slam_begin(self.h, len(cams), arr))

    def is_fleet_slam(self):
        on = C.c_int()
        self._ck(self.lib.aslam_is_fleet_slam(self.h, C.byref(on)))
        return bool(on.value)

    def fleet_get_state(self, robot):
        """robot's (mu, Sigma), as get_state"""
        n = C.c_int()
        self._ck(self.lib.aslam_fleet_get_state(self.h, int(robot), C.byref(n), None, None))
        N = n.value
        mu = np.zeros(N)
        sigma = np.zeros((N, N), order="F")
        self._ck(self.lib.aslam_fleet_get_state(self.h, int(robot), C.byref(n), _ptr(mu, _dp), _ptr(sigma, _dp)))
        return mu, np.array(sigma)

    def fleet_set_state(self, robot, mu, sigma, landmark_ids):
        mu = np.ascontiguousarray(mu, dtype=np.float64)
        sig = np.asfortranarray(sigma, dtype=np.float64)
        ids = np.ascontiguousarray(landmark_ids, dtype=np.int32)
        self._ck(self.lib.aslam_fleet_set_state(self.h, int(robot), int(mu.size), _ptr(mu, _dp), _ptr(sig, _dp),
                                                _ptr(ids, _ip) if ids.size else None))

    def fleet_get_landmark_ids(self, robot):
        n = C.c_int()
        ids = np.zeros(max(int(self.init.max_landmarks), 1), np.int32)
        self._ck(self.lib.aslam_fleet_get_landmark_ids(self.h, int(robot), C.byref(n), _ptr(ids, _ip)))
        return ids[: n.value].copy()

    # -- landmark removal: marginalise landmarks out of a SLAM map on the device ---------------------------------
    def remove_landmarks(self, ids):
        """remove every landmark whose marker id is in ids from the SLAM map (mu, Sigma, id tables, last-observed list), in place
        on the device; returns the number of landmarks removed"""
        ids = np.ascontiguousarray(ids, dtype=np.int32).ravel()
        removed = C.c_int()
        self._ck(self.lib.aslam_remove_landmarks(self.h, int(ids.size), _ptr(ids, _ip) if ids.size else None, C.byref(removed)))
        return removed.value

    def fleet_remove_landmarks(self, ids, robots=None):
        """remove_landmarks on the listed robots of the active SLAM fleet (None: every robot) in one call; returns the number of
        landmarks removed per listed robot, in list order"""
        ids = np.ascontiguousarray(ids, dtype=np.int32).ravel()
        if robots is None:
            n_robots, rp = max(self.is_fleet(), 0), None
        else:
            robots = np.ascontiguousarray(robots, dtype=np.int32).ravel()
            n_robots, rp = int(robots.size), _ptr(robots, _ip) if robots.size else _ptr(np.zeros(1, np.int32), _ip)
        removed = np.zeros(max(n_robots, 1), np.int32)
        self._ck(self.lib.aslam_fleet_remove_landmarks(self.h, int(ids.size), _ptr(ids, _ip) if ids.size else None, n_robots, rp,
                                                       _ptr(removed, _ip)))
        return removed[:n_robots].copy()

    # -- map merge: one shared map from N maps in N frames -----------------------------------------------------
    def _merged(self, call, n_maps):
        """run call(max, n, ids, xyth, sigmas, n_seen, rounds, T) -> (ids, xyth n x 3, sigmas n x 3 x 3, n_seen, rounds, T n_maps x 3)"""
        n = C.c_int()
        ids = np.zeros(ID_TABLE_SIZE, np.int32); seen = np.zeros(ID_TABLE_SIZE, np.int32)
        xyth = np.zeros((ID_TABLE_SIZE, 3)); sig = np.zeros((ID_TABLE_SIZE, 3, 3))
        rounds = np.zeros(n_maps, np.int32); T = np.zeros((n_maps, 3))
        self._ck(call(ID_TABLE_SIZE, C.byref(n), _ptr(ids, _ip), _ptr(xyth, _dp), _ptr(sig, _dp), _ptr(seen, _ip), _ptr(rounds, _ip), _ptr(T, _dp)))
        k = n.value
        return ids[:k].copy(), xyth[:k].copy(), sig[:k].copy(), seen[:k].copy(), rounds, T

    def merge_map_records(self, records, n_maps, per_map, anchor=0, min_common=2, on_device=False):
        """align n_maps maps of per_map 104-byte records each into map `anchor`'s frame and fuse them per marker id.  records: a numpy
        array holding the records (e.g. of dist.MAP_DTYPE), or with on_device=True the address of a device buffer"""
        if on_device:
            ptr = C.c_void_p(int(records))
        else:
            records = np.ascontiguousarray(records)
            if records.nbytes != int(n_maps) * int(per_map) * MAP_RECORD_BYTES:
                raise ValueError("records must hold n_maps x per_map records of MAP_RECORD_BYTES bytes")
            ptr = records.ctypes.data_as(C.c_void_p)
        return self._merged(lambda *out: self.lib.aslam_merge_map_records(self.h, ptr, 1 if on_device else 0, int(n_maps), int(per_map),
                                                                          int(anchor), int(min_common), *out), int(n_maps))

    def fleet_merge_maps(self, anchor=0, min_common=2):
        """merge_map_records on the maps of the active SLAM fleet's robots (map r = robot r)"""
        return self._merged(lambda *out: self.lib.aslam_fleet_merge_maps(self.h, int(anchor), int(min_common), *out), max(self.is_fleet(), 1))

    def merge_scratch_bytes(self):
        """device memory the merge calls hold at present (0 before the first merge and after fleet_end)"""
        b = C.c_longlong()
        self._ck(self.lib.aslam_merge_scratch_bytes(self.h, C.byref(b)))
        return b.value

    # -- relocalization: lost poses from one frame against the frozen map ---------------------------------------
    def _reloc_params(self, params):
        """None when no parameter is given (the library's defaults), else the defaults with the given fields replaced"""
        if not params:
            return None
        p = RelocalizeParams()
        self.lib.aslam_default_relocalize_params(C.byref(p))
        for k, v in params.items():
            if k not in ("tol_xy", "tol_th", "min_inliers"):
                raise KeyError(k)
            setattr(p, k, v)
        return C.byref(p)

    def relocalize(self, slot, apply=True, **params):
        """the localizing filter's pose from slot's observation list; params: tol_xy, tol_th, min_inliers.  A RELOC_DTYPE record"""
        out = np.zeros(1, RELOC_DTYPE)
        self._ck(self.lib.aslam_relocalize(self.h, int(slot), self._reloc_params(params), 1 if apply else 0, out.ctypes.data_as(C.c_void_p)))
        return out[0]

    def fleet_relocalize(self, first, robots, apply=True, **params):
        """slot first + i is robot robots[i]'s frame; one RELOC_DTYPE record per slot"""
        rs = np.ascontiguousarray(robots, dtype=np.int32).reshape(-1)
        out = np.zeros(max(rs.size, 1), RELOC_DTYPE)
        self._ck(self.lib.aslam_fleet_relocalize(self.h, int(first), int(rs.size), _ptr(rs, _ip), self._reloc_params(params), 1 if apply else 0,
                                                 out.ctypes.data_as(C.c_void_p)))
        return out[:rs.size]

    def slam_relocalize(self, slot, apply=True, **params):
        """the SLAM (or rig SLAM) filter's pose from slot's observation list against its own map; with apply a solved
        slot seats pose, Sigma_xx and the pose <-> landmark strip.  A RELOC_DTYPE record"""
        out = np.zeros(1, RELOC_DTYPE)
        self._ck(self.lib.aslam_slam_relocalize(self.h, int(slot), self._reloc_params(params), 1 if apply else 0, out.ctypes.data_as(C.c_void_p)))
        return out[0]

    def fleet_slam_relocalize(self, first, robots, apply=True, **params):
        """fleet SLAM: slot first + i is robot robots[i]'s frame, solved against that robot's own map; one RELOC_DTYPE record per slot"""
        rs = np.ascontiguousarray(robots, dtype=np.int32).reshape(-1)
        out = np.zeros(max(rs.size, 1), RELOC_DTYPE)
        self._ck(self.lib.aslam_fleet_slam_relocalize(self.h, int(first), int(rs.size), _ptr(rs, _ip), self._reloc_params(params),
                                                      1 if apply else 0, out.ctypes.data_as(C.c_void_p)))
        return out[:rs.size]

    # -- innovation gate and lost-track detection ---------------------------------------------------------------
    def set_innovation_gate(self, params=True, **kw):
        """set_innovation_gate(gate_d2=..., min_attempted=..., min_accept_percent=..., lost_after=...): the library's defaults with the
        given fields replaced (gate_d2=inf: monitor only); set_innovation_gate(None): off"""
        if params is None:
            if kw:
                raise ValueError("set_innovation_gate(None) takes no parameters")
            self._ck(self.lib.aslam_set_innovation_gate(self.h, None))
            return
        p = GateParams()
        self.lib.aslam_default_gate_params(C.byref(p))
        for k, v in kw.items():
            if k not in ("gate_d2", "min_attempted", "min_accept_percent", "lost_after"):
                raise KeyError(k)
            setattr(p, k, v)
        self._ck(self.lib.aslam_set_innovation_gate(self.h, C.byref(p)))

    def get_innovation_gate(self):
        """None while the gate is off, else its parameters as a dict"""
        on, p = C.c_int(), GateParams()
        self._ck(self.lib.aslam_get_innovation_gate(self.h, C.byref(on), C.byref(p)))
        if not on.value:
            return None
        return dict(gate_d2=p.gate_d2, min_attempted=p.min_attempted, min_accept_percent=p.min_accept_percent, lost_after=p.lost_after)

    # -- innovation gate of the SLAM chains ----------------------------------------------------------------------
    def set_slam_gate(self, params=True, **kw):
        """set_slam_gate(gate_d2=..., min_attempted=..., min_accept_percent=..., lost_after=...): the library's defaults with the given
        fields replaced (gate_d2=inf: monitor only); set_slam_gate(None): off"""
        if params is None:
            if kw:
                raise ValueError("set_slam_gate(None) takes no parameters")
            self._ck(self.lib.aslam_set_slam_gate(self.h, None))
            return
        p = GateParams()
        self.lib.aslam_default_gate_params(C.byref(p))
        for k, v in kw.items():
            if k not in ("gate_d2", "min_attempted", "min_accept_percent", "lost_after"):
                raise KeyError(k)
            setattr(p, k, v)
        self._ck(self.lib.aslam_set_slam_gate(self.h, C.byref(p)))

    def get_slam_gate(self):
        """None while the SLAM gate is off, else its parameters as a dict"""
        on, p = C.c_int(), GateParams()
        self._ck(self.lib.aslam_get_slam_gate(self.h, C.byref(on), C.byref(p)))
        if not on.value:
            return None
        return dict(gate_d2=p.gate_d2, min_attempted=p.min_attempted, min_accept_percent=p.min_accept_percent, lost_after=p.lost_after)

    # -- the SLAM gate inside EKF windows -------------------------------------------------------------------------
    def set_slam_gate_windows(self, on=True):
        """keep the EKF windows of staged batches while the SLAM gate is set (off by default)"""
        self._ck(self.lib.aslam_set_slam_gate_windows(self.h, 1 if on else 0))

    def get_slam_gate_windows(self):
        on = C.c_int()
        self._ck(self.lib.aslam_get_slam_gate_windows(self.h, C.byref(on)))
        return bool(on.value)

    # -- landmark confirmation -------------------------------------------------------------------------------------
    def set_landmark_confirmation(self, params=True, **kw):
        """set_landmark_confirmation(min_sightings=..., max_gap=...): the library's defaults with the given fields replaced;
        set_landmark_confirmation(None): off"""
        if params is None:
            if kw:
                raise ValueError("set_landmark_confirmation(None) takes no parameters")
            self._ck(self.lib.aslam_set_landmark_confirmation(self.h, None))
            return
        p = ConfirmParams()
        self.lib.aslam_default_confirm_params(C.byref(p))
        for k, v in kw.items():
            if k not in ("min_sightings", "max_gap"):
                raise KeyError(k)
            setattr(p, k, int(v))
        self._ck(self.lib.aslam_set_landmark_confirmation(self.h, C.byref(p)))

    def get_landmark_confirmation(self):
        """None while landmark confirmation is off, else its parameters as a dict"""
        on, p = C.c_int(), ConfirmParams()
        self._ck(self.lib.aslam_get_landmark_confirmation(self.h, C.byref(on), C.byref(p)))
        if not on.value:
            return None
        return dict(min_sightings=p.min_sightings, max_gap=p.max_gap)

    def get_slot_confirm(self, first, count):
        """one SLOT_CONFIRM_DTYPE record per EKF slot first .. first + count - 1"""
        out = np.zeros(max(int(count), 1), SLOT_CONFIRM_DTYPE)
        self._ck(self.lib.aslam_get_slot_confirm(self.h, int(first), int(count), out.ctypes.data_as(C.c_void_p)))
        return out[:max(int(count), 0)]

    def _tentative(self, call):
        ids, counts, ages = (np.zeros(1024, np.int32) for _ in range(3))
        n = C.c_int()
        self._ck(call(1024, C.byref(n), _ptr(ids, _ip), _ptr(counts, _ip), _ptr(ages, _ip)))
        return ids[:n.value].copy(), counts[:n.value].copy(), ages[:n.value].copy()

    def get_tentative(self):
        """(ids, counts, ages) of the single SLAM filter's tentative ids, ascending by id"""
        return self._tentative(lambda *a: self.lib.aslam_get_tentative(self.h, *a))

    def fleet_get_tentative(self, robot):
        """(ids, counts, ages) of robot's tentative ids in a SLAM fleet, ascending by id"""
        return self._tentative(lambda *a: self.lib.aslam_fleet_get_tentative(self.h, int(robot), *a))

    # -- pose ambiguity check ---------------------------------------------------------------------------------------
    def set_pose_ambiguity(self, params=True, **kw):
        """set_pose_ambiguity(ratio=..., floor_px=..., min_dtheta=..., reject=...): the library's defaults with the given fields
        replaced; set_pose_ambiguity(None): off"""
        if params is None:
            if kw:
                raise ValueError("set_pose_ambiguity(None) takes no parameters")
            self._ck(self.lib.aslam_set_pose_ambiguity(self.h, None))
            return
        p = PoseAmbiguityParams()
        self.lib.aslam_default_pose_ambiguity_params(C.byref(p))
        for k, v in kw.items():
            if k not in ("ratio", "floor_px", "min_dtheta", "reject"):
                raise KeyError(k)
            setattr(p, k, int(v) if k == "reject" else float(v))
        self._ck(self.lib.aslam_set_pose_ambiguity(self.h, C.byref(p)))

    def get_pose_ambiguity(self):
        """None while the pose ambiguity check is off, else its parameters as a dict"""
        on, p = C.c_int(), PoseAmbiguityParams()
        self._ck(self.lib.aslam_get_pose_ambiguity(self.h, C.byref(on), C.byref(p)))
        if not on.value:
            return None
        return dict(ratio=p.ratio, floor_px=p.floor_px, min_dtheta=p.min_dtheta, reject=p.reject)

    def get_slot_pose_ambiguity(self, slot):
        """(records, sum) of a frame slot's last checked pose stage: one POSE_AMBIGUITY_DTYPE record per marker of its list and the
        slot's SLOT_POSE_AMBIGUITY_DTYPE sum"""
        out = np.zeros(MARKER_MAX, POSE_AMBIGUITY_DTYPE)
        s = np.zeros(1, SLOT_POSE_AMBIGUITY_DTYPE)
        n = C.c_int()
        self._ck(self.lib.aslam_get_slot_pose_ambiguity(self.h, int(slot), MARKER_MAX, C.byref(n), out.ctypes.data_as(C.c_void_p),
                                                        s.ctypes.data_as(C.c_void_p)))
        return out[:n.value].copy(), s[0].copy()

    # -- observation covariance -------------------------------------------------------------------------------------
    _OBS_COV_FIELDS = ("sigma_px", "scale", "floor_xy", "floor_th", "gate_norm", "use_residual")

    def set_observation_covariance(self, params=True, **kw):
        """set_observation_covariance(sigma_px=..., scale=..., floor_xy=..., floor_th=..., gate_norm=..., use_residual=...): the
        library's defaults with the given fields replaced; set_observation_covariance(None): off"""
        if params is None:
            if kw:
                raise ValueError("set_observation_covariance(None) takes no parameters")
            self._ck(self.lib.aslam_set_observation_covariance(self.h, None))
            return
        p = ObsCovarianceParams()
        self.lib.aslam_default_obs_covariance_params(C.byref(p))
        for k, v in kw.items():
            if k not in self._OBS_COV_FIELDS:
                raise KeyError(k)
            setattr(p, k, int(v) if k == "use_residual" else float(v))
        self._ck(self.lib.aslam_set_observation_covariance(self.h, C.byref(p)))

    def get_observation_covariance(self):
        """None while the observation covariance is off, else its parameters as a dict"""
        on, p = C.c_int(), ObsCovarianceParams()
        self._ck(self.lib.aslam_get_observation_covariance(self.h, C.byref(on), C.byref(p)))
        if not on.value:
            return None
        return {k: getattr(p, k) for k in self._OBS_COV_FIELDS}

    def get_slot_obs_covariance(self, slot):
        """(records, sum) of a frame slot's last pose stage under the switch: one OBS_COVARIANCE_DTYPE record per marker of its list
        and the slot's SLOT_OBS_COVARIANCE_DTYPE sum"""
        out = np.zeros(MARKER_MAX, OBS_COVARIANCE_DTYPE)
        s = np.zeros(1, SLOT_OBS_COVARIANCE_DTYPE)
        n = C.c_int()
        self._ck(self.lib.aslam_get_slot_obs_covariance(self.h, int(slot), MARKER_MAX, C.byref(n), out.ctypes.data_as(C.c_void_p),
                                                        s.ctypes.data_as(C.c_void_p)))
        return out[:n.value].copy(), s[0].copy()

    # -- consistent innovations ---------------------------------------------------------------------------------------
    def set_consistent_innovations(self, on=True):
        """every correction of a frame is formed at the mean the previous one left (e_i = ze_i - H_i (mu_{i-1} - mu_0)); off: the
        reference's frozen-mean innovations.  While it is on no EKF window is planned unless set_consistent_windows is on too."""
        self._ck(self.lib.aslam_set_consistent_innovations(self.h, int(bool(on))))

    def get_consistent_innovations(self):
        on = C.c_int()
        self._ck(self.lib.aslam_get_consistent_innovations(self.h, C.byref(on)))
        return bool(on.value)

    # -- consistent innovations inside EKF windows ------------------------------------------------------------------
    def set_consistent_windows(self, on=True):
        """while consistent innovations are on, plan EKF windows again: the window chain corrects its mean with the running
        innovation.  Off by default; changes nothing while consistent innovations are off."""
        self._ck(self.lib.aslam_set_consistent_windows(self.h, int(bool(on))))

    def get_consistent_windows(self):
        on = C.c_int()
        self._ck(self.lib.aslam_get_consistent_windows(self.h, C.byref(on)))
        return bool(on.value)

    # -- the SLAM gate on the running innovation inside EKF windows ---------------------------------------------------
    def set_gated_consistent_windows(self, on=True):
        """with a SLAM gate, consistent innovations, set_slam_gate_windows and set_consistent_windows all on, plan EKF windows again:
        the gated window chain judges and applies the running innovation.  Off by default; changes nothing in any other combination.
        `on` goes to the library as it is: anything but 0 / 1 (False / True) is refused."""
        self._ck(self.lib.aslam_set_gated_consistent_windows(self.h, int(on)))

    def get_gated_consistent_windows(self):
        on = C.c_int()
        self._ck(self.lib.aslam_get_gated_consistent_windows(self.h, C.byref(on)))
        return bool(on.value)

    def get_slot_health(self, first, count):
        """one SLOT_HEALTH_DTYPE record per EKF slot first .. first + count - 1"""
        out = np.zeros(max(int(count), 1), SLOT_HEALTH_DTYPE)
        self._ck(self.lib.aslam_get_slot_health(self.h, int(first), int(count), out.ctypes.data_as(C.c_void_p)))
        return out[:max(int(count), 0)]

    def get_track_health(self):
        """the single filter's TRACK_HEALTH_DTYPE record (localizing: the innovation gate's; SLAM, rig SLAM: the SLAM gate's)"""
        out = np.zeros(1, TRACK_HEALTH_DTYPE)
        self._ck(self.lib.aslam_get_track_health(self.h, out.ctypes.data_as(C.c_void_p)))
        return out[0]

    def fleet_get_health(self):
        """one TRACK_HEALTH_DTYPE record per robot of the fleet (localization fleet: the innovation gate's; SLAM fleet: the SLAM gate's)"""
        n = C.c_int()
        out = np.zeros(MAX_ROBOTS, TRACK_HEALTH_DTYPE)
        self._ck(self.lib.aslam_fleet_get_health(self.h, MAX_ROBOTS, C.byref(n), out.ctypes.data_as(C.c_void_p)))
        return out[:n.value].copy()

    def save_state(self, path):
        self._ck(self.lib.aslam_save_state(self.h, str(path).encode()))

    def load_state(self, path):
        self._ck(self.lib.aslam_load_state(self.h, str(path).encode()))

    # -- host-fed stream (pinned ring, asynchronous upload) -------------------------------------
    def stream_open(self, rows, cols, channels, frames_per_submit):
        self._ck(self.lib.aslam_stream_open(self.h, int(rows), int(cols), int(channels), int(frames_per_submit)))

    def stream_push(self, img, wl, wr, dt):
        """one frame, gray (rows, cols) or bgr8 (rows, cols, 3); rows may be padded (a view into a wider array): the array goes
        through as it is, with its strides[0], when each row is contiguous in itself, and is copied only otherwise"""
        img = np.asarray(img)
        row = img.shape[1] * (img.shape[2] if img.ndim == 3 else 1) if img.ndim in (2, 3) else -1
        if (img.dtype != np.uint8 or row < 0 or img.strides[1:] != ((1,) if img.ndim == 2 else (img.shape[2], 1))
                or (img.shape[0] > 1 and img.strides[0] < row)):
            img = np.ascontiguousarray(img, dtype=np.uint8)
        self._ck(self.lib.aslam_stream_push(self.h, img.ctypes.data_as(C.c_void_p), img.strides[0], float(wl), float(wr), float(dt)))

    def stream_slot(self, rows, cols, channels=1):
        """numpy view of the next pinned slot (fill it, then stream_commit)"""
        p, st = C.c_void_p(), C.c_size_t()
        self._ck(self.lib.aslam_stream_acquire(self.h, C.byref(p), C.byref(st)))
        buf = (C.c_uint8 * (rows * st.value)).from_address(p.value)
        a = np.frombuffer(buf, np.uint8).reshape(rows, st.value)
        return a[:, :cols * channels].reshape((rows, cols) if channels == 1 else (rows, cols, channels))

    def stream_commit(self, wl, wr, dt):
        self._ck(self.lib.aslam_stream_commit(self.h, float(wl), float(wr), float(dt)))

    def stream_flush(self):
        self._ck(self.lib.aslam_stream_flush(self.h))

    def set_detector_params(self, **kw):
        """cv::aruco::DetectorParameters fields by name; anything not given keeps its OpenCV 3.2.0 default"""
        p = DetectorParams()
        self.lib.aslam_default_detector_params(C.byref(p))
        for k, v in kw.items():
            if not hasattr(p, k):
                raise KeyError(k)
            setattr(p, k, v)
        self._ck(self.lib.aslam_set_detector_params(self.h, C.byref(p)))

    def set_dictionary(self, bits, max_correction_bits=0):
        """bits: n x ms x ms (1 = white); replaces the built-in DICT_ARUCO_ORIGINAL"""
        b = np.ascontiguousarray(bits, dtype=np.uint8)
        self._ck(self.lib.aslam_set_dictionary(self.h, int(b.shape[1]), int(b.shape[0]), int(max_correction_bits), b.ctypes.data_as(C.c_void_p)))

    def set_dictionary_bytes(self, bytes_list, marker_size, max_correction_bits=0):
        """bytes_list: cv::aruco::Dictionary::bytesList as an n x nbytes x 4 uint8 array"""
        b = np.ascontiguousarray(bytes_list, dtype=np.uint8)
        self._ck(self.lib.aslam_set_dictionary_bytes(self.h, int(marker_size), int(b.shape[0]), int(max_correction_bits), b.ctypes.data_as(C.c_void_p)))

    def add_encoder(self, wl, wr, t_now):
        self._ck(self.lib.aslam_add_encoder(self.h, float(wl), float(wr), float(t_now)))

    def add_image(self, img):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        rows, cols = img.shape[:2]
        ch = 1 if img.ndim == 2 else img.shape[2]
        self._ck(self.lib.aslam_add_image(self.h, _ptr(img, _u8p), rows, cols, ch, cols * ch))

    def get_state(self):
        n = C.c_int()
        self._ck(self.lib.aslam_get_state(self.h, C.byref(n), None, None))
        N = n.value
        mu = np.zeros(N)
        sigma = np.zeros((N, N), order="F")
        self._ck(self.lib.aslam_get_state(self.h, C.byref(n), _ptr(mu, _dp), _ptr(sigma, _dp)))
        return mu, np.array(sigma)

    def set_state(self, mu, sigma, landmark_ids):
        mu = np.ascontiguousarray(mu, dtype=np.float64)
        sig = np.asfortranarray(sigma, dtype=np.float64)
        ids = np.ascontiguousarray(landmark_ids, dtype=np.int32)
        self._ck(self.lib.aslam_set_state(self.h, int(mu.size), _ptr(mu, _dp), _ptr(sig, _dp), _ptr(ids, _ip) if ids.size else None))

    def _detections(self, fn, *pre):
        m = C.c_int()
        ids = np.zeros(MARKER_MAX, np.int32)
        corners = np.zeros((MARKER_MAX, 4, 2), np.float32)
        rv = np.zeros((MARKER_MAX, 3))
        tv = np.zeros((MARKER_MAX, 3))
        self._ck(fn(self.h, *pre, C.byref(m), _ptr(ids, _ip), _ptr(corners, _fp), _ptr(rv, _dp), _ptr(tv, _dp)))
        M = m.value
        return ids[:M].copy(), corners[:M].copy(), rv[:M].copy(), tv[:M].copy()

    def get_detections(self):
        return self._detections(self.lib.aslam_get_detections)

    def get_slot_detections(self, slot):
        return self._detections(self.lib.aslam_get_slot_detections, int(slot))

    def get_observations(self):
        n = C.c_int()
        ids = np.zeros(MARKER_MAX, np.int32); idx = np.zeros(MARKER_MAX, np.int32); act = np.zeros(MARKER_MAX, np.int32)
        xyth = np.zeros((MARKER_MAX, 3)); R = np.zeros((MARKER_MAX, 3))
        self._ck(self.lib.aslam_get_observations(self.h, C.byref(n), _ptr(ids, _ip), _ptr(idx, _ip), _ptr(act, _ip), _ptr(xyth, _dp), _ptr(R, _dp)))
        k = n.value
        return ids[:k].copy(), idx[:k].copy(), act[:k].copy(), xyth[:k].copy(), R[:k].copy()

    def get_slot_raw_observations(self, slot):
        n = C.c_int()
        ids = np.zeros(MARKER_MAX, np.int32); valid = np.zeros(MARKER_MAX, np.int32)
        xyth = np.zeros((MARKER_MAX, 3)); R = np.zeros((MARKER_MAX, 3))
        self._ck(self.lib.aslam_get_slot_raw_observations(self.h, int(slot), C.byref(n), _ptr(ids, _ip), _ptr(valid, _ip), _ptr(xyth, _dp), _ptr(R, _dp)))
        k = n.value
        return ids[:k].copy(), valid[:k].copy(), xyth[:k].copy(), R[:k].copy()

    def get_slot_ekf_stats(self, first, count):
        """count x 4 ints: markers detected, landmarks appended, corrections fused, stationary no-ops of every slot's EKF step"""
        st = np.zeros((int(count), 4), np.int32)
        self._ck(self.lib.aslam_get_slot_ekf_stats(self.h, int(first), int(count), _ptr(st, _ip)))
        return st

    def get_landmark_ids(self):
        n = C.c_int()
        ids = np.zeros(max(int(self.init.max_landmarks), 1), np.int32)
        self._ck(self.lib.aslam_get_landmark_ids(self.h, C.byref(n), _ptr(ids, _ip)))
        return ids[: n.value].copy()

    # -- staged (device-resident) stream API ------------------------------------------------------
    def stage_frames(self, frames, slot0=0):
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.ndim == 2 or (frames.ndim == 3 and frames.shape[-1] == 3):
            frames = frames[None]                      # one gray (rows, cols) or one bgr8 (rows, cols, 3) frame
        n, rows, cols = frames.shape[:3]
        ch = 1 if frames.ndim == 3 else frames.shape[3]
        self._ck(self.lib.aslam_stage_frames(self.h, int(slot0), _ptr(frames, _u8p), n, rows, cols, ch, cols * ch, rows * cols * ch))

    def stage_encoders(self, wl, wr, dt, slot0=0):
        wl = np.ascontiguousarray(wl, dtype=np.float64); wr = np.ascontiguousarray(wr, dtype=np.float64)
        dt = np.ascontiguousarray(dt, dtype=np.float64)
        self._ck(self.lib.aslam_stage_encoders(self.h, int(slot0), int(wl.size), _ptr(wl, _dp), _ptr(wr, _dp), _ptr(dt, _dp)))

    def run_staged(self, first, count, with_ekf=True):
        """with_ekf: False/0 detection + pose only, True/1 full path, 2 EKF steps only (injected observations)"""
        self._ck(self.lib.aslam_run_staged(self.h, int(first), int(count), int(with_ekf)))

    # -- camera rig: C cameras, one EKF step per rig step ---------------------------------------------
    def set_camera_rig(self, cams):
        """cams: Camera structs, or (K, D, (mount_x, mount_y, mount_yaw)) tuples"""
        cams = [c if isinstance(c, Camera) else Camera.make(*c) for c in cams]
        arr = (Camera * max(len(cams), 1))(*cams)
        self._ck(self.lib.aslam_set_camera_rig(self.h, len(cams), arr))

    def add_images(self, imgs):
        """one rig step: one image per camera (all of one size), after the step's add_encoder"""
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in imgs]
        if any(im.shape != imgs[0].shape for im in imgs):
            raise ValueError("the images of a rig step must all have the same size and channels")
        rows, cols = imgs[0].shape[:2]
        ch = 1 if imgs[0].ndim == 2 else imgs[0].shape[2]
        ptrs = (C.c_void_p * len(imgs))(*[im.ctypes.data for im in imgs])
        steps = (C.c_size_t * len(imgs))(*[im.strides[0] for im in imgs])
        self._ck(self.lib.aslam_add_images(self.h, len(imgs), ptrs, rows, cols, ch, steps))

    def run_staged_rig(self, first, n_steps, with_ekf=True):
        """n_steps rig steps from slot `first`: slot first + s * C + c holds camera c's frame of step s"""
        self._ck(self.lib.aslam_run_staged_rig(self.h, int(first), int(n_steps), int(with_ekf)))

    def get_rig_observations(self):
        """get_observations of the last rig step plus the camera of each popped observation: ids, idx, action, cam, xyth, Rdiag"""
        n = C.c_int()
        ids = np.zeros(MARKER_MAX, np.int32); idx = np.zeros(MARKER_MAX, np.int32); act = np.zeros(MARKER_MAX, np.int32)
        cam = np.zeros(MARKER_MAX, np.int32); xyth = np.zeros((MARKER_MAX, 3)); R = np.zeros((MARKER_MAX, 3))
        self._ck(self.lib.aslam_get_rig_observations(self.h, C.byref(n), _ptr(ids, _ip), _ptr(idx, _ip), _ptr(act, _ip), _ptr(cam, _ip),
                                                     _ptr(xyth, _dp), _ptr(R, _dp)))
        k = n.value
        return ids[:k].copy(), idx[:k].copy(), act[:k].copy(), cam[:k].copy(), xyth[:k].copy(), R[:k].copy()

    def get_rig_step_ekf_stats(self, first, count):
        """count x 4 ints per rig step (step s of a call from slot `first` is step first + s): markers detected over all cameras,
        landmarks appended, corrections fused, stationary no-ops"""
        st = np.zeros((int(count), 4), np.int32)
        self._ck(self.lib.aslam_get_rig_step_ekf_stats(self.h, int(first), int(count), _ptr(st, _ip)))
        return st

    def inject_observations(self, slot, ids, valid, xyth, Rdiag):
        ids = np.ascontiguousarray(ids, dtype=np.int32); valid = np.ascontiguousarray(valid, dtype=np.int32)
        xyth = np.ascontiguousarray(xyth, dtype=np.float64).reshape(-1, 3); Rdiag = np.ascontiguousarray(Rdiag, dtype=np.float64).reshape(-1, 3)
        self._ck(self.lib.aslam_debug_inject_observations(self.h, int(slot), int(ids.size), _ptr(ids, _ip), _ptr(valid, _ip), _ptr(xyth, _dp), _ptr(Rdiag, _dp)))

    def inject_candidates(self, slot, ids, rots, corners):
        """overwrite slot's final candidate list: ids (-1 = rejected), corner rotations 0..3, corners n x 4 x 2 (float32)"""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1); rots = np.ascontiguousarray(rots, dtype=np.int32).reshape(-1)
        corners = np.ascontiguousarray(corners, dtype=np.float32).reshape(-1, 8)
        if not ids.size == rots.size == corners.shape[0]:
            raise ValueError("one id, one rotation and 4 corners per candidate")
        self._ck(self.lib.aslam_debug_inject_candidates(self.h, int(slot), int(ids.size), _ptr(ids, _ip), _ptr(rots, _ip), _ptr(corners, _fp)))

    def run_pose(self, first, count, robot_of_slot=None, refine=False):
        """the pose stage alone on the slots' injected candidates (robot_of_slot: a fleet's robot of each slot); refine: with the
        corner refinement of a detection call, over the slots' staged frames"""
        rs = None if robot_of_slot is None else np.ascontiguousarray(robot_of_slot, dtype=np.int32).reshape(-1)
        if rs is not None and rs.size != count:
            raise ValueError("one robot per slot")
        fn = self.lib.aslam_debug_run_pose_refined if refine else self.lib.aslam_debug_run_pose
        self._ck(fn(self.h, int(first), int(count), _ptr(rs, _ip)))

    def run_identify(self, first, count):
        """the identification stage alone on the slots' injected candidates, over the grey frames their last detection read"""
        self._ck(self.lib.aslam_debug_run_identify(self.h, int(first), int(count)))

    def get_identified(self, slot):
        """what run_identify decided per candidate: ids (-1 rejected), rotations, cells (n x nc x nc, border included) and info
        (n x 8: branch 0 Otsu / 1 all zero / 2 all one, Otsu T, border errors, inner sum, inner sum of squares, recorded id,
        recorded rotation, nc)"""
        n = C.c_int()
        ids = np.zeros(CAND_MAX, np.int32); rots = np.zeros(CAND_MAX, np.int32)
        cells = np.zeros((CAND_MAX, 81), np.uint8); info = np.zeros((CAND_MAX, 8), np.int64)
        self._ck(self.lib.aslam_debug_get_identified(self.h, int(slot), CAND_MAX, C.byref(n), _ptr(ids, _ip), _ptr(rots, _ip),
                                                     _ptr(cells, _u8p), _ptr(info, _llp)))
        k = n.value
        nc = int(info[0, 7]) if k else 0
        return ids[:k].copy(), rots[:k].copy(), cells[:k, :nc * nc].reshape(k, nc, nc).copy(), info[:k].copy()

    def inject_contours(self, slot, contours, scales, keys):
        """overwrite slot's kept-contour list: contours = closed point lists (m x 2 ints each), one scale and discovery key each"""
        sizes = np.array([len(p) for p in contours], np.int32)
        pts = np.ascontiguousarray(np.concatenate([np.asarray(p, np.int64).reshape(-1, 2) for p in contours]) if len(contours) else
                                   np.zeros((0, 2)), dtype=np.int32)
        scales = np.ascontiguousarray(scales, dtype=np.int32).reshape(-1); keys = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1)
        if not sizes.size == scales.size == keys.size:
            raise ValueError("one scale and one key per contour")
        self._ck(self.lib.aslam_debug_inject_contours(self.h, int(slot), int(sizes.size), _ptr(scales, _ip), _ptr(keys, _ip), _ptr(sizes, _ip),
                                                      _ptr(pts, _ip)))

    def inject_quads(self, slot, corners, sizes, scales, keys):
        """overwrite slot's quad list (what the quad stage emits): corners n x 4 x 2 ints, contour point counts, scales, keys"""
        corners = np.ascontiguousarray(corners, dtype=np.int32).reshape(-1, 8); sizes = np.ascontiguousarray(sizes, dtype=np.int32).reshape(-1)
        scales = np.ascontiguousarray(scales, dtype=np.int32).reshape(-1); keys = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1)
        if not corners.shape[0] == sizes.size == scales.size == keys.size:
            raise ValueError("4 corners, one size, one scale and one key per quad")
        self._ck(self.lib.aslam_debug_inject_quads(self.h, int(slot), int(sizes.size), _ptr(corners, _ip), _ptr(sizes, _ip), _ptr(scales, _ip),
                                                   _ptr(keys, _ip)))

    def run_quads(self, first, count, stages):
        """the quad stage (stages & 1) and candidate assembly (stages & 2) alone on the slots' injected lists; waits, and raises on
        an overflowed list as sync() does"""
        self._ck(self.lib.aslam_debug_run_quads(self.h, int(first), int(count), int(stages)))

    def run_contours(self, first, count, cut_grid=0, lds_nodes=-1):
        """the contour stage alone on staged frames (threshold, border nodes, segments, cycle resolution, point writer); waits, and
        raises on an overflowed list as sync() does.  cut_grid 0 / 32 / 64; lds_nodes >= 0: node count above which the serial form
        resolves a frame"""
        self._ck(self.lib.aslam_debug_run_contours(self.h, int(first), int(count), int(cut_grid), int(lds_nodes)))

    def debug_nodes(self, slot):
        """(state, next, steps, area) of the slot's node list: packed states as listed (0xFFFFFFFF = unused entry) and segment records"""
        n = C.c_int()
        self.lib.aslam_debug_get_nodes(self.h, int(slot), 0, C.byref(n), None, None, None, None)     # (the size; E_CAPACITY unless empty)
        k = n.value
        state = np.zeros(k, np.uint32); nxt = np.zeros(k, np.uint32); steps = np.zeros(k, np.uint32); area = np.zeros(k, np.int32)
        self._ck(self.lib.aslam_debug_get_nodes(self.h, int(slot), k, C.byref(n), _ptr(state, _up), _ptr(nxt, _up), _ptr(steps, _up), _ptr(area, _ip)))
        return state, nxt, steps, area

    def debug_write_tickets(self, slot):
        """(state, contour, rel, cnt) of the slot's write tickets; cnt = points | steps skipped first << 16"""
        n = C.c_int()
        self.lib.aslam_debug_get_write_tickets(self.h, int(slot), 0, C.byref(n), None, None, None, None)
        k = n.value
        state = np.zeros(k, np.uint32); ci = np.zeros(k, np.uint32); rel = np.zeros(k, np.uint32); cnt = np.zeros(k, np.uint32)
        self._ck(self.lib.aslam_debug_get_write_tickets(self.h, int(slot), k, C.byref(n), _ptr(state, _up), _ptr(ci, _up), _ptr(rel, _up), _ptr(cnt, _up)))
        return state, ci, rel, cnt

    def debug_link_todo(self, slot):
        v = C.c_int()
        self._ck(self.lib.aslam_debug_get_link_todo(self.h, int(slot), C.byref(v)))
        return v.value

    def sync(self):
        self._ck(self.lib.aslam_sync(self.h))

    def detect_batch(self, frames, max_per_frame=64):
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n, rows, cols = frames.shape[:3]
        ch = 1 if frames.ndim == 3 else frames.shape[3]
        counts = np.zeros(n, np.int32)
        ids = np.full((n, max_per_frame), -1, np.int32)
        corners = np.zeros((n, max_per_frame, 4, 2), np.float32)
        rv = np.zeros((n, max_per_frame, 3)); tv = np.zeros((n, max_per_frame, 3))
        self._ck(self.lib.aslam_detect_batch(self.h, _ptr(frames, _u8p), n, rows, cols, ch, cols * ch, rows * cols * ch,
                                             max_per_frame, _ptr(counts, _ip), _ptr(ids, _ip), _ptr(corners, _fp), _ptr(rv, _dp), _ptr(tv, _dp)))
        return counts, ids, corners, rv, tv

    def export_map(self):
        buf = np.zeros(int(self.init.max_landmarks) * MAP_RECORD_BYTES, np.uint8)
        self._ck(self.lib.aslam_export_map(self.h, buf.ctypes.data_as(C.c_void_p), 0))
        return buf

    # -- map gather over RCCL through the C-ABI (no torch) ----------------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * 128)()
        rc = load().aslam_comm_get_unique_id(buf)
        if rc != ASLAM_OK:
            raise AslamError(rc, "aslam_comm_get_unique_id failed (librccl.so not found?)")
        return bytes(buf)

    def comm_create(self, uid, world, rank):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._ck(self.lib.aslam_comm_create(self.h, buf, int(world), int(rank)))
        self._comm_world = int(world)

    def comm_gather_maps(self):
        out = np.zeros(self._comm_world * int(self.init.max_landmarks) * MAP_RECORD_BYTES, np.uint8)
        self._ck(self.lib.aslam_comm_gather_maps(self.h, out.ctypes.data_as(C.c_void_p), 0))
        return out

    def comm_gather_maps_to_device(self, device_ptr):
        """the gathered records (world x max_landmarks, rank-major) into a device buffer, e.g. for merge_map_records(on_device=True)"""
        self._ck(self.lib.aslam_comm_gather_maps(self.h, C.c_void_p(int(device_ptr)), 1))

    def comm_destroy(self):
        self._ck(self.lib.aslam_comm_destroy(self.h))

    def export_map_to_device(self, device_ptr):
        self._ck(self.lib.aslam_export_map(self.h, C.c_void_p(int(device_ptr)), 1))

    # -- instrumentation ------------------------------------------------------------------------------
    def debug_nbr(self, slot, scale, rows, cols):
        out = np.zeros((rows, cols), np.uint8)
        self._ck(self.lib.aslam_debug_get_nbr(self.h, int(slot), int(scale), _ptr(out, _u8p)))
        return out

    def debug_frame_counts(self, slot):
        """list sizes of one slot after its last detection pass"""
        out = (C.c_uint * 6)()
        self._ck(self.lib.aslam_debug_get_frame_counts(self.h, int(slot), out))
        return dict(zip(("nodes", "contours", "points", "write_tickets", "quad_candidates", "serial_link"), [int(v) for v in out]))

    def debug_contours(self, slot, scale, max_contours=20000, max_points=4_000_000):
        n = C.c_int(); tot = C.c_longlong()
        sizes = np.zeros(max_contours, np.int32); keys = np.zeros(max_contours, np.int32)
        pts = np.zeros((max_points, 2), np.int32)
        self._ck(self.lib.aslam_debug_get_contours(self.h, int(slot), int(scale), max_contours, max_points, C.byref(n),
                                                   _ptr(sizes, _ip), _ptr(keys, _ip), _ptr(pts, _ip), C.byref(tot)))
        k = n.value
        return sizes[:k].copy(), keys[:k].copy(), pts[: tot.value].copy()

    def debug_candidates(self, slot, stage):
        n = C.c_int()
        corners = np.zeros((CAND_MAX, 4, 2), np.float32); sizes = np.zeros(CAND_MAX, np.int32); ids = np.zeros(CAND_MAX, np.int32)
        self._ck(self.lib.aslam_debug_get_candidates(self.h, int(slot), int(stage), CAND_MAX, C.byref(n), _ptr(corners, _fp), _ptr(sizes, _ip), _ptr(ids, _ip)))
        k = n.value
        return corners[:k].copy(), sizes[:k].copy(), ids[:k].copy()

    def profile_enable(self, on=True):
        self._ck(self.lib.aslam_profile_enable(self.h, 1 if on else 0))

    def profile_reset(self):
        self._ck(self.lib.aslam_profile_reset(self.h))

    def last_timing(self):
        """host-clock breakdown of the last add_image, microseconds"""
        out = np.zeros(6)
        self._ck(self.lib.aslam_get_last_timing(self.h, _ptr(out, _dp)))
        return dict(zip(("upload", "enqueue_detect", "enqueue_ekf", "wait", "readback", "total"), out.tolist()))

    def plan_stats(self):
        """frames fused inside windows / on the per-frame chain, windows formed, frames left to the device's own plan (since profile_reset)"""
        out = np.zeros(4, np.int64)
        self._ck(self.lib.aslam_get_plan_stats(self.h, _ptr(out, _llp)))
        return dict(frames_in_windows=int(out[0]), frames_per_frame_chain=int(out[1]), windows=int(out[2]), frames_device_planned=int(out[3]))

    def profile_get(self):
        names = (C.c_char_p * 64)(); calls = np.zeros(64, np.int32); ms = np.zeros(64)
        n = self.lib.aslam_profile_get(self.h, 64, names, _ptr(calls, _ip), _ptr(ms, _dp))
        return {names[i].decode(): (int(calls[i]), float(ms[i])) for i in range(n)}

    def synth_render(self, slot, rows, cols, K, ids, poses, marker_length=0.27, background=128, noise_amp=0, seed=0,
                     supersample=4, download=True):
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 12)
        out = np.zeros((rows, cols), np.uint8) if download else None
        self._ck(self.lib.aslam_synth_render(self.h, int(slot), rows, cols, _ptr(K, _dp), int(ids.size), _ptr(ids, _ip) if ids.size else None,
                                             _ptr(poses, _dp) if ids.size else None, float(marker_length), int(background), int(noise_amp),
                                             int(seed), int(supersample), _ptr(out, _u8p)))
        return out
