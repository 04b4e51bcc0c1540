/* aruco_slam_hip.h — C-ABI of libaruco_slam_hip.so, the MI355X (gfx950) drop-in for the hot path of
 * gitAugust/Aruco_Slam: per-frame ArUco detect + per-marker pose + SE(2) EKF-SLAM predict/update.
 *
 * The reference has no FFI layer; its boundary is the C++ class `ArucoSlam`
 * (include/aruco_slam/aruco_slam.h:101-193) whose headers drag in Eigen, OpenCV and ROS.  This header is
 * the POD-only surface a maintainer binds instead; include/aruco_slam/aruco_slam.h wraps it in the
 * reference's own class (same names and signatures).  Every entry point cites the reference interface it replaces.
 *
 * Conventions: every function returns 0 on success and a negative ASLAM_E_* code on failure (never
 * throws); aslam_last_error() gives the text.  A context is bound to one HIP device (it owns a few HIP streams there:
 * detection, EKF chain, uploads) and is NOT thread-safe (the reference relies on the single-threaded ROS spinner, aruco_slam_node.cpp:79).
 * Pointers are plain host pointers unless the parameter name starts with d_.  There is no CPU fallback: on a
 * machine without a usable gfx950 device aslam_create fails with ASLAM_E_NO_DEVICE.
 */
#ifndef ARUCO_SLAM_HIP_H
#define ARUCO_SLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct aslam_ctx aslam_ctx;

enum {
    ASLAM_OK = 0,
    ASLAM_E_INVALID = -1,     /* bad argument */
    ASLAM_E_NO_DEVICE = -2,   /* no HIP device / HIP runtime error at start-up */
    ASLAM_E_HIP = -3,         /* HIP runtime error during a call */
    ASLAM_E_CAPACITY = -4,    /* a device-side list overflowed (see aslam_last_error) */
    ASLAM_E_STATE = -5        /* call out of order (e.g. image before camera parameters) */
};

/* Mirrors struct ArucoSlamIniteData (aruco_slam.h:40-60) plus device/capacity settings.
 * r2c_* is transformStamped_r2c (base_link <- camera_frame_optical); only translation x,y enter the
 * arithmetic (aruco_slam.cpp:359-360), the rest is carried for the visualisation getters. */
typedef struct {
    double Q_k, R_x, R_y, R_theta;       /* parameters.yaml:5-8 */
    double kl, kr, b;                    /* parameters.yaml:11-13 */
    double marker_length;                /* parameters.yaml:17 */
    int    markers_dictionary;           /* parameters.yaml:16 ; 16 = DICT_ARUCO_ORIGINAL */
    float  useful_distance_threshold;    /* aruco_slam.h:58, default 3 (the YAML key never takes effect) */
    double r2c_t[3], r2c_q[4];
    int    device_id;
    int    max_landmarks;                /* capacity of the EKF state: N_max = 3 + 3*max_landmarks */
    int    max_rows, max_cols;           /* largest frame that will be handed over */
    int    max_batch;                    /* frames staged / processed per call of the *_staged functions */
    int    persistent_waves;             /* wavefronts of the work-queue kernels; 0 = default (4096) */
    int    max_updates_per_frame;        /* EKF corrections fused per frame; <= 24 selects the 3-kernel fast chain,
                                            larger values (up to 128) the general 5-kernel chain; exceeding it at run
                                            time is reported as ASLAM_E_CAPACITY.  A frame over the cap keeps its prediction
                                            and its new landmarks and applies none of its corrections: its statistics count
                                            0 fused corrections, while its pop list (action 1) and the last-observed list
                                            are written as if they had been fused */
    unsigned cap_starts_per_frame;       /* 0 = defaults */
    unsigned cap_contours_per_frame;
    unsigned cap_points_per_frame;
    int    ekf_reserved_cus_per_xcd;     /* CUs of every XCD (32 each) kept free of batched detection while an EKF chain runs
                                            beside it (CU-masked detection stream); 0 = default (16), negative = no masking */
} aslam_init;

/* fills *init with the reference's shipped parameters.yaml values and sane capacities */
void aslam_default_init(aslam_init* init);

/* ArucoSlam::ArucoSlam(const ArucoSlamIniteData&)  — aruco_slam.h:109, aruco_slam.cpp:3-19 */
int  aslam_create(const aslam_init* init, aslam_ctx** out);
void aslam_destroy(aslam_ctx* ctx);
const char* aslam_last_error(const aslam_ctx* ctx);

/* ArucoSlam::setCameraParameters(pair<cv::Mat K, cv::Mat D>) — aruco_slam.h:129-133; K row-major 3x3, D n x 1: the plumb-bob
 * k1, k2, p1, p2, k3.  More than 5 coefficients only if every one after the fifth is zero (ASLAM_E_INVALID otherwise: the rational
 * model's k4..k6 are not supported). */
int aslam_set_camera(aslam_ctx* ctx, const double K[9], const double* D, int nD);

/* cv::aruco::DetectorParameters (OpenCV 3.2.0 field names and defaults).  The reference passes none (aruco_slam.cpp:313 uses
 * DetectorParameters::create()), so the defaults are what parity is checked with; this is the knob a maintainer gets
 * instead of the cv::Ptr.  Limits of the build, refused (never ignored) when exceeded: at most 3 threshold windows of 3..23
 * pixels (LDS tile halo, three mask planes), perspectiveRemovePixelPerCell 2..8, markerBorderBits 1, maxMarkerPerimeterRate x
 * the larger side of the frame at most 65534 points (16-bit distances along a border).  doCornerRefinement (off in the reference) runs cv::cornerSubPix on the kept markers, one lane per corner,
 * with cornerRefinementWinSize 1..7. */
typedef struct {
    int    adaptiveThreshWinSizeMin, adaptiveThreshWinSizeMax, adaptiveThreshWinSizeStep;
    double adaptiveThreshConstant;
    double minMarkerPerimeterRate, maxMarkerPerimeterRate;
    double polygonalApproxAccuracyRate;
    double minCornerDistanceRate;
    int    minDistanceToBorder;
    double minMarkerDistanceRate;
    int    doCornerRefinement;
    int    cornerRefinementWinSize, cornerRefinementMaxIterations;
    double cornerRefinementMinAccuracy;
    int    markerBorderBits;
    int    perspectiveRemovePixelPerCell;
    double perspectiveRemoveIgnoredMarginPerCell;
    double maxErroneousBitsInBorderRate;
    double minOtsuStdDev;
    double errorCorrectionRate;
} aslam_detector_params;
void aslam_default_detector_params(aslam_detector_params* p);
int  aslam_set_detector_params(aslam_ctx* ctx, const aslam_detector_params* p);

/* dictionary_ = cv::aruco::getPredefinedDictionary(markers_dictionary) — aruco_slam.cpp:11-12, aruco_slam.h:176.  Only
 * DICT_ARUCO_ORIGINAL (16, the shipped parameters.yaml value) can be generated without OpenCV's tables, so every other
 * dictionary is handed over as data after aslam_create: either bits[n_markers][marker_size^2] (row-major, 1 = white, what
 * Dictionary::getBitsFromByteList returns) or OpenCV's own Dictionary::bytesList buffer (n rows x ceil(ms^2/8) columns x
 * 4 channels, e.g. dictionary->bytesList.data) with dictionary->markerSize / maxCorrectionBits.  marker_size 3..7. */
int aslam_set_dictionary(aslam_ctx* ctx, int marker_size, int n_markers, int max_correction_bits, const uint8_t* bits);
int aslam_set_dictionary_bytes(aslam_ctx* ctx, int marker_size, int n_markers, int max_correction_bits,
                               const uint8_t* bytes_list);

/* ArucoSlam::addEncoder(wl, wr) — aruco_slam.h:116, aruco_slam.cpp:21-74.  t_now_sec stands in for the two
 * ros::Time::now() calls (:26,:31-32); the adapter passes ros::Time::now().toSec(). */
int aslam_add_encoder(aslam_ctx* ctx, double wl, double wr, double t_now_sec);

/* ArucoSlam::addImage(const cv::Mat&) — aruco_slam.h:122, aruco_slam.cpp:76-287.  px is borrowed for the
 * call only (cv_bridge::toCvShare aliasing, aruco_slam_node.cpp:93); channels 1 (gray) or 3 (bgr8). */
int aslam_add_image(aslam_ctx* ctx, const uint8_t* px, int rows, int cols, int channels, size_t step_bytes);
/* host-clock breakdown of the last aslam_add_image in microseconds: upload of the borrowed pixels, enqueueing detection + pose,
 * enqueueing the EKF step, waiting for the device, read-back of the overflow flags, total (instrumentation; no reference counterpart) */
int aslam_get_last_timing(aslam_ctx* ctx, double out[6]);

/* mu_ / sigma_ (aruco_slam.h:182-183).  sigma is written column-major with leading dimension N, exactly
 * Eigen::MatrixXd's layout.  Pass NULL for mu/sigma to query N only. */
int aslam_get_state(aslam_ctx* ctx, int* N, double* mu, double* sigma);
/* overwrite the state (no reference counterpart: used by tests and warm starts) */
int aslam_set_state(aslam_ctx* ctx, int N, const double* mu, const double* sigma, const int* landmark_ids);

/* marker_corners / IDs / rvs / tvs of getObservations (aruco_slam.cpp:309-314) for the last frame of the last
 * call; corners M*8 floats (x0,y0,...,x3,y3), rvecs/tvecs M*3 doubles.  Arrays may be NULL. */
int aslam_get_detections(aslam_ctx* ctx, int* M, int* ids, float* corners, double* rvecs, double* tvecs);
/* the observations popped from obs_ in pop order (aruco_slam.cpp:92-95) for the last frame: id, landmark index
 * at push time (-1 new), action (0 augment, 1 update, 2 stationary no-op, 3 update rejected by the innovation gate of a localizing
 * filter or by the SLAM gate), (x,y,theta), diag(R). */
int aslam_get_observations(aslam_ctx* ctx, int* n, int* ids, int* idx, int* action, double* xyth, double* Rdiag);
/* aruco_id_map inverted: ids[i] = marker id of landmark index i (aruco_slam.h:164) */
int aslam_get_landmark_ids(aslam_ctx* ctx, int* L, int* ids);

/* ---- device-resident stream API (throughput path: frames staged once in HBM) -------------------------
 * aslam_stage_frames uploads nframes tightly packed frames into slots [slot0, slot0+nframes);
 * aslam_stage_encoders stores, per slot, the encoder sample (wl, wr, dt) that precedes that frame;
 * aslam_run_staged(first, count, with_ekf) then runs (with_ekf: 0 detection+pose only, 1 full path, 2 EKF steps only), entirely on the device and asynchronously on the context's
 * stream: detection + pose for all `count` frames batched, followed (with_ekf != 0) by `count` sequential
 * addEncoder(dt) + addImage EKF steps.  Any other with_ekf is refused with ASLAM_E_INVALID, here and in the rig and
 * fleet staged calls.  aslam_sync waits and reports device-side overflow.
 * Re-staging rule: aslam_run_staged returns before the batch has run (its EKF work is even enqueued one call
 * later, once its observations have reached the host).  aslam_stage_frames / aslam_stage_encoders on slots a
 * submitted batch still reads first finish that batch's use of them (they enqueue the deferred EKF work and
 * wait for it), so the new samples can never reach the old batch; slots outside the range are not waited for. */
int aslam_stage_frames(aslam_ctx* ctx, int slot0, const uint8_t* frames, int nframes, int rows, int cols,
                       int channels, size_t step_bytes, size_t frame_stride_bytes);
int aslam_stage_encoders(aslam_ctx* ctx, int slot0, int n, const double* wl, const double* wr, const double* dt);
int aslam_run_staged(aslam_ctx* ctx, int first, int count, int with_ekf);
int aslam_sync(aslam_ctx* ctx);
/* per-slot results of the last aslam_run_staged */
int aslam_get_slot_detections(aslam_ctx* ctx, int slot, int* M, int* ids, float* corners, double* rvecs, double* tvecs);
int aslam_get_slot_raw_observations(aslam_ctx* ctx, int slot, int* n, int* ids, int* valid, double* xyth, double* Rdiag);
/* what the EKF step of each slot in [first, first + count) did, 4 ints per slot: markers detected, landmarks appended
 * (aruco_slam.cpp:208-260), corrections fused (:108-207) and "stationary" no-ops (:192-198).  Lets a caller assert per frame
 * that no observation was lost to the range / covariance gates (aruco_slam.cpp:327-333, :367-368). */
int aslam_get_slot_ekf_stats(aslam_ctx* ctx, int first, int count, int* stats);

/* ---- camera rig: several cameras on one robot feeding one filter (no reference counterpart) --------------
 * Camera c has its own K / D and a planar mount (mount_x, mount_y, mount_yaw) in base_link: optical axis horizontal, pointing at
 * heading mount_yaw in (-pi, pi], optical frame as in the reference (x right, y down, z forward).  A marker seen by camera c is
 * observed at x = cos(yaw) x0 - sin(yaw) y0 + mount_x, y = sin(yaw) x0 + cos(yaw) y0 + mount_y, theta = normAngle(theta0 + yaw),
 * where (x0, y0, theta0) = (t_z, -t_x, normAngle(atan2(-R02, R22))) is the reference's forward-camera observation
 * (aruco_slam.cpp:359-361); the gates and the diagonal covariance are the reference's.  A rig step = one encoder sample, then
 * one image per camera, all taken at the same instant: one EKF step whose queue receives camera 0's observations in detection
 * order, then camera 1's, and so on.  The single-camera configuration (aslam_set_camera, r2c_t) is untouched; only the calls
 * below use the rig.  Rig calls leave aslam_get_detected_markers / aslam_draw_detected_markers refusing with ASLAM_E_STATE. */
#define ASLAM_MAX_CAMERAS 8
typedef struct { double K[9]; double D[5]; int nD; int pad; double mount_x, mount_y, mount_yaw; } aslam_camera;
/* the rig's cameras (1..ASLAM_MAX_CAMERAS and at most max_batch, nD <= 5, mount_yaw in (-pi, pi]); may be called again between calls */
int aslam_set_camera_rig(aslam_ctx* ctx, int n_cams, const aslam_camera* cams);
/* aslam_add_image for a rig step: px[c] (borrowed, step_bytes[c]) is camera c's image, all of one size; one batched detection pass
 * over slots 0..n_cams-1, then one EKF step; synchronous, a no-op before the first encoder sample.  Detections: aslam_get_slot_detections(c) */
int aslam_add_images(aslam_ctx* ctx, int n_cams, const uint8_t* const* px, int rows, int cols, int channels, const size_t* step_bytes);
/* aslam_run_staged for n_steps rig steps: slot first + s*C + c holds camera c's frame of step s, the encoder sample staged in slot
 * first + s*C is the step's (the other slots' samples are ignored); n_steps*C <= max_batch, same with_ekf values, asynchrony and re-staging rules */
int aslam_run_staged_rig(aslam_ctx* ctx, int first, int n_steps, int with_ekf);
/* aslam_get_observations of the last rig step, plus the camera each popped observation came from */
int aslam_get_rig_observations(aslam_ctx* ctx, int* n, int* ids, int* idx, int* action, int* cam, double* xyth, double* Rdiag);
/* the 4 counts of aslam_get_slot_ekf_stats per rig step (all cameras together); step s of a call that started at slot first is step first + s */
int aslam_get_rig_step_ekf_stats(aslam_ctx* ctx, int first_step, int count, int* stats);

/* ---- what the node publishes (aruco_slam_node.cpp:99-118), as plain data for the adapter to wrap in ROS messages ----
 * aslam_get_pose_msg = ArucoSlam::toRosPose (aruco_slam.cpp:378-410): frame "world", z = 0.1, yaw-only quaternion
 * (x, y, z, w) and the 6x6 row-major covariance with sigma_(0..2, 0..2) scattered to rows/columns 0, 1, 5.
 * aslam_get_map_markers = detected_map_ (aruco_slam.cpp:265-281): frame "world", CUBE (L, L, 0.01), rgba (1, .5, 1, .5),
 * z = 0.3, setRPY(0, 1.5708, theta), lifetime 0; id = landmark index.
 * aslam_get_detected_markers = detected_markers_ of the last frame (aruco_slam.cpp:325-347): markers inside the range gate,
 * frame "base_link", rgba (1, 0, 0, 1), pose = transformStamped_r2c applied to (rvec, tvec), lifetime 0.1 s.
 * *n receives the number available; at most max are written. */
typedef struct { double position[3]; double orientation[4]; double covariance[36]; } aslam_pose_msg;
typedef struct { int id; int pad; double scale[3]; float color[4]; double position[3]; double orientation[4]; double lifetime_sec; } aslam_marker_msg;
int aslam_get_pose_msg(aslam_ctx* ctx, aslam_pose_msg* out);
int aslam_get_map_markers(aslam_ctx* ctx, int max, int* n, aslam_marker_msg* out);
int aslam_get_detected_markers(aslam_ctx* ctx, int max, int* n, aslam_marker_msg* out);

/* markered_img_ = img.clone(); cv::aruco::drawDetectedMarkers(markered_img_, marker_corners, IDs) (aruco_slam.cpp:318-319, returned
 * by getMarkedImg(), aruco_slam.h:152): draws the last frame's detections into the caller's bgr8 buffer - quad outline (0,255,0),
 * 7x7 square outline (0,0,255) around corner 0.  Host code; the "id=N" label of the original is not rendered. */
int aslam_draw_detected_markers(aslam_ctx* ctx, uint8_t* bgr, int rows, int cols, size_t step_bytes);

/* MapLoader::loadMap (map_loader.cpp:7-118): the ground-truth map file "id length x y [z [roll [pitch [yaw]]]]" behind the
 * latched real_map topic, parsed with the loader's own rules ('#' comments, malformed line => empty map, short line skipped,
 * the crossed roll / yaw fallbacks) into marker messages (frame "world", rgba (1,1,1,.5)).  Host only; ctx may be NULL. */
int aslam_load_map_txt(aslam_ctx* ctx, const char* path, int max, int* n, aslam_marker_msg* out);

/* ---- localization: track the pose against a fixed, known marker map (no reference counterpart) ----------------
 * The reference's addImage update (aruco_slam.cpp:88-207) applied to a state whose landmark blocks are frozen: mu_l fixed,
 * Sigma_ll = 0, Sigma_xl = 0.  With those zero blocks the reference's K has zero landmark rows, so every correction is
 *     S = H Sigma_xx H^T + R,  K_x = Sigma_xx H^T S^-1,  mu_x += K_x ze,  Sigma_xx <- (I - K_x H) Sigma_xx     (H = pose part of Gxm)
 * and the landmark rows and blocks stay bit for bit unchanged.  Everything else is the reference's: the predict, the observation
 * assembly and its gates, z_hat from the frame-start pose, the single normAngle wrap, the "stationary" no-op against the previous
 * step's list.  An observation whose id is not in the map is dropped before the queue like a gated one: nothing is ever appended.
 * The state keeps the SLAM layout (mu = [pose, map], Sigma = blockdiag(Sigma_xx, 0)), so the state, pose, map, export and gather
 * getters and aslam_save_state work unchanged.  While localizing, every image entry point (aslam_add_image, aslam_run_staged,
 * aslam_add_images, aslam_run_staged_rig, the host-fed stream) runs localization steps: one kernel launch per call, behind the
 * detection, never counted by aslam_get_plan_stats; the EKF stats report 0 landmarks appended; aslam_get_observations lists the
 * popped (known-id) observations with action 1 or 2 and their map index.  aslam_set_state / aslam_load_state refuse with
 * ASLAM_E_STATE.  Every marker has the one init.marker_length (per-marker lengths of a map file are not used), and only a
 * landmark's (x, y, heading) enters: the map's z, roll and pitch do not. */
/* enter localization: state := [pose, map], Sigma := blockdiag(pose_sigma, 0), id tables := map, last-observed list cleared;
   arming (is_init / last_time) untouched.  1 <= n <= max_landmarks, ids unique in [0, 1024), finite values, pose_sigma symmetric. */
int aslam_localize_begin(aslam_ctx* ctx, int n, const int* ids, const double* xyth /* n x 3 */,
                         const double pose[3], const double pose_sigma[9] /* row-major */);
/* leave it: the state stays as it is and later steps are SLAM steps (new ids augment again) */
int aslam_localize_end(aslam_ctx* ctx);
int aslam_is_localizing(aslam_ctx* ctx, int* on);
/* host only, ctx may be NULL: MapLoader markers (aslam_load_map_txt) -> planar landmarks: id, (x, y) = position,
   theta = normAngle(atan2(r_y, r_x)) with r = third column of Matrix3x3(orientation) (the marker's +z axis, which is what
   the observation's atan2(-R02, R22) measures); refuses (ASLAM_E_INVALID, names the id in aslam_last_error(NULL)) a marker
   whose +z axis has no horizontal component (|(r_x, r_y)| < 1e-6) */
int aslam_landmarks_from_markers(int n, const aslam_marker_msg* in, int* ids, double* xyth);

/* ---- fleet localization: many robots tracked against one shared frozen map (no reference counterpart) ------
 * A fleet is R robots, 1 <= R <= min(max_batch, ASLAM_MAX_ROBOTS).  Each robot has one camera (aslam_camera: K, D and planar mount,
 * as in a rig), its own pose filter (mu_x, Sigma_xx), its own last-observed list and its own armed flag; all share one frozen map
 * given as to aslam_localize_begin.  For every robot, the frames it is given produce bit for bit what a single localizing context
 * produces on them (aslam_set_camera_rig with that one camera, aslam_localize_begin with the same map, pose and Sigma, driven by
 * aslam_run_staged_rig): its first frame after aslam_fleet_begin or aslam_fleet_set_pose only arms it (that frame's encoder
 * sample is not applied), and every rule of localization holds per robot, the "stationary" test against its own previous list.
 * A call may carry any subset of the robots; a robot named in several slots of one staged call takes them in ascending order.
 * Robots never interact.  Per call: one batched detection pass, then one EKF kernel launch with one workgroup per robot present.
 * aslam_get_slot_detections, aslam_get_slot_raw_observations and aslam_get_slot_ekf_stats (appended = 0) work on fleet slots.
 * While a fleet is active every entry point that reads or writes the single filter refuses with ASLAM_E_STATE (aslam_add_encoder,
 * aslam_add_image, aslam_add_images, aslam_run_staged / aslam_run_staged_rig with EKF, the host-fed stream, aslam_localize_begin /
 * _end, the state get / set / save / load, the pose / map / detected-marker messages and the overlay, aslam_get_observations,
 * aslam_get_rig_observations, the map export and gather), and so do aslam_set_camera and aslam_set_camera_rig.  Detection-only
 * calls and detector / dictionary changes stay allowed.  Outside fleet mode the fleet calls refuse with ASLAM_E_STATE. */
#define ASLAM_MAX_ROBOTS 256
/* enter fleet mode: cams, poses (R x 3) and pose_sigmas (R x 9, row-major) one per robot, map (ids, xyth) as aslam_localize_begin;
   the camera checks of aslam_set_camera_rig, the map and pose checks of aslam_localize_begin; every robot disarmed.  Refuses with
   ASLAM_E_STATE while localizing.  Called again while a fleet is active, it starts a new fleet. */
int aslam_fleet_begin(aslam_ctx* ctx, int n_robots, const aslam_camera* cams, int n, const int* ids, const double* xyth /* n x 3 */,
                      const double* poses /* R x 3 */, const double* pose_sigmas /* R x 9 */);
/* one batched call, synchronous: n frames (px[i] borrowed, step_bytes[i]; all of one size) of n distinct robots robots[i], each with
   its own encoder sample (wl[i], wr[i], dt[i]) taken before the frame; uses frame slots 0 .. n-1 */
int aslam_fleet_add_images(aslam_ctx* ctx, int n, const int* robots, const double* wl, const double* wr, const double* dt,
                           const uint8_t* const* px, int rows, int cols, int channels, const size_t* step_bytes);
/* staged frames / encoder samples (aslam_stage_frames / aslam_stage_encoders): slot first + i belongs to robot robot_of_slot[i];
   with_ekf as aslam_run_staged (0 detection only, 1 detection + EKF, 2 EKF on injected observations), asynchronous as it */
int aslam_fleet_run_staged(aslam_ctx* ctx, int first, int count, const int* robot_of_slot, int with_ekf);
/* *n_robots = R; the first min(max, R) robots' poses (x, y, theta) and Sigma_xx (row-major) */
int aslam_fleet_get_poses(aslam_ctx* ctx, int max, int* n_robots, double* poses /* R x 3 */, double* sigmas /* R x 9 */);
/* re-seat one robot: pose and Sigma_xx replaced, its last-observed list emptied, disarmed (pose / sigma checked as at begin) */
int aslam_fleet_set_pose(aslam_ctx* ctx, int robot, const double pose[3], const double sigma[9]);
/* leave fleet mode: the single filter is as aslam_create leaves it (empty map, disarmed); cameras and detector settings stay */
int aslam_fleet_end(aslam_ctx* ctx);
/* *n_robots = R of the active fleet (either kind), 0 outside fleet mode */
int aslam_is_fleet(aslam_ctx* ctx, int* n_robots);

/* ---- localization on an uncertain map: Schmidt-Kalman ("consider") steps, single filter and fleet ---------------
 * A map surveyed by SLAM comes with a covariance per landmark (aslam_fleet_merge_maps / aslam_merge_map_records: sigmas, n x 9).
 * The two calls below start localization / a localization fleet that takes it into account: the landmarks are still not estimated
 * (their means and covariances never change), but their covariance enters every S and the pose <-> landmark cross-covariance is
 * carried.  This is the reference's update (aruco_slam.cpp:88-207) with the landmark rows of K set to zero and the covariance
 * updated consistently for that gain; with every landmark covariance zero it is the frozen-map filter above.
 *
 * Per filter X = [Sigma_xx | Sigma_xl] is a 3 x (3 + 3L) strip.  Sigma_ll is fixed and block-diagonal, one 3 x 3 block C_i per
 * landmark; correlations between different landmarks are dropped, as the merge drops them.  Exactly as in the frozen-map steps:
 * the predict's pose arithmetic, the id lookup (unknown ids dropped), the pop order including the heap replay for an id seen twice,
 * the "stationary" no-op, ze and the pose Jacobian Hx from the frame-start pose, and R.  New:
 *   predict     X <- D X on all columns (D = the predict's pose Jacobian, differing from I in (0,2) and (1,2) only), then
 *               Sigma_xx <- (D Sigma_xx) D^T + Q in the frozen-map filter's expression order.
 *   correction  on landmark i, in pop order, with Hl = [[c, s, 0], [-s, c, 0], [0, 0, 1]] (c, s of the frame-start heading: the
 *               landmark part of the reference's Gxm):
 *                   cst = Hx X                                (3 x (3 + 3L))
 *                   cst[:, block i] += Hl C_i
 *                   cst[:, 0:3]     += Hl (X[:, block i])^T
 *                   S = cst[:, 0:3] Hx^T + cst[:, block i] Hl^T + diag(R)
 *                   K = (cst[:, 0:3])^T S^-1                  (3 x 3)
 *                   mu_x += K ze,   X <- X - K cst
 *   gate        when set (aslam_set_innovation_gate): d2 = ze^T S^-1 ze with this S; a rejected correction leaves mu_x and the
 *               whole strip untouched; slot and track records, action 3 and the compaction of the last-observed list as for the
 *               frozen map; ref_flagged uses this K.
 *   reseat      every seat of a pose zeroes that filter's Sigma_xl: aslam_fleet_set_pose and a solved apply != 0 of aslam_relocalize /
 *               aslam_fleet_relocalize.  A relocalized pose IS correlated with the map it was solved against; that correlation is
 *               deliberately dropped (relocalization uses the map means only).
 * The calls that started on an exact map (aslam_localize_begin, aslam_fleet_begin) keep their filter and their kernels.  Every mode
 * rule of localization and of fleets holds unchanged. */
/* aslam_localize_begin with landmark covariances: its checks, and map_sigmas finite; C_i = (S_i + S_i^T) / 2 is used (as the merge
   does), its diagonal must be >= 0 and C_jk^2 <= C_jj C_kk for each pair, else ASLAM_E_INVALID naming the id, the state untouched.
   An all-zero block is legal (what the merge returns for n_seen = 0).  State := [pose, map], Sigma := blockdiag(pose_sigma, C_0 ..
   C_{n-1}); the strip lives in rows 0..2 of Sigma, mirrored into columns 0..2, so aslam_get_state, aslam_export_map (which reports
   C_i) and aslam_save_state work unchanged, and aslam_localize_end leaves a valid SLAM state whose later steps move the landmarks. */
int aslam_localize_begin_uncertain(aslam_ctx* ctx, int n, const int* ids, const double* xyth /* n x 3 */,
                                   const double* map_sigmas /* n x 9 row-major */, const double pose[3], const double pose_sigma[9]);
/* aslam_fleet_begin with one shared table of landmark covariances (checked as above); every robot gets a zeroed cross strip of
   3 x 3n doubles, freed by aslam_fleet_end / aslam_destroy (and by the next begin).  ASLAM_E_CAPACITY if the strips do not fit:
   then no fleet is active. */
int aslam_fleet_begin_uncertain(aslam_ctx* ctx, int n_robots, const aslam_camera* cams, int n, const int* ids, const double* xyth,
                                const double* map_sigmas /* n x 9 */, const double* poses /* R x 3 */, const double* pose_sigmas /* R x 9 */);
/* *on = 1 while the active localization or localization fleet runs on an uncertain map */
int aslam_is_map_uncertain(aslam_ctx* ctx, int* on);
/* one robot's Sigma_xl (waits for the enqueued work as the other fleet getters do): *L = landmarks, cross (may be NULL) receives
   3 x 3L doubles, row-major.  ASLAM_E_STATE outside an uncertain-map fleet. */
int aslam_fleet_get_cross(aslam_ctx* ctx, int robot, int* L, double* cross /* 3 x 3L */);

/* ---- fleet SLAM: many robots, each building its own map, in one context (no reference counterpart) -----------
 * A SLAM fleet is R robots, 1 <= R <= min(max_batch, ASLAM_MAX_ROBOTS), each with one camera (aslam_camera) and a complete EKF-SLAM
 * filter of its own: mu and Sigma of capacity init.max_landmarks, id <-> index tables, last-observed list, pop list and armed flag.
 * A robot starts as aslam_create leaves the single filter (mu = 0, Sigma = 0, empty map, disarmed; its first frame only arms it).
 * For every robot, the frames it is given produce bit for bit what one SLAM context produces on them: aslam_set_camera_rig with that
 * one camera, the same aslam_init, every frame on the per-frame chain (windows off, as with ASLAM_NO_WINDOWS), driven by
 * aslam_run_staged_rig: mu, Sigma, landmark ids and order, the per-slot statistics of aslam_get_slot_ekf_stats and the detections.
 * A call may carry any subset of the robots; a robot named in several slots of one staged call takes them in ascending slot order;
 * robots never interact, and one that overflows its map or its corrections per frame is reported as the single filter reports it
 * (ASLAM_E_CAPACITY at the next sync) without touching the others.  aslam_fleet_add_images and aslam_fleet_run_staged (with_ekf 0, 1
 * or 2) serve both fleet kinds; a SLAM call is one batched detection pass, then rounds: round k holds the k-th slot of every robot
 * that has one and is one launch of each kernel of the configured chain for all its robots.  aslam_fleet_get_poses returns every
 * robot's pose and Sigma_xx; aslam_fleet_set_pose refuses with ASLAM_E_STATE (a robot's pose is correlated with its map: re-seat it
 * with aslam_fleet_set_state).  The mode rules of fleet localization hold: the single-filter entry points refuse while either kind is
 * active, aslam_fleet_begin / aslam_fleet_slam_begin start a new fleet of the requested kind, aslam_fleet_end leaves the single
 * filter as aslam_create does and frees the robots' filters.  Outside fleet SLAM the per-robot calls below refuse with
 * ASLAM_E_STATE; a robot index outside the fleet is ASLAM_E_INVALID. */
/* enter fleet SLAM: one camera per robot, checked as by aslam_set_camera_rig; ASLAM_E_STATE while localizing; ASLAM_E_CAPACITY when
   the R filters (about 18 MB each at max_landmarks 256) cannot be allocated, leaving no fleet active */
int aslam_fleet_slam_begin(aslam_ctx* ctx, int n_robots, const aslam_camera* cams);
/* *on = 1 while a SLAM fleet is active */
int aslam_is_fleet_slam(aslam_ctx* ctx, int* on);
/* one robot's filter, with the checks and layouts of aslam_get_state / aslam_set_state / aslam_get_landmark_ids; set_state empties
   the robot's last-observed list and leaves its armed flag */
int aslam_fleet_get_state(aslam_ctx* ctx, int robot, int* N, double* mu, double* sigma);
int aslam_fleet_set_state(aslam_ctx* ctx, int robot, int N, const double* mu, const double* sigma, const int* landmark_ids);
int aslam_fleet_get_landmark_ids(aslam_ctx* ctx, int robot, int* L, int* ids);

/* ---- landmark removal: take landmarks out of a SLAM map on the device -------------------------------------------
 * The reference can only grow its map: after its outlier test it carries "// TODO: Remove map point?" (aruco_slam.cpp:156-175) and
 * never does.  These calls marginalise landmarks out of a SLAM filter, which for a Gaussian is exact and needs no arithmetic: the
 * landmark's three rows and columns of mu and Sigma are deleted, in place on the device, with no copy of mu or Sigma to the host.
 * Which landmarks to remove is the caller's decision (aslam_export_map gives every landmark's 3 x 3 covariance to select on).
 * For one filter, with L landmarks and N = 3 + 3 L before the call:
 * - The call first does what aslam_set_state does: the pending batch is finalised and the streams are synchronised.  On return the
 *   removal has happened.
 * - Landmark i is removed iff its marker id (entry i of aslam_get_landmark_ids) is in ids.  An id that is not in the map is ignored;
 *   an id listed twice counts once; a map that aslam_set_state seeded with one id twice loses both landmarks.  The kept landmarks
 *   keep their relative order; L' is their number, N' = 3 + 3 L'.
 * - mu' and Sigma' are the kept entries bit for bit: with map(a) the old state index of new state index a (pose block first),
 *   mu'[a] = mu[map(a)] and Sigma'[a, b] = Sigma[map(a), map(b)].  Every entry of the device array with row or column in [N', N) is
 *   0.0, as aslam_set_state leaves the unused part, so the filter goes on exactly as one seeded with (mu', Sigma', kept ids).
 * - Landmark ids: entry i < L' is the i-th kept id.  A kept id that occurs twice is still looked up at its first landmark.  A removed
 *   id seen again is appended at index L' like any new id (action 0), and a full map that lost k landmarks takes k new ones.
 * - last_observed_marker_: entries of removed ids are deleted, the others stay, unchanged and in order.  This is the one difference
 *   from aslam_get_state, deleting on the host and aslam_set_state, which empties the list: a kept marker seen again at the same
 *   place is still the reference's "stationary" no-op on the next frame.
 * - Left alone: the pop list of the last frame (aslam_get_observations) and the per-slot statistics are history, and the landmark
 *   indices in them refer to the map BEFORE the removal; the armed flag and the time of the last encoder sample; the innovation gate.
 * ASLAM_E_INVALID, with the state untouched: a null context, n < 0, n > 0 with ids == NULL, an id outside [0, 1024).  n == 0 is
 * ASLAM_OK and changes nothing.  *removed (may be NULL) receives L - L'. */
/* SLAM mode only (a camera rig is SLAM mode); ASLAM_E_STATE while localizing (the map is the caller's there: pass a shorter one to
   aslam_localize_begin) or while a fleet is active */
int aslam_remove_landmarks(aslam_ctx* ctx, int n, const int* ids, int* removed);
/* the same id set removed from every listed robot of the active SLAM fleet, each robot's filter on its own as above, in one launch of
   each kernel for all of them; robots not listed are untouched.  robots == NULL: every robot of the fleet (n_robots is not read);
   removed (may be NULL): one entry per listed robot, in list order (R entries with robots == NULL).  ASLAM_E_STATE outside fleet
   SLAM.  ASLAM_E_INVALID in addition to the above: n_robots < 0, a robot outside [0, R), a robot listed twice.  n_robots == 0 is
   ASLAM_OK and changes nothing. */
int aslam_fleet_remove_landmarks(aslam_ctx* ctx, int n, const int* ids, int n_robots, const int* robots, int* removed);

/* ---- map merge: one shared map from the robots of a SLAM fleet or from gathered GPUs (no reference counterpart) ----
 * Input: n_maps maps (1 <= n_maps <= ASLAM_MAX_ROBOTS) of per_map records each (1 <= per_map <= 1024), map-major, every record the
 * ASLAM_MAP_RECORD_BYTES record of aslam_export_map { int32 id, int32 index, f64 x, y, theta, f64 S[9] }.  A record whose id is outside
 * [0, 1024) is unused (id = -1 included); of two records of one map with the same id the one at the lower position counts.  Every
 * map is in a frame of its own (a SLAM robot's map is in its start frame).  anchor in [0, n_maps) names the map whose frame the
 * result is in; min_common in [2, 1024] is the number of shared ids an alignment needs.
 * A reference table holds per marker id a presence flag and a mean (x, y, theta) in the anchor frame.  It starts as the anchor's
 * records; the anchor has round 0 and the identity transform.  Rounds k = 1, 2, ...: first every map not yet aligned is tested
 * against the table as the round found it.  With K the ids both have (ascending), p_j the map's positions and q_j the table's:
 * |K| < min_common, the map waits; otherwise, in f64, pm / qm the centroids, a = sum (p_j - pm) x (q_j - qm) (2-D cross product),
 * b = sum (p_j - pm) . (q_j - qm); a = b = 0 (every common landmark on one point), the map waits; otherwise phi = atan2(a, b),
 * t = qm - R(phi) pm and the map is aligned in round k with T = (t_x, t_y, phi).  Headings do not enter the alignment.  Then every
 * id the table lacks is inserted from the lowest-indexed map aligned in this round that has it, as (R(phi)(x, y) + t,
 * wrap(theta + phi)), wrap being the library's single normAngle wrap, which maps into [-pi, pi): a heading of exactly pi comes out
 * as -pi.  The rounds end when one aligns no map or all are aligned;
 * a map never aligned has round -1, T = (0, 0, 0) and contributes nothing.
 * Fusion, once per id of the table, over the aligned maps that hold it in ascending map order: C = (S + S^T) / 2, C' = J C J^T with
 * J = blockdiag(R(phi), 1), m' the transformed mean; a contribution whose C' has a non-finite entry or a leading principal minor
 * <= 0 is skipped.  With m0 the table's mean and d = m' - m0 (theta component wrapped): Lambda = sum C'^-1,
 * m = m0 + Lambda^-1 sum C'^-1 d (theta wrapped), covariance Lambda^-1, n_seen = contributions used; none usable: m0, a zero
 * covariance, n_seen 0.  Deliberately dropped: the uncertainty of the alignment itself, and the correlations between different
 * landmarks of one map (a frozen localization map has Sigma_ll = 0 anyway).  No floating-point atomics: the same input gives the
 * same bits.
 * Output, one entry per id of the table in ascending id order: ids, xyth (n x 3), sigmas (n x 9, row-major), n_seen - exactly what
 * aslam_localize_begin / aslam_fleet_begin take as a map; per map map_round and map_T (3 per map).  *n receives the number of
 * entries available, at most max are written; any output pointer may be NULL. */
/* a pure function of its input: allowed in every mode, touches no filter, synchronous.  records_on_device != 0: records is a
   device pointer, e.g. the destination of aslam_comm_gather_maps (n_maps = world, per_map = max_landmarks).  ASLAM_E_INVALID: a null
   context or records, n_maps, per_map, anchor or min_common outside the ranges above, max < 0.  The limit on per_map holds for
   device records too: a gather from contexts created with max_landmarks > 1024 is refused here (a map holds at most 1024 distinct
   ids, so such a buffer can be compacted to 1024 records per map first). */
int aslam_merge_map_records(aslam_ctx* ctx, const void* records, int records_on_device, int n_maps, int per_map, int anchor,
                            int min_common, int max, int* n, int* ids, double* xyth, double* sigmas, int* n_seen, int* map_round,
                            double* map_T);
/* the same on the R maps of the active SLAM fleet (map r = robot r, per_map = max_landmarks): does what aslam_sync does and returns
   its error if any, exports all robots' maps with one launch and merges them; no robot's filter changes.  ASLAM_E_STATE outside
   fleet SLAM; ASLAM_E_INVALID: a null context, anchor outside [0, R), min_common outside [2, 1024], max < 0.  max_landmarks is not
   limited here: a fleet of any capacity merges.  The scratch tables and the record buffer of both calls are allocated on first use
   and freed by aslam_fleet_end / aslam_destroy. */
int aslam_fleet_merge_maps(aslam_ctx* ctx, int anchor, int min_common, int max, int* n, int* ids, double* xyth, double* sigmas,
                           int* n_seen, int* robot_round, double* robot_T);
/* device memory the two calls above hold at present: tables plus record buffer, 0 before the first merge and after aslam_fleet_end */
int aslam_merge_scratch_bytes(aslam_ctx* ctx, long long* bytes);

/* ---- relocalization: lost poses from one frame against the frozen map (no reference counterpart) ---------------
 * Localization and fleet localization need a pose and a Sigma_xx from the caller before the first frame, and a filter whose pose is
 * wrong by a metre never converges (its corrections are linearised at that pose).  These calls turn one slot's observation list
 * (what aslam_get_slot_raw_observations returns: already in the base frame) and the frozen map into a pose and a covariance, on the
 * device, for any number of slots in one launch.  Read-only apart from the optional seating of the pose (apply != 0).
 * Parameters: tol_xy (m) and tol_th (rad) bound the distance between two pose hypotheses that support each other, min_inliers is
 * the consensus a solution needs.  The defaults (0.25 m, 0.2 rad, 2) are the maintainer's choice; nobody has measured them.
 * ASLAM_E_INVALID: tol_xy or tol_th not finite or not positive, tol_th >= pi, min_inliers outside [1, 128].
 * For one slot, over its first nM = min(number of observations, 128) observations in list order:
 * 1. Candidates.  Observation j is a candidate iff valid != 0, 0 <= id < 1024, the id is in the map, x, y, theta are finite and
 *    r0, r1, r2 are finite and > 0.  An id seen twice gives two candidates.
 * 2. Hypotheses.  With the id's landmark (lx, ly, lt): theta_j = wrap(lt - theta), c = cos theta_j, s = sin theta_j,
 *    x_j = lx - (c x - s y), y_j = ly - (s x + c y): the pose at which the localization step's z_hat equals the observation.  wrap is
 *    the library's single normAngle wrap, into [-pi, pi).
 * 3. Consensus.  Candidate k supports candidate j iff (x_k - x_j)^2 + (y_k - y_j)^2 <= tol_xy^2 and |wrap(theta_k - theta_j)| <=
 *    tol_th; a candidate supports itself.  count_j = supporters of j.  The winner b has the greatest count, ties to the lowest list
 *    position.  runner_up = the greatest count among the candidates that do not support b, 0 if there is none: reported only, so that
 *    a caller can reject an ambiguous frame (two places of the map that look alike).
 * 4. Status.  1: no candidate (n_candidates = n_inliers = runner_up = 0, best = -1).  2: count_b < min_inliers (n_inliers = count_b,
 *    best, runner_up and n_candidates as found).  0: solved.  With status != 0 pose and sigma are zero and nothing is seated.
 * 5. Fusion over the supporters of b in ascending list position, in information form around m0 = hypothesis b:
 *    J = [[-c, s, -(s x + c y)], [-s, -c, c x - s y], [0, 0, -1]] (the hypothesis' derivative by the observation), C = J diag(r) J^T,
 *    Lambda = sum C^-1, m = m0 + Lambda^-1 sum C^-1 d with d = m_j - m0, its theta component wrapped (headings fuse across the wrap);
 *    pose = m with theta wrapped, sigma = Lambda^-1 (row-major), n_inliers = count_b, best = b's list position.
 * Every sum has a fixed order and there is no floating-point atomic: the same input gives the same bits, whatever else the call
 * carries.  Dropped: the map's own uncertainty (zero in a frozen map) and any accumulation over several frames. */
typedef struct { double tol_xy, tol_th; int min_inliers; } aslam_relocalize_params;
typedef struct { int status, n_candidates, n_inliers, runner_up, best; double pose[3], sigma[9]; } aslam_relocalize_result;
void aslam_default_relocalize_params(aslam_relocalize_params* params);
/* Both calls are synchronous.  Their one kernel launch runs behind the detection and the EKF steps submitted so far, so they may
   follow aslam_run_staged / aslam_fleet_run_staged (with_ekf = 0) or an injection directly; the results come back in one copy.
   params NULL = the defaults.  The result records live in a device buffer allocated by the first call and freed by aslam_fleet_end /
   aslam_destroy.
   aslam_relocalize: the single filter, only while localizing (ASLAM_E_STATE otherwise); a bad slot is ASLAM_E_INVALID.  With apply
   and status 0 the pose and Sigma_xx are replaced and the last-observed list is emptied; the arming is left as aslam_localize_begin
   leaves it. */
int aslam_relocalize(aslam_ctx* ctx, int slot, const aslam_relocalize_params* params, int apply, aslam_relocalize_result* out);
/* slot first + i belongs to robot robot_of_slot[i], its result is out[i].  Only in fleet localization (ASLAM_E_STATE otherwise: a
   SLAM fleet has no shared map); ASLAM_E_INVALID: a slot range outside [0, max_batch), a robot index outside the fleet, a robot named
   twice.  With apply every solved robot is seated as by aslam_fleet_set_pose (pose, Sigma_xx, list emptied, disarmed: its next frame
   only arms it); unsolved robots are untouched. */
int aslam_fleet_relocalize(aslam_ctx* ctx, int first, int count, const int* robot_of_slot, const aslam_relocalize_params* params,
                           int apply, aslam_relocalize_result* out /* count */);

/* ---- SLAM relocalization: a lost SLAM filter against its own, live map (no reference counterpart) -----------------
 * The recovery that follows `lost` in SLAM, rig SLAM and fleet SLAM (the two gate sections below), and the inverse of the reference's
 * augment: the augment makes a landmark a function of the pose and an observation, this makes the pose a function of landmarks and
 * observations.  A pose derived from the map's own landmarks is correlated with exactly those landmarks; a seat that wrote Sigma_xl =
 * 0 would make the next corrections count the same information twice.  So the covariance follows to first order, on the device, in
 * place: Sigma_xx' AND the strip Sigma_lx'.  Parameters, defaults, the result struct and the ASLAM_E_INVALID cases are those of the
 * section above.
 * The filter has mean mu, covariance Sigma (column-major, N = 3 + 3 L) and its id table.  For one slot, over its first nM =
 * min(number of observations, 128) observations in list order:
 * 1. Candidates, hypotheses, consensus, winner, runner-up and status are steps 1-4 of the section above, word for word; the "map" is
 *    the filter's own: id -> landmark index i through its id table, (lx, ly, lt) = mu[3 + 3 i .. 5 + 3 i].  An empty map gives
 *    status 1.
 * 2. Fusion weights.  For supporter j of the winner b, in ascending list position, with landmark index i_j: c, s = cos, sin of
 *    theta_j and (x, y) the observation's; J_j as in step 5 above; G_j = d hypothesis / d landmark = [[1, 0, s x + c y], [0, 1,
 *    -(c x - s y)], [0, 0, 1]]; P_j = the 3 x 3 block Sigma(3 + 3 i_j.., 3 + 3 i_j..), taken from its upper triangle and mirrored;
 *    C_j = J_j diag(r_j) J_j^T + G_j P_j G_j^T (upper triangle, mirrored); Lambda = sum_j C_j^-1; d_j = m_j - m0 with the heading
 *    wrapped; m = m0 + Lambda^-1 sum_j C_j^-1 d_j with the heading wrapped; A_j = Lambda^-1 C_j^-1 and M_j = A_j G_j.
 * 3. Covariance, first order and exact for these weights.  B is 3 x N and zero except B[:, 3 + 3 i_j .. 5 + 3 i_j] += M_j (an id
 *    sighted twice adds twice).  Sigma_lx' = Sigma_ll B^T, read as Sigma(c, 3 + 3 i_j + k) for c = 3 .. N - 1 (the landmark's
 *    columns), accumulated in ascending j.  Sigma_xx' = sum_j A_j (J_j diag(r_j) J_j^T) A_j^T + B Sigma B^T, upper triangle mirrored.
 *    pose = m, sigma = Sigma_xx' (row-major).  With Sigma_ll = 0 this is the section above's Lambda^-1.
 * 4. Seat (apply != 0 and status 0): mu[0..2] = m; Sigma(0..2, 0..2) = Sigma_xx'; rows 3 .. N - 1 of columns 0..2 receive
 *    Sigma_lx' and columns 3 .. N - 1 of rows 0..2 its transpose, bit for bit; the last-observed list is emptied.  Nothing else is
 *    written: not mu_l, not Sigma_ll, not the id tables, nothing at or beyond index N.  The arming is left as it is (as
 *    aslam_set_state / aslam_fleet_set_state leave it); the filter's track record of the SLAM gate is cleared.
 * 5. Unsolved slots, and every slot with apply = 0, write nothing but the record.
 * 6. No floating-point atomic and a fixed order of every sum: a slot's record and seat do not depend on the other slots of the call.
 * Dropped: the weights ignore the cross-correlation between DIFFERENT landmarks (the estimator stays unbiased and the reported
 * covariance is exact for the weights used; it is not the generalised-least-squares optimum); no accumulation over several frames; no
 * relinearisation; the old pose's information is discarded entirely - that is the point.  The default tolerances are the section
 * above's, as unmeasured.
 * Both calls are synchronous: two kernel launches behind the detection and the EKF steps submitted so far (a batch still pending is
 * enqueued first), so they may follow aslam_run_staged / aslam_fleet_run_staged (with_ekf = 0) or an injection directly.  The seat
 * tables live in a device buffer of max_batch entries allocated by the first call and freed by aslam_fleet_end / aslam_destroy.
 * aslam_slam_relocalize: SLAM and rig SLAM (any camera's slot: its list is already in the base frame); ASLAM_E_STATE while
 * localizing and in either kind of fleet.  aslam_relocalize keeps refusing outside localization. */
int aslam_slam_relocalize(aslam_ctx* ctx, int slot, const aslam_relocalize_params* params, int apply, aslam_relocalize_result* out);
/* slot first + i belongs to robot robot_of_slot[i], its result is out[i].  Only in fleet SLAM (ASLAM_E_STATE otherwise;
   aslam_fleet_relocalize keeps refusing a SLAM fleet); ASLAM_E_INVALID: a slot range outside [0, max_batch), a robot index outside
   the fleet, a robot named twice.  With apply every solved robot's filter is seated as above; unsolved robots are untouched. */
int aslam_fleet_slam_relocalize(aslam_ctx* ctx, int first, int count, const int* robot_of_slot, const aslam_relocalize_params* params,
                                int apply, aslam_relocalize_result* out /* count */);

/* ---- innovation gate and lost-track detection for localization and localization fleets ------------------------
 * The reference tests every correction with `ze.norm() >= 1 || K.norm() >= 10` (aruco_slam.cpp:156-175) but only prints the result
 * ("Outlier test logs only"; the skip is a commented-out `continue`).  Here the test becomes a chi-square gate
 * with a consequence, and every filter keeps a record from which a caller sees that it is lost and should be relocalized.
 * The gate is off by default, and with it off every kernel, call and result is what it is without this section.  It can be set in
 * any mode and persists, but takes effect only in the localization steps of the single localizing filter (aslam_localize_begin;
 * single-camera and rig steps) and of a localization fleet (aslam_fleet_begin).  SLAM, rig SLAM and fleet SLAM ignore it: they have
 * a switch of their own, aslam_set_slam_gate below.  (Their per-frame chains compose a frame's corrections into one factorisation,
 * but each pivot block of that factorisation is one correction's S, so a per-correction gate does fit that form.)
 * With a gate set those steps run a gated variant of the chain.  Everything up to the chain is unchanged: the predict, the lookup of
 * ids, the pop order, the "stationary" test against the previous step's list and every correction's H, ze and R from the
 * frame-start pose.  Then for each prepared correction (action 1), in pop order:
 * 1. S = H P H^T + R from the live P, S^-1 and K = P H^T S^-1, exactly as without the gate.
 * 2. d2 = ze^T S^-1 ze, the squared Mahalanobis distance of the innovation.
 * 3. The correction is rejected iff gate_d2 is finite and !(d2 <= gate_d2); a NaN d2 therefore rejects.
 * 4. A rejected correction changes neither the pose nor P.
 * 5. With gate_d2 = +inf (monitor only) nothing is rejected, and pose, Sigma_xx, last-observed list, pop list and EKF stats are
 *    bit for bit those of the ungated call.
 * 6. The correction counts as ref_flagged iff ||ze||_2 >= 1 || ||K||_F >= 10, accepted or not: the reference's own test, K being
 *    the 3 x 3 pose gain (the frozen map zeroes the landmark rows of the reference's K).
 * A rejected observation is left out of the list the step leaves as last_observed_marker_ (what the reference's `continue` would
 * do): that list holds the accepted updates and the stationary no-ops, in pop order.  Stationary no-ops are not corrections: they
 * are neither attempted nor gated.  aslam_get_observations reports a rejected observation with action 3; count [2] of
 * aslam_get_slot_ekf_stats ("corrections fused") counts the accepted corrections only.
 * Per EKF slot the step leaves an aslam_slot_health: attempted = corrections the step prepared, accepted = fused, rejected =
 * skipped by the gate, ref_flagged as above, nis_sum = sum of d2 over the accepted in pop order, d2_max = the greatest non-NaN d2
 * over the attempted (0 if none), worst_id = the id of the observation with d2_max (the first in pop order of equal ones; -1 if
 * none).  A record describes the last gated step of its slot (zero before any).
 * Per filter (one per robot; one for the single filter) an aslam_track_health: frames = gated frames stepped since the last seat,
 * accepted_total / rejected_total = corrections fused / skipped since then, bad_streak = consecutive bad frames, lost =
 * bad_streak >= lost_after.  In integers: a frame is bad iff attempted >= min_attempted and 100 accepted < min_accept_percent
 * attempted; good iff attempted >= min_attempted and not bad.  A good frame sets bad_streak to 0, a bad one adds 1, a frame with
 * fewer than min_attempted corrections leaves it; the streak is carried across the slots of a call and across calls.  Every seat
 * clears the record: aslam_localize_begin, aslam_fleet_begin, aslam_fleet_set_pose, and a solved apply != 0 of aslam_relocalize /
 * aslam_fleet_relocalize (the solved robots only).  `lost` only reports: the gate works the same way afterwards, and recovery is the
 * caller's aslam_relocalize / aslam_fleet_relocalize (in the SLAM modes, under the SLAM gate below: aslam_slam_relocalize /
 * aslam_fleet_slam_relocalize).
 * Defaults: gate_d2 = 16.266, the 0.999 quantile of chi-square with 3 degrees of freedom; min_attempted 2, min_accept_percent 50,
 * lost_after 3.  They are the maintainer's choice; nobody has measured them.  ASLAM_E_INVALID: gate_d2 not > 0 (NaN included; +inf
 * is allowed), min_attempted < 1, min_accept_percent outside [0, 100], lost_after < 1.
 * No floating-point atomics and a fixed order of every sum: a robot's results do not depend on the other robots of the call. */
typedef struct { double gate_d2; int min_attempted, min_accept_percent, lost_after, pad; } aslam_gate_params;
void aslam_default_gate_params(aslam_gate_params* params);
/* params NULL: the gate is off again.  Allowed in every mode; the first call with parameters allocates the health records
   (2 max_batch slot records, ASLAM_MAX_ROBOTS + 1 track records, and a page-locked copy of each), aslam_destroy frees them.  The
   track records are not touched by this call. */
int aslam_set_innovation_gate(aslam_ctx* ctx, const aslam_gate_params* params /* NULL: off */);
/* *on = 1 while a gate is set; out (may be NULL) receives the parameters in force, the defaults while it is off */
int aslam_get_innovation_gate(aslam_ctx* ctx, int* on, aslam_gate_params* out);
typedef struct { int attempted, accepted, rejected, ref_flagged; double nis_sum, d2_max; int worst_id, pad; } aslam_slot_health;
/* The getters wait for the submitted work as aslam_get_slot_ekf_stats does and refuse with ASLAM_E_STATE while no gate is set or in
   a mode the gate does not work in (the slot records: localization and fleet localization; aslam_get_track_health: localization;
   aslam_fleet_get_health: fleet localization).  In the SLAM modes they read the SLAM gate's records while aslam_set_slam_gate is
   in force (the section below).
   aslam_get_slot_health: EKF slots [first, first + count) within [0, 2 max_batch) - a frame slot for single-camera and fleet calls,
   max_batch + step for a rig step (step as in aslam_get_rig_step_ekf_stats). */
int aslam_get_slot_health(aslam_ctx* ctx, int first, int count, aslam_slot_health* out);
typedef struct { int frames, accepted_total, rejected_total, bad_streak, lost, pad[3]; } aslam_track_health;
int aslam_get_track_health(aslam_ctx* ctx, aslam_track_health* out);                          /* the single localizing filter */
/* *n_robots = robots of the fleet; the records of the first min(max, *n_robots) robots go to out */
int aslam_fleet_get_health(aslam_ctx* ctx, int max, int* n_robots, aslam_track_health* out);  /* a localization fleet */

/* ---- innovation gate for SLAM, rig SLAM and fleet SLAM ------------------------------------------------------------
 * A filter that is building a map fuses every known-id sighting it is handed; the reference computes its outlier test in exactly this
 * place (aruco_slam.cpp:156-175), only logs it, and leaves `// TODO: Remove map point?` with a commented-out `continue`.  One misread
 * id or one moved marker is then written into mu and Sigma of the whole map.  This switch is the reference's sequential filter with
 * that `continue` in force, judged by d2 instead of ||ze|| >= 1.
 * It is a switch of its own, separate from aslam_set_innovation_gate: same struct, same defaults, same ASLAM_E_INVALID cases.  It can
 * be set in any mode and persists; it takes effect in SLAM, rig SLAM (aslam_set_camera_rig, more than one camera) and fleet SLAM
 * (aslam_fleet_slam_begin) and has no effect in the localization modes.  Off by default, and with it off every launch, kernel and
 * result is what it is without this section.
 * With the gate set a step is unchanged up to the solve: predict, id lookup, pop order, augments, the "stationary" test, and every
 * prepared correction's ze and Jacobian at the frozen pre-frame mean.  Augments (new ids) and stationary no-ops are neither attempted
 * nor gated.  Then per prepared correction (action 1), in pop order:
 * 1. S = H Sigma H^T + R and S^-1 as the chain forms them (the pivot block of its block Gauss-Jordan sweep); Sigma here follows the
 *    corrections ACCEPTED before this one in the frame.
 * 2. d2 = ze^T S^-1 ze with the frozen-mean innovation ze, the one the reference would test.
 * 3. The correction is rejected iff gate_d2 is finite and !(d2 <= gate_d2); a NaN d2 therefore rejects.
 * 4. A rejected correction changes nothing in mu or Sigma: its pivot is not eliminated, which is exactly the frame without it.
 * 5. With gate_d2 = +inf (monitor only) mu, Sigma, ids, last-observed list, pop list and EKF stats are bit for bit those of the same
 *    context with the gate off and windows off.
 * 6. ref_flagged counts ||ze||_2 >= 1 only.  The reference's other half, K.norm() >= 10, needs the full N x 3 gain, which these
 *    chains never form.
 * A rejected observation is left out of the list the step leaves as last_observed_marker_ (so the same sighting in the next frame is
 * judged again, not "stationary"), is reported by aslam_get_observations with action 3, and is not counted in entry [2] of
 * aslam_get_slot_ekf_stats.
 * Records: an aslam_slot_health per EKF slot (a frame slot; max_batch + step for a rig step) and one aslam_track_health per filter
 * (the single filter's; robot r's in fleet SLAM), with the fields and the integer streak rule of the section above, carried across
 * slots, rounds and calls on the device.  Every seat of a SLAM filter clears its track record: aslam_set_state, aslam_load_state,
 * aslam_localize_end and aslam_fleet_end (the single filter starts anew), aslam_fleet_slam_begin (every robot), aslam_fleet_set_state,
 * aslam_remove_landmarks and aslam_fleet_remove_landmarks (the robots named), and a solved apply != 0 of aslam_slam_relocalize /
 * aslam_fleet_slam_relocalize (the solved robots only).  `lost` only reports: recovery is the caller's aslam_slam_relocalize /
 * aslam_fleet_slam_relocalize.
 * aslam_get_slot_health, aslam_get_track_health and aslam_fleet_get_health are readable in the SLAM modes exactly while the SLAM gate
 * is set (slot records: SLAM, rig SLAM, fleet SLAM; aslam_get_track_health: SLAM and rig SLAM; aslam_fleet_get_health: fleet SLAM);
 * with only the innovation gate set they refuse there with ASLAM_E_STATE.  The record storage is the section above's, made by
 * whichever setter runs first.
 * Windows: while the SLAM gate is set aslam_run_staged takes the per-frame path (what ASLAM_NO_WINDOWS selects) unless
 * aslam_set_slam_gate_windows (the next section) keeps the windows, and setting or clearing the gate first enqueues a batch still
 * pending.
 * Not covered: a misread id that is NEW to the map is an augment and enters as a landmark; aslam_set_landmark_confirmation (the
 * section on landmark confirmation below) is the switch that keeps it out, and aslam_remove_landmarks removes one that got in.
 * Nothing tunes gate_d2 or R.  No floating-point atomics, every sum in pop order: a robot's result does not depend on the other
 * robots of the call. */
int aslam_set_slam_gate(aslam_ctx* ctx, const aslam_gate_params* params /* NULL: off */);
/* *on = 1 while the SLAM gate is set; out (may be NULL) receives the parameters in force, the defaults while it is off */
int aslam_get_slam_gate(aslam_ctx* ctx, int* on, aslam_gate_params* out);

/* ---- the SLAM gate inside EKF windows ------------------------------------------------------------------------------
 * An opt-in switch, off by default, settable in any mode, persistent.  It changes which path a staged batch takes under the SLAM gate,
 * not what the gate means.  The gated window path is taken only when all of these hold: the SLAM gate is set, windows are enabled (no
 * ASLAM_NO_WINDOWS) and the one-launch window form is in use (no ASLAM_WIN_PIECE: the piece schedule is not gated).  Otherwise a gated
 * context takes the per-frame path exactly as without this switch.  With the switch on but no gate set every launch, kernel and
 * result is the ungated window's.  The setter first enqueues a batch still pending, as aslam_set_slam_gate does.  The verdicts travel
 * in the window's step log, so the switch allocates nothing.  ASLAM_E_INVALID: a null context, or a null `on` in the getter.
 * Inside a window the reference's corrections are sequential rank-3 steps on the window's block of Sigma.  Per correction step:
 * 1. c = H P, S = c H^T + R and S^-1 exactly as the ungated window forms them from the live P, which follows the corrections ACCEPTED
 *    before this one.
 * 2. d2 = ze^T S^-1 ze with the frozen-mean ze of the frame.  The correction is rejected iff gate_d2 is finite and !(d2 <= gate_d2);
 *    a NaN d2 rejects.
 * 3. A rejected step changes nothing: not P, not mu, and not the accumulators from which the rest of Sigma and mu follow once per
 *    window, whatever its ze holds (NaN and infinities included).  It stays a step, because the host planned the step count.
 * 4. With gate_d2 = +inf nothing is rejected and every step performs the ungated step's operations in the ungated order: the results
 *    are bit for bit the ungated window's on the same plan.
 * Planner: the host plans one call behind and treats every prepared correction as accepted.  An entry of its last-observed mirror
 * that came from an action-1 observation of a frame planned under the gate is unconfirmed.  A sighting that tests "stationary"
 * against an unconfirmed entry cannot be decided on the host (the predecessor's verdict decides): the open window is closed and
 * this frame and the rest of its batch run on the gated per-frame chain, planned on the device from the exact list (counted in entry
 * [3] of aslam_get_plan_stats); the next batch reads the list back and forms windows again.  A test that fails needs no verdict: a
 * rejected predecessor is absent from the list and an accepted one is too far away, both give action 1.  Everything else about
 * windows (eligibility, cuts, widening, step counts) is unchanged, so the results are the gated per-frame path's up to rounding.
 * Records: every window frame gets its aslam_slot_health and the accepted count in entry [2] of aslam_get_slot_ekf_stats; the
 * window's last frame leaves the pop list with action 3 for rejected observations and the last-observed list without them; the
 * filter's aslam_track_health advances frame by frame and is carried across windows, per-frame frames, batches and calls.  Rig steps
 * use EKF slots max_batch + step.  Fleet SLAM has no windows and is unaffected. */
int aslam_set_slam_gate_windows(aslam_ctx* ctx, int on);
int aslam_get_slam_gate_windows(aslam_ctx* ctx, int* on);

/* ---- landmark confirmation: new landmarks confirmed by repeated sightings (no reference counterpart) ------------------
 * A SLAM filter appends a landmark the first time any unknown marker id shows up with valid != 0, so one misread id becomes three rows
 * of mu and Sigma for good.  With this switch a new id enters the map only after min_sightings judged frames have seen it.
 * Switch.  aslam_set_landmark_confirmation(ctx, params).  It is off by default, settable in any mode, and persists.
 * Where it takes effect.  Only in EKF steps of SLAM filters, through every entry point that runs such a step:
 * - SLAM, rig SLAM and fleet SLAM;
 * - aslam_add_image, aslam_add_images, aslam_run_staged, aslam_run_staged_rig, the host-fed stream, aslam_fleet_add_images,
 *   aslam_fleet_run_staged;
 * - with_ekf 1 and 2; windows on or off; SLAM gate on or off.
 * Localization and localization fleets never judge anything, because unknown ids are dropped there already.  With the switch off, no
 * launch, kernel or result differs from today.
 * Parameters and per-filter state.
 * - min_sightings K is in [2, 127].
 * - max_gap G is in [1, 1 000 000] frames.
 * - Each SLAM filter keeps, for every id in [0, 1024): confirmed, count and last.
 * - Each SLAM filter keeps a frame counter t.
 * Judging one EKF slot.  An EKF slot is a frame slot, or max_batch + step for a rig step's merged list.  A slot is judged once per EKF
 * call that covers it, before that call's EKF work, over its first min(n, 128) observations.
 * 1. t += 1.  A slot with no observations still advances t.
 * 2. Step A.  U is the set of distinct ids that have at least one sighting with valid != 0 and 0 <= id < 1024, and that are not
 *    confirmed.  For each id in U:
 *    - if count > 0 && t - last > G, set count = 0 (the run went stale);
 *    - count += 1; last = t;
 *    - if count >= K, set confirmed = 1, count = 0 (promoted).
 *    - An id sighted twice in one slot counts once.
 * 3. Step B.  Every sighting with valid != 0, id in range and id still not confirmed gets valid = 0 in the slot's list, in place, and
 *    its bit is set in the slot's mask.
 * 4. Everything else stays untouched and keeps its order:
 *    - confirmed ids;
 *    - ids outside [0, 1024), which only injection can deliver;
 *    - sightings that already have valid == 0;
 *    - x, y, theta, R.
 * 5. The EKF step then runs on the list as it stands.
 *    - In the slot where an id is promoted, all its sightings pass.
 *    - The first is the reference's augment; a second one in the same slot is whatever it is today for an id that is twice in the
 *      list of the frame that first sees it (a second augment: the id is looked up before the frame's augments).
 * The result is a pure function of the filter's table and the list.  It does not depend on lane order, on the other robots of a call,
 * or on how a batch was cut.  Withheld sightings look exactly like sightings dropped by the range or covariance gates (valid = 0), to
 * every chain, to the window planner and to aslam_get_slot_raw_observations.
 * Seeding.  "Reseed" means: confirmed := the ids in the filter's landmark id table, all counts 0, t = 0.  These calls reseed:
 * - the setter when called with parameters, for every SLAM filter present; it first enqueues a pending batch and synchronises, as
 *   aslam_set_slam_gate does;
 * - aslam_set_state, aslam_load_state, aslam_localize_end, aslam_fleet_end (the single filter);
 * - aslam_fleet_slam_begin, for every robot;
 * - aslam_fleet_set_state, for that robot;
 * - aslam_remove_landmarks and aslam_fleet_remove_landmarks, for the filters named (a call that names no id returns before it touches
 *   anything and reseeds nothing).  A removed id must therefore earn its place again, and the tentative counts restart.
 * aslam_slam_relocalize does not reseed, because the map is untouched.  Calling the setter with NULL switches confirmation off; calling
 * it again later reseeds.
 * Records.  An aslam_slot_confirm per EKF slot in [0, 2 max_batch): judged = sightings with valid != 0 and id in range; tentative = the
 * size of U; withheld = sightings invalidated; promoted = ids confirmed in this slot; bit i % 32 of withheld_mask[i / 32] marks list
 * position i.  aslam_get_tentative / aslam_fleet_get_tentative list, in ascending id order, the ids with count > 0 && t - last <= G,
 * with age = t - last; *n receives how many there are, of which the first `max` are written.  They wait for the enqueued work, as the
 * health getters do.
 * Errors.  ASLAM_E_INVALID: a null context, parameters out of range, a bad slot range, or a robot outside the fleet.  ASLAM_E_STATE:
 * the record and tentative getters while the switch is off; aslam_get_tentative in any fleet mode or while localizing;
 * aslam_fleet_get_tentative outside fleet SLAM.  A refused call changes nothing.
 * Lifetime.  The tables (one per robot a fleet can hold and the single filter's, 8 KB each) and records are allocated by the first
 * setter call with parameters and freed by aslam_destroy.  Robots' tables are reseeded with the fleet: they mean nothing outside it.
 * Dropped.  There is no spatial test on tentative sightings, because their world position needs the live pose, which this stage never
 * reads.  Tentative sightings carry no information into the filter until promotion.  The tables are not saved by aslam_save_state.
 * The defaults K = 3, G = 10 are the maintainer's choice.  Nobody has measured them. */
typedef struct { int min_sightings, max_gap; } aslam_confirm_params;
typedef struct { int judged, tentative, withheld, promoted; uint32_t withheld_mask[4]; } aslam_slot_confirm;
void aslam_default_confirm_params(aslam_confirm_params* p);
int aslam_set_landmark_confirmation(aslam_ctx* ctx, const aslam_confirm_params* params /* NULL: off */);
/* *on = 1 while confirmation is set; out (may be NULL) receives the parameters in force, the defaults while it is off */
int aslam_get_landmark_confirmation(aslam_ctx* ctx, int* on, aslam_confirm_params* out);
int aslam_get_slot_confirm(aslam_ctx* ctx, int first, int count, aslam_slot_confirm* out);   /* EKF slots in [0, 2 max_batch) */
int aslam_get_tentative(aslam_ctx* ctx, int max, int* n, int* ids, int* counts, int* ages);
int aslam_fleet_get_tentative(aslam_ctx* ctx, int robot, int max, int* n, int* ids, int* counts, int* ages);

/* ---- pose ambiguity check: markers with a second plausible pose flagged and dropped (no reference counterpart) ---------
 * The pose stage returns one pose per marker: the minimum the homography start leads the Levenberg-Marquardt solve to.  A square seen
 * from a distance has a second, mirrored pose - its normal reflected about the line of sight - that fits the four corners almost as
 * well.  The two differ in exactly what the filter consumes: theta = atan2(-R02, R22) comes out tens of degrees apart while (x, y)
 * barely moves.  The SLAM gate sees such a flip only on a known id and landmark confirmation counts sightings without judging them.
 * Switch.  aslam_set_pose_ambiguity(ctx, params).  It is off by default, settable in any mode, and persists.  With the switch off, no
 * launch, kernel or result differs from today.
 * Where it runs.  One kernel, k_pose_alt, directly behind the pose kernel on the same stream with the same camera source, in every
 * entry point that runs detection: the single camera, rigs (ahead of the merge of a step's lists, so a rejection survives it), both
 * fleet kinds, localization, the host-fed stream, aslam_detect_batch, aslam_debug_run_pose and aslam_debug_run_pose_refined.
 * aslam_run_staged(..., with_ekf = 2) runs no pose stage and so no check.
 * Parameters.  ratio >= 1, finite; floor_px >= 0, finite; min_dtheta in [0, pi); reject 0 or 1.
 * Per marker k of a frame's marker list, all M <= 128 of them, whatever their valid flag:
 * 1. Primary pose.  (r1, t1) is what the pose stage stored, m the marker's 8 float corners as doubles, e1 the sum of squared
 *    reprojection residuals in double, rms = sqrt(e1 / 4).
 * 2. Mirrored start.  With R1 = rodrigues(r1) and v = t1 / |t1|: R' = (I - 2 v v^T) R1 diag(1, 1, -1) - the normal reflected about
 *    the line of sight, the in-plane axes kept, determinant +1.  The start is (rodrigues_inv(R'), t1).
 * 3. Refinement.  The damped iteration of the primary solve from there: Levenberg-Marquardt on the 8 residuals, lambda = 10^k from
 *    k = -3, at most 20 accepted steps, stop when |dp| / |p| < FLT_EPSILON.  Result: (r2, t2) = rvec_alt, tvec_alt, e2,
 *    rms_alt = sqrt(e2 / 4), iters = accepted steps.  The arithmetic order is the kernel's own and fixed, without floating-point
 *    atomics: the same marker gives the same bits whatever else the call carries.  A non-finite result sets flag 4, zeroes the alt
 *    fields (rvec_alt, tvec_alt, xyth_alt, rms_alt, dtheta) and is never ambiguous.
 * 4. Alternate observation.  xyth_alt is (r2, t2) put through the pose stage's observation formula with the frame's mount;
 *    dtheta = |wrap(xyth_alt.theta - observation.theta)|.
 * 5. Flag 1 (ambiguous): rms_alt <= max(ratio * rms, floor_px) && dtheta > min_dtheta, on the doubles stored in the record.  Where the
 *    second minimum does not exist (roughly below 1 m for the reference's marker) the descent returns to the primary pose, dtheta ~ 0
 *    and the marker passes; a second pose that differs in pitch only is harmless to an SE(2) filter and passes too.
 * 6. Flag 2 (rejected): flag 1, reject set and the sighting's valid nonzero.  Then valid = 0 in the slot's raw observation list, in
 *    place: downstream - every chain, the window planner, landmark confirmation, aslam_get_slot_raw_observations - it looks exactly
 *    like a sighting the range gate dropped.  The marker list and aslam_get_slot_detections are not touched.
 * 7. Slot sum: checked = M, ambiguous = markers with flag 1, rejected = markers with flag 2.
 * Records.  aslam_get_slot_pose_ambiguity(ctx, slot, max, n, out, sum) waits for the enqueued work, as the health getters do.  *n = the
 * markers of the slot's last checked pose stage, of which the first `max` records are written to out (may be NULL with max = 0); sum
 * (may be NULL) receives the slot sum.  A slot never checked reads as empty.
 * Errors.  ASLAM_E_INVALID: a null context, parameters out of range, a slot outside [0, max_batch), max < 0 or records without an
 * array.  ASLAM_E_STATE: the slot getter while the switch is off.  A refused call changes nothing.  The setter first enqueues a pending
 * batch and synchronises, as aslam_set_slam_gate does.
 * Lifetime.  max_batch x 128 records and max_batch sums, allocated by the first setter call with parameters, freed by aslam_destroy.
 * Dropped.  No swap to the better-fitting pose: that would change what the pose stage reports.  No use of the filter's prediction to
 * pick a side: the gate does that.  No accumulation over frames.
 * The defaults ratio = 1.5, floor_px = 0.5, min_dtheta = 0.05, reject = 1 are the maintainer's choice.  Nobody has measured them. */
typedef struct { double ratio, floor_px, min_dtheta; int reject, pad; } aslam_pose_ambiguity_params;
typedef struct { double rvec_alt[3], tvec_alt[3], xyth_alt[3]; double rms, rms_alt, dtheta; int flags, iters; } aslam_pose_ambiguity;
typedef struct { int checked, ambiguous, rejected, pad; } aslam_slot_pose_ambiguity;
void aslam_default_pose_ambiguity_params(aslam_pose_ambiguity_params* p);
int aslam_set_pose_ambiguity(aslam_ctx* ctx, const aslam_pose_ambiguity_params* params /* NULL: off */);
/* *on = 1 while the check is set; out (may be NULL) receives the parameters in force, the defaults while it is off */
int aslam_get_pose_ambiguity(aslam_ctx* ctx, int* on, aslam_pose_ambiguity_params* out);
int aslam_get_slot_pose_ambiguity(aslam_ctx* ctx, int slot, int max, int* n, aslam_pose_ambiguity* out, aslam_slot_pose_ambiguity* sum);

/* ---- observation covariance: R of every sighting from the pose solve's own Jacobian (no reference counterpart) ---------
 * Every gate and every filter step of the library takes a sighting's R from the reference's CalculateCovariance: one scalar
 * reprojection error times (R_x, R_y, R_theta) plus (1e-2, 1e-2, 1e-3).  That is not a covariance of anything: against
 * the first-order covariance of the pose solve it is off by a factor of hundreds in (x, y), and too small in theta for a distant
 * frontal marker.  With this switch set, R is the diagonal of that first-order covariance instead.
 * Switch.  aslam_set_observation_covariance(ctx, params).  It is off by default, settable in any mode, and persists.  With the switch
 * off, no launch, kernel or result differs from today.
 * Where it runs.  One kernel, k_pose_cov, directly behind the pose kernel and ahead of the pose ambiguity check (which reads valid), on
 * the same stream with the same camera source, in every entry point that runs detection: the single camera, rigs (ahead of the merge
 * of a step's lists), both fleet kinds, localization and uncertain-map localization, the host-fed stream, aslam_detect_batch,
 * aslam_debug_run_pose and aslam_debug_run_pose_refined.  aslam_run_staged(..., with_ekf = 2) runs no pose stage and so none of this.
 * Every consumer of a slot's raw observation list sees the new R and valid without a change of its own: every chain, the window
 * planner, landmark confirmation, the gates, aslam_get_observations and aslam_get_slot_raw_observations.
 * Parameters.  sigma_px > 0, finite; scale > 0, finite; floor_xy >= 0 and floor_th >= 0, finite; gate_norm > 0, +inf allowed;
 * use_residual 0 or 1.
 * Per marker k of a frame's marker list, all M <= 128 of them, with p = (r, t) the pose the pose stage stored and m the marker's 8 float
 * corners as doubles:
 * 1. Jacobian.  J is the 8 x 6 Jacobian of the projection of the 4 corners (pinhole + plumb-bob) at p, N = J^T J, and
 *    e2 = |project(p) - m|^2, the sum of the 8 squared residuals, in double.
 * 2. Pixel variance.  sigma2 = sigma_px^2, plus e2 / 8 when use_residual is set: a marker that fits badly (blur, occlusion) gets a
 *    larger covariance, the one thing the reference's object_error did.
 * 3. Observation Jacobian.  G is the 3 x 6 Jacobian of the camera-frame observation (t_z, -t_x, atan2(-R02, R22)) with respect to
 *    (r, t): the translation rows are the constants e_6 and -e_4, the heading row is
 *    (R02 dR22/dr_j - R22 dR02/dr_j) / (R02^2 + R22^2) for j < 3 and zero for t.  M = blkdiag(Rot(psi), 1) is the frame's mount.
 * 4. Covariance.  cov = sigma2 M G N^-1 G^T M^T, row-major over (x, y, theta) in the base frame, stored symmetric to the bit.  It is
 *    neither scaled nor floored.  N is factored by Cholesky; the arithmetic order is the kernel's own and fixed, without
 *    floating-point atomics: the same marker gives the same bits whatever else the call carries.
 * 5. Flag 1 (degenerate): an entry of cov is non-finite or a diagonal entry is <= 0.  cov is then zeroed, the sighting gets valid = 0,
 *    R keeps the pose stage's values and flag 2 is not evaluated.
 * 6. Otherwise R is replaced: R[0] = scale cov[0] + floor_xy, R[1] = scale cov[4] + floor_xy, R[2] = scale cov[8] + floor_th.
 *    r_ref keeps what the pose stage had written.  The chains stay diagonal: cov's off-diagonal entries are reported, not consumed.
 * 7. valid is recomputed, not inherited - the pose stage's flag mixes the range gate with the reference's bound on its own R, which
 *    no longer applies.  Flag 4: the range gate in the pose stage's expression, (float)|t| > useful_distance_threshold.  Flag 2:
 *    sqrt(R0^2 + R1^2 + R2^2) > gate_norm on the new R (gate_norm = 1 is the reference's bound, aruco_slam.cpp:367).
 *    valid = !(flags & 7).  A sighting the reference's covariance gate had dropped can therefore come back.
 * 8. Slot sum: checked = M, degenerate = markers with flag 1, gated = markers with flag 2.
 * Records.  aslam_get_slot_obs_covariance(ctx, slot, max, n, out, sum) waits for the enqueued work, as the health getters do.  *n = the
 * markers of the slot's last pose stage under the switch, of which the first `max` records are written to out (may be NULL with
 * max = 0); sum (may be NULL) receives the slot sum.  A slot never processed reads as empty.
 * Errors.  ASLAM_E_INVALID: a null context, parameters out of range, a slot outside [0, max_batch), max < 0 or records without an
 * array.  ASLAM_E_STATE: the slot getter while the switch is off.  A refused call changes nothing.  The setter first enqueues a pending
 * batch and synchronises, as aslam_set_pose_ambiguity does.
 * Lifetime.  max_batch x 128 records and max_batch sums, allocated by the first setter call with parameters, freed by aslam_destroy.
 * Dropped.  The full 3 x 3 R inside the EKF chains: they stay diagonal, and the record carries the full matrix so that a caller can
 * see what the diagonal leaves out.  No estimation of sigma_px from data.  No fusion of k_pose_cov into k_pose_alt when both are on.
 * No change of any gate default.
 * The defaults sigma_px = 0.5, use_residual = 1, scale = 1, floor_xy = 1e-6, floor_th = 1e-6 and gate_norm = 1 (the reference's own
 * bound) are the maintainer's choice.  sigma_px and the two floors are untuned: nobody has measured them. */
typedef struct { double sigma_px, scale, floor_xy, floor_th, gate_norm; int use_residual, pad; } aslam_obs_covariance_params;
typedef struct { double cov[9];      /* row-major 3x3 of (x, y, theta) in the base frame: sigma2 * M G N^-1 G^T M^T, unscaled, no floors */
                 double sigma2;      /* the pixel variance used for this marker */
                 double e2;          /* sum of the 8 squared reprojection residuals at the primary pose, double */
                 double r_ref[3];    /* the CalculateCovariance diagonal k_pose had written and this replaced */
                 int flags, pad; } aslam_obs_covariance;
typedef struct { int checked, degenerate, gated, pad; } aslam_slot_obs_covariance;
void aslam_default_obs_covariance_params(aslam_obs_covariance_params* p);
int aslam_set_observation_covariance(aslam_ctx* ctx, const aslam_obs_covariance_params* params /* NULL: off */);
/* *on = 1 while the switch is set; out (may be NULL) receives the parameters in force, the defaults while it is off */
int aslam_get_observation_covariance(aslam_ctx* ctx, int* on, aslam_obs_covariance_params* out);
int aslam_get_slot_obs_covariance(aslam_ctx* ctx, int slot, int max, int* n, aslam_obs_covariance* out, aslam_slot_obs_covariance* sum);

/* ---- consistent innovations: correct from the mean the previous correction left (no reference counterpart) -----------
 * The reference forms all innovations of a frame at the frame's predicted mean mu_0 (quirk Q1) and then applies the m corrections one
 * after the other, each adding K_i ze_i.  With an honest R (aslam_set_observation_covariance) a frame of m sightings then moves the
 * mean by about H_m = 1 + 1/2 + ... + 1/m innovations instead of one, and every d2 the gates compute is inflated with it.
 * Switch.  aslam_set_consistent_innovations(ctx, on), on = 0 or 1.  Off by default, settable in any mode, kept across
 * aslam_localize_begin / _end and the fleet begins and ends.  With the switch off, no launch, kernel or result differs from today.
 * Semantics.  In pop order, correction i with the reference's ze_i and H_i, both formed at mu_0 exactly as today:
 *     e_i = ze_i - H_i (mu_{i-1} - mu_0)        mu_i = mu_{i-1} + K_i e_i
 * The difference is plain (no angle wrap, and e_i's third component is not wrapped again).  S_i, K_i and the covariance update do not
 * depend on the innovation and keep their bits.  A rejected correction contributes nothing to mu.  This is the exact linear sequential
 * update: the mean equals the joint update mu_0 + Sigma_0 H^T (H Sigma_0 H^T + blockdiag R)^-1 ze over the accepted corrections.
 * On an uncertain map the landmarks are not estimated, so only the pose columns of H_i enter.
 * Gates.  Everything that judges a correction uses e_i: d2, the verdict, nis_sum, d2_max and worst_id, in the innovation gate of
 * localization and fleets and in the SLAM gate.  ref_flagged stays the reference's logged test on ze_i (and on K where the chain forms
 * it): the record of what the reference would have logged.
 * Where it runs.  The localization steps (single and fleet, fixed and uncertain map, gated or not) and the per-frame SLAM chains
 * (single, rig and fleet SLAM, every chain size, gated or not), each in an instantiation of its own beside the existing kernels.
 * Dropped.  Relinearisation: H_i stays the Jacobian at mu_0, one meaning for every chain.  EKF windows: while the switch is on,
 * aslam_run_staged and the host-fed stream plan no windows, gated windows included, and every frame takes the per-frame chain
 * (aslam_get_plan_stats shows it); the window chain keeps the reference's frozen-mean corrections, unless
 * aslam_set_consistent_windows (the next section) is on as well.  With a SLAM gate set, windows come back only with
 * aslam_set_gated_consistent_windows (the section after it) on top of both window switches.
 * Errors.  ASLAM_E_INVALID: a null context or output, on outside {0, 1}.  A refused call changes nothing.  The setter first enqueues a
 * pending batch and synchronises, as the other setters do. */
int aslam_set_consistent_innovations(aslam_ctx* ctx, int on);
int aslam_get_consistent_innovations(aslam_ctx* ctx, int* on);

/* ---- consistent innovations inside EKF windows (no reference counterpart) ------------------------------------------------
 * While consistent innovations are on, every frame takes the per-frame chain (above).  aslam_set_consistent_windows(ctx, on), on = 0
 * or 1, lets aslam_run_staged and the host-fed stream plan EKF windows again: the window chain then corrects its mean with the same
 * e_i = ze_i - H_i (mu_{i-1} - mu_0), the log header carries e_i, so that the means outside the window's set follow, and the
 * covariance keeps the bits of a frozen-mean window.  aslam_get_plan_stats reports the windows.
 * Switch.  Off by default, settable in any mode, kept across aslam_localize_begin / _end and the fleet begins and ends.  With
 * consistent innovations off it changes nothing: the same kernels, the same bits.  With consistent innovations on and this switch off
 * everything is as described above.
 * Where it runs.  SLAM and rig SLAM without a SLAM gate, in the one-launch window with the mean on the chain's logger wave (the
 * defaults; ASLAM_WIN_PIECE or ASLAM_WIN_LOGGER_PARTS other than 3 keep the per-frame chain).  A context with a SLAM gate keeps the
 * per-frame chain while consistent innovations are on, whatever aslam_set_slam_gate_windows says, unless the gated consistent
 * window is switched on as well: aslam_set_gated_consistent_windows (the next section).  Localization, fleets and fleet SLAM have no
 * windows and do not look at the switch.
 * Errors.  ASLAM_E_INVALID: a null context or output, on outside {0, 1}.  A refused call changes nothing.  The setter first enqueues a
 * pending batch and synchronises, as the other setters do. */
int aslam_set_consistent_windows(aslam_ctx* ctx, int on);
int aslam_get_consistent_windows(aslam_ctx* ctx, int* on);

/* ---- the SLAM gate on the running innovation inside EKF windows (no reference counterpart) ------------------------------
 * The robust filter is three switches together: an honest R (aslam_set_observation_covariance), consistent innovations and the SLAM
 * gate.  With all three on, the two window switches above leave every frame on the per-frame chain.
 * aslam_set_gated_consistent_windows(ctx, on), on = 0 or 1, lets aslam_run_staged, aslam_run_staged_rig and the host-fed stream plan
 * EKF windows again, with the gated window's planner unchanged (a repeat of a sighting still unconfirmed closes the window; the tail
 * of the batch takes the gated consistent per-frame chain, aslam_get_plan_stats entry [3]).
 * Semantics.  The gated window's rules with the consistent window's innovation.  Correction i of a window frame, in pop order, with
 * ze_i and H_i formed at the frame's predicted mean mu_0 as today and S_i from the live covariance:
 *     e_i = ze_i - H_i (mu_{i-1} - mu_0)    d2 = e_i^T S_i^-1 e_i    rejected iff gate_d2 is finite and !(d2 <= gate_d2) (a NaN rejects)
 * An accepted correction adds K_i e_i to the mean; a rejected one changes nothing, so mu_i = mu_{i-1} and the next e does not see
 * it.  The records: nis_sum, d2_max, worst_id and the verdicts come from e_i; ref_flagged stays the reference's logged test
 * ||ze_i|| >= 1 on the frozen-mean ze_i.  With gate_d2 = +inf the state is, bit for bit, the ungated consistent window's on the
 * same plan.  Slot records, accepted counts, action 3 in the last frame's pop list, the last-observed list and the track record are
 * the gated window's.
 * Switch.  Off by default, settable in any mode, kept across aslam_localize_begin / _end and the fleet begins and ends.  It takes
 * effect only when a SLAM gate is set and consistent innovations, aslam_set_slam_gate_windows and aslam_set_consistent_windows are all
 * on, windows are enabled and the one-launch form is in use (no ASLAM_NO_WINDOWS, no ASLAM_WIN_PIECE).  In every other combination
 * every launch, kernel and result is what it is with the switch off.  It allocates nothing.
 * Where it runs.  SLAM and rig SLAM (EKF slots max_batch + step), in one form of the one-launch window per width, whatever
 * ASLAM_WIN_LOGGER_PARTS and ASLAM_WIN_WORKER_PUBLISH say.  Localization, fleets and fleet SLAM have no windows and do not look at
 * the switch.
 * Errors.  ASLAM_E_INVALID: a null context or output, on outside {0, 1}.  A refused call changes nothing.  The setter first enqueues a
 * pending batch and synchronises, as the other setters do. */
int aslam_set_gated_consistent_windows(aslam_ctx* ctx, int on);
int aslam_get_gated_consistent_windows(aslam_ctx* ctx, int* on);

/* filter state (mu, sigma, landmark ids, armed flag) to / from a file; no counterpart in the reference (warm starts) */
int aslam_save_state(aslam_ctx* ctx, const char* path);
int aslam_load_state(aslam_ctx* ctx, const char* path);

/* ---- host-fed stream: pinned ring + asynchronous upload (the input step before the path, aruco_slam_node.cpp:85-96) ----
 * aslam_stream_open page-locks a ring of two half batches of frames_per_submit frames (<= max_batch / 2).
 * aslam_stream_push copies one frame and the encoder sample (wl, wr, dt) that precedes it into the ring (px is borrowed
 * for the call only); aslam_stream_acquire / aslam_stream_commit hand the pinned slot to the producer instead (no host
 * copy).  Every frames_per_submit frames the half is uploaded on a copy stream and its detection + EKF steps are
 * enqueued, so the upload of one half overlaps the processing of the other; the calls only block when the ring is full.
 * aslam_stream_flush submits what is pending, waits and reports device-side overflow; then the getters are valid.
 * A half is submitted when it holds frames_per_submit frames, or at a flush if it holds at least one; a submit moves on to the
 * other half; a flush with nothing pending submits nothing and stays on its half.  Frame k of a half of the ring lands in
 * slot half * frames_per_submit + k.
 * - The ring keeps the frame shape (rows, cols, channels) of its aslam_stream_open.  A call that gives the context another
 *   frame shape afterwards (aslam_stage_frames, aslam_add_image(s), aslam_detect_batch, aslam_synth_render with other rows,
 *   cols or channels) leaves the stream unusable: aslam_stream_acquire, _push, _commit and _flush then return ASLAM_E_STATE
 *   and do nothing, until aslam_stream_open is called again.  Nothing is reconfigured silently.
 * - aslam_stream_open on an open stream first submits the frames already committed and waits for them, as aslam_stream_flush
 *   does (at the shape they were committed with, and also when the new rows, cols or channels are then refused), so no committed
 *   frame is lost; a slot that was acquired but not committed is dropped.  The filter carries on across the call.
 * - A refused aslam_stream_push (step_bytes smaller than a row) consumes no slot. */
int aslam_stream_open(aslam_ctx* ctx, int rows, int cols, int channels, int frames_per_submit);
int aslam_stream_push(aslam_ctx* ctx, const uint8_t* px, size_t step_bytes, double wl, double wr, double dt);
int aslam_stream_acquire(aslam_ctx* ctx, uint8_t** px, size_t* step_bytes);
int aslam_stream_commit(aslam_ctx* ctx, double wl, double wr, double dt);
int aslam_stream_flush(aslam_ctx* ctx);

/* cv::aruco::detectMarkers + estimatePoseSingleMarkers on a batch of independent host frames, no EKF
 * (BASELINE config 5).  counts[nframes]; ids/corners/rvecs/tvecs hold max_per_frame entries per frame. */
int aslam_detect_batch(aslam_ctx* ctx, const uint8_t* frames, int nframes, int rows, int cols, int channels,
                       size_t step_bytes, size_t frame_stride_bytes, int max_per_frame, int* counts, int* ids,
                       float* corners, double* rvecs, double* tvecs);

/* ---- landmark-map record for the multi-GPU gather ---------------------------------------
 * Fixed-size record per landmark: { int32 id, int32 index, f64 x, y, theta, f64 Sigma_ll[9] } = 104 bytes.
 * Writes max_landmarks records (unused ones have id = -1) to a host or device buffer. */
int aslam_export_map(aslam_ctx* ctx, void* dst, int dst_is_device);
/* the same without stalling the pipeline: the export is enqueued behind the EKF steps submitted so far and lands in the
 * device buffer d_dst; aslam_export_wait(buffer) blocks until that particular export (buffer 0 or 1) is complete, so a caller
 * can gather step k-1's map while step k is already running on the GPU */
int aslam_export_map_async(aslam_ctx* ctx, void* d_dst, int buffer);
int aslam_export_wait(aslam_ctx* ctx, int buffer);
#define ASLAM_MAP_RECORD_BYTES 104

/* The gather itself for a C / C++ node (one process and one context per GPU): RCCL's all-gather over xGMI straight from the
 * device buffers, librccl.so dlopen'ed on first use (no link-time dependency; a process that already uses RCCL - e.g. through
 * torch - shares its copy).  Rank 0 calls aslam_comm_get_unique_id and hands the 128 bytes to the other ranks by any
 * out-of-band means (ROS parameter, file, socket); every rank then calls aslam_comm_create(ctx, id, world, rank).
 * aslam_comm_gather_maps exports this rank's map behind the EKF steps enqueued so far, all-gathers, and writes
 * world x max_landmarks records (rank-major) to dst (host, or device if dst_is_device).  Read-only: nothing is fused back into
 * any filter (aslam_merge_map_records makes one map of the gathered ones). */
#define ASLAM_COMM_ID_BYTES 128
int aslam_comm_get_unique_id(void* id /* ASLAM_COMM_ID_BYTES */);
int aslam_comm_create(aslam_ctx* ctx, const void* id, int world, int rank);
int aslam_comm_gather_maps(aslam_ctx* ctx, void* dst, int dst_is_device);
int aslam_comm_destroy(aslam_ctx* ctx);

/* ---- instrumentation ---------------------------------------------------------------------------------
 * Stage taps used by the parity tests (tests/): what each detector stage produced for a staged slot. */
int aslam_debug_get_nbr(aslam_ctx* ctx, int slot, int scale, uint8_t* out /* rows*cols */);
/* list sizes of one slot after its last detection pass: border nodes, kept contours, contour points, write tickets, quad candidates, and
 * whether the frame's node cycles went through the serial fallback kernel (more nodes / borders than the LDS image holds) */
int aslam_debug_get_frame_counts(aslam_ctx* ctx, int slot, unsigned out[6]);
int aslam_debug_get_contours(aslam_ctx* ctx, int slot, int scale, int max_contours, long long max_points,
                             int* n_contours, int* sizes, int* keys, int* points_xy, long long* n_points);
int aslam_debug_get_candidates(aslam_ctx* ctx, int slot, int stage /*0 quads (unordered), 2 final*/, int max,
                               int* n, float* corners, int* sizes, int* ids);
/* overwrite a slot's per-marker observations (id, passed-the-gates flag, (x,y,theta), diag R); together with
 * aslam_run_staged(..., with_ekf = 2) = "EKF steps only" this replays recorded observation sequences through the
 * device EKF without the detector (tests/test_ekf_golden.py).  Only this call can deliver an id outside [0, 1024) (a dictionary
 * holds at most 1024 markers): with the flag set, such an observation is a new landmark in every frame, nothing is written to the
 * id table, and aslam_get_landmark_ids reports the id as given (tests/test_plan_kernel.py). */
int aslam_debug_inject_observations(aslam_ctx* ctx, int slot, int n, const int* ids, const int* valid, const double* xyth,
                                    const double* Rdiag);
/* the pose stage on given quads, without the detector (tests/test_pose_kernel.py).  aslam_debug_inject_candidates overwrites a slot's
 * final candidate list with n <= 2048 quads: ids[i] (-1 = rejected), rots[i] in 0..3 (the corner rotation identification found) and
 * corners[8 i .. 8 i + 7] (x0 y0 .. x3 y3 before the rotation).  aslam_debug_run_pose then launches on slots [first, first + count)
 * what a detection call launches after identification: the ordered list of identified candidates (at most 128), the same-id
 * inside-quad filter, solvePnP, the observation and its gates, without corner refinement (aslam_debug_run_pose_refined runs it).  Slot first + i is camera i % n of the rig
 * when one is set (the single camera otherwise); robot_of_slot[i] names its robot while a fleet is active (NULL otherwise).  The
 * results read back through aslam_get_slot_detections / aslam_get_slot_raw_observations, and aslam_run_staged(..., with_ekf = 2)
 * fuses them. */
int aslam_debug_inject_candidates(aslam_ctx* ctx, int slot, int n, const int* ids, const int* rots, const float* corners /* n x 8 */);
int aslam_debug_run_pose(aslam_ctx* ctx, int first, int count, const int* robot_of_slot /* count entries, or NULL */);
/* the same with the corner refinement of a detection call between the filter and solvePnP (tests/test_subpix_kernel.py): cv::cornerSubPix
 * on the 4 corners of every kept marker with the detector parameters in force (window, iteration count clamped to 1..100, accuracy),
 * reading the grey frame a detection pass reads: a gray slot as staged, a bgr8 slot as its last detection pass converted it.  Refused
 * with ASLAM_E_STATE when doCornerRefinement is not set or a slot of the range holds no frame of the current shape, and with
 * ASLAM_E_INVALID when an identified candidate (id >= 0) has a corner outside [0, cols) x [0, rows): a detection pass never produces
 * one, and the refinement starts from a point inside the image. */
int aslam_debug_run_pose_refined(aslam_ctx* ctx, int first, int count, const int* robot_of_slot /* count entries, or NULL */);
/* the identification stage on given quads (tests/test_identify_kernel.py).  aslam_debug_run_identify launches on slots [first,
 * first + count) what a detection call launches at identification, with the context's dictionary and detector parameters: the
 * perspective removal, the inner-region meanStdDev, Otsu, the cell votes, _getBorderErrors and Dictionary::identify, on every
 * candidate aslam_debug_inject_candidates wrote (its corners; the injected ids and rotations are overwritten), reading the grey
 * frame a detection pass reads: a gray slot as staged, a bgr8 slot as its last detection pass converted it.  It runs the
 * instrumented build of the kernel, which also records every decision.  aslam_debug_get_identified returns slot's first
 * min(n, max) candidates: ids[i] (-1 rejected), rots[i], cells[81 i .. 81 i + 80] (the nc x nc cell bits, border included,
 * row-major, zero-padded to 9 x 9) and info[8 i .. 8 i + 7] = {branch (0 Otsu, 1 uniform dark: all bits 0, 2 uniform bright:
 * all bits 1), Otsu threshold (0 off that branch), border errors, inner-region sum, inner-region sum of squares, recorded id,
 * recorded rotation, nc}. */
int aslam_debug_run_identify(aslam_ctx* ctx, int first, int count);
int aslam_debug_get_identified(aslam_ctx* ctx, int slot, int max, int* n, int* ids, int* rots, uint8_t* cells /* max x 81 */,
                               long long* info /* max x 8 */);
/* the quad and assembly stages on given contours / quads (tests/test_quads_kernel.py).  The slots must hold staged frames of the
 * current shape: their shape and the detector parameters in force are the launch's.
 * aslam_debug_inject_contours overwrites a slot's kept-contour list with n closed point lists (contour i: sizes[i] points, packed one
 * after the other in points_xy as x y pairs; scales[i] = its threshold window, keys[i] = its discovery key y * cols + x (+ 1 for a
 * hole border)).  Refused with ASLAM_E_INVALID: n > cap_contours_per_frame, more points in all than cap_points_per_frame, a size
 * outside [1, 65534], a scale that is not a threshold window in force, a key outside [0, rows * cols], a (scale, key) pair twice, a
 * coordinate outside [-16384, 16383] (the 16-bit packing would hold twice that; the quad kernel's integer reductions need squared
 * distances below 2^32).  The perimeter limits (minMarkerPerimeterRate, maxMarkerPerimeterRate) are NOT applied: they are the
 * contour stage's, upstream of this list.
 * aslam_debug_inject_quads overwrites a slot's quad list (what the quad stage would have emitted) with n <= 2048 quads: corners
 * [8 i .. 8 i + 7] = x0 y0 .. x3 y3, sizes[i] = the contour's point count, scales / keys as above, the same checks.
 * aslam_debug_run_quads launches on slots [first, first + count) what a detection call launches for the quad stage (stages & 1) and
 * for candidate assembly (stages & 2), with the queue heads (and, with stages & 1, the quad counts) reset as a detection call
 * resets them; it waits, and reports an overflowed quad or near-pair list as aslam_sync does (ASLAM_E_CAPACITY).  Results:
 * aslam_debug_get_candidates, stage 0 (quads, sorted into candidate order) and stage 2. */
int aslam_debug_inject_contours(aslam_ctx* ctx, int slot, int n, const int* scales, const int* keys, const int* sizes,
                                const int* points_xy);
int aslam_debug_inject_quads(aslam_ctx* ctx, int slot, int n, const int* corners /* n x 8 */, const int* sizes, const int* scales,
                             const int* keys);
int aslam_debug_run_quads(aslam_ctx* ctx, int first, int count, int stages);
/* the contour stage on staged frames (tests/test_contours_kernel.py).  aslam_debug_run_contours launches on slots [first, first +
 * count), which must hold staged frames of the current shape, exactly what a detection call launches up to and including the contour
 * points: the counts cleared, the threshold and border-node kernel, the segment walks, both forms of the cycle resolution and the
 * point writer; then it waits, and reports an overflowed node, contour or point list as aslam_sync does (ASLAM_E_CAPACITY).
 * cut_grid: 0 = the cut lattice a detection call of `count` frames would choose, 32 or 64 = that pitch (anything else:
 * ASLAM_E_INVALID).  lds_nodes < 0: the default; otherwise a frame with more nodes than that is resolved by the serial form (0: every
 * frame with a node).  The slots' ticket lists are filled with unused tickets first, so that a ticket no kernel wrote reads as unused.
 * No camera is needed.  Results: aslam_debug_get_nbr, aslam_debug_get_contours, aslam_debug_get_frame_counts and
 *   aslam_debug_get_nodes: the slot's node list as the threshold kernel wrote it - state[i] = x | y << 12 | s << 24 | scale << 27 |
 *     type << 29 (type 0 cut state, 1 outer start candidate, 2 hole start candidate; 0xFFFFFFFF = an unused staged entry) - and for each
 *     node the segment record: next[i] = index of the next node of its border (0xFFFFFFFF: the walk was cut beyond the largest kept
 *     perimeter, or an unused entry), steps[i], area[i] = the shoelace partial sum over those steps;
 *   aslam_debug_get_write_tickets: state[i], contour[i] (index into the slot's contour list in emission order; 0xFFFFFFFF = a reserved
 *     ticket that is not used), rel[i] = offset of its first point in the contour, cnt[i] = points | steps skipped first << 16;
 *   aslam_debug_get_link_todo: 1 when the serial form resolved the slot's frame, 0 when the LDS form did.
 * The getters fail with ASLAM_E_CAPACITY (and set *n) when the list has more than max entries. */
int aslam_debug_run_contours(aslam_ctx* ctx, int first, int count, int cut_grid, int lds_nodes);
int aslam_debug_get_nodes(aslam_ctx* ctx, int slot, int max, int* n, unsigned* state, unsigned* next, unsigned* steps, int* area);
int aslam_debug_get_write_tickets(aslam_ctx* ctx, int slot, int max, int* n, unsigned* state, unsigned* contour, unsigned* rel,
                                  unsigned* cnt);
int aslam_debug_get_link_todo(aslam_ctx* ctx, int slot, int* flag);
/* HIP-event timing of each kernel family on the context's stream, accumulated since the last reset:
 * names[i] (static strings), calls[i], total_ms[i]; returns the number of entries. */
int aslam_profile_enable(aslam_ctx* ctx, int on);
int aslam_profile_reset(aslam_ctx* ctx);
int aslam_profile_get(aslam_ctx* ctx, int max, const char** names, int* calls, double* total_ms);
/* how the frames submitted with an EKF step since the last aslam_profile_reset were scheduled: out[0] frames fused inside
 * windows (ekf_window.hip), out[1] frames on the per-frame chain, out[2] windows formed, out[3] frames whose bookkeeping was left
 * to the device (a new landmark, one id twice) - the windowed path is an optimisation, never a different result. */
int aslam_get_plan_stats(aslam_ctx* ctx, long long out[4]);

/* deterministic synthetic frame renderer (input generation for tests and bench; not on the hot path).
 * markers: per marker 12 doubles = rotation (row-major 3x3, marker->camera) then translation;
 * ids: dictionary id per marker.  Writes gray frames (rows*cols) into staged slots (on_device=1) or to out. */
int aslam_synth_render(aslam_ctx* ctx, int slot, int rows, int cols, const double K[9], int n_markers, const int* ids,
                       const double* poses, double marker_length, int background, int noise_amp, unsigned seed,
                       int supersample, uint8_t* out_host /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif
