// Host-side launcher of the marker finalisation / pose / observation kernel (pose.hip).
#pragma once
#include "common.h"

namespace aslam {

// cv::cornerSubPix on the kept markers before the pose solve (DetectorParameters::doCornerRefinement; off in the reference)
struct RefineCfg {
    int on, win, max_iters, rows, cols;
    double eps2;                      // cornerRefinementMinAccuracy squared
    const float* mask;                // (2 win + 1)^2 window weights, built on the host with the same expf as the oracle
    const uint8_t* gray;              // tight gray planes of the call's frames
};

void launch_pose(hipStream_t st, int nframes, const FinalCand* finals, const unsigned* n_final, Marker* markers,
                 unsigned* n_markers, ObsRaw* obs, const PoseCams& cams, const SlamParams& sp, Counters* ctr, const RefineCfg& rf);
// launch_pose with frame f's camera read from a device table: tab[cam_of_frame[f]] (a fleet, one camera per robot)
void launch_pose_table(hipStream_t st, int nframes, const FinalCand* finals, const unsigned* n_final, Marker* markers, unsigned* n_markers,
                       ObsRaw* obs, const RigCam* tab, const int* cam_of_frame, const SlamParams& sp, Counters* ctr, const RefineCfg& rf);
// Pose ambiguity check: what k_pose_alt leaves per marker and per frame slot.  The layouts are those of
// aslam_pose_ambiguity / aslam_slot_pose_ambiguity (include/aruco_slam_hip.h): the getter copies them as they are.
struct PoseAmbiguity {
    double rvec_alt[3], tvec_alt[3], xyth_alt[3];
    double rms, rms_alt, dtheta;
    int flags, iters;                 // flags: 1 ambiguous, 2 rejected (valid := 0), 4 the refinement ended non-finite
};
struct SlotPoseAmbiguity { int checked, ambiguous, rejected, pad; };
struct PoseAmbArg {
    double ratio, floor_px, min_dtheta;
    int reject, pad;
    PoseAmbiguity* rec;               // kMarkerMax records per frame, frame 0 of the launch first
    SlotPoseAmbiguity* sum;           // one per frame
};
// k_pose_alt behind k_pose on the same frames, marker lists and camera source: the mirrored second pose of every marker of the
// lists, the records, and valid := 0 in obs for rejected sightings
void launch_pose_alt(hipStream_t st, int nframes, const Marker* markers, const unsigned* n_markers, ObsRaw* obs, const PoseCams& cams,
                     const SlamParams& sp, const PoseAmbArg& arg);
void launch_pose_alt_table(hipStream_t st, int nframes, const Marker* markers, const unsigned* n_markers, ObsRaw* obs, const RigCam* tab,
                           const int* cam_of_frame, const SlamParams& sp, const PoseAmbArg& arg);
// Observation covariance: what k_pose_cov leaves per marker and per frame slot.  The layouts are those of
// aslam_obs_covariance / aslam_slot_obs_covariance (include/aruco_slam_hip.h): the getter copies them as they are.
struct ObsCovariance {
    double cov[9];                    // sigma2 M G N^-1 G^T M^T, row-major (x, y, theta), base frame; zero with flag 1
    double sigma2, e2;
    double r_ref[3];                  // what k_pose had written to ObsRaw::r
    int flags, pad;                   // flags: 1 degenerate, 2 |r| > gate_norm, 4 the range gate
};
struct SlotObsCovariance { int checked, degenerate, gated, pad; };
struct ObsCovArg {
    double sigma_px, scale, floor_xy, floor_th, gate_norm;
    int use_residual, pad;
    ObsCovariance* rec;               // kMarkerMax records per frame, frame 0 of the launch first
    SlotObsCovariance* sum;           // one per frame
};
// k_pose_cov behind k_pose (and ahead of k_pose_alt) on the same frames, marker lists and camera source: ObsRaw::r and valid of
// every marker of the lists replaced by the first-order covariance of its pose solve and the gates on it, and the records
void launch_pose_cov(hipStream_t st, int nframes, const Marker* markers, const unsigned* n_markers, ObsRaw* obs, const PoseCams& cams,
                     const SlamParams& sp, const ObsCovArg& arg);
void launch_pose_cov_table(hipStream_t st, int nframes, const Marker* markers, const unsigned* n_markers, ObsRaw* obs, const RigCam* tab,
                           const int* cam_of_frame, const SlamParams& sp, const ObsCovArg& arg);
// concatenates the observation lists of n_steps rig steps (C = n_cams frames each, from slot frame0) into step lists at slots step0..
void launch_rig_merge(hipStream_t st, int n_steps, ObsRaw* obs, unsigned* n_markers, double* enc, int frame0, int n_cams, int step0, Counters* ctr);

} // namespace aslam
