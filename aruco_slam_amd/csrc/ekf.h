// EKF-SLAM state resident in HBM and the launchers of the EKF kernels (ekf.hip).
// Replaces Eigen's role in ArucoSlam::addEncoder / addImage (src/aruco_slam.cpp:21-74, 88-263).
#pragma once
#include "common.h"

namespace aslam {

constexpr int kIdTableSize = 1024;     // marker id -> landmark index (std::map<int,int> aruco_id_map, aruco_slam.h:164)

struct PopRec {                        // one popped observation (aruco_slam.cpp:92-95) and what was done with it
    int id, index, action, det;        // action: 0 augment, 1 update, 2 stationary no-op, 3 update rejected by the innovation gate; det: position in the frame's observation list
    double z[3];
    double r[3];
};
struct LastObs {                       // last_observed_marker_ entry (aruco_slam.h:188): id + last_observation_
    int id, pad;
    double z[3];                       // NaN = never set (quirk Q2/Q3: never matches)
};
struct UpdRec {                        // one fused EKF correction
    int li, pad;                       // state offset of the landmark: 3 + 3*index
    double Gxm[18];                    // 3 x 6 Jacobian block (aruco_slam.cpp:140-143)
    double ze[3];                      // innovation (aruco_slam.cpp:137-138)
    double r[3];                       // diag of Rk
};
struct MapRecord {                     // 104-byte landmark record gathered across GPUs
    int id, index;
    double x, y, theta;
    double S[9];
};

// ---- windowed EKF (ekf_window.hip): runs of frames whose fused landmarks stay inside one set S --------------------------
constexpr int kWinFrames = 64;         // frames per window at most
constexpr int kWinPieceMax = 16;       // frames per chain piece at most (its step table lives in LDS)
constexpr int kWinCorrMax = 63;        // corrections fused per window frame at most (one lane of the prepare wave each)
constexpr int kWinSMax = 63;           // landmarks in a window's set S at most: 3 + 3 * 63 = 192 = 12 MFMA tiles
constexpr int kWinHdr = 24;            // doubles of scalar header per logged step (after the 3 operand rows)
constexpr int kWinSyncLine = 16;       // 64-bit words per hand-off counter of the one-launch window (one 128-B line each)
constexpr int kWinSyncCounters = 1 + 192 / 8 + 1;   // the chain's step count, one per replay workgroup, the workgroup ticket
struct WinFrame {                      // host-planned bookkeeping of one window frame (aruco_slam.cpp:92-95, 192-198, 423-435 replayed on the host)
    int m;                             // corrections fused, in pop order = ascending landmark index (aruco_slam.h:85-88)
    int npop;                          // popped observations: the m corrections + the "stationary" no-ops
    int n_markers;                     // detections of the frame (statistics)
    int pad;
    unsigned char cdet[64];            // correction a: index of its detection in the frame's observation list
    unsigned char cpos[64];            // ... and the position of its landmark in S (rows 3 + 3 pos .. 5 + 3 pos of the S block)
    unsigned char pdet[64];            // popped observation i: detection index
    unsigned char pact[64];            // ... 1 = update, 2 = stationary no-op
    short pidx[64];                    // ... landmark index
};
struct WinDesc {                       // one chain piece / one window (kernel argument)
    int first_slot, K;                 // slots first_slot .. first_slot + K - 1
    int nS, T;                         // landmarks in S; MFMA tiles per side: SP = 16 T >= s = 3 + 3 nS  (T = 4, 8 or 12)
    int piece, log0;                   // index of the piece within its window; steps logged by the earlier pieces
    int last;                          // 1 = the window's last piece: mu_S goes back to the state, the last frame's pop list / last-observation list are left behind
    int wpar;                          // parity of the window within its batch: which of the two P / mu hand-over images it uses
    int from_image;                    // first piece of a window whose P and mu_S were prepared in the image (k_ekf_win_next) instead of read from Sigma / mu
    int mu_out;                        // the chain writes mu_S back into the state (piece schedule: the window's last piece); otherwise k_ekf_win_fix does
    unsigned epoch;                    // one-launch window: tag of its hand-off counters (unique per window of the context, never 0)
    int nsteps;                        // one-launch window: steps of the whole window (frames + corrections)
    short li[kWinSMax + 1];            // state offset 3 + 3 index of every landmark of S, ascending
};

struct EkfState {
    int max_landmarks, ld;             // ld = 3 + 3*max_landmarks: leading dimension of sigma (column-major)
    double* d_mu;
    double* d_sigma;
    int* d_L;                          // landmarks in the map (N = 3 + 3 L)
    int* d_id2idx;
    int* d_idx2id;
    LastObs* d_last;
    LastObs* d_lastNext;               // staging of the next frame's list while the current one is still read
    int* d_nlast;
    PopRec* d_pop;
    int* d_npop;
    UpdRec* d_upd;
    int* d_m;                          // fused updates this frame
    double *d_V, *d_Wt, *d_T;          // 3m x ld each, row k contiguous
    double *d_Sv, *d_Sw, *d_alpha, *d_gamma, *d_G, *d_g;
    MapRecord* d_maprec;
    double* d_win_log;                 // per window step: operand rows -K^T (3 x SP) + header (ekf_window.hip)
    double* d_win_tlog;                // per window step: t = H Lambda and u = S^-1 t (4 x SP each, 4th row zero)
    double* d_win_small;               // two P images and mu_S images (hand-over between the pieces of a window), Lambda, Psi images (SP x SP) and psi
    double* d_win_next;                // early start of the next window, four-launch path only (ASLAM_WIN_NEXT_SPLIT): Y_0 columns S' (Vg), Psi Vg, Lambda Vg, Sigma[S',S'] (each SPm x SPm)
    int* d_win_next_idx;               // ... position in the previous S of every entry of S' (or -1), and nS' (at [SPm])
    int* d_win_sidx;                   // per state index: position in S or -1
    WinFrame* d_win_frames;            // per staged slot: the host's plan of the frame
    int win_sp_max, win_steps_max;     // capacity: largest SP and most steps (frames + corrections) per window
    unsigned long long* d_win_sync;    // one-launch window: kWinSyncCounters hand-off counters, kWinSyncLine words apart ({epoch, count})
    unsigned* d_win_err;               // one-launch window: non-zero = a workgroup gave up waiting (1: replay on the chain, 2: Psi on the replay)
    int* d_slot_stat;                  // per staged slot, written by k_ekf_plan: detections, augments, fused updates, stationary no-ops
    int max_slots;
};

hipError_t ekf_alloc(EkfState& E, int max_landmarks, int max_slots, int max_updates_per_frame);
void ekf_free(EkfState& E);
void launch_ekf_predict_only(hipStream_t st, const EkfState& E, const SlamParams& sp, double wl, double wr, double dt);
void launch_ekf_plan(hipStream_t st, const EkfState& E, const SlamParams& sp, double wl, double wr, double dt, int do_predict,
                     const ObsRaw* obs, const unsigned* n_markers, Counters* ctr, int max_m, int slot);
struct SlamGateArg;                    // below: the SLAM gate of a launch; nullptr = the ungated kernel.  consistent: the RunningMean solve
void launch_ekf_mid(hipStream_t st, const EkfState& E, const SlamGateArg* gate = nullptr, bool consistent = false);
void launch_ekf_apply(hipStream_t st, const EkfState& E);
int ekf_fast_max_updates();
int ekf_mid_max_updates();
void launch_ekf_mid64(hipStream_t st, const EkfState& E, const SlamGateArg* gate = nullptr, bool consistent = false);
void launch_ekf_update_mfma(hipStream_t st, const EkfState& E, int depth = -1);   // depth >= 0: rows of d_T / d_Wt to contract instead of 3 * *d_m
void launch_ekf_gather(hipStream_t st, const EkfState& E);
void launch_ekf_small(hipStream_t st, const EkfState& E, const SlamGateArg* gate = nullptr, bool consistent = false);
void launch_ekf_T(hipStream_t st, const EkfState& E);
void launch_ekf_export_map(hipStream_t st, const EkfState& E);
// innovation gate of the localization steps (ekf_localize.h): the parameters in force and where the gated kernels
// leave their records.  SlotHealth / TrackHealth have the layout of aslam_slot_health / aslam_track_health.
struct SlotHealth {                    // one gated step: what became of its prepared corrections
    int attempted, accepted, rejected, ref_flagged;
    double nis_sum, d2_max;
    int worst_id, pad;
};
struct TrackHealth {                   // one filter since it was last seated
    int frames, accepted_total, rejected_total, bad_streak, lost, pad[3];
};
constexpr int kTrackSingle = 256;      // the single filter's track record; a fleet's robot r has record r (< ASLAM_MAX_ROBOTS = 256)
struct GateState {
    double gate_d2;                    // > 0, or +inf: monitor only
    int min_attempted, min_accept_percent, lost_after;
    SlotHealth* slot;                  // per EKF slot (max_slots records)
    TrackHealth* track;                // kTrackSingle + 1 records
};
// innovation gate of the SLAM chains (ekf_slam_gate.h): the parameters and records as above, and the buffer in which
// a gated solve kernel leaves d2 and its verdict per correction for k_ekf_gate_finish (2 kMarkerMax doubles per filter of a launch)
struct SlamGateArg {
    GateState g;
    double* verdicts;
};
// behind a gated solve of the single filter's frame in EKF slot `slot`: actions, last-observed list, slot record, track record
void launch_ekf_gate_finish(hipStream_t st, const EkfState& E, const SlamGateArg& gate, int slot);
// uncertain map of the localization steps (ekf_localize.h): the landmarks' fixed covariance blocks and, for a fleet,
// the robots' pose <-> landmark cross strips.  The single filter's strip lives in Sigma itself (rows 0..2, mirrored into columns 0..2).
struct MapCov {
    const double* C;                   // L x 9: block C_i of landmark index i, row-major, symmetric
    double* cross;                     // fleet: robot r's strip Sigma_xl (3 x 3L row-major) at cross + 9 L r; nullptr for the single filter
    int L;                             // landmarks of the map
};
// localization steps of EKF slots [first, first + count) in one launch (ekf_localize.h): the map stays frozen, only the pose block
// is corrected; predict_first = 0: the first slot's encoder sample only arms the filter (or came with aslam_add_encoder).
// gate, umap and consistent choose the instantiation of k_loc_steps<G, M, C> / k_fleet_steps<G, M, C>.  gate != nullptr: the Gated
// kernels with those parameters; umap != nullptr: the Schmidt-Kalman kernels (UncertainMap) on that map
void launch_loc_steps(hipStream_t st, const EkfState& E, const SlamParams& sp, const ObsRaw* obs, const unsigned* n_markers,
                      const double* enc, int first, int count, int predict_first, const GateState* gate = nullptr, const MapCov* umap = nullptr,
                      bool consistent = false);   // consistent: the RunningMean kernels
void launch_umap_clear_cross(hipStream_t st, const EkfState& E, int L);   // the single filter's Sigma_xl := 0 (a seat of its pose)
// fleet localization (ekf_fleet.h): one workgroup per robot of the work list (n_groups robots), each on its own filter in F
constexpr int kFleetState = 12;        // doubles per robot: mu_x (3), then Sigma_xx row-major (9)
struct FleetState {
    double* pose;                      // R x kFleetState
    LastObs* last;                     // R x kMarkerMax: each robot's last_observed_marker_
    int* nlast;                        // R: their lengths
};
void launch_fleet_steps(hipStream_t st, const EkfState& E, const FleetState& F, const SlamParams& sp, const ObsRaw* obs,
                        const unsigned* n_markers, const double* enc, const int* work, int n_groups, const GateState* gate = nullptr,
                        const MapCov* umap = nullptr, bool consistent = false);
// fleet SLAM (ekf_fleet_slam.h): R complete filters with the single filter's chain layouts in one allocation; robot r's buffers lie
// r * stride bytes past robot 0's.  No window buffers; d_slot_stat and max_slots are the context's.
struct FleetSlam {
    EkfState base;                     // robot 0's filter
    size_t stride;                     // bytes from one robot's buffers to the next one's
    void* mem;                         // the allocation (nullptr: none)
    int n;                             // robots
};
hipError_t ekf_fleet_alloc(FleetSlam& F, int n_robots, const EkfState& single);
void ekf_fleet_free(FleetSlam& F);
EkfState ekf_fleet_robot(const FleetSlam& F, int robot);   // robot's filter (device pointers)
// one round of a fleet SLAM call: n robots, one frame each, robot k = workgroups with blockIdx.z = k.  work: n device rows
// {robot, slot, predict, 0}; enc: the context's per-slot encoder samples.  The launchers below run the per-frame chain's kernels in
// their fleet instantiation with the single filter's grids in x / y.
struct FleetRound {
    FleetSlam F;
    const int* work;
    const double* enc;
    int n;
};
void launch_ekf_plan(hipStream_t st, const FleetRound& R, const SlamParams& sp, const ObsRaw* obs, const unsigned* n_markers, Counters* ctr, int max_m);
void launch_ekf_mid(hipStream_t st, const FleetRound& R, const SlamGateArg* gate = nullptr, bool consistent = false);
void launch_ekf_apply(hipStream_t st, const FleetRound& R);
void launch_ekf_mid64(hipStream_t st, const FleetRound& R, const SlamGateArg* gate = nullptr, bool consistent = false);
void launch_ekf_update_mfma(hipStream_t st, const FleetRound& R);
void launch_ekf_gather(hipStream_t st, const FleetRound& R);
void launch_ekf_small(hipStream_t st, const FleetRound& R, const SlamGateArg* gate = nullptr, bool consistent = false);
void launch_ekf_gate_finish(hipStream_t st, const FleetRound& R, const SlamGateArg& gate, int slot = 0);   // every robot of the round; slot: unused (the work list's)
void launch_ekf_T(hipStream_t st, const FleetRound& R);
// map merge (fleet_merge.h): n_maps <= kMergeMaxMaps maps of per_map MapRecord records each, aligned
// into the anchor map's frame and fused per marker id.  The tables are one allocation made on first use (merge_alloc); rec is the
// context's own record buffer (host records uploaded, or a fleet's export), grown on demand.
constexpr int kMergeMaxMaps = 256;
struct MergeBufs {
    int* index;                        // n_maps x kIdTableSize: position of the id's record in its map, or -1
    int* present;                      // reference table, per id: 1 = has a mean
    double* mean;                      // ... (x, y, theta) in the anchor frame
    int* round;                        // per map: round it was aligned in (0 the anchor, -1 not aligned)
    double* T;                         // per map: (t_x, t_y, phi) into the anchor frame
    int* aligned;                      // maps aligned so far
    int* out_n;                        // ids in the table = output entries
    int *out_ids, *out_seen;           // per output entry, ascending id: marker id, contributions fused
    double *out_xyth, *out_sigma;      // ... mean (3) and covariance (9, row-major)
    void* mem;                         // the allocation holding the tables above (nullptr: none), in the order above
    size_t mem_bytes;
    char* h_out;                       // page-locked copy of the allocation's tail, round ... out_sigma: what a merge returns
    size_t out_bytes;
    int* h_aligned;                    // page-locked word *aligned is read back into after every round
    MapRecord* rec;
    size_t rec_cap;                    // records rec holds
};
hipError_t merge_alloc(MergeBufs& M);
void merge_free(MergeBufs& M);
hipError_t merge_reserve_records(MergeBufs& M, size_t count);
void launch_fleet_export_maps(hipStream_t st, const FleetSlam& F, MapRecord* out);   // F.n x max_landmarks records, robot-major
// the whole merge of rec (device) on st; waits for st once per round and leaves the results in M.out_* (enqueued, not waited for);
// *rounds = alignment rounds run
hipError_t merge_run(hipStream_t st, const MergeBufs& M, const MapRecord* rec, int n_maps, int per_map, int anchor, int min_common,
                     int* rounds);
// map edit (map_edit.h): landmarks removed from n filters in place, filter k = robot[k] of a SLAM fleet (base, stride
// as in FleetSlam) or the single filter (n = 1, stride 0, robot[0] = 0).  The tables are made on first use: per filter of a call
// src_of (ld entries: new state index -> old state index) and a meta row {N before, N after, landmarks removed, 0}.
constexpr int kMapEditMaxFilters = 256;
struct MapEdit {                       // kernel argument of the three map-edit kernels
    EkfState base;                     // robot 0's filter, or the single filter
    size_t stride;
    int n;                             // filters of the call = gridDim.z
    unsigned ids[kIdTableSize / 32];   // bit id set: landmarks with this marker id go
    unsigned char robot[kMapEditMaxFilters];
    int* src_of;
    int* meta;
};
struct MapEditBufs {
    int* src_of;                       // cap x ld
    int* meta;                         // cap x 4
    int* h_meta;                       // page-locked copy of meta: what a call reads back
    int cap;                           // filters the tables hold (0: none)
};
hipError_t map_edit_reserve(MapEditBufs& B, int filters, int ld);
void map_edit_free(MapEditBufs& B);
void launch_map_plan(hipStream_t st, const MapEdit& J);
void launch_map_cols(hipStream_t st, const MapEdit& J);
void launch_map_rows(hipStream_t st, const MapEdit& J);
// landmark confirmation (landmark_confirm.h): a filter on the observation lists of EKF slots, in front of everything
// that reads them.  One table per SLAM filter (robot r's at tables[r], the single filter's at tables[kConfirmSingle]) and one record
// per EKF slot, in device buffers made by the first aslam_set_landmark_confirmation.  SlotConfirm has the layout of aslam_slot_confirm.
constexpr int kConfirmSingle = 256;    // the single filter's table follows the robots' (< ASLAM_MAX_ROBOTS = 256)
struct ConfirmTable {
    int cnt[kIdTableSize];             // per marker id: sightings of the running tentative count, or -1 = confirmed
    int last[kIdTableSize];            // ... the filter's frame counter at its last counted sighting
    int t, pad[3];                     // the filter's frame counter
};
struct SlotConfirm {
    int judged, tentative, withheld, promoted;
    unsigned withheld_mask[4];
};
struct ConfirmArg {                    // kernel argument of k_confirm: workgroup blockIdx.z is one filter of the launch
    ConfirmTable* tables;
    const int* work;                   // a fleet round's rows {robot, slot, predict, 0}: filter k = robot work[4 k] on slot work[4 k + 1];
    int first, count;                  // nullptr: the single filter on EKF slots [first, first + count), ascending
    int min_sightings, max_gap;
    ObsRaw* obs;                       // the context's per-slot lists and their lengths
    const unsigned* n_markers;
    SlotConfirm* rec;                  // per EKF slot
};
struct ConfirmReseed {                 // kernel argument of k_confirm_reseed: filter k = robot[k] of a SLAM fleet, or the single filter
    EkfState base;                     // robot 0's filter, or the single filter
    size_t stride;                     // as in FleetSlam (0 for the single filter)
    ConfirmTable* tables;
    int n, single;                     // filters of the call = gridDim.z; single: filter 0 is the single filter (table kConfirmSingle)
    unsigned char robot[256];
};
void launch_confirm(hipStream_t st, const ConfirmArg& A, int filters);
void launch_confirm_reseed(hipStream_t st, const ConfirmReseed& A);
// relocalization (relocalize.h): per slot of a call one 128-byte result record (16 doubles: the five counts as int32
// in the first four, then pose and covariance), in a device buffer made on first use together with its page-locked copy
struct RelocParams {
    double tol_xy2, tol_th;            // tol_xy squared; heading tolerance
    int min_inliers;
};
struct RelocRecord {
    int status, n_candidates, n_inliers, runner_up, best, pad[3];
    double pose[3];
    double sigma[9];                   // row-major
};
struct RelocBufs {
    RelocRecord* d;                    // one record per slot of a call (nullptr: none)
    RelocRecord* h;                    // page-locked: what a call reads back
    int cap;                           // records each holds
};
hipError_t reloc_alloc(RelocBufs& B, int slots);
void reloc_free(RelocBufs& B);
// slots [first, first + count), workgroup i on slot first + i, its record out[i].  robot_of_slot (device, count entries): with apply
// a solved slot seats that robot's pose block in F; nullptr: the single filter's (mu_x, Sigma_xx of E, last-observed length 0)
void launch_relocalize(hipStream_t st, const EkfState& E, const FleetState& F, const RelocParams& prm, const ObsRaw* obs,
                       const unsigned* n_markers, int first, int count, const int* robot_of_slot, int apply, RelocRecord* out);
// SLAM relocalization (slam_relocalize.h): a SLAM filter's pose from one slot's list against the filter's own map,
// with Sigma_xx' and the strip Sigma_lx' that follow to first order.  Per slot of a call one seat table, written by
// k_slam_reloc_solve and read by k_slam_reloc_seat, in a device buffer made on first use; the records are RelocBufs'.
constexpr int kSlamRelocTile = 256;    // state indices (= lanes) of a k_slam_reloc_seat workgroup
struct SlamRelocSeat {
    int n_sup, N;                      // supporters fused (0: the slot is unsolved, nothing to seat); the state size 3 + 3 L the solve saw
    double m[3];                       // the pose
    double meas[9];                    // sum_j A_j (J_j R_j J_j^T) A_j^T: the measurement term of Sigma_xx', row-major, symmetric
    int idx[kMarkerMax];               // per supporter, in list order: its landmark index
    double M[kMarkerMax][9];           // ... and M_j = Lambda^-1 C_j^-1 G_j, row-major
};
struct SlamRelocBufs {
    SlamRelocSeat* seat;               // one table per slot of a call (nullptr: none)
    int cap;
};
struct SlamReloc {                     // kernel argument of both kernels: workgroup (slot) i works on slot first + i, record out[i], seat[i]
    EkfState base;                     // the single filter, or robot 0's of a SLAM fleet
    size_t stride;                     // as in FleetSlam (0 for the single filter)
    const int* robot_of_slot;          // device, one robot per slot of the call; nullptr: the single filter
    RelocParams prm;
    const ObsRaw* obs;                 // the context's per-slot lists and their lengths
    const unsigned* n_markers;
    int first, apply;
    RelocRecord* out;
    SlamRelocSeat* seat;
};
hipError_t slam_reloc_alloc(SlamRelocBufs& B, int slots);
void slam_reloc_free(SlamRelocBufs& B);
void launch_slam_reloc_solve(hipStream_t st, const SlamReloc& A, int count);   // record (sigma left zero) and seat table of every slot
void launch_slam_reloc_seat(hipStream_t st, const SlamReloc& A, int count);    // sigma of every solved record; with apply the seat itself
inline int ekf_win_tiles(int nS) { return nS <= 20 ? 4 : nS <= 41 ? 8 : 12; }   // T for a set of nS landmarks (4, 8 or 12)
// one launch of a window: the chain of piece wd (wd.K == 0: none), the replay (scan) of piece s_*, the Psi product of piece q_*
// (nsteps == 0: none); obs / enc: the context's per-slot arrays.  launch_ekf_win_one: the whole window wd (K frames, nsteps steps,
// epoch set) in one launch, the three roles following each other through in-launch counters
// gate != nullptr: the gated instantiation, to be followed on the same stream by launch_ekf_win_gate_finish
// consistent: the RunningMean instantiation, one form per width whatever logger_parts and worker_publish say: ungated
// beside logger_parts = 3, gated beside logger_parts = 1, both with the width's default worker_publish
// logger_parts: what the chain's logger wave takes over from its prepare wave (bit 0: the log header's S^-1, bit 1: mu_S; the
// results are the same to the bit whatever it is, 0 is the comparison path)
// worker_publish: how the chain's worker waves publish the landmark rows of the step after next (bit 0: packed rows written 16
// bytes at a time, bit 1: the step table's entry read a phase ahead; the same results to the bit whatever it is, 0 is the comparison
// path, negative: the default of the window's width).  One launch: the forms are built beside logger_parts = 3, any other
// logger_parts runs the width's default
constexpr int kWinWorkerPublishAll = 3;
// the default by width (T = 4, 8, 12 tiles: 64, 128, 192 columns), from the EKF-only timings of DESIGN.md §8 "The workers' publication"
constexpr int win_worker_publish_default(int T) { return T == 4 ? 3 : T == 8 ? 1 : 2; }
void launch_ekf_win_one(hipStream_t st, const EkfState& E, const SlamParams& sp, const WinDesc& wd, const ObsRaw* obs, const double* enc,
                        const SlamGateArg* gate = nullptr, int logger_parts = 3, int worker_publish = -1, bool consistent = false);
// behind a gated window: slot records and accepted counts of its K frames, the track record, the last frame's actions and last-observed list
// consistent: behind the gated consistent window, whose headers carry e and, apart, ||ze|| for ref_flagged
void launch_ekf_win_gate_finish(hipStream_t st, const EkfState& E, const WinDesc& wd, const SlamGateArg& gate, const ObsRaw* obs, bool consistent = false);
void launch_ekf_win_step(hipStream_t st, const EkfState& E, const SlamParams& sp, const WinDesc& wd, const ObsRaw* obs, const double* enc,
                         int s_piece, int s_log0, int s_nsteps, int q_piece, int q_log0, int q_nsteps, int worker_publish = -1);
void launch_ekf_win_gather(hipStream_t st, const EkfState& E, const WinDesc& wd);               // Y_0 = rows S of Sigma, position table
// P and mu_S of the NEXT window (set nx) from the previous window's (pv) P_K, Lambda, Psi, psi, Y_0 and the not yet flushed Sigma / mu
void launch_ekf_win_next(hipStream_t st, const EkfState& E, const WinDesc& pv, const WinDesc& nx, bool split);   // split: the four-launch path (comparison)
void launch_ekf_win_flush(hipStream_t st, const EkfState& E, const WinDesc& wd);                 // thin products, Sigma pass, rows / columns of S

} // namespace aslam
