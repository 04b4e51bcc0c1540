// C-ABI of libaruco_slam_hip.so (include/aruco_slam_hip.h): context, device buffers, stream orchestration.
// Host logic only; all arithmetic of the hot path runs in the kernels of detect.hip / pose.hip / ekf.hip.
#include "common.h"
#include "detect.h"
#include "pose.h"
#include "ekf.h"
#include "win_plan.h"
#include "synth.h"
#include "../../include/aruco_slam_hip.h"
#include <string>
#include <vector>
#include <cfloat>
#include <fstream>
#include <sstream>
#include <cctype>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <dlfcn.h>
#include <cstdio>
#include <cmath>
#include <algorithm>
#include <chrono>

using namespace aslam;

namespace {

enum ProfId { P_THRESH, P_SEG, P_LINK, P_WRITE, P_QUADS, P_ASSEMBLE, P_IDENTIFY, P_POSE, P_EKF_PLAN, P_EKF_GATHER, P_EKF_SMALL,
              P_EKF_T, P_EKF_UPDATE, P_EKF_MID, P_EKF_APPLY, P_EKF_MID64, P_EKF_WIN_CHAIN, P_EKF_WIN_SCAN, P_EKF_WIN_FLUSH, P_EKF_WIN_NEXT, P_LOC_STEPS, P_FLEET_STEPS,
              P_MAP_PLAN, P_MAP_COLS, P_MAP_ROWS, P_EKF_GATE_FINISH, P_EKF_WIN_GATE_FINISH, P_SLAM_RELOC_SOLVE,
              P_SLAM_RELOC_SEAT, P_CONFIRM, P_POSE_ALT, P_POSE_COV, P_COUNT };
const char* kProfNames[P_COUNT] = {"k_threshold", "k_seg", "k_link", "k_trace_write", "k_quads", "k_assemble", "k_identify", "k_pose",
                                   "k_ekf_plan", "k_ekf_gather", "k_ekf_small", "k_ekf_T", "k_ekf_update_mfma", "k_ekf_mid", "k_ekf_apply",
                                   "k_ekf_mid64", "k_ekf_win_step", "k_ekf_win_drain", "k_ekf_win_flush", "k_ekf_win_next", "k_loc_steps",
                                   "k_fleet_steps", "k_map_plan", "k_map_cols", "k_map_rows", "k_ekf_gate_finish", "k_ekf_win_gate_finish",
                                   "k_slam_reloc_solve", "k_slam_reloc_seat", "confirm", "k_pose_alt", "k_pose_cov"};

struct ProfSpan { int id; hipEvent_t a, b; hipStream_t st; };

// Which filter the context runs.  The single filter serves Slam and Localize (aslam_localize_begin: the map is frozen, every EKF step
// is a k_loc_steps step); the two fleet modes run R robots instead.
enum class Mode { Slam, Localize, FleetLocalize, FleetSlam };

// a per-call table that goes up from page-locked memory in two alternating halves: a half is rewritten only after its copy ran
struct PinnedPair {
    int* h[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool ev_set[2] = {false, false};
    int half = 0;
};

} // namespace

struct aslam_ctx {
    aslam_init init{};
    hipStream_t stream = nullptr;         // detection + pose (batched over frames)
    hipStream_t stream_part = nullptr;    // detection beside an EKF chain: CU-masked so that part of every XCD stays free for the chain
    hipStream_t last_detect = nullptr;    // stream of the most recent detection (ordering when it changes)
    hipEvent_t ev_export[2] = {nullptr, nullptr};   // aslam_export_map_async: the records of buffer 0 / 1 are in place
    hipStream_t stream_copy = nullptr;    // host-fed stream: uploads from the pinned ring
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_det[2] = {nullptr, nullptr};   // per ring half: upload done / detection done with the slots
    bool ev_det_set[2] = {false, false}, ev_up_set[2] = {false, false};
    uint8_t* h_ring = nullptr;            // two half batches of page-locked frames
    std::vector<double> ring_enc;         // encoder samples of the half being filled
    int ring_H = 0, ring_half = 0, ring_fill = 0;
    int ring_rows = 0, ring_cols = 0, ring_channels = 0;   // the frame shape the ring was opened with: its addressing never follows
    size_t ring_fb = 0;                   // the context's live shape (bytes per frame = ring_rows * ring_cols * ring_channels)
    bool ring_acquired = false;
    hipStream_t stream_ekf = nullptr;     // EKF chain (sequential over frames); overlaps the next batch's detection
    hipEvent_t ev_detect = nullptr, ev_ekf = nullptr;
    int ekf_first = 0, ekf_count = 0;     // slots the in-flight EKF chain still reads
    std::string err;
    bool have_cam = false;
    CamParams cam{};
    SlamParams sp{};
    // camera rig (aslam_set_camera_rig): the rig calls detect C frames per step and run one EKF step on the merged list.  The EKF
    // works on slots [0, 2 max_batch): frame slots below max_batch, and the merged list of step s of a rig call that started at frame
    // slot `first` at slot max_batch + first + s (its inputs: d_obs / d_nmarkers / d_enc / h_obs / h_nm / enc_host there)
    int rig_n = 0;
    PoseCams rig{};
    bool rig_last = false;                // the last detection / EKF call was a rig call
    int rig_last_slot0 = 0, rig_last_n = 0;   // frame slot of camera 0 of its last step, cameras
    int merge_lo = 0, merge_hi = 0;       // frame slots the last merge read (its encoder samples, lists)
    std::vector<unsigned long long> slot_shape;   // per frame slot: rows, cols, channels it was staged with (rig steps must agree)

    // staged batch
    int rows = 0, cols = 0, channels = 0;
    int max_batch = 0, nwaves = 0;
    DetectCfg cfg{};
    int last_first = 0, last_count = 0;

    uint8_t* d_in = nullptr;
    uint8_t* d_gray = nullptr;
    uint8_t* d_nbr = nullptr;
    unsigned* d_starts = nullptr;          // per frame: cap_starts entries
    unsigned* d_nstarts = nullptr;
    Counters* d_ctr = nullptr;
    ContourRec* d_contours = nullptr;      // per frame: cap_contours records
    unsigned* d_ncontours = nullptr;
    unsigned* d_points = nullptr;          // per frame: cap_points packed (x, y)
    unsigned* d_npoints = nullptr;
    unsigned* d_nodeplane = nullptr;       // per frame and scale: index of a pixel's first border node (tiled like the mask planes; only entries of pixels that carry nodes are ever written or read)
    NodeRec* d_nodes = nullptr;            // per frame: cap_starts segments (k_seg)
    WriteRec* d_wlist = nullptr;           // per frame: cap_write write tickets (k_link)
    unsigned* d_nwrite = nullptr;
    unsigned* d_link_todo = nullptr;       // per frame: left to k_link_serial
    unsigned* d_pre_write = nullptr;
    unsigned* d_pre_trace = nullptr;       // ticket ranges of the work-queue kernels
    unsigned* d_pre_quads = nullptr;
    CandRec* d_cands = nullptr;
    unsigned* d_ncand = nullptr;
    FinalCand* d_finals = nullptr;
    unsigned* d_nfinal = nullptr;
    IdentWork* d_work = nullptr;
    IdentRecord* d_ident_rec = nullptr;    // k_identify_record's output, kCandMax per slot (allocated by the first aslam_debug_run_identify)
    unsigned long long* d_dict = nullptr;
    Marker* d_markers = nullptr;
    unsigned* d_nmarkers = nullptr;
    ObsRaw* d_obs = nullptr;
    double* d_enc = nullptr;          // per slot: wl, wr, dt
    std::vector<double> enc_host;
    SynthMarker* d_synth = nullptr;
    size_t in_frame_bytes = 0, pitch = 0;
    int dict_ms = 5, dict_n = 1024, dict_maxcorr = 0;
    float* d_refine_mask = nullptr;       // cornerSubPix window weights (15 x 15 at most)
    aslam_detector_params dp{};           // cv::aruco::DetectorParameters in force (defaults of 3.2.0 unless aslam_set_detector_params)
    std::vector<unsigned long long> dict_cells;   // per id: (ms+2)^2 cell image incl. border (for the renderer)

    EkfState ekf{};
    double last_time = 0;
    bool is_init = false;
    Mode mode = Mode::Slam;               // changed by enter_mode only

    // fleet localization (aslam_fleet_begin): R robots, each with its own camera and pose filter, on the frozen map in
    // the id table and the landmark rows of mu.  Device buffers are allocated by the first aslam_fleet_begin for min(max_batch, 256)
    // robots.
    int fleet_n = 0;                      // robots of the active fleet: nonzero exactly in the two fleet modes
    int fleet_cap = 0;                    // robots the device buffers hold
    std::vector<char> fleet_armed;        // per robot: its first frame has armed the filter (the next one predicts)
    FleetState fleet{};                   // poses / Sigma_xx, last_observed_marker_ lists and their lengths
    RigCam* d_fleet_cams = nullptr;       // per robot
    int* d_fleet_camidx = nullptr;        // per frame slot: the robot whose camera k_pose uses
    int* d_fleet_work = nullptr;          // the work list of a k_fleet_steps launch (ekf_fleet.h)
    PinnedPair fleet_camidx_up, fleet_work_up;   // the uploads of d_fleet_camidx / d_fleet_work
    // fleet SLAM (aslam_fleet_slam_begin): every robot a complete SLAM filter (ekf_fleet_slam.h), allocated for the R
    // requested; the cameras, armed flags and work-list buffers above serve it as they serve fleet localization
    FleetSlam fslam{};
    MergeBufs merge{};                    // map merge: tables allocated by the first merge, freed at aslam_fleet_end / aslam_destroy
    RelocBufs reloc{};                    // relocalization: result records, allocated by the first call, freed at the same two places
    SlamRelocBufs slam_reloc{};           // SLAM relocalization: seat tables, allocated by the first call, freed where reloc is
    MapEditBufs map_edit{};               // landmark removal: src_of / meta tables, allocated by the first call, freed at aslam_destroy
    // innovation gate (aslam_set_innovation_gate): off unless set; only the localization and localization-fleet steps
    // look at it.  The health records (one per EKF slot, one track record per robot and one for the single filter) and their
    // page-locked copies are made by the first aslam_set_innovation_gate and freed by aslam_destroy.
    bool gate_on = false;
    aslam_gate_params gate_prm{};
    GateState gate{};                     // the parameters in force and the device records, as the gated kernels take them
    SlotHealth* h_slot_health = nullptr;  // page-locked: 2 max_batch
    // SLAM innovation gate (aslam_set_slam_gate): a switch of its own; only the per-frame chains of SLAM, rig SLAM and
    // fleet SLAM look at it, and while it is set aslam_run_staged plans no windows (unless slam_gate_windows below keeps them).  The records are the ones above, made by whichever
    // setter runs first; the verdict buffer (2 kMarkerMax doubles per filter of a launch) is made by the first aslam_set_slam_gate.
    bool slam_gate_on = false;
    aslam_gate_params slam_gate_prm{};
    SlamGateArg slam_gate{};
    // gated windows (aslam_set_slam_gate_windows): with the SLAM gate set, windows enabled and the one-launch form in use,
    // a staged batch keeps its windows, run by the gated step kernels with k_ekf_win_gate_finish behind each.  The verdicts travel in
    // the window's log header, so the switch needs no storage of its own.
    bool slam_gate_windows = false;
    // uncertain map (aslam_localize_begin_uncertain / aslam_fleet_begin_uncertain): on exactly while the active
    // localization or localization fleet was begun with landmark covariances.  The C table (max_landmarks x 9) is made by the first
    // such begin and freed by aslam_destroy; a fleet's cross strips (R x 3 x 3n) live from its begin to aslam_fleet_end / aslam_destroy.
    bool umap_on = false;
    MapCov umap{};                        // the C table, the fleet's strips (nullptr: the single filter's strip is in Sigma), landmarks
    double* d_map_c = nullptr;
    TrackHealth* h_track_health = nullptr;   // page-locked: ASLAM_MAX_ROBOTS + 1
    // landmark confirmation (aslam_set_landmark_confirmation): off unless set; only EKF steps of SLAM filters look at it.
    // The tables (one per robot a fleet can have, then the single filter's), the per-slot records and the page-locked buffer the getters
    // read through are made by the first setter call with parameters and freed by aslam_destroy.  k_confirm runs on whichever stream
    // carries the list it judges; ev_confirm orders a launch behind the previous one when the stream changes (they share the tables).
    bool confirm_on = false;
    aslam_confirm_params confirm_prm{};
    ConfirmTable* d_confirm = nullptr;    // kConfirmSingle + 1 tables
    SlotConfirm* d_confirm_rec = nullptr; // 2 max_batch records
    char* h_confirm = nullptr;            // page-locked: one table, or 2 max_batch records
    hipEvent_t ev_confirm = nullptr;
    hipStream_t confirm_stream = nullptr; // stream of the most recent k_confirm (nullptr: none since the last full synchronisation)
    // pose ambiguity check (aslam_set_pose_ambiguity): off unless set; k_pose_alt then follows every k_pose on its
    // stream.  The records (kMarkerMax per frame slot) and slot sums are made by the first setter call with parameters and freed by
    // aslam_destroy.
    bool pose_amb_on = false;
    aslam_pose_ambiguity_params pose_amb_prm{};
    PoseAmbiguity* d_pose_amb = nullptr;        // max_batch x kMarkerMax
    SlotPoseAmbiguity* d_pose_amb_sum = nullptr;   // max_batch
    // observation covariance (aslam_set_observation_covariance): off unless set; k_pose_cov then follows every k_pose
    // on its stream, ahead of k_pose_alt.  Records and slot sums as for the ambiguity check.
    bool obs_cov_on = false;
    aslam_obs_covariance_params obs_cov_prm{};
    ObsCovariance* d_obs_cov = nullptr;         // max_batch x kMarkerMax
    SlotObsCovariance* d_obs_cov_sum = nullptr; // max_batch
    // consistent innovations (aslam_set_consistent_innovations): off unless set, kept across mode changes.  Every
    // per-frame solve and every localization step then runs in its RunningMean instantiation, and aslam_run_staged plans no windows.
    bool consistent_on = false;
    // consistent windows (aslam_set_consistent_windows): off unless set, kept across mode changes.  With it and
    // consistent_on both set, windows are planned again and their chain runs in its RunningMean instantiation (consistent_windows below)
    bool consistent_windows = false;
    // gated consistent windows (aslam_set_gated_consistent_windows): off unless set, kept across mode changes.  With the SLAM
    // gate, slam_gate_windows, consistent_on and consistent_windows all set, a staged batch keeps its windows and their chain runs gated in
    // its RunningMean instantiation (gated_consistent_windows below).  Nothing to allocate: e and ||ze|| travel in the window's log header
    bool gated_consistent_windows = false;

    // windowed EKF (ekf_window.hip): the observations of a batch come back to the host, which cuts the batch into runs of
    // frames that fuse the same landmarks; the batch's EKF work is enqueued one call later (or at the next synchronisation),
    // behind the NEXT batch's detection, so that the detection stream never waits for the host
    bool win_enabled = true;
    int win_piece = kWinChainFrames;      // frames per chain piece (ASLAM_WIN_PIECE, 1..kWinChainFrames: a test knob)
    bool win_pieces = false;              // ASLAM_WIN_PIECE set: the piece schedule (several launches per window) instead of one launch per window
    unsigned win_epoch = 0;               // one-launch windows enqueued so far: the tag of a window's hand-off counters
    bool win_no_early = false;            // ASLAM_WIN_NO_EARLY: every window waits for its own flush (test / comparison knob)
    bool win_next_split = false;          // ASLAM_WIN_NEXT_SPLIT: the early start as four launches instead of one kernel (comparison knob)
    int win_logger_parts = 3;             // ASLAM_WIN_LOGGER_PARTS: what the chain's logger wave takes over from the prepare wave (bit 0: the header's S^-1,
                                          // bit 1: mu_S; 0: the prepare wave does both, the comparison path)
    int win_worker_publish = -1;          // ASLAM_WIN_WORKER_PUBLISH: how the chain's workers publish (bit 0: packed rows, bit 1: the step table a
                                          // phase ahead; 0: the comparison path; unset: the default of each window's width)
    bool detect_wait_at_head = false;     // ASLAM_DETECT_WAIT_AT_HEAD: detection waits for EKF work on reused slots in front of its first kernel,
                                          // not in front of its first pose stage (comparison knob)
    struct Pending { bool active = false; int first = 0, count = 0, ev = 0; } pend;
    hipEvent_t ev_obs[2] = {nullptr, nullptr}, ev_idx = nullptr;
    hipStream_t stream_win = nullptr;     // scan / flush of the windows, beside the chain on stream_ekf
    hipEvent_t ev_win[64] = {};
    unsigned win_count = 0;               // windows enqueued so far (parity = which hand-over image a window uses)
    unsigned ev_win_next = 0;
    int ev_obs_next = 0;
    bool ev_idx_set = false;
    ObsRaw* h_obs = nullptr;              // pinned: max_batch x kMarkerMax
    unsigned* h_nm = nullptr;             // pinned: max_batch
    WinFrame* h_win_frames = nullptr;     // pinned: max_batch frame plans (uploaded to ekf.d_win_frames per batch)
    PlanMirror mirror;                    // host mirror of the id -> landmark table, the landmark count and last_observed_marker_, valid unless mirror_dirty
    bool mirror_dirty = true;             // the device planned frames the host could not follow: read the tables back before planning
    int ekf_lo = 0, ekf_hi = 0;           // union of the slot ranges of EKF work enqueued since the last wait on ev_ekf
    double last_timing[6] = {0, 0, 0, 0, 0, 0};   // aslam_add_image, host clock, microseconds: upload, detection enqueue, EKF enqueue, wait, read-back / checks, total
    long long plan_stats[4] = {0, 0, 0, 0};   // frames inside windows, frames on the per-frame chain, windows, frames left to the device's own plan

    // map gather over RCCL without torch (aslam_comm_*): librccl is dlopen'ed on first use
    void* comm = nullptr;
    int comm_world = 0, comm_rank = 0;
    uint8_t* d_gather = nullptr;          // world x max_landmarks records

    bool prof_on = false;
    std::vector<ProfSpan> spans;
    double prof_empty_ms = 0.0;           // what an event pair around NOTHING measures on the EKF stream (subtracted per span)
    int prof_calls[P_COUNT] = {0};
    double prof_ms[P_COUNT] = {0};
};

namespace {

int finalize_pending(aslam_ctx* c);     // defined with run_staged below

int fail(aslam_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

#define HIP_TRY(c, expr)                                                                                  \
    do {                                                                                                  \
        hipError_t e__ = (expr);                                                                          \
        if (e__ != hipSuccess) return fail((c), ASLAM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

template <class T> hipError_t dalloc(T** p, size_t count) { return hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T)); }

// the modes an entry point runs in, as a set: every mode-dependent entry point states its rule as `if (int r = allow(c, ...)) return r;`
constexpr unsigned in(Mode m) { return 1u << (int)m; }
constexpr unsigned kSlam = in(Mode::Slam), kLocalize = in(Mode::Localize), kFleetLocalize = in(Mode::FleetLocalize),
                   kFleetSlam = in(Mode::FleetSlam);
constexpr unsigned kSingle = kSlam | kLocalize, kFleet = kFleetLocalize | kFleetSlam, kAnyMode = kSingle | kFleet;

// ASLAM_OK if the context's mode is in `allowed`, else ASLAM_E_STATE and why
int allow(aslam_ctx* c, unsigned allowed) {
    const unsigned now = in(c->mode);
    if (allowed & now) return ASLAM_OK;
    const char* why;
    if ((now & kFleet) && !(allowed & kFleet)) why = "a fleet is active: this call reads or writes the single filter or camera (aslam_fleet_end first)";
    else if (c->mode == Mode::FleetSlam) why = "fleet SLAM: a robot's pose is correlated with its map (aslam_fleet_set_state)";
    else if (allowed == kFleetSlam) why = "no fleet SLAM (aslam_fleet_slam_begin first)";
    else if (allowed == kLocalize) why = "not localizing (aslam_localize_begin first)";
    else if (!(allowed & kSingle)) why = "no fleet (aslam_fleet_begin first)";
    else if (allowed & kFleet) why = "localizing: one filter is active (aslam_localize_end first)";     // a call that starts a fleet
    else why = "localizing: the map is frozen (aslam_localize_end first)";
    return fail(c, ASLAM_E_STATE, why);
}

// a seat clears the track records [first, first + count) of the innovation gate (if it was ever set): at once, or behind the work
// enqueued on st
int clear_track_health(aslam_ctx* c, int first, int count, hipStream_t st = nullptr) {
    if (!c->gate.track) return ASLAM_OK;
    if (st) HIP_TRY(c, hipMemsetAsync(c->gate.track + first, 0, sizeof(TrackHealth) * count, st));
    else HIP_TRY(c, hipMemset(c->gate.track + first, 0, sizeof(TrackHealth) * count));
    return ASLAM_OK;
}

int pinned_alloc(aslam_ctx* c, PinnedPair& p, size_t n) {
    for (int h = 0; h < 2; h++) {
        HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&p.h[h]), sizeof(int) * n, hipHostMallocDefault));
        HIP_TRY(c, hipEventCreateWithFlags(&p.ev[h], hipEventDisableTiming));
    }
    return ASLAM_OK;
}

void pinned_free(PinnedPair& p) {
    for (int h = 0; h < 2; h++) {
        if (p.h[h]) hipHostFree(p.h[h]);
        if (p.ev[h]) hipEventDestroy(p.ev[h]);
    }
}

// n ints from src to d_dst on stream st, through the next half
int pinned_upload(aslam_ctx* c, PinnedPair& p, int* d_dst, const int* src, size_t n, hipStream_t st) {
    const int h = p.half;
    p.half ^= 1;
    if (p.ev_set[h]) HIP_TRY(c, hipEventSynchronize(p.ev[h]));     // the copy that last read this half ran
    std::memcpy(p.h[h], src, sizeof(int) * n);
    HIP_TRY(c, hipMemcpyAsync(d_dst, p.h[h], sizeof(int) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipEventRecord(p.ev[h], st));
    p.ev_set[h] = true;
    return ASLAM_OK;
}

// DICT_ARUCO_ORIGINAL from first principles: 5 rows x 2 id bits (MSB first) through the words
// 10000 / 10111 / 01001 / 01110 (original ArUco library).  parameters.yaml:16 selects enum 16.
void make_dict_aruco_original(std::vector<unsigned long long>& codes, std::vector<unsigned long long>& cells) {
    static const int words[4] = {0x10, 0x17, 0x09, 0x0e};
    const int n = 5;
    codes.resize(1024 * 4);
    cells.resize(1024 * 2);
    for (int id = 0; id < 1024; id++) {
        int B[5][5];
        for (int y = 0; y < n; y++) {
            int val = words[(id >> (2 * (4 - y))) & 3];
            for (int x = 0; x < n; x++) B[y][x] = (val >> (4 - x)) & 1;
        }
        unsigned long long c[4] = {0, 0, 0, 0};
        for (int row = 0; row < n; row++)
            for (int col = 0; col < n; col++) {
                c[0] = (c[0] << 1) | (unsigned)B[row][col];
                c[1] = (c[1] << 1) | (unsigned)B[col][n - 1 - row];
                c[2] = (c[2] << 1) | (unsigned)B[n - 1 - row][n - 1 - col];
                c[3] = (c[3] << 1) | (unsigned)B[n - 1 - col][row];
            }
        for (int r = 0; r < 4; r++) codes[(size_t)id * 4 + r] = c[r];
        unsigned long long lo = 0;     // 7x7 cells incl. black border, bit index = r*7 + c
        for (int row = 0; row < n; row++)
            for (int col = 0; col < n; col++)
                if (B[row][col]) lo |= 1ull << ((row + 1) * 7 + col + 1);
        cells[(size_t)id * 2] = lo;
        cells[(size_t)id * 2 + 1] = 0;
    }
}

void prof_begin(aslam_ctx* c, int id, hipStream_t st) {
    if (!c->prof_on) return;
    ProfSpan s;
    s.id = id;
    s.st = st;
    hipEventCreate(&s.a);
    hipEventCreate(&s.b);
    hipEventRecord(s.a, st);
    c->spans.push_back(s);
}
void prof_end(aslam_ctx* c) {
    if (!c->prof_on) return;
    hipEventRecord(c->spans.back().b, c->spans.back().st);
}
void prof_collect(aslam_ctx* c) {
    for (ProfSpan& s : c->spans) {
        float ms = 0;
        hipEventSynchronize(s.b);
        hipEventElapsedTime(&ms, s.a, s.b);
        c->prof_calls[s.id]++;
        c->prof_ms[s.id] += ms;
        hipEventDestroy(s.a);
        hipEventDestroy(s.b);
    }
    c->spans.clear();
}

// codes (4 rotations per id, row-major bit string, first bit most significant - the order k_identify assembles the sampled
// bits in) and the (ms+2)^2 cell image incl. the black border (renderer) from bits[n][ms*ms], 1 = white
void make_dict_from_bits(int n, int nm, const uint8_t* bits, std::vector<unsigned long long>& codes, std::vector<unsigned long long>& cells) {
    codes.assign((size_t)nm * 4, 0ull);
    cells.assign((size_t)nm * 2, 0ull);
    const int nc = n + 2;
    for (int id = 0; id < nm; id++) {
        const uint8_t* B = bits + (size_t)id * n * n;
        unsigned long long c[4] = {0, 0, 0, 0};
        for (int row = 0; row < n; row++)
            for (int col = 0; col < n; col++) {
                c[0] = (c[0] << 1) | (unsigned)(B[row * n + col] & 1);
                c[1] = (c[1] << 1) | (unsigned)(B[col * n + (n - 1 - row)] & 1);
                c[2] = (c[2] << 1) | (unsigned)(B[(n - 1 - row) * n + (n - 1 - col)] & 1);
                c[3] = (c[3] << 1) | (unsigned)(B[(n - 1 - col) * n + row] & 1);
                if (B[row * n + col] & 1) {
                    const int bit = (row + 1) * nc + col + 1;
                    cells[(size_t)id * 2 + (bit >> 6)] |= 1ull << (bit & 63);
                }
            }
        for (int r = 0; r < 4; r++) codes[(size_t)id * 4 + r] = c[r];
    }
}

int sync_streams(aslam_ctx* c);

int configure_frames(aslam_ctx* c, int rows, int cols, int channels) {
    if (rows <= 0 || cols <= 0 || rows > c->init.max_rows || cols > c->init.max_cols || rows > 4095 || cols > 4095)
        return fail(c, ASLAM_E_INVALID, "frame size outside [1, max_rows x max_cols]");
    if (channels != 1 && channels != 3) return fail(c, ASLAM_E_INVALID, "channels must be 1 (gray) or 3 (bgr8)");
    c->rows = rows; c->cols = cols; c->channels = channels;
    DetectCfg& g = c->cfg;
    g.rows = rows; g.cols = cols;
    g.pitch = (cols + 63) / 64 * 64;
    // cv::aruco::DetectorParameters: OpenCV 3.2.0 defaults (the reference passes none, aruco_slam.cpp:313) unless replaced
    const aslam_detector_params& dp = c->dp;
    {
        // aruco.cpp::_detectInitialCandidates: nScales = (max - min) / step + 1 windows min + i step, even sizes bumped to odd
        const int ns = (dp.adaptiveThreshWinSizeMax - dp.adaptiveThreshWinSizeMin) / dp.adaptiveThreshWinSizeStep + 1;
        g.n_scales = ns;
        for (int i = 0; i < kScales; i++) {
            int win = dp.adaptiveThreshWinSizeMin + i * dp.adaptiveThreshWinSizeStep;
            if (win % 2 == 0) win++;
            g.win_r[i] = i < ns ? win / 2 : 0;
        }
    }
    g.thresh_c = (int)std::floor(dp.adaptiveThreshConstant);             // THRESH_BINARY_INV: src - mean <= -floor(C)
    g.min_perim = (int)(unsigned)(dp.minMarkerPerimeterRate * std::max(cols, rows));
    g.max_perim = (int)(unsigned)(dp.maxMarkerPerimeterRate * std::max(cols, rows));
    g.approx_rate = dp.polygonalApproxAccuracyRate;
    g.min_corner_rate = dp.minCornerDistanceRate;
    g.min_marker_dist_rate = dp.minMarkerDistanceRate;
    g.min_border_dist = dp.minDistanceToBorder;
    g.marker_size = c->dict_ms;
    g.border_bits = dp.markerBorderBits;
    g.cell_px = dp.perspectiveRemovePixelPerCell;
    g.cell_margin = (int)(dp.perspectiveRemoveIgnoredMarginPerCell * g.cell_px);
    g.max_border_err = (int)(c->dict_ms * c->dict_ms * dp.maxErroneousBitsInBorderRate);
    g.max_corr = (int)((double)c->dict_maxcorr * dp.errorCorrectionRate);
    g.n_dict = c->dict_n;
    g.min_otsu_std = dp.minOtsuStdDev;
    g.cap_starts = c->init.cap_starts_per_frame;
    g.cap_contours = c->init.cap_contours_per_frame;
    g.cap_points = c->init.cap_points_per_frame;
    g.cap_write = g.cap_points / kWriteChunk + g.cap_contours;
    return ASLAM_OK;
}

unsigned long long frame_shape(const aslam_ctx* c) { return ((unsigned long long)c->rows << 32) | ((unsigned long long)c->cols << 8) | (unsigned)c->channels; }
void note_slot_shape(aslam_ctx* c, int slot0, int n) {
    c->slot_shape.resize(c->max_batch, 0ull);
    for (int i = slot0; i < slot0 + n; i++) c->slot_shape[i] = frame_shape(c);
}

int check_slot_range(aslam_ctx* c, int first, int count) {
    if (first < 0 || count <= 0 || first + count > c->max_batch) return fail(c, ASLAM_E_INVALID, "slot range outside [0, max_batch)");
    return ASLAM_OK;
}

// Before the host rewrites the inputs of slots [slot0, slot0 + n) (frames, encoder samples, injected observations): work that
// still reads them must have finished.  A batch whose EKF work is still pending (run_staged defers it by one call) reads its
// encoder samples and observations only when it is finalised, and the chain kernels read d_enc when they run.
int quiesce_slots(aslam_ctx* c, int slot0, int n) {
    if (c->pend.active && slot0 < c->pend.first + c->pend.count && c->pend.first < slot0 + n) {
        int r = finalize_pending(c);
        if (r) return r;
    }
    if (c->ekf_count > 0 && slot0 < c->ekf_hi && c->ekf_lo < slot0 + n) {
        HIP_TRY(c, hipEventSynchronize(c->ev_ekf));
        c->ekf_count = 0;
    }
    if (c->last_detect && slot0 < c->last_first + c->last_count && c->last_first < slot0 + n) HIP_TRY(c, hipEventSynchronize(c->ev_detect));
    if (c->merge_hi > c->merge_lo && slot0 < c->merge_hi && c->merge_lo < slot0 + n) {
        HIP_TRY(c, hipEventSynchronize(c->ev_detect));     // a rig merge still reads these slots' lists / encoder samples
        c->merge_hi = c->merge_lo;
    }
    return ASLAM_OK;
}

// the single-camera configuration as a camera table: aslam_set_camera's intrinsics, mounted at (r2c.x, r2c.y) looking forward
PoseCams single_camera(const aslam_ctx* c) {
    PoseCams pc{};
    pc.n = 1;
    pc.e[0].cam = c->cam;
    pc.e[0].mx = c->sp.r2c_tx; pc.e[0].my = c->sp.r2c_ty;
    pc.e[0].cpsi = 1.0; pc.e[0].spsi = 0.0; pc.e[0].psi = 0.0;
    return pc;
}

// What a staged or one-shot call runs: detection + pose over frame slots [first, first + count), then `steps` filter steps on EKF slots
// [ekf_first, ekf_first + steps).  The camera source and the filter go together: the single camera and filter; a rig (frame first + i is
// camera i % rig->n, step s is EKF slot max_batch + first + s: its frames' merged lists); or a fleet (frame first + i is robot robots[i]'s,
// host array of count entries).
struct Call {
    int first, count;
    const PoseCams* rig;
    const int* robots;
    int ekf_first, steps;
};
Call single_call(int first, int count) { return {first, count, nullptr, nullptr, first, count}; }
Call rig_call(const aslam_ctx* c, int first, int n_steps) { return {first, n_steps * c->rig_n, &c->rig, nullptr, c->max_batch + first, n_steps}; }
Call fleet_call(int first, int count, const int* robots) { return {first, count, nullptr, robots, first, count}; }

// frames per launch of the detection kernels: everything of the call at once (the work queues balance it) unless
// ASLAM_DETECT_CHUNK asks for smaller sub-batches (an experiment knob: mask planes of fewer frames stay cache-resident
// between k_threshold and k_trace, at the price of one longest-walk tail per sub-batch)
int detect_chunk() {
    static const int chunk_env = [] { const char* e = std::getenv("ASLAM_DETECT_CHUNK"); return e ? std::max(1, std::atoi(e)) : 0; }();
    return chunk_env > 0 ? std::min(chunk_env, max_frames_per_call()) : max_frames_per_call();
}

// k_pose over frames [f0, f0 + nf) of call k, on stream st (a fleet's camera indices are already on the stream), and behind it
// k_pose_cov while the observation covariance is set and k_pose_alt while the pose ambiguity check is set
void launch_pose_stage(aslam_ctx* c, const Call& k, hipStream_t st, int f0, int nf, const RefineCfg& rf) {
    prof_begin(c, P_POSE, st);
    if (k.robots) {
        launch_pose_table(st, nf, c->d_finals + (size_t)f0 * kCandMax, c->d_nfinal + f0, c->d_markers + (size_t)f0 * kMarkerMax,
                          c->d_nmarkers + f0, c->d_obs + (size_t)f0 * kMarkerMax, c->d_fleet_cams, c->d_fleet_camidx + f0, c->sp, c->d_ctr, rf);
    } else {
        PoseCams cams = k.rig ? *k.rig : single_camera(c);
        cams.cam0 = (f0 - k.first) % cams.n;
        launch_pose(st, nf, c->d_finals + (size_t)f0 * kCandMax, c->d_nfinal + f0, c->d_markers + (size_t)f0 * kMarkerMax,
                    c->d_nmarkers + f0, c->d_obs + (size_t)f0 * kMarkerMax, cams, c->sp, c->d_ctr, rf);
    }
    prof_end(c);
    if (c->obs_cov_on) {
        // R and valid of the same frames from the pose solve's Jacobian: ahead of the ambiguity check, which reads valid
        const aslam_obs_covariance_params& p = c->obs_cov_prm;
        const ObsCovArg arg{p.sigma_px, p.scale, p.floor_xy, p.floor_th, p.gate_norm, p.use_residual, 0,
                            c->d_obs_cov + (size_t)f0 * kMarkerMax, c->d_obs_cov_sum + f0};
        prof_begin(c, P_POSE_COV, st);
        if (k.robots) {
            launch_pose_cov_table(st, nf, c->d_markers + (size_t)f0 * kMarkerMax, c->d_nmarkers + f0, c->d_obs + (size_t)f0 * kMarkerMax,
                                  c->d_fleet_cams, c->d_fleet_camidx + f0, c->sp, arg);
        } else {
            PoseCams cams = k.rig ? *k.rig : single_camera(c);
            cams.cam0 = (f0 - k.first) % cams.n;
            launch_pose_cov(st, nf, c->d_markers + (size_t)f0 * kMarkerMax, c->d_nmarkers + f0, c->d_obs + (size_t)f0 * kMarkerMax, cams, c->sp, arg);
        }
        prof_end(c);
    }
    if (!c->pose_amb_on) return;
    // the ambiguity check of the same frames, with the same camera source
    const aslam_pose_ambiguity_params& p = c->pose_amb_prm;
    const PoseAmbArg arg{p.ratio, p.floor_px, p.min_dtheta, p.reject, 0, c->d_pose_amb + (size_t)f0 * kMarkerMax, c->d_pose_amb_sum + f0};
    prof_begin(c, P_POSE_ALT, st);
    if (k.robots) {
        launch_pose_alt_table(st, nf, c->d_markers + (size_t)f0 * kMarkerMax, c->d_nmarkers + f0, c->d_obs + (size_t)f0 * kMarkerMax,
                              c->d_fleet_cams, c->d_fleet_camidx + f0, c->sp, arg);
    } else {
        PoseCams cams = k.rig ? *k.rig : single_camera(c);
        cams.cam0 = (f0 - k.first) % cams.n;
        launch_pose_alt(st, nf, c->d_markers + (size_t)f0 * kMarkerMax, c->d_nmarkers + f0, c->d_obs + (size_t)f0 * kMarkerMax, cams, c->sp, arg);
    }
    prof_end(c);
}

// the grey frame of slot f0 a detection pass reads: a gray slot in place, a bgr8 slot as k_threshold converted it
const uint8_t* slot_gray(const aslam_ctx* c, int f0) {
    return c->channels == 1 ? c->d_in + (size_t)f0 * c->in_frame_bytes : c->d_gray + (size_t)f0 * c->rows * c->cols;
}

// k_pose's corner refinement for a launch whose first frame is slot f0 (run_detect and aslam_debug_run_pose_refined): the detector
// parameters' window, cv::cornerSubPix's iteration count (clamped to 1..100) and squared accuracy, the mask aslam_set_detector_params
// uploaded and the grey frames from slot f0 on
RefineCfg refine_cfg(const aslam_ctx* c, int f0) {
    const double eps = std::max(c->dp.cornerRefinementMinAccuracy, 0.0);
    return RefineCfg{c->dp.doCornerRefinement ? 1 : 0, c->dp.cornerRefinementWinSize, std::min(std::max(c->dp.cornerRefinementMaxIterations, 1), 100),
                     c->cfg.rows, c->cfg.cols, eps * eps, c->d_refine_mask, slot_gray(c, f0)};
}

// k_identify over the work list of the frames from f0 on (rec: k_identify_record instead, writing the records of those frames)
void launch_identify_stage(aslam_ctx* c, hipStream_t st, const DetectCfg& g, int f0, IdentRecord* rec = nullptr) {
    prof_begin(c, P_IDENTIFY, st);
    launch_identify(st, c->nwaves, g, c->d_ctr, slot_gray(c, f0), c->d_finals + (size_t)f0 * kCandMax, c->d_work, c->d_dict,
                    rec ? rec + (size_t)f0 * kCandMax : nullptr);
    prof_end(c);
}

// pitch of the cut lattice of a call of `count` frames (latency: the configuration of a one-frame call): one frame gets a finer
// lattice - its longest segment sets the latency of k_seg / k_trace_write, and the extra nodes (x 1.6) still fit k_link's LDS image
// for frames up to a megapixel or so
int cut_grid_of_call(const DetectCfg& g, int count, bool latency) {
    return (count == 1 || latency) && (size_t)g.rows * g.cols <= (size_t)1200 * 1000 ? kCutGridSingle : kCutGrid;
}

// The contour stage of frames [f0, f0 + nf) on stream st: counts cleared, k_threshold, k_prefix, k_seg, k_link, k_link_serial, k_prefix,
// k_trace_write.  g carries the call's cut lattice; lds_nodes < 0: k_link's own hand-over limit.  run_detect and
// aslam_debug_run_contours both launch it from here.
void launch_contour_stage(aslam_ctx* c, hipStream_t st, const DetectCfg& g, int f0, int nf, int lds_nodes = -1) {
    const size_t frame_px = (size_t)g.rows * g.cols;
    const bool alias_gray = c->channels == 1;              // staged gray frames are tight: the detector reads them in place
    // queue heads, work count and the per-frame list sizes of these frames, in one launch (the overflow mask is sticky)
    launch_clear_counts(st, nf, c->d_ctr, c->d_nstarts + f0, c->d_ncontours + f0, c->d_npoints + f0, c->d_nwrite + f0, c->d_ncand + f0);
    const uint8_t* in = c->d_in + (size_t)f0 * c->in_frame_bytes;
    uint8_t* nbr = c->d_nbr + (size_t)f0 * kScales * nbr_plane_bytes(g.rows, g.pitch);
    unsigned* starts = c->d_starts + (size_t)f0 * g.cap_starts;
    ContourRec* contours = c->d_contours + (size_t)f0 * g.cap_contours;
    unsigned* points = c->d_points + (size_t)f0 * g.cap_points;
    prof_begin(c, P_THRESH, st);
    launch_threshold(st, in, c->channels, c->in_frame_bytes, (size_t)g.cols * c->channels, nf,
                     alias_gray ? nullptr : c->d_gray + (size_t)f0 * frame_px, nbr, g, starts, c->d_nstarts + f0,
                     c->d_nodeplane + (size_t)f0 * kScales * nbr_plane_bytes(g.rows, g.pitch), c->d_ctr);
    prof_end(c);
    prof_begin(c, P_SEG, st);
    launch_prefix(st, nf, c->d_nstarts + f0, g.cap_starts, 1u, c->d_pre_trace);
    NodeRec* nodes = c->d_nodes + (size_t)f0 * g.cap_starts;
    WriteRec* wlist = c->d_wlist + (size_t)f0 * g.cap_write;
    launch_seg(st, c->nwaves, nbr, g, nf, starts, c->d_nstarts + f0, c->d_nodeplane + (size_t)f0 * kScales * nbr_plane_bytes(g.rows, g.pitch),
               c->d_pre_trace, c->d_ctr, nodes);
    prof_end(c);
    prof_begin(c, P_LINK, st);
    launch_link(st, g, nf, c->d_nstarts + f0, c->d_ctr, nodes, c->d_link_todo + f0, contours, c->d_ncontours + f0, c->d_npoints + f0, wlist,
                c->d_nwrite + f0, lds_nodes);
    prof_end(c);
    prof_begin(c, P_WRITE, st);
    launch_prefix(st, nf, c->d_nwrite + f0, g.cap_write, 1u, c->d_pre_write);
    launch_trace_write(st, std::max(64, c->nwaves / 4), nbr, g, nf, c->d_pre_write, c->d_ctr, contours, wlist, c->d_nwrite + f0, points);
    prof_end(c);
}

// detection + pose of the call's frames (asynchronous on the stream).  latency: the configuration of a one-frame call (one rig step)
int run_detect(aslam_ctx* c, const Call& k, bool latency, bool beside_ekf = false, hipEvent_t wait_before = nullptr) {
    const int first = k.first, count = k.count;
    if (c->rows == 0) return fail(c, ASLAM_E_STATE, "no frames staged");
    if (!k.rig && !k.robots && !c->have_cam) return fail(c, ASLAM_E_STATE, "camera parameters not set (aslam_set_camera)");
    // the CU-masked stream only pays off while an EKF chain is actually in flight beside this detection; the first batch after
    // a synchronisation gets the whole GPU
    hipStream_t st = (beside_ekf && c->stream_part && (c->ekf_count > 0 || c->pend.active)) ? c->stream_part : c->stream;
    if (c->last_detect && c->last_detect != st) HIP_TRY(c, hipStreamWaitEvent(st, c->ev_detect, 0));   // slots / work lists are shared
    c->last_detect = st;
    if (wait_before) HIP_TRY(c, hipStreamWaitEvent(st, wait_before, 0));          // frames still in flight on the copy stream
    DetectCfg g = c->cfg;
    g.cut_mask = cut_grid_of_call(g, count, latency) - 1;
    c->last_first = first;
    c->last_count = count;
    // EKF work in flight still reads observations of these slots.  Of all that detection writes, the EKF stream's kernels read d_obs
    // and d_nmarkers alone ("What the EKF stream reads of a detection"), and k_pose is the one kernel that writes them:
    // the wait stands in front of the first pose stage, so that the contour, quad and identification stages of this call run beside
    // the EKF work of the call before last.  A fleet call waits at the head (its camera-index upload comes first), and so does every
    // call under ASLAM_DETECT_WAIT_AT_HEAD, the comparison path.
    bool wait_ekf = c->ekf_count > 0 && first < c->ekf_hi && c->ekf_lo < first + count;
    if (wait_ekf) c->ekf_count = 0;
    if (wait_ekf && (k.robots || c->detect_wait_at_head)) {
        HIP_TRY(c, hipStreamWaitEvent(st, c->ev_ekf, 0));
        wait_ekf = false;
    }
    if (k.robots) {                                         // the frames' camera indices, on the stream ahead of k_pose
        int r = pinned_upload(c, c->fleet_camidx_up, c->d_fleet_camidx + first, k.robots, count, st);
        if (r) return r;
    }
    const int chunk = detect_chunk();
    for (int f0 = first; f0 < first + count; f0 += chunk) {
        const int nf = std::min(chunk, first + count - f0);
        launch_contour_stage(c, st, g, f0, nf);
        const ContourRec* contours = c->d_contours + (size_t)f0 * g.cap_contours;
        const unsigned* points = c->d_points + (size_t)f0 * g.cap_points;
        prof_begin(c, P_QUADS, st);
        launch_prefix(st, nf, c->d_ncontours + f0, g.cap_contours, 1u, c->d_pre_quads);
        launch_quads(st, c->nwaves, g, nf, c->d_ctr, contours, c->d_ncontours + f0, c->d_pre_quads, points,
                     c->d_cands + (size_t)f0 * kCandMax, c->d_ncand + f0);
        prof_end(c);
        prof_begin(c, P_ASSEMBLE, st);
        launch_assemble(st, nf, g, c->d_ctr, c->d_cands + (size_t)f0 * kCandMax, c->d_ncand + f0,
                        c->d_finals + (size_t)f0 * kCandMax, c->d_nfinal + f0, c->d_work);
        prof_end(c);
        launch_identify_stage(c, st, g, f0);
        if (wait_ekf) {                                     // (the event's record is the one the head of this call saw: nothing was enqueued since)
            HIP_TRY(c, hipStreamWaitEvent(st, c->ev_ekf, 0));
            wait_ekf = false;
        }
        launch_pose_stage(c, k, st, f0, nf, refine_cfg(c, f0));
    }
    HIP_TRY(c, hipEventRecord(c->ev_detect, st));
    HIP_TRY(c, hipGetLastError());
    return ASLAM_OK;
}

// the per-frame chain behind k_ekf_plan, sized by max_updates_per_frame: on the single filter (s = c->ekf) or on one round of a fleet
// SLAM call (s = FleetRound).  With the SLAM gate set the solve kernel is the gated one and k_ekf_gate_finish follows it (slot: the
// single filter's EKF slot; a round's slots are in its work list).
template <class S> int run_chain(aslam_ctx* c, const S& s, int slot = 0) {
    hipStream_t st = c->stream_ekf;
    const bool fast = c->init.max_updates_per_frame <= ekf_fast_max_updates();
    const SlamGateArg* gate = c->slam_gate_on ? &c->slam_gate : nullptr;
    auto finish = [&]() {
        if (!gate) return;
        prof_begin(c, P_EKF_GATE_FINISH, st);
        launch_ekf_gate_finish(st, s, *gate, slot);
        prof_end(c);
    };
    if (fast) {
        prof_begin(c, P_EKF_MID, st);
        launch_ekf_mid(st, s, gate, c->consistent_on);
        prof_end(c);
        finish();
        prof_begin(c, P_EKF_APPLY, st);
        launch_ekf_apply(st, s);
        prof_end(c);
    } else if (c->init.max_updates_per_frame <= ekf_mid_max_updates()) {
        prof_begin(c, P_EKF_MID64, st);
        launch_ekf_mid64(st, s, gate, c->consistent_on);
        prof_end(c);
        finish();
        prof_begin(c, P_EKF_T, st);
        launch_ekf_T(st, s);
        prof_end(c);
        prof_begin(c, P_EKF_UPDATE, st);
        launch_ekf_update_mfma(st, s);
        prof_end(c);
    } else {
        prof_begin(c, P_EKF_GATHER, st);
        launch_ekf_gather(st, s);
        prof_end(c);
        prof_begin(c, P_EKF_SMALL, st);
        launch_ekf_small(st, s, gate, c->consistent_on);
        prof_end(c);
        finish();
        prof_begin(c, P_EKF_T, st);
        launch_ekf_T(st, s);
        prof_end(c);
        prof_begin(c, P_EKF_UPDATE, st);
        launch_ekf_update_mfma(st, s);
        prof_end(c);
    }
    HIP_TRY(c, hipGetLastError());
    return ASLAM_OK;
}

int run_ekf_frame(aslam_ctx* c, int slot, double wl, double wr, double dt, bool do_predict) {
    hipStream_t st = c->stream_ekf;
    prof_begin(c, P_EKF_PLAN, st);
    launch_ekf_plan(st, c->ekf, c->sp, wl, wr, dt, do_predict ? 1 : 0, c->d_obs + (size_t)slot * kMarkerMax, c->d_nmarkers + slot, c->d_ctr,
                    c->init.max_updates_per_frame, slot);
    prof_end(c);
    return run_chain(c, c->ekf, slot);
}

// localization steps of EKF slots [first, first + count) on the EKF stream, behind the detection that produced their lists: one
// launch for all of them, no host round trip and no window planning
int run_loc_steps(aslam_ctx* c, int first, int count, bool predict_first) {
    hipStream_t st = c->stream_ekf;
    HIP_TRY(c, hipStreamWaitEvent(st, c->ev_detect, 0));
    prof_begin(c, P_LOC_STEPS, st);
    launch_loc_steps(st, c->ekf, c->sp, c->d_obs, c->d_nmarkers, c->d_enc, first, count, predict_first ? 1 : 0, c->gate_on ? &c->gate : nullptr,
                     c->umap_on ? &c->umap : nullptr, c->consistent_on);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    return ASLAM_OK;
}

// Landmark confirmation of a launch's filters on stream st, in front of whatever reads their slots' lists there: the
// launch follows the previous k_confirm (the filters' tables) and, on another stream than the EKF's, EKF work still reading these slots.
int launch_confirm_on(aslam_ctx* c, hipStream_t st, ConfirmArg& A, int filters, int first, int count) {
    if (c->confirm_stream && c->confirm_stream != st) HIP_TRY(c, hipStreamWaitEvent(st, c->ev_confirm, 0));
    if (st != c->stream_ekf && c->ekf_count > 0 && first < c->ekf_hi && c->ekf_lo < first + count) HIP_TRY(c, hipStreamWaitEvent(st, c->ev_ekf, 0));
    A.tables = c->d_confirm;
    A.min_sightings = c->confirm_prm.min_sightings; A.max_gap = c->confirm_prm.max_gap;
    A.obs = c->d_obs; A.n_markers = c->d_nmarkers; A.rec = c->d_confirm_rec;
    prof_begin(c, P_CONFIRM, st);
    launch_confirm(st, A, filters);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev_confirm, st));
    c->confirm_stream = st;
    return ASLAM_OK;
}

// the single SLAM filter's EKF slots [first, first + count) judged on st (nothing while the switch is off or the map is frozen)
int confirm_slots(aslam_ctx* c, hipStream_t st, int first, int count) {
    if (!c->confirm_on || c->mode != Mode::Slam) return ASLAM_OK;
    ConfirmArg A{};
    A.first = first; A.count = count;
    return launch_confirm_on(c, st, A, 1, first, count);
}

// one round of a fleet SLAM call judged on st: n robots, one slot each, rows {robot, slot, predict, 0} at d_work
int confirm_round(aslam_ctx* c, hipStream_t st, const int* d_work, int n) {
    if (!c->confirm_on) return ASLAM_OK;
    ConfirmArg A{};
    A.work = d_work;
    return launch_confirm_on(c, st, A, n, 0, 0);
}

// Reseed of n SLAM filters: the single one (robots == nullptr) or the listed robots of the SLAM fleet.  Streams
// synchronised by the caller; the tables are in place when this returns.  Nothing while the switch is off: switching it on reseeds.
int confirm_reseed(aslam_ctx* c, int n, const int* robots) {
    if (!c->confirm_on || n <= 0) return ASLAM_OK;
    ConfirmReseed A{};
    A.tables = c->d_confirm;
    A.n = n;
    if (robots) {
        A.base = c->fslam.base; A.stride = c->fslam.stride;
        for (int k = 0; k < n; k++) A.robot[k] = (unsigned char)robots[k];
    } else {
        A.base = c->ekf; A.stride = 0; A.single = 1;
    }
    launch_confirm_reseed(c->stream_ekf, A);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream_ekf));
    return ASLAM_OK;
}
int confirm_reseed_fleet(aslam_ctx* c) {
    std::vector<int> all(c->fleet_n);
    for (int r = 0; r < c->fleet_n; r++) all[r] = r;
    return confirm_reseed(c, c->fleet_n, all.data());
}

int sync_streams(aslam_ctx* c) {
    { int r = finalize_pending(c); if (r) return r; }
    if (c->stream_copy) HIP_TRY(c, hipStreamSynchronize(c->stream_copy));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->stream_part) HIP_TRY(c, hipStreamSynchronize(c->stream_part));
    HIP_TRY(c, hipStreamSynchronize(c->stream_ekf));
    if (c->stream_win) HIP_TRY(c, hipStreamSynchronize(c->stream_win));
    c->ekf_count = 0;
    c->confirm_stream = nullptr;
    return ASLAM_OK;
}

int install_dictionary(aslam_ctx* c, int ms, int n, int maxcorr, const uint8_t* bits) {
    if (ms < 3 || ms + 2 > kDictMaxCells || n < 1 || n > kIdTableSize || maxcorr < 0 || !bits)
        return fail(c, ASLAM_E_INVALID, "dictionary: marker size 3..7, 1..1024 markers (the id -> landmark table), maxCorrectionBits >= 0");
    std::vector<unsigned long long> codes;
    make_dict_from_bits(ms, n, bits, codes, c->dict_cells);
    int r = sync_streams(c);
    if (r) return r;
    unsigned long long* d_new = nullptr;
    HIP_TRY(c, dalloc(&d_new, codes.size()));
    HIP_TRY(c, hipMemcpy(d_new, codes.data(), codes.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    hipFree(c->d_dict);
    c->d_dict = d_new;
    c->dict_ms = ms; c->dict_n = n; c->dict_maxcorr = maxcorr;
    if (c->rows > 0) return configure_frames(c, c->rows, c->cols, c->channels);      // marker size / error budgets follow
    return ASLAM_OK;
}

int sync_and_check(aslam_ctx* c) {
    int rs = sync_streams(c);
    if (rs) return rs;
    prof_collect(c);
    Counters h{};
    HIP_TRY(c, hipMemcpy(&h, c->d_ctr, sizeof(h), hipMemcpyDeviceToHost));
    if (h.win_err) {
        unsigned zero = 0;
        hipMemcpy(&c->d_ctr->win_err, &zero, sizeof(unsigned), hipMemcpyHostToDevice);
        char buf[160];
        snprintf(buf, sizeof(buf), "windowed EKF: a %s workgroup of a window launch gave up waiting (code %u); the filter state is not valid",
                 h.win_err == 1 ? "replay" : "Psi", h.win_err);
        return fail(c, ASLAM_E_HIP, buf);
    }
    if (h.overflow) {
        unsigned zero = 0;
        hipMemcpy(&c->d_ctr->overflow, &zero, sizeof(unsigned), hipMemcpyHostToDevice);
        char buf[256];
        snprintf(buf, sizeof(buf), "device list overflow (mask 0x%x: 1 starts, 2 contours, 4 points, 8 candidates, 16 markers, 32 landmarks, 64 fused updates > max_updates_per_frame)", h.overflow);
        return fail(c, ASLAM_E_CAPACITY, buf);
    }
    return ASLAM_OK;
}

// the four per-step counts k_ekf_plan / the window chain left at EKF slots [slot, slot + count)
int read_ekf_stats(aslam_ctx* c, int slot, int count, int* stats) {
    { int rs = sync_streams(c); if (rs) return rs; }
    HIP_TRY(c, hipMemcpy(stats, c->ekf.d_slot_stat + (size_t)4 * slot, sizeof(int) * 4 * count, hipMemcpyDeviceToHost));
    return ASLAM_OK;
}

} // namespace

extern "C" {

void aslam_default_init(aslam_init* i) {
    std::memset(i, 0, sizeof(*i));
    i->Q_k = 0.01; i->R_x = 100; i->R_y = 100; i->R_theta = 10;          // parameters.yaml:5-8
    i->kl = 0.05; i->kr = 0.05; i->b = 0.09;                              // parameters.yaml:11-13
    i->marker_length = 0.27; i->markers_dictionary = 16;                  // parameters.yaml:16-17
    i->useful_distance_threshold = 3.0f;                                  // aruco_slam.h:58
    i->r2c_q[3] = 1.0;
    i->device_id = 0;
    i->max_landmarks = 256;
    i->max_rows = 720; i->max_cols = 1280;
    i->max_batch = 1;
    i->persistent_waves = 0;
    i->ekf_reserved_cus_per_xcd = 0;
    i->max_updates_per_frame = 24;
    i->cap_starts_per_frame = 0; i->cap_contours_per_frame = 0; i->cap_points_per_frame = 0;
}

int aslam_create(const aslam_init* init, aslam_ctx** out) {
    if (!init || !out) return ASLAM_E_INVALID;
    *out = nullptr;
    if (init->markers_dictionary != 16) return ASLAM_E_INVALID;   // only DICT_ARUCO_ORIGINAL can be generated offline
    if (init->max_rows <= 0 || init->max_cols <= 0 || init->max_batch <= 0 || init->max_landmarks <= 0) return ASLAM_E_INVALID;
    if (init->max_updates_per_frame <= 0 || init->max_updates_per_frame > kMarkerMax) return ASLAM_E_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || init->device_id >= ndev) return ASLAM_E_NO_DEVICE;
    if (hipSetDevice(init->device_id) != hipSuccess) return ASLAM_E_NO_DEVICE;
    aslam_ctx* c = new aslam_ctx();
    c->init = *init;
    // default capacity of the start-candidate list: textured / noisy frames produce a candidate every few pixels
    if (c->init.cap_starts_per_frame == 0)
        c->init.cap_starts_per_frame = std::max(1u << 16, (unsigned)((size_t)init->max_rows * init->max_cols / 2));
    if (c->init.cap_contours_per_frame == 0) c->init.cap_contours_per_frame = 1u << 12;
    if (c->init.cap_points_per_frame == 0) c->init.cap_points_per_frame = 1u << 19;
    c->max_batch = init->max_batch;
    c->nwaves = init->persistent_waves > 0 ? init->persistent_waves : 4096;
    if (init->persistent_waves <= 0) {                       // tuning knob for callers that cannot reach aslam_init (the class adapter)
        const char* e = std::getenv("ASLAM_PERSISTENT_WAVES");
        if (e && std::atoi(e) > 0) c->nwaves = std::atoi(e);
    }
    c->sp.Q_k = init->Q_k; c->sp.R_x = init->R_x; c->sp.R_y = init->R_y; c->sp.R_theta = init->R_theta;
    c->sp.kl = init->kl; c->sp.kr = init->kr; c->sp.b = init->b; c->sp.marker_length = init->marker_length;
    c->sp.r2c_tx = init->r2c_t[0]; c->sp.r2c_ty = init->r2c_t[1];
    c->sp.useful_distance_threshold = init->useful_distance_threshold;

    c->win_enabled = std::getenv("ASLAM_NO_WINDOWS") == nullptr;
    c->win_no_early = std::getenv("ASLAM_WIN_NO_EARLY") != nullptr;
    c->win_next_split = std::getenv("ASLAM_WIN_NEXT_SPLIT") != nullptr;
    if (const char* e = std::getenv("ASLAM_WIN_LOGGER_PARTS")) c->win_logger_parts = std::atoi(e) & 3;
    if (const char* e = std::getenv("ASLAM_WIN_WORKER_PUBLISH")) c->win_worker_publish = std::atoi(e) & kWinWorkerPublishAll;
    c->detect_wait_at_head = std::getenv("ASLAM_DETECT_WAIT_AT_HEAD") != nullptr;
    if (const char* e = std::getenv("ASLAM_WIN_PIECE")) { c->win_piece = std::min(kWinChainFrames, std::max(1, std::atoi(e))); c->win_pieces = true; }
    const int B = c->max_batch;
    const size_t px = (size_t)init->max_rows * init->max_cols;
    const size_t pitch = ((size_t)init->max_cols + 63) / 64 * 64;
    int prio_lo = 0, prio_hi = 0;
    hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);      // the latency-bound EKF chain outranks the batched detection
    bool ok = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_lo) == hipSuccess;
    ok = ok && hipStreamCreateWithPriority(&c->stream_ekf, hipStreamNonBlocking, prio_hi) == hipSuccess;
    {
        // Detection that runs beside an EKF chain is confined to part of every XCD (CU-masked stream), so that the chain's
        // small dependent kernels always find idle CUs.  Mask bit i is CU i / nxcd of XCD i % nxcd (MI355X: 256 CUs = 8 XCDs
        // x 32); the layout is only assumed on the device it was measured on (gfx950 with 256 CUs), elsewhere no mask is used.
        hipDeviceProp_t prop{};
        const bool known = hipGetDeviceProperties(&prop, init->device_id) == hipSuccess && prop.multiProcessorCount == 256 &&
                           std::strncmp(prop.gcnArchName, "gfx950", 6) == 0;
        const int nxcd = 8, per_xcd = 32;
        // windowed EKF: one chain workgroup, 16 scan workgroups and a tile pass per window instead of three kernels per frame
        const int res = init->ekf_reserved_cus_per_xcd == 0 ? (c->win_enabled ? 4 : 16) : init->ekf_reserved_cus_per_xcd;
        if (known && res > 0 && res < per_xcd) {
            uint32_t mask[8];
            for (int w = 0; w < 8; w++) { mask[w] = 0; for (int b = 0; b < 32; b++) if ((w * 32 + b) / nxcd >= res) mask[w] |= 1u << b; }
            if (hipExtStreamCreateWithCUMask(&c->stream_part, 8, mask) != hipSuccess) { c->stream_part = nullptr; (void)hipGetLastError(); }
        }
    }
    ok = ok && hipEventCreateWithFlags(&c->ev_detect, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->ev_ekf, hipEventDisableTiming) == hipSuccess;
    ok = ok && dalloc(&c->d_in, px * 3 * B) == hipSuccess;
    ok = ok && dalloc(&c->d_gray, px * B) == hipSuccess;
    ok = ok && dalloc(&c->d_nbr, (size_t)kScales * nbr_plane_bytes(init->max_rows, (int)pitch) * B) == hipSuccess;
    ok = ok && dalloc(&c->d_starts, (size_t)c->init.cap_starts_per_frame * B) == hipSuccess;
    ok = ok && dalloc(&c->d_nstarts, B) == hipSuccess;
    ok = ok && dalloc(&c->d_ctr, 1) == hipSuccess;
    ok = ok && dalloc(&c->d_contours, (size_t)c->init.cap_contours_per_frame * B) == hipSuccess;
    ok = ok && dalloc(&c->d_ncontours, B) == hipSuccess;
    ok = ok && dalloc(&c->d_points, (size_t)c->init.cap_points_per_frame * B) == hipSuccess;
    ok = ok && dalloc(&c->d_npoints, B) == hipSuccess;
    ok = ok && dalloc(&c->d_nodeplane, (size_t)kScales * nbr_plane_bytes(init->max_rows, (int)pitch) * B) == hipSuccess;
    ok = ok && dalloc(&c->d_nodes, (size_t)c->init.cap_starts_per_frame * B) == hipSuccess;
    ok = ok && dalloc(&c->d_wlist, ((size_t)c->init.cap_points_per_frame / kWriteChunk + c->init.cap_contours_per_frame) * B) == hipSuccess;
    ok = ok && dalloc(&c->d_nwrite, B) == hipSuccess;
    ok = ok && dalloc(&c->d_link_todo, B) == hipSuccess;
    ok = ok && dalloc(&c->d_pre_write, (size_t)max_frames_per_call() + 1) == hipSuccess;
    ok = ok && dalloc(&c->d_refine_mask, 15 * 15) == hipSuccess;
    ok = ok && dalloc(&c->d_pre_trace, (size_t)max_frames_per_call() + 1) == hipSuccess;
    ok = ok && dalloc(&c->d_pre_quads, (size_t)max_frames_per_call() + 1) == hipSuccess;
    ok = ok && dalloc(&c->d_cands, (size_t)kCandMax * B) == hipSuccess;
    ok = ok && dalloc(&c->d_ncand, B) == hipSuccess;
    ok = ok && dalloc(&c->d_finals, (size_t)kCandMax * B) == hipSuccess;
    ok = ok && dalloc(&c->d_nfinal, B) == hipSuccess;
    ok = ok && dalloc(&c->d_work, (size_t)kCandMax * B) == hipSuccess;
    ok = ok && dalloc(&c->d_markers, (size_t)kMarkerMax * B) == hipSuccess;
    ok = ok && dalloc(&c->d_nmarkers, 2 * B) == hipSuccess;              // frame slots, then the rig steps' merged lists
    ok = ok && dalloc(&c->d_obs, (size_t)kMarkerMax * 2 * B) == hipSuccess;
    ok = ok && dalloc(&c->d_enc, (size_t)3 * 2 * B) == hipSuccess;
    ok = ok && dalloc(&c->d_synth, 256) == hipSuccess;
    std::vector<unsigned long long> codes;
    aslam_default_detector_params(&c->dp);
    make_dict_aruco_original(codes, c->dict_cells);
    ok = ok && dalloc(&c->d_dict, codes.size()) == hipSuccess;
    ok = ok && hipMemcpy(c->d_dict, codes.data(), codes.size() * sizeof(unsigned long long), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemset(c->d_ctr, 0, sizeof(Counters)) == hipSuccess;
    ok = ok && hipMemset(c->d_nstarts, 0, sizeof(unsigned) * B) == hipSuccess;
    ok = ok && hipMemset(c->d_ncontours, 0, sizeof(unsigned) * B) == hipSuccess;
    ok = ok && hipMemset(c->d_npoints, 0, sizeof(unsigned) * B) == hipSuccess;
    ok = ok && hipMemset(c->d_nmarkers, 0, sizeof(unsigned) * 2 * B) == hipSuccess;
    ok = ok && hipMemset(c->d_nfinal, 0, sizeof(unsigned) * B) == hipSuccess;
    ok = ok && hipMemset(c->d_ncand, 0, sizeof(unsigned) * B) == hipSuccess;
    ok = ok && hipMemset(c->d_enc, 0, sizeof(double) * 3 * 2 * B) == hipSuccess;
    ok = ok && ekf_alloc(c->ekf, init->max_landmarks, 2 * init->max_batch, init->max_updates_per_frame) == hipSuccess;
    if (ok) c->ekf.d_win_err = &c->d_ctr->win_err;                  // read back with the call's counters (sync_and_check)
    ok = ok && hipEventCreateWithFlags(&c->ev_obs[0], hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->ev_obs[1], hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->ev_idx, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipStreamCreateWithPriority(&c->stream_win, hipStreamNonBlocking, prio_hi) == hipSuccess;
    for (int i = 0; i < 64; i++) ok = ok && hipEventCreateWithFlags(&c->ev_win[i], hipEventDisableTiming) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void**>(&c->h_obs), (size_t)2 * B * kMarkerMax * sizeof(ObsRaw), hipHostMallocDefault) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void**>(&c->h_nm), (size_t)2 * B * sizeof(unsigned), hipHostMallocDefault) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void**>(&c->h_win_frames), (size_t)2 * B * sizeof(WinFrame), hipHostMallocDefault) == hipSuccess;
    if (!ok) { aslam_destroy(c); return ASLAM_E_NO_DEVICE; }
    *out = c;
    return ASLAM_OK;
}

void aslam_destroy(aslam_ctx* c) {
    if (!c) return;
    c->pend.active = false;
    aslam_comm_destroy(c);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->stream_part) hipStreamSynchronize(c->stream_part);
    if (c->stream_ekf) hipStreamSynchronize(c->stream_ekf);
    prof_collect(c);
    hipFree(c->d_in); hipFree(c->d_gray); hipFree(c->d_nbr); hipFree(c->d_starts); hipFree(c->d_ctr);
    hipFree(c->d_refine_mask);
    hipFree(c->d_nodeplane); hipFree(c->d_nodes); hipFree(c->d_wlist); hipFree(c->d_nwrite); hipFree(c->d_link_todo); hipFree(c->d_pre_write);
    hipFree(c->d_nstarts); hipFree(c->d_ncontours); hipFree(c->d_npoints); hipFree(c->d_pre_trace); hipFree(c->d_pre_quads);
    hipFree(c->d_contours); hipFree(c->d_points); hipFree(c->d_cands); hipFree(c->d_ncand); hipFree(c->d_finals);
    hipFree(c->d_nfinal); hipFree(c->d_work); hipFree(c->d_dict); hipFree(c->d_markers); hipFree(c->d_nmarkers);
    hipFree(c->d_obs); hipFree(c->d_enc); hipFree(c->d_synth); hipFree(c->d_ident_rec);
    ekf_free(c->ekf);
    ekf_fleet_free(c->fslam);
    merge_free(c->merge);
    reloc_free(c->reloc);
    slam_reloc_free(c->slam_reloc);
    map_edit_free(c->map_edit);
    hipFree(c->d_confirm); hipFree(c->d_confirm_rec);
    if (c->h_confirm) hipHostFree(c->h_confirm);
    if (c->ev_confirm) hipEventDestroy(c->ev_confirm);
    hipFree(c->d_pose_amb); hipFree(c->d_pose_amb_sum);
    hipFree(c->d_obs_cov); hipFree(c->d_obs_cov_sum);
    if (c->umap.cross) hipFree(c->umap.cross);
    if (c->d_map_c) hipFree(c->d_map_c);
    hipFree(c->gate.slot); hipFree(c->gate.track); hipFree(c->slam_gate.verdicts);
    if (c->h_slot_health) hipHostFree(c->h_slot_health);
    if (c->h_track_health) hipHostFree(c->h_track_health);
    hipFree(c->fleet.pose); hipFree(c->fleet.last); hipFree(c->fleet.nlast);
    hipFree(c->d_fleet_cams); hipFree(c->d_fleet_camidx); hipFree(c->d_fleet_work);
    pinned_free(c->fleet_camidx_up);
    pinned_free(c->fleet_work_up);
    if (c->ev_detect) hipEventDestroy(c->ev_detect);
    if (c->ev_ekf) hipEventDestroy(c->ev_ekf);
    if (c->stream_copy) { hipStreamSynchronize(c->stream_copy); hipStreamDestroy(c->stream_copy); }
    for (int h = 0; h < 2; h++) { if (c->ev_up[h]) hipEventDestroy(c->ev_up[h]); if (c->ev_det[h]) hipEventDestroy(c->ev_det[h]); }
    for (int h = 0; h < 2; h++) if (c->ev_export[h]) hipEventDestroy(c->ev_export[h]);
    if (c->h_ring) hipHostFree(c->h_ring);
    if (c->h_obs) hipHostFree(c->h_obs);
    if (c->h_nm) hipHostFree(c->h_nm);
    if (c->h_win_frames) hipHostFree(c->h_win_frames);
    for (int h = 0; h < 2; h++) if (c->ev_obs[h]) hipEventDestroy(c->ev_obs[h]);
    if (c->ev_idx) hipEventDestroy(c->ev_idx);
    for (int i = 0; i < 64; i++) if (c->ev_win[i]) hipEventDestroy(c->ev_win[i]);
    if (c->stream_win) { hipStreamSynchronize(c->stream_win); hipStreamDestroy(c->stream_win); }
    if (c->stream) hipStreamDestroy(c->stream);
    if (c->stream_part) hipStreamDestroy(c->stream_part);
    if (c->stream_ekf) hipStreamDestroy(c->stream_ekf);
    delete c;
}

namespace {
thread_local std::string host_err;      // the last refusal of a host-only call made without a context (aslam_landmarks_from_markers)
}
const char* aslam_last_error(const aslam_ctx* c) { return c ? c->err.c_str() : (host_err.empty() ? "null context" : host_err.c_str()); }

int aslam_set_camera(aslam_ctx* c, const double K[9], const double* D, int nD) {
    if (!c || !K || nD < 0 || (nD > 0 && !D)) return fail(c, ASLAM_E_INVALID, "bad camera arguments");
    if (int r = allow(c, kSingle)) return r;
    // k_pose has the 5-coefficient plumb-bob model (k1, k2, p1, p2, k3).  A longer vector is taken only zero-padded: the reference's
    // estimatePoseSingleMarkers would use k4..k6 of the 8-coefficient rational model, which k_pose does not have.
    for (int i = 5; i < nD; i++)
        if (D[i] != 0.0) return fail(c, ASLAM_E_INVALID, "camera distortion: a coefficient after the fifth is nonzero (the rational model k4..k6 is not supported; plumb-bob k1, k2, p1, p2, k3 only)");
    c->cam.fx = K[0]; c->cam.fy = K[4]; c->cam.cx = K[2]; c->cam.cy = K[5];
    c->cam.nD = std::min(nD, 5);
    for (int i = 0; i < 5; i++) c->cam.k[i] = i < c->cam.nD ? D[i] : 0.0;
    c->have_cam = true;
    return ASLAM_OK;
}

int aslam_stage_frames(aslam_ctx* c, int slot0, const uint8_t* frames, int nframes, int rows, int cols, int channels,
                       size_t step, size_t frame_stride) {
    if (!c || !frames) return fail(c, ASLAM_E_INVALID, "null argument");
    int r = check_slot_range(c, slot0, nframes);
    if (r) return r;
    if (rows != c->rows || cols != c->cols || channels != c->channels) {
        r = configure_frames(c, rows, cols, channels);
        if (r) return r;
    }
    if (step < (size_t)cols * channels) return fail(c, ASLAM_E_INVALID, "step smaller than a row");
    r = quiesce_slots(c, slot0, nframes);
    if (r) return r;
    c->in_frame_bytes = (size_t)rows * cols * channels;
    note_slot_shape(c, slot0, nframes);
    const bool tight = step == (size_t)cols * channels;        // (a plain copy for tight rows: the 2-D path goes row by row for pageable memory)
    if (tight && (nframes == 1 || frame_stride == c->in_frame_bytes)) {
        HIP_TRY(c, hipMemcpyAsync(c->d_in + (size_t)slot0 * c->in_frame_bytes, frames, c->in_frame_bytes * nframes, hipMemcpyHostToDevice, c->stream));
    } else {
        for (int f = 0; f < nframes; f++) {
            if (tight)
                HIP_TRY(c, hipMemcpyAsync(c->d_in + (size_t)(slot0 + f) * c->in_frame_bytes, frames + (size_t)f * frame_stride, c->in_frame_bytes,
                                          hipMemcpyHostToDevice, c->stream));
            else
                HIP_TRY(c, hipMemcpy2DAsync(c->d_in + (size_t)(slot0 + f) * c->in_frame_bytes, (size_t)cols * channels,
                                            frames + (size_t)f * frame_stride, step, (size_t)cols * channels, rows,
                                            hipMemcpyHostToDevice, c->stream));
        }
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // px is borrowed for the call only
    return ASLAM_OK;
}

int aslam_stage_encoders(aslam_ctx* c, int slot0, int n, const double* wl, const double* wr, const double* dt) {
    if (!c || !wl || !wr || !dt) return fail(c, ASLAM_E_INVALID, "null argument");
    int r = check_slot_range(c, slot0, n);
    if (r) return r;
    r = quiesce_slots(c, slot0, n);              // a pending / in-flight batch still reads the samples in these slots
    if (r) return r;
    std::vector<double> h((size_t)3 * n);
    for (int i = 0; i < n; i++) { h[3 * i] = wl[i]; h[3 * i + 1] = wr[i]; h[3 * i + 2] = dt[i]; }
    HIP_TRY(c, hipMemcpy(c->d_enc + (size_t)3 * slot0, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    c->enc_host.resize((size_t)3 * 2 * c->max_batch);
    std::memcpy(&c->enc_host[(size_t)3 * slot0], h.data(), h.size() * sizeof(double));
    return ASLAM_OK;
}

void note_ekf_range(aslam_ctx* c, int first, int count) {
    if (c->ekf_count == 0) { c->ekf_lo = first; c->ekf_hi = first + count; }
    else { c->ekf_lo = std::min(c->ekf_lo, first); c->ekf_hi = std::max(c->ekf_hi, first + count); }
    c->ekf_first = first;
    c->ekf_count = count;
}

int read_mirror(aslam_ctx* c) {
    HIP_TRY(c, hipStreamSynchronize(c->stream_ekf));
    PlanMirror& M = c->mirror;
    M.id2idx.resize(kIdTableSize);
    HIP_TRY(c, hipMemcpy(M.id2idx.data(), c->ekf.d_id2idx, sizeof(int) * kIdTableSize, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(&M.L, c->ekf.d_L, sizeof(int), hipMemcpyDeviceToHost));
    int nl = 0;
    HIP_TRY(c, hipMemcpy(&nl, c->ekf.d_nlast, sizeof(int), hipMemcpyDeviceToHost));
    nl = std::min(std::max(nl, 0), (int)kMarkerMax);
    std::vector<LastObs> h(std::max(nl, 1));
    if (nl) HIP_TRY(c, hipMemcpy(h.data(), c->ekf.d_last, sizeof(LastObs) * nl, hipMemcpyDeviceToHost));
    M.last.resize(nl);
    for (int i = 0; i < nl; i++) { M.last[i].id = h[i].id; M.last[i].unconfirmed = false; for (int k = 0; k < 3; k++) M.last[i].z[k] = h[i].z[k]; }
    c->mirror_dirty = false;
    return ASLAM_OK;
}

}  // extern "C": the window launcher below is internal

namespace {
bool gated_windows(const aslam_ctx* c) { return c->slam_gate_on && c->slam_gate_windows && c->win_enabled && !c->win_pieces; }
// consistent innovations inside windows: the one-launch window with the mean on the logger wave, ungated.  A gated
// context keeps the per-frame path while consistent innovations are on, unless the gated consistent window is switched on too
bool consistent_windows(const aslam_ctx* c) {
    return c->consistent_on && c->consistent_windows && c->win_enabled && !c->win_pieces && c->win_logger_parts == 3 && !c->slam_gate_on;
}
// the gate on the running innovation inside windows: the gated one-launch window in its RunningMean instantiation, one form
// per width whatever the logger-parts and worker-publish knobs say.  Its own switch on top of the gate's and the consistent window's
bool gated_consistent_windows(const aslam_ctx* c) {
    return gated_windows(c) && c->consistent_on && c->consistent_windows && c->gated_consistent_windows;
}

hipEvent_t new_win_event(aslam_ctx* c) { return c->ev_win[c->ev_win_next++ & 63]; }

// classic order: flush, then the EKF stream goes on
int win_flush_now(aslam_ctx* c, const WinDesc& fwd) {
    hipStream_t sa = c->stream_ekf, sb = c->stream_win;
    hipEvent_t evr = new_win_event(c);
    HIP_TRY(c, hipEventRecord(evr, sa));                             // the window's replay (Lambda, Psi, psi) is complete
    HIP_TRY(c, hipStreamWaitEvent(sb, evr, 0));
    prof_begin(c, P_EKF_WIN_FLUSH, sb);
    launch_ekf_win_flush(sb, c->ekf, fwd);
    prof_end(c);
    hipEvent_t ev = new_win_event(c);
    HIP_TRY(c, hipEventRecord(ev, sb));
    HIP_TRY(c, hipStreamWaitEvent(sa, ev, 0));                       // whatever follows on the EKF stream sees the flushed Sigma
    return ASLAM_OK;
}

int win_steps(const aslam_ctx* c, int first_slot, int K) {           // steps of K window frames: one per frame and one per correction
    int n = 0;
    for (int k = 0; k < K; k++) n += 1 + c->h_win_frames[first_slot + k].m;
    return n;
}

// The whole window in one launch (ekf_window.hip: k_ekf_win_step, ONE): the chain, the replay of its log and the Psi
// product follow each other through in-launch counters.  The chain leaves mu_S in its image only: k_ekf_win_fix puts it
// back into the state, behind the previous window's flush, so the launch itself waits for nothing.
void enqueue_window_one(aslam_ctx* c, const WinOp& o, const WinDesc& wd) {
    hipStream_t sa = c->stream_ekf;
    WinDesc cw = wd;
    cw.first_slot = o.frame; cw.K = o.K; cw.piece = 0; cw.log0 = 0; cw.last = 1; cw.mu_out = 0;
    if (++c->win_epoch == 0) c->win_epoch = 1;
    cw.epoch = c->win_epoch;
    cw.nsteps = win_steps(c, o.frame, o.K);
    prof_begin(c, P_EKF_WIN_CHAIN, sa);
    const bool gated = gated_windows(c), gated_consistent = gated_consistent_windows(c);
    launch_ekf_win_one(sa, c->ekf, c->sp, cw, c->d_obs, c->d_enc, gated ? &c->slam_gate : nullptr, c->win_logger_parts, c->win_worker_publish,
                       consistent_windows(c) || gated_consistent);
    prof_end(c);
    if (gated) {                                                     // verdicts into records, counts, actions and the last-observed list
        prof_begin(c, P_EKF_WIN_GATE_FINISH, sa);
        launch_ekf_win_gate_finish(sa, c->ekf, cw, c->slam_gate, c->d_obs, gated_consistent);
        prof_end(c);
    }
}

// The pieces of the window (win_piece_sizes), back to back on the EKF stream: launch i carries the chain of piece i, the replay of
// piece i - 1 and the Psi product of piece i - 2 (ekf_window.hip: k_ekf_win_step), so nothing but the stream orders them; two more
// launches drain the replay.  What follows the window waits for that drain.
int enqueue_window_pieces(aslam_ctx* c, const WinOp& o, const WinDesc& wd, hipEvent_t ev_prev_flush) {
    hipStream_t sa = c->stream_ekf;
    struct Piece { WinDesc sub; int nsteps; };
    std::vector<Piece> pieces;
    int log0 = 0, k0 = 0;
    for (int kn : win_piece_sizes(o.K, c->win_piece)) {
        Piece pc;
        pc.sub = wd;
        pc.sub.first_slot = o.frame + k0;
        pc.sub.K = kn;
        pc.sub.piece = (int)pieces.size();
        pc.sub.log0 = log0;
        pc.sub.last = k0 + kn == o.K ? 1 : 0;
        pc.sub.mu_out = pc.sub.last;
        pc.nsteps = win_steps(c, pc.sub.first_slot, kn);
        log0 += pc.nsteps;
        k0 += kn;
        pieces.push_back(pc);
    }
    const int P = (int)pieces.size();
    for (int i = 0; i < P + 2; i++) {
        WinDesc cw = wd;
        cw.K = 0;
        if (i < P) cw = pieces[i].sub;
        const Piece* ps = (i >= 1 && i <= P) ? &pieces[i - 1] : nullptr;
        const Piece* pq = (i >= 2) ? &pieces[i - 2] : nullptr;
        if (i < P && cw.last && ev_prev_flush) HIP_TRY(c, hipStreamWaitEvent(sa, ev_prev_flush, 0));   // mu_S goes back into the state: after the previous flush's mu_R pass
        prof_begin(c, i < P ? P_EKF_WIN_CHAIN : P_EKF_WIN_SCAN, sa);
        launch_ekf_win_step(sa, c->ekf, c->sp, cw, c->d_obs, c->d_enc, ps ? ps->sub.piece : 0, ps ? ps->sub.log0 : 0, ps ? ps->nsteps : 0,
                            pq ? pq->sub.piece : 0, pq ? pq->sub.log0 : 0, pq ? pq->nsteps : 0, c->win_worker_publish);
        prof_end(c);
    }
    return ASLAM_OK;
}

// Streams: sa = the EKF stream (chain pieces with their replay, per-frame chains), sb = the window's gather and its flush.  A window
// that is followed by another window does not wait for its own flush: the next window's P and mu_S are derived from this window's
// small results (launch_ekf_win_next, on sa) while the pass over Sigma runs on sb; only the next window's LAST piece (which writes
// mu back) and whatever is not a window wait for the flush.
int enqueue_plan(aslam_ctx* c, const std::vector<WinOp>& ops) {
    hipStream_t sa = c->stream_ekf, sb = c->stream_win;
    struct { bool active = false; WinDesc wd{}; hipEvent_t ev_flush = nullptr; } pf;   // the previous window's flush, not yet enqueued (and its predecessor's flush)
    for (size_t oi = 0; oi < ops.size(); oi++) {
        const WinOp& o = ops[oi];
        if (o.K == 0) {
            if (pf.active) { int r = win_flush_now(c, pf.wd); if (r) return r; pf.active = false; }
            const double* e = &c->enc_host[(size_t)3 * o.frame];
            int r = run_ekf_frame(c, o.frame, e[0], e[1], e[2], o.predict);
            if (r) return r;
            continue;
        }
        // One window = K frames on the set S: its chain on sa, its gather and its flush on sb
        WinDesc wd{};
        wd.nS = (int)o.S.size();
        wd.T = ekf_win_tiles(wd.nS);
        wd.wpar = (int)(c->win_count++ & 1u);
        for (int a = 0; a < wd.nS; a++) wd.li[a] = (short)(3 + 3 * o.S[a]);
        hipEvent_t ev_prev_flush = nullptr;
        if (pf.active) {
            // the previous window's mu outside its S (and P_K, mu images of this parity) are as the flush before it leaves them
            if (pf.ev_flush) HIP_TRY(c, hipStreamWaitEvent(sa, pf.ev_flush, 0));
            prof_begin(c, P_EKF_WIN_NEXT, sa);                       // (the previous window's Lambda, Psi, psi are complete: same stream)
            launch_ekf_win_next(sa, c->ekf, pf.wd, wd, c->win_next_split);
            prof_end(c);
            hipEvent_t ev_next = new_win_event(c);
            HIP_TRY(c, hipEventRecord(ev_next, sa));
            HIP_TRY(c, hipStreamWaitEvent(sb, ev_next, 0));          // the flush rewrites what launch_ekf_win_next reads (Sigma, mu, Y_0)
            prof_begin(c, P_EKF_WIN_FLUSH, sb);
            launch_ekf_win_flush(sb, c->ekf, pf.wd);
            prof_end(c);
            ev_prev_flush = new_win_event(c);
            HIP_TRY(c, hipEventRecord(ev_prev_flush, sb));
            pf.active = false;
            wd.from_image = 1;
        } else {
            hipEvent_t ev = new_win_event(c);
            HIP_TRY(c, hipEventRecord(ev, sa));
            HIP_TRY(c, hipStreamWaitEvent(sb, ev, 0));               // Sigma as the EKF stream leaves it
        }
        launch_ekf_win_gather(sb, c->ekf, wd);                       // Y_0 of this window (behind the previous window's flush: same stream)
        if (!c->win_pieces) enqueue_window_one(c, o, wd);
        else if (int r = enqueue_window_pieces(c, o, wd, ev_prev_flush)) return r;
        HIP_TRY(c, hipGetLastError());
        const bool next_is_window = oi + 1 < ops.size() && ops[oi + 1].K > 0 && !c->win_no_early;
        if (next_is_window) {
            pf.active = true; pf.wd = wd; pf.ev_flush = ev_prev_flush;
        } else {
            int r = win_flush_now(c, wd);
            if (r) return r;
        }
    }
    if (pf.active) { int r = win_flush_now(c, pf.wd); if (r) return r; }
    HIP_TRY(c, hipGetLastError());
    return ASLAM_OK;
}

// The EKF work of the pending batch: planned on the host (win_plan.h) from the observations read back from the device, then enqueued
int finalize_pending(aslam_ctx* c) {
    if (!c->pend.active) return ASLAM_OK;
    const aslam_ctx::Pending p = c->pend;
    c->pend.active = false;
    HIP_TRY(c, hipEventSynchronize(c->ev_obs[p.ev]));
    if (c->mirror_dirty) { int r = read_mirror(c); if (r) return r; }
    if (c->ev_idx_set) HIP_TRY(c, hipEventSynchronize(c->ev_idx));          // the previous batch's upload has left the pinned rows
    HIP_TRY(c, hipStreamWaitEvent(c->stream_ekf, c->ev_obs[p.ev], 0));
    const PlanLimits lim{c->ekf.max_landmarks, c->init.max_updates_per_frame, win_s_cap(c->ekf.win_sp_max), c->slam_gate_on};
    const BatchPlan plan = plan_batch(c->mirror, c->is_init, c->mirror_dirty, lim, c->h_obs, c->h_nm, p.first, p.count, c->h_win_frames);
    if (plan.any_window) {                                                  // the window frames' plans: one upload per batch
        HIP_TRY(c, hipMemcpyAsync(c->ekf.d_win_frames + p.first, c->h_win_frames + p.first, (size_t)p.count * sizeof(WinFrame),
                                  hipMemcpyHostToDevice, c->stream_ekf));
        HIP_TRY(c, hipEventRecord(c->ev_idx, c->stream_ekf));
        c->ev_idx_set = true;
    }
    c->plan_stats[3] += plan.frames_left_to_device;
    for (const WinOp& o : plan.ops) {
        if (o.K == 0) c->plan_stats[1]++;
        else { c->plan_stats[0] += o.K; c->plan_stats[2]++; }
    }
    if (int r = enqueue_plan(c, plan.ops)) return r;
    HIP_TRY(c, hipEventRecord(c->ev_ekf, c->stream_ekf));
    note_ekf_range(c, p.first, p.count);
    return ASLAM_OK;
}
}  // namespace

extern "C" {

// the EKF steps of EKF slots [first, first + count) (frames, or rig steps' merged lists), behind the detection that produced them
int schedule_ekf(aslam_ctx* c, int first, int count) {
    int r = ASLAM_OK;
    if (c->mode == Mode::Localize) {           // frozen map: one k_loc_steps launch, not counted by aslam_get_plan_stats
        r = finalize_pending(c);
        if (r) return r;
        r = run_loc_steps(c, first, count, arm_filter(c->is_init));
        if (r) return r;
        HIP_TRY(c, hipEventRecord(c->ev_ekf, c->stream_ekf));
        note_ekf_range(c, first, count);
        return ASLAM_OK;
    }
    // consistent innovations: the window chain's default form makes the reference's frozen-mean corrections, so no window
    // is planned unless the consistent window (gated: §37) is switched on and can run
    if (!c->win_enabled || (c->consistent_on && !consistent_windows(c) && !gated_consistent_windows(c)) || (c->slam_gate_on && !gated_windows(c))) {  // every frame on the per-frame chain, enqueued at once
        r = finalize_pending(c);
        if (r) return r;
        // the SLAM gate: the window planner runs the "stationary" test on the host from a mirror of the last-observed
        // list, which a rejection on the device changes; the mirror is stale from here on.  Frames the device planned while the
        // consistent switch kept a window-enabled context on this path are frames the host did not follow either.
        if (c->slam_gate_on || c->consistent_on) c->mirror_dirty = true;
        HIP_TRY(c, hipStreamWaitEvent(c->stream_ekf, c->ev_detect, 0));
        r = confirm_slots(c, c->stream_ekf, first, count);
        if (r) return r;
        for (int i = 0; i < count; i++) {
            const double* e = &c->enc_host[(size_t)3 * (first + i)];
            r = run_ekf_frame(c, first + i, e[0], e[1], e[2], arm_filter(c->is_init));
            if (r) return r;
            c->plan_stats[1]++;
        }
        HIP_TRY(c, hipEventRecord(c->ev_ekf, c->stream_ekf));
        note_ekf_range(c, first, count);
        return ASLAM_OK;
    }
    // observations of the batch to the host, behind its detection; the batch's EKF work is enqueued by finalize_pending
    hipStream_t st = c->last_detect;
    const int e = c->ev_obs_next;
    c->ev_obs_next ^= 1;
    r = confirm_slots(c, st, first, count);    // the host planner and its mirror only ever see the judged lists
    if (r) return r;
    HIP_TRY(c, hipMemcpyAsync(c->h_obs + (size_t)first * kMarkerMax, c->d_obs + (size_t)first * kMarkerMax, (size_t)count * kMarkerMax * sizeof(ObsRaw),
                              hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(c->h_nm + first, c->d_nmarkers + first, (size_t)count * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipEventRecord(c->ev_obs[e], st));
    r = finalize_pending(c);                   // the PREVIOUS batch: its detection has long finished, this one's is already queued
    if (r) return r;
    c->pend.active = true; c->pend.first = first; c->pend.count = count; c->pend.ev = e;
    return ASLAM_OK;
}

namespace {
int merge_rig_steps(aslam_ctx* c, int first, int n_steps);
int run_fleet_ekf(aslam_ctx* c, int first, int count, const int* robots);

// which kind of call ran last: aslam_get_rig_observations and the single-camera message getters depend on it
void note_last_call(aslam_ctx* c, const Call& k) {
    c->rig_last = k.rig != nullptr;
    if (k.rig) { c->rig_last_slot0 = k.first + (k.steps - 1) * k.rig->n; c->rig_last_n = k.rig->n; }
}

// a staged call (aslam_run_staged, aslam_run_staged_rig, aslam_fleet_run_staged, a submit of the host-fed stream).  with_ekf: 0 detection
// only, 1 detection + EKF, 2 EKF only on the observations already in the slots; wait_before: frames still in flight on the copy stream
int run_staged(aslam_ctx* c, const Call& k, int with_ekf, hipEvent_t wait_before = nullptr) {
    int r = check_slot_range(c, k.first, k.count);
    if (r) return r;
    if (with_ekf < 0 || with_ekf > 2) return fail(c, ASLAM_E_INVALID, "with_ekf: 0, 1 or 2");
    if (k.robots)
        for (int i = 0; i < k.count; i++)
            if (k.robots[i] < 0 || k.robots[i] >= c->fleet_n) return fail(c, ASLAM_E_INVALID, "robot index outside the fleet");
    if (with_ekf && c->enc_host.size() < (size_t)3 * (k.first + k.count)) return fail(c, ASLAM_E_STATE, "encoders not staged");
    if (with_ekf != 2 && (k.rig || k.robots)) {  // (the host-fed stream's ring records no slot shapes)
        for (int i = k.first; i < k.first + k.count; i++)
            if ((int)c->slot_shape.size() <= i || c->slot_shape[i] != frame_shape(c))
                return fail(c, ASLAM_E_INVALID, "the frames of a rig or fleet call must all be staged with the same rows, cols and channels");
    }
    const aslam_ctx::Pending& p = c->pend;
    if (p.active && ((k.first < p.first + p.count && p.first < k.first + k.count) ||
                     (k.ekf_first < p.first + p.count && p.first < k.ekf_first + k.steps))) {
        r = finalize_pending(c);               // the pending batch still needs the observations in these slots
        if (r) return r;
    }
    if (with_ekf != 2) {
        r = run_detect(c, k, k.steps == 1, with_ekf == 1 && !k.robots, wait_before);   // (a fleet's steps do not take the CU-masked stream)
        if (r) return r;
    } else {                                   // EKF only: the slots' lists as if c->stream had just produced them
        if (c->last_detect && c->last_detect != c->stream) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_detect, 0));
        c->last_detect = c->stream;
        HIP_TRY(c, hipEventRecord(c->ev_detect, c->stream));
    }
    note_last_call(c, k);
    if (!with_ekf) return ASLAM_OK;
    if (k.robots) return run_fleet_ekf(c, k.first, k.count, k.robots);
    if (k.rig) {
        r = merge_rig_steps(c, k.first, k.steps);
        if (r) return r;
    }
    return schedule_ekf(c, k.ekf_first, k.steps);
}

// a one-shot call (aslam_add_image, aslam_add_images, aslam_fleet_add_images): frame i of px (rows of step[i] bytes) into slot first + i,
// with its encoder sample (wl, wr, dt) = enc[0..2][i] if enc is given; detection in the latency configuration; the EKF step(s); synchronised
// and checked, host times in last_timing.  The single filter's prediction came with aslam_add_encoder.
int add_frames(aslam_ctx* c, const Call& k, const uint8_t* const* px, int rows, int cols, int channels, const size_t* step,
               const double* const* enc = nullptr) {
    int r = finalize_pending(c);
    if (r) return r;
    if (!k.robots && !c->is_init) return ASLAM_OK;   // aruco_slam.cpp:84-85: nothing happens before the first encoder message (a robot arms on its own)
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    c->mirror_dirty = true;                  // planned on the device: the host's copy of the tables is stale afterwards
    for (int i = 0; i < k.count; i++) {
        r = aslam_stage_frames(c, k.first + i, px[i], 1, rows, cols, channels, step[i], 0);
        if (r) return r;
    }
    if (enc) {
        r = aslam_stage_encoders(c, k.first, k.count, enc[0], enc[1], enc[2]);
        if (r) return r;
    }
    const auto t1 = clk::now();
    r = run_detect(c, k, true);              // one batched pass over the call's frames
    if (r) return r;
    note_last_call(c, k);
    if (k.rig) {
        r = merge_rig_steps(c, k.first, k.steps);
        if (r) return r;
    }
    const auto t2 = clk::now();
    if (k.robots) {
        r = run_fleet_ekf(c, k.first, k.count, k.robots);
    } else if (c->mode == Mode::Localize) {
        r = run_loc_steps(c, k.ekf_first, 1, false);
    } else {
        HIP_TRY(c, hipStreamWaitEvent(c->stream_ekf, c->ev_detect, 0));
        r = confirm_slots(c, c->stream_ekf, k.ekf_first, 1);
        if (r) return r;
        r = run_ekf_frame(c, k.ekf_first, 0, 0, 0, false);
    }
    if (r) return r;
    const auto t3 = clk::now();
    r = sync_streams(c);
    const auto t4 = clk::now();
    if (!r) r = sync_and_check(c);
    const auto t5 = clk::now();
    auto us = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    c->last_timing[0] = us(t0, t1); c->last_timing[1] = us(t1, t2); c->last_timing[2] = us(t2, t3); c->last_timing[3] = us(t3, t4);
    c->last_timing[4] = us(t4, t5); c->last_timing[5] = us(t0, t5);
    return r;
}
}  // namespace

int aslam_run_staged(aslam_ctx* c, int first, int count, int with_ekf) {
    if (!c) return ASLAM_E_INVALID;
    if (int r = allow(c, with_ekf ? kSingle : kAnyMode)) return r;
    return run_staged(c, single_call(first, count), with_ekf);
}

// ---- camera rig (include/aruco_slam_hip.h): C frames per step, one batched detection pass, one EKF step per rig step ---------
namespace {
// one aslam_camera checked (nD <= 5, finite mount, heading in (-pi, pi]) and converted for k_pose
int rig_camera(aslam_ctx* c, const aslam_camera& a, RigCam& e) {
    const double PI = 3.14159265358979323846;
    if (a.nD < 0 || a.nD > 5) return fail(c, ASLAM_E_INVALID, "camera distortion: 0..5 plumb-bob coefficients");
    if (!(a.mount_yaw > -PI && a.mount_yaw <= PI) || !std::isfinite(a.mount_x) || !std::isfinite(a.mount_y))
        return fail(c, ASLAM_E_INVALID, "camera mount: finite (x, y) and a heading in (-pi, pi]");
    e.cam.fx = a.K[0]; e.cam.fy = a.K[4]; e.cam.cx = a.K[2]; e.cam.cy = a.K[5];
    e.cam.nD = a.nD;
    for (int i = 0; i < 5; i++) e.cam.k[i] = i < a.nD ? a.D[i] : 0.0;
    e.mx = a.mount_x; e.my = a.mount_y;
    e.psi = a.mount_yaw; e.cpsi = std::cos(a.mount_yaw); e.spsi = std::sin(a.mount_yaw);
    return ASLAM_OK;
}
}  // namespace

int aslam_set_camera_rig(aslam_ctx* c, int n_cams, const aslam_camera* cams) {
    if (!c) return ASLAM_E_INVALID;
    if (int r = allow(c, kSingle)) return r;
    if (n_cams < 1 || n_cams > ASLAM_MAX_CAMERAS || !cams) return fail(c, ASLAM_E_INVALID, "a rig has 1..ASLAM_MAX_CAMERAS cameras");
    if (n_cams > c->max_batch) return fail(c, ASLAM_E_INVALID, "a rig step (one frame per camera) must fit into max_batch slots");
    PoseCams pc{};
    pc.n = n_cams;
    for (int k = 0; k < n_cams; k++) {
        int r = rig_camera(c, cams[k], pc.e[k]);
        if (r) return r;
    }
    c->rig = pc;                               // taken by value at every launch: batches already submitted keep their cameras
    c->rig_n = n_cams;
    return ASLAM_OK;
}

namespace {
// the EKF slot of rig step s of a call whose frames start at slot `first`
int rig_step_slot(const aslam_ctx* c, int first, int s) { return c->max_batch + first + s; }

// observation lists of n_steps rig steps (frames from slot `first`) merged into their step slots, behind the detection on its stream
int merge_rig_steps(aslam_ctx* c, int first, int n_steps) {
    const int C = c->rig_n, e0 = rig_step_slot(c, first, 0);
    hipStream_t st = c->last_detect ? c->last_detect : c->stream;
    if (c->ekf_count > 0 && e0 < c->ekf_hi && c->ekf_lo < e0 + n_steps) HIP_TRY(c, hipStreamWaitEvent(st, c->ev_ekf, 0));   // EKF work in flight still reads these step lists
    launch_rig_merge(st, n_steps, c->d_obs, c->d_nmarkers, c->d_enc, first, C, e0, c->d_ctr);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev_detect, st));
    c->last_detect = st;
    c->merge_lo = first; c->merge_hi = first + n_steps * C;
    c->enc_host.resize((size_t)3 * 2 * c->max_batch);
    for (int s = 0; s < n_steps; s++)
        std::memcpy(&c->enc_host[(size_t)3 * (e0 + s)], &c->enc_host[(size_t)3 * (first + s * C)], 3 * sizeof(double));
    return ASLAM_OK;
}
}  // namespace

int aslam_add_images(aslam_ctx* c, int n_cams, const uint8_t* const* px, int rows, int cols, int channels, const size_t* step) {
    if (!c || !px || !step) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kSingle)) return r;
    if (c->rig_n == 0) return fail(c, ASLAM_E_STATE, "camera rig not set (aslam_set_camera_rig)");
    if (n_cams != c->rig_n) return fail(c, ASLAM_E_INVALID, "one image per camera of the rig");
    for (int k = 0; k < n_cams; k++) if (!px[k]) return fail(c, ASLAM_E_INVALID, "null image");
    return add_frames(c, rig_call(c, 0, 1), px, rows, cols, channels, step);
}

int aslam_run_staged_rig(aslam_ctx* c, int first, int n_steps, int with_ekf) {
    if (!c) return ASLAM_E_INVALID;
    if (int r = allow(c, with_ekf ? kSingle : kAnyMode)) return r;
    if (c->rig_n == 0) return fail(c, ASLAM_E_STATE, "camera rig not set (aslam_set_camera_rig)");
    if (n_steps <= 0) return fail(c, ASLAM_E_INVALID, "at least one rig step");
    return run_staged(c, rig_call(c, first, n_steps), with_ekf);
}

int aslam_get_rig_observations(aslam_ctx* c, int* n_out, int* ids, int* idx, int* action, int* cam, double* xyth, double* Rdiag) {
    if (!c || !n_out) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kSingle)) return r;
    if (!c->rig_last) return fail(c, ASLAM_E_STATE, "the last call was not a camera-rig call");
    int r = aslam_get_observations(c, n_out, ids, idx, action, xyth, Rdiag);
    if (r || !cam) return r;
    // camera of every popped observation: its position in the step's merged list against the per-camera list sizes
    const int n = *n_out, C = c->rig_last_n;
    std::vector<PopRec> h(std::max(n, 1));
    if (n) HIP_TRY(c, hipMemcpy(h.data(), c->ekf.d_pop, n * sizeof(PopRec), hipMemcpyDeviceToHost));
    std::vector<unsigned> nm(C);
    HIP_TRY(c, hipMemcpy(nm.data(), c->d_nmarkers + c->rig_last_slot0, C * sizeof(unsigned), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) {
        int k = 0, end = (int)std::min(nm[0], (unsigned)kMarkerMax);
        while (k + 1 < C && h[i].det >= end) end += (int)std::min(nm[++k], (unsigned)kMarkerMax);
        cam[i] = k;
    }
    return ASLAM_OK;
}

int aslam_get_rig_step_ekf_stats(aslam_ctx* c, int first_step, int count, int* stats) {
    if (!c || !stats) return fail(c, ASLAM_E_INVALID, "null argument");
    int r = check_slot_range(c, first_step, count);
    if (r) return r;
    return read_ekf_stats(c, rig_step_slot(c, first_step, 0), count, stats);
}

// ---- host-fed stream: pinned ring, asynchronous upload (include/aruco_slam_hip.h) --------------------------------------
namespace {
bool ring_shape_is_live(const aslam_ctx* c) {
    return c->rows == c->ring_rows && c->cols == c->ring_cols && c->channels == c->ring_channels && c->in_frame_bytes == c->ring_fb;
}

// the ring keeps the frame shape of its aslam_stream_open; a call that reconfigured the context since (aslam_stage_frames, aslam_add_image,
// aslam_detect_batch, aslam_synth_render) leaves it unusable until it is opened again: the detector would read the slots at another shape
int ring_usable(aslam_ctx* c) {
    if (!c->h_ring) return fail(c, ASLAM_E_STATE, "aslam_stream_open first");
    if (!ring_shape_is_live(c)) {
        char buf[224];
        snprintf(buf, sizeof(buf), "the frame shape changed since aslam_stream_open (ring %d x %d x %d, context %d x %d x %d): aslam_stream_open again",
                 c->ring_rows, c->ring_cols, c->ring_channels, c->rows, c->cols, c->channels);
        return fail(c, ASLAM_E_STATE, buf);
    }
    return ASLAM_OK;
}
}  // namespace

int ring_submit(aslam_ctx* c) {
    const int n = c->ring_fill, h = c->ring_half, H = c->ring_H;
    if (n == 0) return ASLAM_OK;
    const size_t fb = c->ring_fb;
    const int slot0 = h * H;
    if (c->ev_det_set[h]) HIP_TRY(c, hipStreamWaitEvent(c->stream_copy, c->ev_det[h], 0));     // the detector still reads these slots
    if (c->pend.active && slot0 < c->pend.first + c->pend.count && c->pend.first < slot0 + n) { int rp = finalize_pending(c); if (rp) return rp; }
    if (c->ekf_count > 0 && slot0 < c->ekf_hi && c->ekf_lo < slot0 + n)
        HIP_TRY(c, hipStreamWaitEvent(c->stream_copy, c->ev_ekf, 0));                          // EKF work in flight still reads these slots' encoder samples
    // the encoder samples go to the device as well: the window chain reads them there (ekf_window.hip)
    HIP_TRY(c, hipMemcpyAsync(c->d_enc + (size_t)3 * slot0, c->ring_enc.data(), (size_t)3 * n * sizeof(double), hipMemcpyHostToDevice, c->stream_copy));
    HIP_TRY(c, hipMemcpyAsync(c->d_in + (size_t)slot0 * fb, c->h_ring + (size_t)slot0 * fb, (size_t)n * fb, hipMemcpyHostToDevice, c->stream_copy));
    HIP_TRY(c, hipEventRecord(c->ev_up[h], c->stream_copy));
    c->ev_up_set[h] = true;
    c->enc_host.resize((size_t)3 * 2 * c->max_batch);
    std::memcpy(&c->enc_host[(size_t)3 * slot0], c->ring_enc.data(), (size_t)3 * n * sizeof(double));
    int r = run_staged(c, single_call(slot0, n), 1, c->ev_up[h]);
    if (r) return r;
    HIP_TRY(c, hipEventRecord(c->ev_det[h], c->last_detect));
    c->ev_det_set[h] = true;
    c->ring_half ^= 1;
    c->ring_fill = 0;
    // the other half is filled next: its previous upload must have left the pinned memory
    if (c->ev_up_set[c->ring_half]) HIP_TRY(c, hipEventSynchronize(c->ev_up[c->ring_half]));
    return ASLAM_OK;
}

int aslam_stream_open(aslam_ctx* c, int rows, int cols, int channels, int frames_per_submit) {
    if (!c) return ASLAM_E_INVALID;
    if (int r = allow(c, kSingle)) return r;
    if (frames_per_submit < 1 || 2 * frames_per_submit > c->max_batch) return fail(c, ASLAM_E_INVALID, "frames_per_submit must be in [1, max_batch / 2]");
    int r = ASLAM_OK;
    if (c->h_ring && c->ring_fill > 0) {       // committed frames of the ring that goes away: into the filter first, as aslam_stream_flush does
        if (!ring_shape_is_live(c)) {          // (at the shape they were committed with)
            r = configure_frames(c, c->ring_rows, c->ring_cols, c->ring_channels);
            if (r) return r;
            c->in_frame_bytes = c->ring_fb;
        }
        r = ring_submit(c);
        if (r) return r;
        r = sync_and_check(c);
        if (r) return r;
    }
    r = sync_streams(c);
    if (r) return r;
    r = configure_frames(c, rows, cols, channels);
    if (r) return r;
    c->in_frame_bytes = (size_t)rows * cols * channels;
    if (c->h_ring) { hipHostFree(c->h_ring); c->h_ring = nullptr; }
    c->ring_fill = 0; c->ring_acquired = false;
    HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_ring), (size_t)2 * frames_per_submit * c->in_frame_bytes, hipHostMallocDefault));
    if (!c->stream_copy) {
        HIP_TRY(c, hipStreamCreateWithFlags(&c->stream_copy, hipStreamNonBlocking));
        for (int h = 0; h < 2; h++) {
            HIP_TRY(c, hipEventCreateWithFlags(&c->ev_up[h], hipEventDisableTiming));
            HIP_TRY(c, hipEventCreateWithFlags(&c->ev_det[h], hipEventDisableTiming));
        }
    }
    c->ev_det_set[0] = c->ev_det_set[1] = c->ev_up_set[0] = c->ev_up_set[1] = false;
    c->ring_H = frames_per_submit; c->ring_half = 0;
    c->ring_rows = rows; c->ring_cols = cols; c->ring_channels = channels; c->ring_fb = c->in_frame_bytes;
    c->ring_enc.assign((size_t)3 * frames_per_submit, 0.0);
    return ASLAM_OK;
}

int aslam_stream_acquire(aslam_ctx* c, uint8_t** px, size_t* step) {
    if (!c || !px) return ASLAM_E_INVALID;
    if (int r = allow(c, kSingle)) return r;
    if (int r = ring_usable(c)) return r;
    if (!c->have_cam) return fail(c, ASLAM_E_STATE, "camera parameters not set (aslam_set_camera)");
    *px = c->h_ring + ((size_t)c->ring_half * c->ring_H + c->ring_fill) * c->ring_fb;
    if (step) *step = (size_t)c->ring_cols * c->ring_channels;
    c->ring_acquired = true;
    return ASLAM_OK;
}

int aslam_stream_commit(aslam_ctx* c, double wl, double wr, double dt) {
    if (!c) return ASLAM_E_INVALID;
    if (int r = allow(c, kSingle)) return r;
    if (!c->ring_acquired) return fail(c, ASLAM_E_STATE, "aslam_stream_acquire first");
    if (int r = ring_usable(c)) return r;
    c->ring_acquired = false;
    double* e = &c->ring_enc[(size_t)3 * c->ring_fill];
    e[0] = wl; e[1] = wr; e[2] = dt;
    if (++c->ring_fill == c->ring_H) return ring_submit(c);
    return ASLAM_OK;
}

int aslam_stream_push(aslam_ctx* c, const uint8_t* px, size_t step, double wl, double wr, double dt) {
    if (!c || !px) return ASLAM_E_INVALID;
    if (int r = allow(c, kSingle)) return r;
    const bool held = c->ring_acquired;        // a slot handed out by aslam_stream_acquire: a refused push leaves it as it was
    uint8_t* dst = nullptr;
    size_t dstep = 0;
    int r = aslam_stream_acquire(c, &dst, &dstep);
    if (r) return r;
    if (step < dstep) { c->ring_acquired = held; return fail(c, ASLAM_E_INVALID, "step smaller than a row"); }
    if (step == dstep) std::memcpy(dst, px, (size_t)c->ring_rows * dstep);
    else for (int y = 0; y < c->ring_rows; y++) std::memcpy(dst + (size_t)y * dstep, px + (size_t)y * step, dstep);
    return aslam_stream_commit(c, wl, wr, dt);
}

int aslam_stream_flush(aslam_ctx* c) {
    if (!c) return ASLAM_E_INVALID;
    if (int r = allow(c, kSingle)) return r;
    if (int r = ring_usable(c)) return r;
    int r = ring_submit(c);
    if (r) return r;
    return sync_and_check(c);
}

int aslam_sync(aslam_ctx* c) {
    if (!c) return ASLAM_E_INVALID;
    return sync_and_check(c);
}

void aslam_default_detector_params(aslam_detector_params* p) {
    if (!p) return;
    p->adaptiveThreshWinSizeMin = 3; p->adaptiveThreshWinSizeMax = 23; p->adaptiveThreshWinSizeStep = 10;
    p->adaptiveThreshConstant = 7;
    p->minMarkerPerimeterRate = 0.03; p->maxMarkerPerimeterRate = 4.0;
    p->polygonalApproxAccuracyRate = 0.05;            // 3.2.0 (0.03 from 3.3)
    p->minCornerDistanceRate = 0.05;
    p->minDistanceToBorder = 3;
    p->minMarkerDistanceRate = 0.05;
    p->doCornerRefinement = 0; p->cornerRefinementWinSize = 5; p->cornerRefinementMaxIterations = 30; p->cornerRefinementMinAccuracy = 0.1;
    p->markerBorderBits = 1;
    p->perspectiveRemovePixelPerCell = 8;             // 3.2.0 (4 from 3.3)
    p->perspectiveRemoveIgnoredMarginPerCell = 0.13;
    p->maxErroneousBitsInBorderRate = 0.35;
    p->minOtsuStdDev = 5.0;
    p->errorCorrectionRate = 0.6;
}

int aslam_set_detector_params(aslam_ctx* c, const aslam_detector_params* p) {
    if (!c || !p) return ASLAM_E_INVALID;
    {
        // the LDS tile carries a 12-pixel halo and three mask planes: up to 3 windows of at most 23 pixels
        const int step = p->adaptiveThreshWinSizeStep;
        const int ns = step > 0 && p->adaptiveThreshWinSizeMax >= p->adaptiveThreshWinSizeMin
                           ? (p->adaptiveThreshWinSizeMax - p->adaptiveThreshWinSizeMin) / step + 1 : 0;
        int last = p->adaptiveThreshWinSizeMin + (ns - 1) * step;
        if (last % 2 == 0) last++;
        if (ns < 1 || ns > kScales || p->adaptiveThreshWinSizeMin < 3 || last > 23)
            return fail(c, ASLAM_E_INVALID, "adaptive threshold windows: 1..3 sizes (min + i step) between 3 and 23 pixels");
    }
    if (p->perspectiveRemovePixelPerCell < 2 || p->perspectiveRemovePixelPerCell > kCellPx ||
        p->perspectiveRemovePixelPerCell - 2 * (int)(p->perspectiveRemoveIgnoredMarginPerCell * p->perspectiveRemovePixelPerCell) < 1)
        return fail(c, ASLAM_E_INVALID, "perspectiveRemovePixelPerCell: 2..8, with at least one pixel left inside the margin");
    if (p->markerBorderBits != 1) return fail(c, ASLAM_E_INVALID, "markerBorderBits is compiled in as 1");
    if (p->doCornerRefinement && (p->cornerRefinementWinSize < 1 || p->cornerRefinementWinSize > 7 || p->cornerRefinementMaxIterations < 1 ||
                                  !(p->cornerRefinementMinAccuracy > 0)))
        return fail(c, ASLAM_E_INVALID, "corner refinement: window 1..7, at least one iteration, positive accuracy");
    if (!(p->maxMarkerPerimeterRate > 0) || !(p->minMarkerPerimeterRate > 0) || p->minMarkerPerimeterRate > p->maxMarkerPerimeterRate ||
        p->maxMarkerPerimeterRate * std::max(c->init.max_rows, c->init.max_cols) > 65534.0)
        return fail(c, ASLAM_E_INVALID, "0 < minMarkerPerimeterRate <= maxMarkerPerimeterRate, and the longest kept border (rate x larger frame side) <= 65534 points");
    if (!(p->polygonalApproxAccuracyRate > 0) || p->minCornerDistanceRate < 0 || p->minMarkerDistanceRate < 0 || p->minDistanceToBorder < 0 ||
        p->adaptiveThreshConstant < 0 || p->adaptiveThreshConstant > 255 || p->perspectiveRemoveIgnoredMarginPerCell < 0 ||
        p->perspectiveRemoveIgnoredMarginPerCell >= 0.5 || p->maxErroneousBitsInBorderRate < 0 || p->errorCorrectionRate < 0 || p->minOtsuStdDev < 0)
        return fail(c, ASLAM_E_INVALID, "detector parameter out of range");
    int r = sync_streams(c);
    if (r) return r;
    c->dp = *p;
    if (p->doCornerRefinement) {
        // cornerSubPix's separable window (cornersubpix.cpp): float arithmetic on the host, the same libm as the CPU restatement
        const int win = p->cornerRefinementWinSize, w = 2 * win + 1;
        std::vector<float> mask((size_t)w * w);
        for (int i = 0; i < w; i++) {
            float y = (float)(i - win) / win;
            float vy = std::exp(-y * y);
            for (int j = 0; j < w; j++) {
                float x = (float)(j - win) / win;
                mask[(size_t)i * w + j] = (float)(vy * std::exp(-x * x));
            }
        }
        HIP_TRY(c, hipMemcpy(c->d_refine_mask, mask.data(), mask.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (c->rows > 0) return configure_frames(c, c->rows, c->cols, c->channels);
    return ASLAM_OK;
}

int aslam_set_dictionary(aslam_ctx* c, int marker_size, int n_markers, int max_correction_bits, const uint8_t* bits) {
    if (!c) return ASLAM_E_INVALID;
    return install_dictionary(c, marker_size, n_markers, max_correction_bits, bits);
}

int aslam_set_dictionary_bytes(aslam_ctx* c, int marker_size, int n_markers, int max_correction_bits, const uint8_t* bytes_list) {
    if (!c) return ASLAM_E_INVALID;
    if (marker_size < 3 || marker_size + 2 > kDictMaxCells || n_markers < 1 || !bytes_list)
        return fail(c, ASLAM_E_INVALID, "dictionary: marker size 3..7, at least one marker");
    // cv::aruco::Dictionary::bytesList: n rows x nbytes columns x 4 channels (rotations); channel 0 = the unrotated marker,
    // bits shifted in first-to-last, so a trailing partial byte holds its bits right-aligned (getByteListFromBits)
    const int nb = marker_size * marker_size, nbytes = (nb + 7) / 8, rem = nb % 8;
    std::vector<uint8_t> bits((size_t)n_markers * nb);
    for (int id = 0; id < n_markers; id++)
        for (int j = 0; j < nb; j++) {
            const int b = j / 8, p = j % 8;
            const unsigned v = bytes_list[((size_t)id * nbytes + b) * 4];
            const int width = (b == nbytes - 1 && rem) ? rem : 8;
            bits[(size_t)id * nb + j] = (uint8_t)((v >> (width - 1 - p)) & 1u);
        }
    return install_dictionary(c, marker_size, n_markers, max_correction_bits, bits.data());
}

int aslam_add_encoder(aslam_ctx* c, double wl, double wr, double t_now) {
    if (!c) return ASLAM_E_INVALID;
    if (int r = allow(c, kSingle)) return r;
    { int rp = finalize_pending(c); if (rp) return rp; }     // a pending batch arms the filter itself (is_init is set there)
    if (!c->is_init) {                       // aruco_slam.cpp:24-29
        c->last_time = t_now;
        c->is_init = true;
        return ASLAM_OK;
    }
    double dt = t_now - c->last_time;        // aruco_slam.cpp:31-32
    c->last_time = t_now;
    launch_ekf_predict_only(c->stream_ekf, c->ekf, c->sp, wl, wr, dt);
    HIP_TRY(c, hipGetLastError());
    return ASLAM_OK;
}

int aslam_add_image(aslam_ctx* c, const uint8_t* px, int rows, int cols, int channels, size_t step) {
    if (!c || !px) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kSingle)) return r;
    return add_frames(c, single_call(0, 1), &px, rows, cols, channels, &step);
}

int aslam_get_last_timing(aslam_ctx* c, double out[6]) {
    if (!c || !out) return ASLAM_E_INVALID;
    for (int i = 0; i < 6; i++) out[i] = c->last_timing[i];
    return ASLAM_OK;
}

namespace {
// state of filter E (the single one or a fleet robot's), streams synchronised by the caller
int read_state(aslam_ctx* c, const EkfState& E, int* N, double* mu, double* sigma) {
    int L = 0;
    HIP_TRY(c, hipMemcpy(&L, E.d_L, sizeof(int), hipMemcpyDeviceToHost));
    const int n = 3 + 3 * L;
    *N = n;
    if (mu) HIP_TRY(c, hipMemcpy(mu, E.d_mu, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (sigma) {
        // device layout: column-major with leading dimension ld = N_max; pack to ld = N
        std::vector<double> tmp((size_t)E.ld * n);
        HIP_TRY(c, hipMemcpy(tmp.data(), E.d_sigma, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int col = 0; col < n; col++) std::memcpy(sigma + (size_t)col * n, &tmp[(size_t)col * E.ld], sizeof(double) * n);
    }
    return ASLAM_OK;
}

// filter E := (mu, sigma, ids), its last-observed list emptied (N, L and the ids' presence checked by the caller, streams synchronised)
int write_state(aslam_ctx* c, const EkfState& E, int N, const double* mu, const double* sigma, const int* landmark_ids) {
    const int L = (N - 3) / 3;
    std::vector<double> tmp((size_t)E.ld * E.ld, 0.0);
    for (int col = 0; col < N; col++) std::memcpy(&tmp[(size_t)col * E.ld], sigma + (size_t)col * N, sizeof(double) * N);
    HIP_TRY(c, hipMemcpy(E.d_sigma, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(E.d_mu, mu, sizeof(double) * N, hipMemcpyHostToDevice));
    std::vector<int> id2idx(kIdTableSize, -1), idx2id(E.max_landmarks, -1);
    for (int i = 0; i < L; i++) {
        if (landmark_ids[i] < 0 || landmark_ids[i] >= kIdTableSize) return fail(c, ASLAM_E_INVALID, "landmark id out of range");
        if (id2idx[landmark_ids[i]] < 0) id2idx[landmark_ids[i]] = i;
        idx2id[i] = landmark_ids[i];
    }
    HIP_TRY(c, hipMemcpy(E.d_id2idx, id2idx.data(), sizeof(int) * kIdTableSize, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(E.d_idx2id, idx2id.data(), sizeof(int) * E.max_landmarks, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(E.d_L, &L, sizeof(int), hipMemcpyHostToDevice));
    int zero = 0;
    HIP_TRY(c, hipMemcpy(E.d_nlast, &zero, sizeof(int), hipMemcpyHostToDevice));
    return ASLAM_OK;
}

int read_landmark_ids(aslam_ctx* c, const EkfState& E, int* L, int* ids) {
    int n = 0;
    HIP_TRY(c, hipMemcpy(&n, E.d_L, sizeof(int), hipMemcpyDeviceToHost));
    *L = n;
    if (ids && n) HIP_TRY(c, hipMemcpy(ids, E.d_idx2id, sizeof(int) * n, hipMemcpyDeviceToHost));
    return ASLAM_OK;
}
}  // namespace

int aslam_get_state(aslam_ctx* c, int* N, double* mu, double* sigma) {
    if (!c || !N) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kSingle)) return r;
    { int rs = sync_streams(c); if (rs) return rs; }
    return read_state(c, c->ekf, N, mu, sigma);
}

int aslam_set_state(aslam_ctx* c, int N, const double* mu, const double* sigma, const int* landmark_ids) {
    if (!c || !mu || !sigma || N < 3 || (N - 3) % 3 != 0) return fail(c, ASLAM_E_INVALID, "bad state");
    if (int r = allow(c, kSlam)) return r;
    const int L = (N - 3) / 3;
    if (L > c->ekf.max_landmarks) return fail(c, ASLAM_E_CAPACITY, "state larger than max_landmarks");
    if (L > 0 && !landmark_ids) return fail(c, ASLAM_E_INVALID, "landmark ids required");
    { int rs = sync_streams(c); if (rs) return rs; }
    int r = write_state(c, c->ekf, N, mu, sigma, landmark_ids);
    if (r) return r;
    c->mirror_dirty = true;
    if (int rc = confirm_reseed(c, 1, nullptr)) return rc;
    return clear_track_health(c, kTrackSingle, 1);
}

// ---- host-side result surface (what the node publishes; pure host arithmetic on a few values read back) ---------------
namespace {
// tf2::Quaternion::setRPY(roll, pitch, yaw) -> (x, y, z, w)
void quat_from_rpy(double roll, double pitch, double yaw, double q[4]) {
    const double hy = yaw * 0.5, hp = pitch * 0.5, hr = roll * 0.5;
    const double cy = std::cos(hy), sy = std::sin(hy), cp = std::cos(hp), sp = std::sin(hp), cr = std::cos(hr), sr = std::sin(hr);
    q[0] = sr * cp * cy - cr * sp * sy;
    q[1] = cr * sp * cy + sr * cp * sy;
    q[2] = cr * cp * sy - sr * sp * cy;
    q[3] = cr * cp * cy + sr * sp * sy;
}
// cv::Rodrigues (vector -> matrix), row-major
void rodrigues_host(const double r[3], double R[9]) {
    const double th = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (th < DBL_EPSILON) { for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0; return; }
    const double c = std::cos(th), s = std::sin(th), c1 = 1.0 - c, it = 1.0 / th;
    const double x = r[0] * it, y = r[1] * it, z = r[2] * it;
    R[0] = c + c1 * x * x;     R[1] = c1 * x * y - s * z; R[2] = c1 * x * z + s * y;
    R[3] = c1 * x * y + s * z; R[4] = c + c1 * y * y;     R[5] = c1 * y * z - s * x;
    R[6] = c1 * x * z - s * y; R[7] = c1 * y * z + s * x; R[8] = c + c1 * z * z;
}
// tf2::Matrix3x3::getRotation
void quat_from_matrix(const double m[9], double q[4]) {
    const double trace = m[0] + m[4] + m[8];
    if (trace > 0.0) {
        double s = std::sqrt(trace + 1.0);
        q[3] = s * 0.5;
        s = 0.5 / s;
        q[0] = (m[7] - m[5]) * s; q[1] = (m[2] - m[6]) * s; q[2] = (m[3] - m[1]) * s;
    } else {
        const int i = m[0] < m[4] ? (m[4] < m[8] ? 2 : 1) : (m[0] < m[8] ? 2 : 0);
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        double s = std::sqrt(m[i * 3 + i] - m[j * 3 + j] - m[k * 3 + k] + 1.0);
        q[i] = s * 0.5;
        s = 0.5 / s;
        q[3] = (m[k * 3 + j] - m[j * 3 + k]) * s;
        q[j] = (m[j * 3 + i] + m[i * 3 + j]) * s;
        q[k] = (m[k * 3 + i] + m[i * 3 + k]) * s;
    }
}
void quat_mul(const double a[4], const double b[4], double o[4]) {          // Hamilton product, (x, y, z, w)
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
void quat_rotate(const double q[4], const double v[3], double o[3]) {        // tf2::Matrix3x3(q) * v
    const double d = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3], s = 2.0 / d;
    const double xs = q[0] * s, ys = q[1] * s, zs = q[2] * s;
    const double wx = q[3] * xs, wy = q[3] * ys, wz = q[3] * zs, xx = q[0] * xs, xy = q[0] * ys, xz = q[0] * zs, yy = q[1] * ys, yz = q[1] * zs, zz = q[2] * zs;
    o[0] = (1.0 - (yy + zz)) * v[0] + (xy - wz) * v[1] + (xz + wy) * v[2];
    o[1] = (xy + wz) * v[0] + (1.0 - (xx + zz)) * v[1] + (yz - wx) * v[2];
    o[2] = (xz - wy) * v[0] + (yz + wx) * v[1] + (1.0 - (xx + yy)) * v[2];
}
void fill_marker(aslam_marker_msg& m, int id, double length, double x, double y, double z, const double q[4], float r, float g, float b,
                 float a, double lifetime) {                                 // ArucoSlam::GenerateMarker, aruco_slam.cpp:289-305
    m.id = id;
    m.scale[0] = length; m.scale[1] = length; m.scale[2] = 0.01;
    m.color[0] = r; m.color[1] = g; m.color[2] = b; m.color[3] = a;
    m.position[0] = x; m.position[1] = y; m.position[2] = z;
    for (int k = 0; k < 4; k++) m.orientation[k] = q[k];
    m.lifetime_sec = lifetime;
}
}  // namespace

int aslam_get_pose_msg(aslam_ctx* c, aslam_pose_msg* out) {                   // ArucoSlam::toRosPose, aruco_slam.cpp:378-410
    if (!c || !out) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kSingle)) return r;
    { int rs = sync_streams(c); if (rs) return rs; }
    double mu[3], S[9];
    HIP_TRY(c, hipMemcpy(mu, c->ekf.d_mu, sizeof(mu), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy2D(S, 3 * sizeof(double), c->ekf.d_sigma, (size_t)c->ekf.ld * sizeof(double), 3 * sizeof(double), 3, hipMemcpyDeviceToHost));
    // S[col * 3 + row]
    out->position[0] = mu[0]; out->position[1] = mu[1]; out->position[2] = 0.1;
    quat_from_rpy(0, 0, mu[2], out->orientation);
    for (int i = 0; i < 36; i++) out->covariance[i] = 0.0;
    static const int at[3] = {0, 1, 5};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) out->covariance[at[i] * 6 + at[j]] = S[j * 3 + i];     // sigma_(i, j)
    return ASLAM_OK;
}

int aslam_get_map_markers(aslam_ctx* c, int max, int* n, aslam_marker_msg* out) {   // detected_map_, aruco_slam.cpp:265-281
    if (!c || !n) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kSingle)) return r;
    { int rs = sync_streams(c); if (rs) return rs; }
    int L = 0;
    HIP_TRY(c, hipMemcpy(&L, c->ekf.d_L, sizeof(int), hipMemcpyDeviceToHost));
    *n = L;
    if (!out || L == 0) return ASLAM_OK;
    std::vector<double> mu((size_t)3 + 3 * L);
    HIP_TRY(c, hipMemcpy(mu.data(), c->ekf.d_mu, mu.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int i = 0; i < L && i < max; i++) {
        double q[4];
        quat_from_rpy(0, 1.5708, mu[3 * i + 5], q);
        fill_marker(out[i], i, c->sp.marker_length, mu[3 * i + 3], mu[3 * i + 4], 0.3, q, 1.f, 0.5f, 1.f, 0.5f, 0.0);
    }
    return ASLAM_OK;
}

int aslam_get_detected_markers(aslam_ctx* c, int max, int* n, aslam_marker_msg* out) {   // detected_markers_, aruco_slam.cpp:325-347
    if (!c || !n) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kSingle)) return r;
    if (c->rig_last) return fail(c, ASLAM_E_STATE, "the last call was a camera-rig call: detected-marker messages describe one camera");
    int M = 0;
    int r = aslam_get_detections(c, &M, nullptr, nullptr, nullptr, nullptr);
    if (r) return r;
    std::vector<int> ids(M);
    std::vector<double> rv((size_t)3 * M), tv((size_t)3 * M);
    if (M) { r = aslam_get_detections(c, &M, ids.data(), nullptr, rv.data(), tv.data()); if (r) return r; }
    int k = 0;
    for (int i = 0; i < M; i++) {
        const double* t = &tv[(size_t)3 * i];
        // the range gate precedes the visualisation (aruco_slam.cpp:327-333): float norm against the float threshold
        if ((float)std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) > c->sp.useful_distance_threshold) continue;
        if (out && k < max) {
            double R[9], q[4], qo[4], p[3];
            rodrigues_host(&rv[(size_t)3 * i], R);
            quat_from_matrix(R, q);                                    // fillTransform + getRotation
            quat_rotate(c->init.r2c_q, t, p);                           // tf2::doTransform(pose, pose, transformStamped_r2c_)
            for (int a = 0; a < 3; a++) p[a] += c->init.r2c_t[a];
            quat_mul(c->init.r2c_q, q, qo);
            fill_marker(out[k], ids[i], c->sp.marker_length, p[0], p[1], p[2], qo, 1.f, 0.f, 0.f, 1.f, 0.1);
        }
        k++;
    }
    *n = k;
    return ASLAM_OK;
}

// markered_img_ (aruco_slam.cpp:318-319): cv::aruco::drawDetectedMarkers(img.clone(), corners, ids) with its default colours on a
// bgr8 buffer - the quad outline in (0, 255, 0), a 7 x 7 square outline in (0, 0, 255) around corner 0 (the marker's own
// top-left).  Host drawing from the last frame's detections; the "id=N" text of the original is not rendered (no font here).
namespace {
void put_px(uint8_t* img, int rows, int cols, size_t step, int x, int y, uint8_t b, uint8_t g, uint8_t r) {
    if (x < 0 || y < 0 || x >= cols || y >= rows) return;
    uint8_t* p = img + (size_t)y * step + (size_t)x * 3;
    p[0] = b; p[1] = g; p[2] = r;
}
void draw_line(uint8_t* img, int rows, int cols, size_t step, int x0, int y0, int x1, int y1, uint8_t b, uint8_t g, uint8_t r) {
    const int dx = std::abs(x1 - x0), dy = -std::abs(y1 - y0), sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1;
    int err = dx + dy;
    for (;;) {                                                    // 8-connected Bresenham
        put_px(img, rows, cols, step, x0, y0, b, g, r);
        if (x0 == x1 && y0 == y1) break;
        const int e2 = 2 * err;
        if (e2 >= dy) { err += dy; x0 += sx; }
        if (e2 <= dx) { err += dx; y0 += sy; }
    }
}
}  // namespace

int aslam_draw_detected_markers(aslam_ctx* c, uint8_t* bgr, int rows, int cols, size_t step) {
    if (!c || !bgr || rows <= 0 || cols <= 0 || step < (size_t)cols * 3) return fail(c, ASLAM_E_INVALID, "bad arguments");
    if (int r = allow(c, kSingle)) return r;
    if (c->rig_last) return fail(c, ASLAM_E_STATE, "the last call was a camera-rig call: the overlay describes one camera");
    int M = 0;
    int r = aslam_get_detections(c, &M, nullptr, nullptr, nullptr, nullptr);
    if (r) return r;
    std::vector<float> corners((size_t)std::max(M, 1) * 8);
    if (M) { r = aslam_get_detections(c, &M, nullptr, corners.data(), nullptr, nullptr); if (r) return r; }
    for (int i = 0; i < M; i++) {
        const float* q = &corners[(size_t)i * 8];
        int px[4], py[4];
        for (int k = 0; k < 4; k++) { px[k] = (int)std::lrintf(q[2 * k]); py[k] = (int)std::lrintf(q[2 * k + 1]); }
        for (int k = 0; k < 4; k++) draw_line(bgr, rows, cols, step, px[k], py[k], px[(k + 1) & 3], py[(k + 1) & 3], 0, 255, 0);
        const int x0 = px[0] - 3, y0 = py[0] - 3, x1 = px[0] + 3, y1 = py[0] + 3;
        draw_line(bgr, rows, cols, step, x0, y0, x1, y0, 0, 0, 255); draw_line(bgr, rows, cols, step, x1, y0, x1, y1, 0, 0, 255);
        draw_line(bgr, rows, cols, step, x1, y1, x0, y1, 0, 0, 255); draw_line(bgr, rows, cols, step, x0, y1, x0, y0, 0, 0, 255);
    }
    return ASLAM_OK;
}

// MapLoader::loadMap (map_loader.cpp:7-81) as plain data: the ground-truth map file behind the latched `real_map` topic.
// One marker per line "id length x y [z [roll [pitch [yaw]]]]"; '#' starts a comment line, blank lines are skipped, a line
// that starts with anything else than a digit aborts the whole load with an EMPTY result; a line with fewer than four
// fields is skipped.  The optional fields reproduce the loader's crossed fallbacks: a missing roll zeroes YAW, a missing yaw
// zeroes ROLL (each leaving the other at whatever the previous line left there; 0 at the start).  Orientation =
// setRPY(roll, pitch, yaw); CUBE (length, length, 0.01), rgba (1, 1, 1, 0.5), frame "world", lifetime 0
// (MapLoader::generateMarker, map_loader.cpp:96-118).  Needs no device: ctx may be NULL.
int aslam_load_map_txt(aslam_ctx* c, const char* path, int max, int* n, aslam_marker_msg* out) {
    if (!path || !n) return c ? fail(c, ASLAM_E_INVALID, "null argument") : ASLAM_E_INVALID;
    *n = 0;
    std::ifstream f(path);
    if (!f.good()) return c ? fail(c, ASLAM_E_INVALID, std::string("cannot read ") + path) : ASLAM_E_INVALID;
    std::string line;
    int count = 0;
    int id = 0;
    double length = 0, x = 0, y = 0, z = 0, yaw = 0, pitch = 0, roll = 0;       // deliberately outside the loop: see above
    while (std::getline(f, line)) {
        std::istringstream s(line);
        char first = 0;
        if (!(s >> first)) continue;                          // blank line
        if (first == '#') continue;
        if (!isdigit((unsigned char)first)) { *n = 0; return ASLAM_OK; }       // "Malformed input": the map is cleared
        s.putback(first);
        if (!(s >> id >> length >> x >> y)) continue;
        if (!(s >> z)) z = 0;
        if (!(s >> roll)) yaw = 0;
        if (!(s >> pitch)) pitch = 0;
        if (!(s >> yaw)) roll = 0;
        if (out && count < max) {
            double q[4];
            quat_from_rpy(roll, pitch, yaw, q);
            fill_marker(out[count], id, length, x, y, z, q, 1.f, 1.f, 1.f, 0.5f, 0.0);
        }
        count++;
    }
    *n = count;
    return ASLAM_OK;
}

// ---- localization against a frozen map (include/aruco_slam_hip.h) -------------------------------------------
namespace {
// the frozen map of localization and of a fleet: checked (write = false), or written (write = true) into the id tables and the
// landmark rows of mu, with the pose rows of mu and all of Sigma zero
int install_frozen_map(aslam_ctx* c, int n, const int* ids, const double* xyth, bool write) {
    if (n < 1 || n > c->ekf.max_landmarks) return fail(c, ASLAM_E_INVALID, "a map of 1..max_landmarks landmarks");
    std::vector<int> id2idx(kIdTableSize, -1), idx2id(c->ekf.max_landmarks, -1);
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= kIdTableSize) return fail(c, ASLAM_E_INVALID, "landmark id " + std::to_string(ids[i]) + " outside [0, 1024)");
        if (id2idx[ids[i]] >= 0) return fail(c, ASLAM_E_INVALID, "landmark id " + std::to_string(ids[i]) + " given twice");
        id2idx[ids[i]] = i;
        idx2id[i] = ids[i];
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(xyth[3 * i + k])) return fail(c, ASLAM_E_INVALID, "landmark " + std::to_string(ids[i]) + ": non-finite value");
    }
    if (!write) return ASLAM_OK;
    const size_t ld = (size_t)c->ekf.ld;
    HIP_TRY(c, hipMemset(c->ekf.d_sigma, 0, ld * ld * sizeof(double)));
    std::vector<double> mu(3 + 3 * (size_t)n, 0.0);
    std::memcpy(mu.data() + 3, xyth, sizeof(double) * 3 * n);
    HIP_TRY(c, hipMemset(c->ekf.d_mu, 0, ld * sizeof(double)));
    HIP_TRY(c, hipMemcpy(c->ekf.d_mu, mu.data(), sizeof(double) * mu.size(), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->ekf.d_id2idx, id2idx.data(), sizeof(int) * kIdTableSize, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->ekf.d_idx2id, idx2id.data(), sizeof(int) * c->ekf.max_landmarks, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->ekf.d_L, &n, sizeof(int), hipMemcpyHostToDevice));
    return ASLAM_OK;
}

int check_pose(aslam_ctx* c, const double* pose, const double* sigma) {
    for (int k = 0; k < 3; k++) if (!std::isfinite(pose[k])) return fail(c, ASLAM_E_INVALID, "non-finite pose");
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            if (!std::isfinite(sigma[i * 3 + j])) return fail(c, ASLAM_E_INVALID, "non-finite pose covariance");
            if (sigma[i * 3 + j] != sigma[j * 3 + i]) return fail(c, ASLAM_E_INVALID, "pose covariance not symmetric");
        }
    return ASLAM_OK;
}

// the landmark covariances of an uncertain map: checked, and C = (S + S^T) / 2 per landmark into out (n x 9)
int check_map_sigmas(aslam_ctx* c, int n, const int* ids, const double* map_sigmas, std::vector<double>& out) {
    out.resize((size_t)9 * n);
    for (int k = 0; k < n; k++) {
        const double* S = map_sigmas + 9 * (size_t)k;
        double* C = &out[9 * (size_t)k];
        const std::string who = "landmark " + std::to_string(ids[k]);
        for (int i = 0; i < 9; i++)
            if (!std::isfinite(S[i])) return fail(c, ASLAM_E_INVALID, who + ": non-finite covariance");
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) C[i * 3 + j] = 0.5 * (S[i * 3 + j] + S[j * 3 + i]);
        for (int i = 0; i < 3; i++) {
            if (C[i * 4] < 0.0) return fail(c, ASLAM_E_INVALID, who + ": negative variance");
            for (int j = i + 1; j < 3; j++)
                if (C[i * 3 + j] * C[i * 3 + j] > C[i * 4] * C[j * 4]) return fail(c, ASLAM_E_INVALID, who + ": covariance exceeds its variances");
        }
    }
    return ASLAM_OK;
}

// the C table on the device (made on first use for max_landmarks blocks)
int upload_map_sigmas(aslam_ctx* c, const std::vector<double>& C) {
    if (!c->d_map_c) HIP_TRY(c, dalloc(&c->d_map_c, (size_t)9 * c->ekf.max_landmarks));
    HIP_TRY(c, hipMemcpy(c->d_map_c, C.data(), sizeof(double) * C.size(), hipMemcpyHostToDevice));
    return ASLAM_OK;
}

// a seat of a pose on an uncertain map drops its correlation with the map: Sigma_xl := 0 of the single filter (robot < 0) or of one
// robot, at once (st = nullptr) or behind the work enqueued on st
int clear_cross(aslam_ctx* c, int robot, hipStream_t st = nullptr) {
    if (!c->umap_on) return ASLAM_OK;
    if (robot < 0) {
        launch_umap_clear_cross(st, c->ekf, c->umap.L);
        HIP_TRY(c, hipGetLastError());
        if (!st) HIP_TRY(c, hipStreamSynchronize(nullptr));
        return ASLAM_OK;
    }
    const size_t n = (size_t)9 * c->umap.L;
    if (st) HIP_TRY(c, hipMemsetAsync(c->umap.cross + n * robot, 0, sizeof(double) * n, st));
    else HIP_TRY(c, hipMemset(c->umap.cross + n * robot, 0, sizeof(double) * n));
    return ASLAM_OK;
}
}  // namespace

namespace {
int fleet_alloc(aslam_ctx* c) {
    if (c->fleet_cap) return ASLAM_OK;
    const int R = std::min(c->max_batch, ASLAM_MAX_ROBOTS), B = c->max_batch;
    HIP_TRY(c, dalloc(&c->fleet.pose, (size_t)kFleetState * R));
    HIP_TRY(c, dalloc(&c->fleet.last, (size_t)kMarkerMax * R));
    HIP_TRY(c, dalloc(&c->fleet.nlast, R));
    HIP_TRY(c, dalloc(&c->d_fleet_cams, R));
    HIP_TRY(c, dalloc(&c->d_fleet_camidx, B));
    HIP_TRY(c, dalloc(&c->d_fleet_work, 4 * R + 4 * B));       // a localization call's CSR list, or a SLAM call's 4 ints per slot
    int r = pinned_alloc(c, c->fleet_camidx_up, B);
    if (!r) r = pinned_alloc(c, c->fleet_work_up, 4 * R + 4 * B);
    if (r) return r;
    c->fleet_cap = R;
    return ASLAM_OK;
}

// The one place the mode changes (streams synchronised by the caller; for Localize and FleetLocalize the frozen map is already written).
// Fleet SLAM, and SLAM after a fleet, start from the single filter as aslam_create leaves it (ekf_alloc); the frozen modes start with
// empty last-observed and pop lists.  Leaving a fleet frees its SLAM filters; a fleet of cams.size() robots gets its device tables on
// first use and those cameras, every robot disarmed.
int enter_mode(aslam_ctx* c, Mode m, const std::vector<RigCam>& cams = {}) {
    const bool fleet = m == Mode::FleetLocalize || m == Mode::FleetSlam, was_fleet = c->fleet_n > 0;
    if (fleet) {
        int r = fleet_alloc(c);
        if (r) return r;
    }
    ekf_fleet_free(c->fslam);
    if (c->umap.cross) hipFree(c->umap.cross);          // an uncertain-map fleet's strips; the begin that wants them makes them anew
    c->umap = MapCov{};
    c->umap_on = false;
    c->mode = Mode::Slam;
    c->fleet_n = 0;
    c->fleet_armed.clear();
    c->mirror_dirty = true;
    if (m == Mode::FleetSlam || (m == Mode::Slam && was_fleet)) {
        const size_t ld = (size_t)c->ekf.ld;
        HIP_TRY(c, hipMemset(c->ekf.d_mu, 0, ld * sizeof(double)));
        HIP_TRY(c, hipMemset(c->ekf.d_sigma, 0, ld * ld * sizeof(double)));
        HIP_TRY(c, hipMemset(c->ekf.d_L, 0, sizeof(int)));
        HIP_TRY(c, hipMemset(c->ekf.d_id2idx, 0xFF, kIdTableSize * sizeof(int)));
        HIP_TRY(c, hipMemset(c->ekf.d_idx2id, 0xFF, (size_t)c->ekf.max_landmarks * sizeof(int)));
        HIP_TRY(c, hipMemset(c->ekf.d_m, 0, sizeof(int)));
        c->is_init = false;
        c->last_time = 0;
    }
    if (m != Mode::Slam || was_fleet) {
        const int zero = 0;
        HIP_TRY(c, hipMemcpy(c->ekf.d_nlast, &zero, sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(c->ekf.d_npop, &zero, sizeof(int), hipMemcpyHostToDevice));
    }
    const int R = (int)cams.size();
    if (m == Mode::FleetSlam) {
        const hipError_t e = ekf_fleet_alloc(c->fslam, R, c->ekf);
        if (e != hipSuccess)
            return fail(c, ASLAM_E_CAPACITY, std::to_string(R) + " filters of max_landmarks " + std::to_string(c->ekf.max_landmarks) +
                                                 " do not fit: " + hipGetErrorString(e));
    }
    if (fleet) HIP_TRY(c, hipMemcpy(c->d_fleet_cams, cams.data(), sizeof(RigCam) * R, hipMemcpyHostToDevice));
    c->mode = m;
    c->fleet_n = fleet ? R : 0;
    c->fleet_armed.assign(c->fleet_n, 0);
    // a seat of every SLAM filter the mode starts with (the localization modes' begins clear their own records)
    // ... and a reseed of their landmark confirmation
    if (m == Mode::Slam) {
        if (int r = confirm_reseed(c, 1, nullptr)) return r;
        return clear_track_health(c, kTrackSingle, 1);
    }
    if (m == Mode::FleetSlam) {
        if (int r = confirm_reseed_fleet(c)) return r;
        return clear_track_health(c, 0, R);
    }
    return ASLAM_OK;
}
}  // namespace

int aslam_localize_begin(aslam_ctx* c, int n, const int* ids, const double* xyth, const double pose[3], const double pose_sigma[9]) {
    if (!c || !ids || !xyth || !pose || !pose_sigma) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kSingle)) return r;
    int r = install_frozen_map(c, n, ids, xyth, false);
    if (r) return r;
    r = check_pose(c, pose, pose_sigma);
    if (r) return r;
    { int rs = sync_streams(c); if (rs) return rs; }
    // state := [pose, map], Sigma := blockdiag(pose_sigma, 0) in the SLAM layout (column-major, ld = N_max)
    r = install_frozen_map(c, n, ids, xyth, true);
    if (r) return r;
    const size_t ld = (size_t)c->ekf.ld;
    for (int col = 0; col < 3; col++) {
        const double v[3] = {pose_sigma[col], pose_sigma[3 + col], pose_sigma[6 + col]};
        HIP_TRY(c, hipMemcpy(c->ekf.d_sigma + (size_t)col * ld, v, sizeof(v), hipMemcpyHostToDevice));
    }
    HIP_TRY(c, hipMemcpy(c->ekf.d_mu, pose, 3 * sizeof(double), hipMemcpyHostToDevice));
    if (int rt = clear_track_health(c, kTrackSingle, 1)) return rt;
    return enter_mode(c, Mode::Localize);
}

int aslam_localize_begin_uncertain(aslam_ctx* c, int n, const int* ids, const double* xyth, const double* map_sigmas, const double pose[3],
                                   const double pose_sigma[9]) {
    if (!c || !ids || !xyth || !map_sigmas || !pose || !pose_sigma) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kSingle)) return r;
    if (int r = install_frozen_map(c, n, ids, xyth, false)) return r;
    if (int r = check_pose(c, pose, pose_sigma)) return r;
    std::vector<double> C;
    if (int r = check_map_sigmas(c, n, ids, map_sigmas, C)) return r;
    if (int r = aslam_localize_begin(c, n, ids, xyth, pose, pose_sigma)) return r;
    // Sigma := blockdiag(pose_sigma, C_0 ... C_{n-1}): the blocks beside the frozen-map state; Sigma_xl = 0 already
    if (int r = upload_map_sigmas(c, C)) return r;
    const size_t ld = (size_t)c->ekf.ld;
    for (int k = 0; k < n; k++)
        HIP_TRY(c, hipMemcpy2D(c->ekf.d_sigma + (size_t)(3 + 3 * k) * ld + 3 + 3 * k, ld * sizeof(double), &C[9 * (size_t)k], 3 * sizeof(double),
                               3 * sizeof(double), 3, hipMemcpyHostToDevice));
    c->umap = MapCov{c->d_map_c, nullptr, n};
    c->umap_on = true;
    return ASLAM_OK;
}

int aslam_is_map_uncertain(aslam_ctx* c, int* on) {
    if (!c || !on) return fail(c, ASLAM_E_INVALID, "null argument");
    *on = c->umap_on ? 1 : 0;
    return ASLAM_OK;
}

int aslam_localize_end(aslam_ctx* c) {
    if (!c) return ASLAM_E_INVALID;
    if (int r = allow(c, kSingle)) return r;
    { int rs = sync_streams(c); if (rs) return rs; }
    return enter_mode(c, Mode::Slam);
}

int aslam_is_localizing(aslam_ctx* c, int* on) {
    if (!c || !on) return fail(c, ASLAM_E_INVALID, "null argument");
    *on = c->mode == Mode::Localize ? 1 : 0;
    return ASLAM_OK;
}

// ---- fleet localization: many robots on one frozen map (include/aruco_slam_hip.h) -------------------------------
namespace {
// one robot's filter := (pose, sigma), its last-observed list emptied, disarmed
int fleet_seat(aslam_ctx* c, int robot, const double* pose, const double* sigma) {
    double st[kFleetState];
    for (int k = 0; k < 3; k++) st[k] = pose[k];
    for (int k = 0; k < 9; k++) st[3 + k] = sigma[k];
    HIP_TRY(c, hipMemcpy(c->fleet.pose + (size_t)kFleetState * robot, st, sizeof(st), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemset(c->fleet.nlast + robot, 0, sizeof(int)));
    c->fleet_armed[robot] = 0;
    if (int r = clear_cross(c, robot)) return r;
    return clear_track_health(c, robot, 1);
}

// fleet steps of frame slots [first, first + count), slot first + i belonging to robot robots[i]: one k_fleet_steps workgroup per
// robot present (in order of first appearance), its slots ascending, behind the detection that produced their lists.  The host
// keeps the armed flags: a robot's first frame after aslam_fleet_begin / aslam_fleet_set_pose only arms its filter.
int run_fleet_steps(aslam_ctx* c, int first, int count, const int* robots) {
    std::vector<int> group(c->fleet_n, -1), robot_of_group;
    std::vector<std::vector<int>> slots_of;
    for (int i = 0; i < count; i++) {
        int& g = group[robots[i]];
        if (g < 0) { g = (int)slots_of.size(); slots_of.emplace_back(); robot_of_group.push_back(robots[i]); }
        slots_of[g].push_back(first + i);
    }
    const int ng = (int)slots_of.size();
    std::vector<int> w(4 * ng);             // per group: robot, predicts, its first entry in the slot list, its slots; then the slot list
    for (int g = 0; g < ng; g++) {
        const int r = robot_of_group[g];
        w[4 * g] = r; w[4 * g + 1] = c->fleet_armed[r] ? 1 : 0; w[4 * g + 2] = (int)w.size() - 4 * ng; w[4 * g + 3] = (int)slots_of[g].size();
        w.insert(w.end(), slots_of[g].begin(), slots_of[g].end());
        c->fleet_armed[r] = 1;
    }
    hipStream_t st = c->stream_ekf;
    int rc = pinned_upload(c, c->fleet_work_up, c->d_fleet_work, w.data(), w.size(), st);
    if (rc) return rc;
    HIP_TRY(c, hipStreamWaitEvent(st, c->ev_detect, 0));
    prof_begin(c, P_FLEET_STEPS, st);
    launch_fleet_steps(st, c->ekf, c->fleet, c->sp, c->d_obs, c->d_nmarkers, c->d_enc, c->d_fleet_work, ng, c->gate_on ? &c->gate : nullptr,
                       c->umap_on ? &c->umap : nullptr, c->consistent_on);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev_ekf, st));
    note_ekf_range(c, first, count);
    return ASLAM_OK;
}

// fleet SLAM steps of frame slots [first, first + count), slot first + i belonging to robot robots[i], in rounds: round k holds the k-th
// slot of every robot that has one, and is one launch of each kernel of the per-frame chain with one z-slice per robot.  The work list
// (4 ints per slot: robot, slot, predict, 0, round after round) goes up once per call; the host keeps the armed flags.
int run_fleet_slam(aslam_ctx* c, int first, int count, const int* robots) {
    std::vector<int> taken(c->fleet_n, 0);
    std::vector<std::vector<int>> rounds;
    for (int i = 0; i < count; i++) {
        const int k = taken[robots[i]]++;
        if (k == (int)rounds.size()) rounds.emplace_back();
        rounds[k].push_back(i);
    }
    std::vector<int> w;
    for (const std::vector<int>& rd : rounds)
        for (int i : rd) {
            const int r = robots[i];
            w.insert(w.end(), {r, first + i, c->fleet_armed[r] ? 1 : 0, 0});
            c->fleet_armed[r] = 1;
        }
    hipStream_t st = c->stream_ekf;
    int rc = pinned_upload(c, c->fleet_work_up, c->d_fleet_work, w.data(), w.size(), st);
    if (rc) return rc;
    HIP_TRY(c, hipStreamWaitEvent(st, c->ev_detect, 0));
    int row = 0;
    for (const std::vector<int>& rd : rounds) {
        const FleetRound R{c->fslam, c->d_fleet_work + 4 * row, c->d_enc, (int)rd.size()};
        if (int rj = confirm_round(c, st, R.work, R.n)) return rj;
        prof_begin(c, P_EKF_PLAN, st);
        launch_ekf_plan(st, R, c->sp, c->d_obs, c->d_nmarkers, c->d_ctr, c->init.max_updates_per_frame);
        prof_end(c);
        int r = run_chain(c, R);
        if (r) return r;
        row += (int)rd.size();
    }
    HIP_TRY(c, hipEventRecord(c->ev_ekf, st));
    note_ekf_range(c, first, count);
    return ASLAM_OK;
}

// the EKF part of a fleet call, whichever kind the fleet is
int run_fleet_ekf(aslam_ctx* c, int first, int count, const int* robots) {
    return c->mode == Mode::FleetSlam ? run_fleet_slam(c, first, count, robots) : run_fleet_steps(c, first, count, robots);
}

// the cameras of a new fleet of n_robots, checked and converted for k_pose
int fleet_cameras(aslam_ctx* c, int n_robots, const aslam_camera* cams, std::vector<RigCam>& rc) {
    if (n_robots < 1 || n_robots > std::min(c->max_batch, ASLAM_MAX_ROBOTS))
        return fail(c, ASLAM_E_INVALID, "a fleet has 1..min(max_batch, ASLAM_MAX_ROBOTS) robots");
    rc.resize(n_robots);
    for (int k = 0; k < n_robots; k++) {
        int r = rig_camera(c, cams[k], rc[k]);
        if (r) return r;
    }
    return ASLAM_OK;
}
}  // namespace

int aslam_fleet_begin(aslam_ctx* c, int n_robots, const aslam_camera* cams, int n, const int* ids, const double* xyth, const double* poses,
                      const double* pose_sigmas) {
    if (!c || !cams || !ids || !xyth || !poses || !pose_sigmas) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kSlam | kFleet)) return r;
    std::vector<RigCam> rc;
    int r = fleet_cameras(c, n_robots, cams, rc);
    if (r) return r;
    r = install_frozen_map(c, n, ids, xyth, false);
    if (r) return r;
    for (int k = 0; k < n_robots; k++) {
        r = check_pose(c, poses + 3 * k, pose_sigmas + 9 * k);
        if (r) return r;
    }
    r = sync_streams(c);
    if (r) return r;
    r = install_frozen_map(c, n, ids, xyth, true);
    if (r) return r;
    r = enter_mode(c, Mode::FleetLocalize, rc);
    if (r) return r;
    for (int k = 0; k < n_robots; k++) {
        r = fleet_seat(c, k, poses + 3 * k, pose_sigmas + 9 * k);
        if (r) return r;
    }
    return ASLAM_OK;
}

int aslam_fleet_begin_uncertain(aslam_ctx* c, int n_robots, const aslam_camera* cams, int n, const int* ids, const double* xyth,
                                const double* map_sigmas, const double* poses, const double* pose_sigmas) {
    if (!c || !cams || !ids || !xyth || !map_sigmas || !poses || !pose_sigmas) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kSlam | kFleet)) return r;
    {   // every check of aslam_fleet_begin before anything changes, then the covariances
        std::vector<RigCam> rc;
        if (int r = fleet_cameras(c, n_robots, cams, rc)) return r;
        if (int r = install_frozen_map(c, n, ids, xyth, false)) return r;
        for (int k = 0; k < n_robots; k++)
            if (int r = check_pose(c, poses + 3 * k, pose_sigmas + 9 * k)) return r;
    }
    std::vector<double> C;
    if (int r = check_map_sigmas(c, n, ids, map_sigmas, C)) return r;
    if (int r = aslam_fleet_begin(c, n_robots, cams, n, ids, xyth, poses, pose_sigmas)) return r;
    if (int r = upload_map_sigmas(c, C)) return r;
    double* cross = nullptr;
    const size_t count = (size_t)9 * n * n_robots;
    hipError_t e = dalloc(&cross, count);
    if (e == hipSuccess && (e = hipMemset(cross, 0, sizeof(double) * count)) != hipSuccess) hipFree(cross);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        enter_mode(c, Mode::Slam);
        return fail(c, ASLAM_E_CAPACITY, std::to_string(n_robots) + " cross strips of " + std::to_string(n) + " landmarks do not fit: " + hipGetErrorString(e));
    }
    c->umap = MapCov{c->d_map_c, cross, n};
    c->umap_on = true;
    return ASLAM_OK;
}

int aslam_fleet_get_cross(aslam_ctx* c, int robot, int* L, double* cross) {
    if (!c || !L) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kFleetLocalize)) return r;
    if (!c->umap_on) return fail(c, ASLAM_E_STATE, "the fleet's map is exact (aslam_fleet_begin_uncertain first)");
    if (robot < 0 || robot >= c->fleet_n) return fail(c, ASLAM_E_INVALID, "robot index outside the fleet");
    { int rs = sync_streams(c); if (rs) return rs; }
    *L = c->umap.L;
    const size_t n = (size_t)9 * c->umap.L;
    if (cross) HIP_TRY(c, hipMemcpy(cross, c->umap.cross + n * robot, sizeof(double) * n, hipMemcpyDeviceToHost));
    return ASLAM_OK;
}

int aslam_fleet_add_images(aslam_ctx* c, int n, const int* robots, const double* wl, const double* wr, const double* dt,
                           const uint8_t* const* px, int rows, int cols, int channels, const size_t* step_bytes) {
    if (!c || !robots || !wl || !wr || !dt || !px || !step_bytes) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kFleet)) return r;
    if (n < 1 || n > c->max_batch) return fail(c, ASLAM_E_INVALID, "1..max_batch frames per call");
    std::vector<char> seen(c->fleet_n, 0);
    for (int i = 0; i < n; i++) {
        if (robots[i] < 0 || robots[i] >= c->fleet_n) return fail(c, ASLAM_E_INVALID, "robot index outside the fleet");
        if (seen[robots[i]]) return fail(c, ASLAM_E_INVALID, "a robot named twice in one aslam_fleet_add_images");
        seen[robots[i]] = 1;
        if (!px[i]) return fail(c, ASLAM_E_INVALID, "null image");
    }
    const double* enc[3] = {wl, wr, dt};
    return add_frames(c, fleet_call(0, n, robots), px, rows, cols, channels, step_bytes, enc);
}

int aslam_fleet_run_staged(aslam_ctx* c, int first, int count, const int* robot_of_slot, int with_ekf) {
    if (!c || !robot_of_slot) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kFleet)) return r;
    return run_staged(c, fleet_call(first, count, robot_of_slot), with_ekf);
}

int aslam_fleet_get_poses(aslam_ctx* c, int max, int* n_robots, double* poses, double* sigmas) {
    if (!c || !n_robots) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kFleet)) return r;
    { int rs = sync_streams(c); if (rs) return rs; }
    const int R = c->fleet_n;
    *n_robots = R;
    std::vector<double> h((size_t)kFleetState * R);
    if (c->mode == Mode::FleetSlam) {
        // every robot's mu[0..2] and the first three entries of Sigma's columns 0..2, gathered as rows of kFleetState doubles
        const FleetSlam& F = c->fslam;
        HIP_TRY(c, hipMemcpy2D(h.data(), sizeof(double) * kFleetState, F.base.d_mu, F.stride, 3 * sizeof(double), R, hipMemcpyDeviceToHost));
        for (int j = 0; j < 3; j++)
            HIP_TRY(c, hipMemcpy2D(h.data() + 3 + 3 * j, sizeof(double) * kFleetState, F.base.d_sigma + (size_t)j * F.base.ld, F.stride,
                                   3 * sizeof(double), R, hipMemcpyDeviceToHost));
        for (int k = 0; k < R; k++) {        // column-major -> row-major Sigma_xx
            double* S = &h[(size_t)kFleetState * k + 3];
            std::swap(S[1], S[3]); std::swap(S[2], S[6]); std::swap(S[5], S[7]);
        }
    } else {
        HIP_TRY(c, hipMemcpy(h.data(), c->fleet.pose, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    }
    for (int k = 0; k < std::min(max, R); k++) {
        if (poses) std::memcpy(poses + 3 * k, &h[(size_t)kFleetState * k], 3 * sizeof(double));
        if (sigmas) std::memcpy(sigmas + 9 * k, &h[(size_t)kFleetState * k + 3], 9 * sizeof(double));
    }
    return ASLAM_OK;
}

int aslam_fleet_set_pose(aslam_ctx* c, int robot, const double pose[3], const double sigma[9]) {
    if (!c || !pose || !sigma) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kFleetLocalize)) return r;
    if (robot < 0 || robot >= c->fleet_n) return fail(c, ASLAM_E_INVALID, "robot index outside the fleet");
    int r = check_pose(c, pose, sigma);
    if (r) return r;
    r = sync_streams(c);
    if (r) return r;
    return fleet_seat(c, robot, pose, sigma);
}

int aslam_fleet_end(aslam_ctx* c) {
    if (!c) return ASLAM_E_INVALID;
    if (int r = allow(c, kFleet)) return r;
    { int rs = sync_streams(c); if (rs) return rs; }
    merge_free(c->merge);                               // the map merge's tables and record buffer, if a merge made them
    reloc_free(c->reloc);                               // the relocalization's result records, if a call made them
    slam_reloc_free(c->slam_reloc);                     // the SLAM relocalization's seat tables, likewise
    return enter_mode(c, Mode::Slam);
}

int aslam_is_fleet(aslam_ctx* c, int* n_robots) {
    if (!c || !n_robots) return fail(c, ASLAM_E_INVALID, "null argument");
    *n_robots = c->fleet_n;
    return ASLAM_OK;
}

// ---- fleet SLAM: many robots, each building its own map (include/aruco_slam_hip.h) ------------------------------
int aslam_fleet_slam_begin(aslam_ctx* c, int n_robots, const aslam_camera* cams) {
    if (!c || !cams) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kSlam | kFleet)) return r;
    std::vector<RigCam> rc;
    int r = fleet_cameras(c, n_robots, cams, rc);
    if (r) return r;
    r = sync_streams(c);
    if (r) return r;
    return enter_mode(c, Mode::FleetSlam, rc);          // the fleet active so far, if any, ends
}

int aslam_is_fleet_slam(aslam_ctx* c, int* on) {
    if (!c || !on) return fail(c, ASLAM_E_INVALID, "null argument");
    *on = c->mode == Mode::FleetSlam ? 1 : 0;
    return ASLAM_OK;
}

int aslam_fleet_get_state(aslam_ctx* c, int robot, int* N, double* mu, double* sigma) {
    if (!c || !N) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kFleetSlam)) return r;
    if (robot < 0 || robot >= c->fleet_n) return fail(c, ASLAM_E_INVALID, "robot index outside the fleet");
    { int rs = sync_streams(c); if (rs) return rs; }
    return read_state(c, ekf_fleet_robot(c->fslam, robot), N, mu, sigma);
}

int aslam_fleet_set_state(aslam_ctx* c, int robot, int N, const double* mu, const double* sigma, const int* landmark_ids) {
    if (!c || !mu || !sigma || N < 3 || (N - 3) % 3 != 0) return fail(c, ASLAM_E_INVALID, "bad state");
    if (int r = allow(c, kFleetSlam)) return r;
    if (robot < 0 || robot >= c->fleet_n) return fail(c, ASLAM_E_INVALID, "robot index outside the fleet");
    const int L = (N - 3) / 3;
    if (L > c->ekf.max_landmarks) return fail(c, ASLAM_E_CAPACITY, "state larger than max_landmarks");
    if (L > 0 && !landmark_ids) return fail(c, ASLAM_E_INVALID, "landmark ids required");
    { int rs = sync_streams(c); if (rs) return rs; }
    if (int r = write_state(c, ekf_fleet_robot(c->fslam, robot), N, mu, sigma, landmark_ids)) return r;
    if (int r = confirm_reseed(c, 1, &robot)) return r;
    return clear_track_health(c, robot, 1);
}

int aslam_fleet_get_landmark_ids(aslam_ctx* c, int robot, int* L, int* ids) {
    if (!c || !L) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kFleetSlam)) return r;
    if (robot < 0 || robot >= c->fleet_n) return fail(c, ASLAM_E_INVALID, "robot index outside the fleet");
    { int rs = sync_streams(c); if (rs) return rs; }
    return read_landmark_ids(c, ekf_fleet_robot(c->fslam, robot), L, ids);
}

// ---- landmark removal: marginalise landmarks out of a SLAM map on the device (include/aruco_slam_hip.h) ----------
namespace {
// the ids of a removal as the kernels take them (one bit per marker id); false: an id outside the table
bool removal_set(int n, const int* ids, unsigned* bits) {
    std::memset(bits, 0, sizeof(unsigned) * (kIdTableSize / 32));
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= kIdTableSize) return false;
        bits[ids[i] >> 5] |= 1u << (ids[i] & 31);
    }
    return true;
}

// the removal J.ids on the J.n filters of J (tables not yet set), streams synchronised by the caller: three launches on the EKF
// stream, the meta rows back in one copy, one wait.  removed: J.n entries or nullptr
int run_map_edit(aslam_ctx* c, MapEdit& J, int* removed) {
    HIP_TRY(c, map_edit_reserve(c->map_edit, J.n, J.base.ld));
    J.src_of = c->map_edit.src_of;
    J.meta = c->map_edit.meta;
    hipStream_t st = c->stream_ekf;
    prof_begin(c, P_MAP_PLAN, st);
    launch_map_plan(st, J);
    prof_end(c);
    prof_begin(c, P_MAP_COLS, st);
    launch_map_cols(st, J);
    prof_end(c);
    prof_begin(c, P_MAP_ROWS, st);
    launch_map_rows(st, J);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->map_edit.h_meta, J.meta, sizeof(int) * 4 * J.n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (removed)
        for (int k = 0; k < J.n; k++) removed[k] = c->map_edit.h_meta[4 * k + 2];
    return ASLAM_OK;
}
}  // namespace

int aslam_remove_landmarks(aslam_ctx* c, int n, const int* ids, int* removed) {
    if (!c) return ASLAM_E_INVALID;
    if (int r = allow(c, kSlam)) return r;
    if (n < 0 || (n > 0 && !ids)) return fail(c, ASLAM_E_INVALID, "remove landmarks: n >= 0 ids");
    MapEdit J{};
    if (!removal_set(n, ids, J.ids)) return fail(c, ASLAM_E_INVALID, "landmark id out of range");
    if (removed) *removed = 0;
    if (n == 0) return ASLAM_OK;
    { int rs = sync_streams(c); if (rs) return rs; }
    J.base = c->ekf;
    J.stride = 0;
    J.n = 1;
    int r = run_map_edit(c, J, removed);
    if (r) return r;
    c->mirror_dirty = true;
    if (int rc = confirm_reseed(c, 1, nullptr)) return rc;   // a removed id earns its place again
    return clear_track_health(c, kTrackSingle, 1);
}

int aslam_fleet_remove_landmarks(aslam_ctx* c, int n, const int* ids, int n_robots, const int* robots, int* removed) {
    if (!c) return ASLAM_E_INVALID;
    if (int r = allow(c, kFleetSlam)) return r;
    if (n < 0 || (n > 0 && !ids)) return fail(c, ASLAM_E_INVALID, "remove landmarks: n >= 0 ids");
    MapEdit J{};
    if (!removal_set(n, ids, J.ids)) return fail(c, ASLAM_E_INVALID, "landmark id out of range");
    const int R = c->fleet_n;
    if (!robots) n_robots = R;
    if (n_robots < 0) return fail(c, ASLAM_E_INVALID, "negative robot count");
    std::vector<char> listed(R, 0);
    for (int k = 0; k < n_robots; k++) {
        const int r = robots ? robots[k] : k;
        if (r < 0 || r >= R) return fail(c, ASLAM_E_INVALID, "robot index outside the fleet");
        if (listed[r]) return fail(c, ASLAM_E_INVALID, "robot listed twice");
        listed[r] = 1;
        J.robot[k] = (unsigned char)r;                 // R <= ASLAM_MAX_ROBOTS = kMapEditMaxFilters
    }
    if (removed) std::fill(removed, removed + n_robots, 0);
    if (n == 0 || n_robots == 0) return ASLAM_OK;
    { int rs = sync_streams(c); if (rs) return rs; }
    J.base = c->fslam.base;
    J.stride = c->fslam.stride;
    J.n = n_robots;
    if (int r = run_map_edit(c, J, removed)) return r;
    {
        std::vector<int> named(n_robots);
        for (int k = 0; k < n_robots; k++) named[k] = J.robot[k];
        if (int r = confirm_reseed(c, n_robots, named.data())) return r;
    }
    for (int k = 0; k < n_robots; k++)
        if (int r = clear_track_health(c, J.robot[k], 1)) return r;
    return ASLAM_OK;
}

// ---- map merge: one shared map from N maps in N frames (include/aruco_slam_hip.h) -------------------------------
namespace {
int merge_check(aslam_ctx* c, int n_maps, int anchor, int min_common, int max) {
    if (n_maps < 1 || n_maps > ASLAM_MAX_ROBOTS) return fail(c, ASLAM_E_INVALID, "a merge takes 1..ASLAM_MAX_ROBOTS maps");
    if (anchor < 0 || anchor >= n_maps) return fail(c, ASLAM_E_INVALID, "anchor outside the maps");
    if (min_common < 2 || min_common > kIdTableSize) return fail(c, ASLAM_E_INVALID, "min_common 2..1024");
    if (max < 0) return fail(c, ASLAM_E_INVALID, "negative max");
    return ASLAM_OK;
}

// the merge of n_maps x per_map device records on the EKF stream, and its results to the caller's (host) arrays: rounds, transforms,
// count and entries come back as one copy of the tables' tail into page-locked memory, after one wait
int merge_records(aslam_ctx* c, const MapRecord* d_rec, int n_maps, int per_map, int anchor, int min_common, int max, int* n, int* ids,
                  double* xyth, double* sigmas, int* n_seen, int* map_round, double* map_T) {
    const MergeBufs& M = c->merge;
    hipStream_t st = c->stream_ekf;
    HIP_TRY(c, merge_run(st, M, d_rec, n_maps, per_map, anchor, min_common, nullptr));
    HIP_TRY(c, hipMemcpyAsync(M.h_out, M.round, M.out_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    auto host = [&M](const void* d) { return M.h_out + (static_cast<const char*>(d) - reinterpret_cast<const char*>(M.round)); };
    int total = 0;
    std::memcpy(&total, host(M.out_n), sizeof(int));
    if (n) *n = total;
    if (map_round) std::memcpy(map_round, host(M.round), sizeof(int) * n_maps);
    if (map_T) std::memcpy(map_T, host(M.T), sizeof(double) * 3 * n_maps);
    const size_t k = (size_t)std::min(total, max);
    if (ids) std::memcpy(ids, host(M.out_ids), sizeof(int) * k);
    if (n_seen) std::memcpy(n_seen, host(M.out_seen), sizeof(int) * k);
    if (xyth) std::memcpy(xyth, host(M.out_xyth), sizeof(double) * 3 * k);
    if (sigmas) std::memcpy(sigmas, host(M.out_sigma), sizeof(double) * 9 * k);
    return ASLAM_OK;
}
}  // namespace

int aslam_merge_map_records(aslam_ctx* c, const void* records, int records_on_device, int n_maps, int per_map, int anchor, int min_common,
                            int max, int* n, int* ids, double* xyth, double* sigmas, int* n_seen, int* map_round, double* map_T) {
    if (!c || !records) return fail(c, ASLAM_E_INVALID, "null argument");
    if (per_map < 1 || per_map > kIdTableSize) return fail(c, ASLAM_E_INVALID, "1..1024 records per map");
    if (int r = merge_check(c, n_maps, anchor, min_common, max)) return r;
    HIP_TRY(c, merge_alloc(c->merge));
    const MapRecord* d_rec = static_cast<const MapRecord*>(records);
    if (!records_on_device) {
        const size_t count = (size_t)n_maps * per_map;
        HIP_TRY(c, merge_reserve_records(c->merge, count));
        HIP_TRY(c, hipMemcpyAsync(c->merge.rec, records, count * sizeof(MapRecord), hipMemcpyHostToDevice, c->stream_ekf));
        d_rec = c->merge.rec;
    }
    return merge_records(c, d_rec, n_maps, per_map, anchor, min_common, max, n, ids, xyth, sigmas, n_seen, map_round, map_T);
}

int aslam_fleet_merge_maps(aslam_ctx* c, int anchor, int min_common, int max, int* n, int* ids, double* xyth, double* sigmas, int* n_seen,
                           int* robot_round, double* robot_T) {
    if (!c) return ASLAM_E_INVALID;
    if (int r = allow(c, kFleetSlam)) return r;
    const int R = c->fleet_n, per_map = c->ekf.max_landmarks;
    if (int r = merge_check(c, R, anchor, min_common, max)) return r;     // per_map is the context's own capacity: any size
    { int rs = sync_and_check(c); if (rs) return rs; }
    HIP_TRY(c, merge_alloc(c->merge));
    HIP_TRY(c, merge_reserve_records(c->merge, (size_t)R * per_map));
    launch_fleet_export_maps(c->stream_ekf, c->fslam, c->merge.rec);
    HIP_TRY(c, hipGetLastError());
    return merge_records(c, c->merge.rec, R, per_map, anchor, min_common, max, n, ids, xyth, sigmas, n_seen, robot_round, robot_T);
}

int aslam_merge_scratch_bytes(aslam_ctx* c, long long* bytes) {
    if (!c || !bytes) return fail(c, ASLAM_E_INVALID, "null argument");
    *bytes = (long long)(c->merge.mem_bytes + c->merge.rec_cap * sizeof(MapRecord));
    return ASLAM_OK;
}

// ---- relocalization: lost poses from one frame against the frozen map (include/aruco_slam_hip.h) ----------------
void aslam_default_relocalize_params(aslam_relocalize_params* p) {
    if (!p) return;
    p->tol_xy = 0.25;
    p->tol_th = 0.2;
    p->min_inliers = 2;
}

namespace {
int reloc_params(aslam_ctx* c, const aslam_relocalize_params* params, RelocParams& out) {
    aslam_relocalize_params p;
    aslam_default_relocalize_params(&p);
    if (params) p = *params;
    if (!std::isfinite(p.tol_xy) || !(p.tol_xy > 0.0)) return fail(c, ASLAM_E_INVALID, "tol_xy must be finite and positive");
    if (!std::isfinite(p.tol_th) || !(p.tol_th > 0.0) || p.tol_th >= 3.14159265358979323846)
        return fail(c, ASLAM_E_INVALID, "tol_th must be finite, positive and below pi");
    if (p.min_inliers < 1 || p.min_inliers > kMarkerMax) return fail(c, ASLAM_E_INVALID, "min_inliers 1..128");
    out.tol_xy2 = p.tol_xy * p.tol_xy;
    out.tol_th = p.tol_th;
    out.min_inliers = p.min_inliers;
    return ASLAM_OK;
}

// k_relocalize on slots [first, first + count) on the EKF stream, behind the detection that produced their lists and every EKF step
// enqueued so far: one launch, one copy of the records into page-locked memory, one wait.  d_robots: the robots' indices on the
// device (a fleet), or nullptr (the single filter).
int relocalize_slots(aslam_ctx* c, int first, int count, const int* d_robots, const RelocParams& prm, int apply, aslam_relocalize_result* out) {
    HIP_TRY(c, reloc_alloc(c->reloc, c->max_batch));
    hipStream_t st = c->stream_ekf;
    HIP_TRY(c, hipStreamWaitEvent(st, c->ev_detect, 0));
    launch_relocalize(st, c->ekf, c->fleet, prm, c->d_obs, c->d_nmarkers, first, count, d_robots, apply, c->reloc.d);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->reloc.h, c->reloc.d, sizeof(RelocRecord) * count, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    for (int i = 0; i < count; i++) {
        const RelocRecord& r = c->reloc.h[i];
        aslam_relocalize_result& o = out[i];
        o.status = r.status; o.n_candidates = r.n_candidates; o.n_inliers = r.n_inliers; o.runner_up = r.runner_up; o.best = r.best;
        std::memcpy(o.pose, r.pose, sizeof(o.pose));
        std::memcpy(o.sigma, r.sigma, sizeof(o.sigma));
    }
    return ASLAM_OK;
}
}  // namespace

int aslam_relocalize(aslam_ctx* c, int slot, const aslam_relocalize_params* params, int apply, aslam_relocalize_result* out) {
    if (!c || !out) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kLocalize)) return r;
    RelocParams prm{};
    if (int r = reloc_params(c, params, prm)) return r;
    if (int r = check_slot_range(c, slot, 1)) return r;
    if (int r = finalize_pending(c)) return r;
    if (int r = relocalize_slots(c, slot, 1, nullptr, prm, apply ? 1 : 0, out)) return r;
    if (apply && out->status == 0) {                                            // seated
        if (int r = clear_cross(c, -1, c->stream_ekf)) return r;
        return clear_track_health(c, kTrackSingle, 1, c->stream_ekf);
    }
    return ASLAM_OK;
}

int aslam_fleet_relocalize(aslam_ctx* c, int first, int count, const int* robot_of_slot, const aslam_relocalize_params* params, int apply,
                           aslam_relocalize_result* out) {
    if (!c || !robot_of_slot || !out) return fail(c, ASLAM_E_INVALID, "null argument");
    if (c->mode == Mode::FleetSlam) return fail(c, ASLAM_E_STATE, "fleet SLAM: every robot has a map of its own, there is no shared map to relocalize against");
    if (int r = allow(c, kFleetLocalize)) return r;
    RelocParams prm{};
    if (int r = reloc_params(c, params, prm)) return r;
    if (int r = check_slot_range(c, first, count)) return r;
    std::vector<char> seen(c->fleet_n, 0);
    for (int i = 0; i < count; i++) {
        if (robot_of_slot[i] < 0 || robot_of_slot[i] >= c->fleet_n) return fail(c, ASLAM_E_INVALID, "robot index outside the fleet");
        if (seen[robot_of_slot[i]]) return fail(c, ASLAM_E_INVALID, "a robot named twice in one aslam_fleet_relocalize");
        seen[robot_of_slot[i]] = 1;
    }
    if (int r = finalize_pending(c)) return r;
    if (int r = pinned_upload(c, c->fleet_work_up, c->d_fleet_work, robot_of_slot, count, c->stream_ekf)) return r;
    if (int r = relocalize_slots(c, first, count, c->d_fleet_work, prm, apply ? 1 : 0, out)) return r;
    if (apply)
        for (int i = 0; i < count; i++)
            if (out[i].status == 0) {                                          // seated as by aslam_fleet_set_pose: its next frame only arms it
                c->fleet_armed[robot_of_slot[i]] = 0;
                if (int r = clear_cross(c, robot_of_slot[i], c->stream_ekf)) return r;
                if (int r = clear_track_health(c, robot_of_slot[i], 1, c->stream_ekf)) return r;
            }
    return ASLAM_OK;
}

// ---- SLAM relocalization: a lost SLAM filter against its own map (include/aruco_slam_hip.h) ----------------------
namespace {
// k_slam_reloc_solve and k_slam_reloc_seat on slots [first, first + count) on the EKF stream, behind the detection that produced
// their lists and every EKF step enqueued so far (the caller has finalised a pending batch: its windows end with their flush on this
// stream); the records back in one copy, one wait.  d_robots: the robots' indices on the device (a SLAM fleet), or nullptr
int slam_relocalize_slots(aslam_ctx* c, const EkfState& base, size_t stride, int first, int count, const int* d_robots, const RelocParams& prm,
                          int apply, aslam_relocalize_result* out) {
    HIP_TRY(c, reloc_alloc(c->reloc, c->max_batch));
    HIP_TRY(c, slam_reloc_alloc(c->slam_reloc, c->max_batch));
    hipStream_t st = c->stream_ekf;
    HIP_TRY(c, hipStreamWaitEvent(st, c->ev_detect, 0));
    SlamReloc A{};
    A.base = base; A.stride = stride; A.robot_of_slot = d_robots; A.prm = prm; A.obs = c->d_obs; A.n_markers = c->d_nmarkers;
    A.first = first; A.apply = apply; A.out = c->reloc.d; A.seat = c->slam_reloc.seat;
    prof_begin(c, P_SLAM_RELOC_SOLVE, st);
    launch_slam_reloc_solve(st, A, count);
    prof_end(c);
    prof_begin(c, P_SLAM_RELOC_SEAT, st);
    launch_slam_reloc_seat(st, A, count);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->reloc.h, c->reloc.d, sizeof(RelocRecord) * count, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    for (int i = 0; i < count; i++) {
        const RelocRecord& r = c->reloc.h[i];
        aslam_relocalize_result& o = out[i];
        o.status = r.status; o.n_candidates = r.n_candidates; o.n_inliers = r.n_inliers; o.runner_up = r.runner_up; o.best = r.best;
        std::memcpy(o.pose, r.pose, sizeof(o.pose));
        std::memcpy(o.sigma, r.sigma, sizeof(o.sigma));
    }
    return ASLAM_OK;
}
}  // namespace

int aslam_slam_relocalize(aslam_ctx* c, int slot, const aslam_relocalize_params* params, int apply, aslam_relocalize_result* out) {
    if (!c || !out) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kSlam)) return r;
    RelocParams prm{};
    if (int r = reloc_params(c, params, prm)) return r;
    if (int r = check_slot_range(c, slot, 1)) return r;
    if (int r = finalize_pending(c)) return r;
    if (int r = slam_relocalize_slots(c, c->ekf, 0, slot, 1, nullptr, prm, apply ? 1 : 0, out)) return r;
    if (apply && out->status == 0) {                                            // seated: the window planner's mirror holds the old last-observed list
        c->mirror_dirty = true;
        return clear_track_health(c, kTrackSingle, 1, c->stream_ekf);
    }
    return ASLAM_OK;
}

int aslam_fleet_slam_relocalize(aslam_ctx* c, int first, int count, const int* robot_of_slot, const aslam_relocalize_params* params, int apply,
                                aslam_relocalize_result* out) {
    if (!c || !robot_of_slot || !out) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kFleetSlam)) return r;
    RelocParams prm{};
    if (int r = reloc_params(c, params, prm)) return r;
    if (int r = check_slot_range(c, first, count)) return r;
    std::vector<char> seen(c->fleet_n, 0);
    for (int i = 0; i < count; i++) {
        if (robot_of_slot[i] < 0 || robot_of_slot[i] >= c->fleet_n) return fail(c, ASLAM_E_INVALID, "robot index outside the fleet");
        if (seen[robot_of_slot[i]]) return fail(c, ASLAM_E_INVALID, "a robot named twice in one aslam_fleet_slam_relocalize");
        seen[robot_of_slot[i]] = 1;
    }
    if (int r = finalize_pending(c)) return r;
    if (int r = pinned_upload(c, c->fleet_work_up, c->d_fleet_work, robot_of_slot, count, c->stream_ekf)) return r;
    if (int r = slam_relocalize_slots(c, c->fslam.base, c->fslam.stride, first, count, c->d_fleet_work, prm, apply ? 1 : 0, out)) return r;
    if (apply)
        for (int i = 0; i < count; i++)
            if (out[i].status == 0)                                            // seated as by aslam_fleet_set_state: the arming stays
                if (int r = clear_track_health(c, robot_of_slot[i], 1, c->stream_ekf)) return r;
    return ASLAM_OK;
}

// ---- innovation gate and lost-track detection (include/aruco_slam_hip.h) -------------------------------------------
static_assert(kTrackSingle == ASLAM_MAX_ROBOTS, "the single filter's track record follows the robots'");
static_assert(sizeof(SlotHealth) == sizeof(aslam_slot_health) && sizeof(TrackHealth) == sizeof(aslam_track_health), "records are copied as they are");

void aslam_default_gate_params(aslam_gate_params* p) {
    if (!p) return;
    p->gate_d2 = 16.266;                 // the 0.999 quantile of chi-square with 3 degrees of freedom
    p->min_attempted = 2;
    p->min_accept_percent = 50;
    p->lost_after = 3;
    p->pad = 0;
}

namespace {
int check_gate_params(aslam_ctx* c, const aslam_gate_params& p) {
    if (!(p.gate_d2 > 0.0)) return fail(c, ASLAM_E_INVALID, "gate_d2 must be positive, or +inf to monitor only");
    if (p.min_attempted < 1) return fail(c, ASLAM_E_INVALID, "min_attempted >= 1");
    if (p.min_accept_percent < 0 || p.min_accept_percent > 100) return fail(c, ASLAM_E_INVALID, "min_accept_percent 0..100");
    if (p.lost_after < 1) return fail(c, ASLAM_E_INVALID, "lost_after >= 1");
    return ASLAM_OK;
}

// the health records and their page-locked copies, made by whichever gate is set first
int alloc_health(aslam_ctx* c) {
    if (!c->gate.track) {
        const size_t ns = (size_t)c->ekf.max_slots, nt = (size_t)kTrackSingle + 1;
        SlotHealth* d_slot = nullptr;
        HIP_TRY(c, dalloc(&d_slot, ns));
        c->gate.slot = d_slot;
        HIP_TRY(c, hipMemset(c->gate.slot, 0, ns * sizeof(SlotHealth)));
        HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_slot_health), ns * sizeof(SlotHealth), hipHostMallocDefault));
        HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_track_health), nt * sizeof(TrackHealth), hipHostMallocDefault));
        TrackHealth* d_track = nullptr;
        HIP_TRY(c, dalloc(&d_track, nt));
        HIP_TRY(c, hipMemset(d_track, 0, nt * sizeof(TrackHealth)));
        c->gate.track = d_track;         // set last: the records exist exactly when this is set
    }
    return ASLAM_OK;
}
}  // namespace

int aslam_set_innovation_gate(aslam_ctx* c, const aslam_gate_params* params) {
    if (!c) return ASLAM_E_INVALID;
    if (!params) { c->gate_on = false; return ASLAM_OK; }
    const aslam_gate_params& p = *params;
    if (int r = check_gate_params(c, p)) return r;
    if (int r = alloc_health(c)) return r;
    c->gate_prm = p;
    c->gate_prm.pad = 0;
    c->gate.gate_d2 = p.gate_d2;
    c->gate.min_attempted = p.min_attempted;
    c->gate.min_accept_percent = p.min_accept_percent;
    c->gate.lost_after = p.lost_after;
    c->gate_on = true;
    return ASLAM_OK;
}

int aslam_get_innovation_gate(aslam_ctx* c, int* on, aslam_gate_params* out) {
    if (!c || !on) return fail(c, ASLAM_E_INVALID, "null argument");
    *on = c->gate_on ? 1 : 0;
    if (out) {
        if (c->gate_on) *out = c->gate_prm;
        else aslam_default_gate_params(out);
    }
    return ASLAM_OK;
}

// ---- innovation gate of the SLAM chains (include/aruco_slam_hip.h) --------------------------------------------------
int aslam_set_slam_gate(aslam_ctx* c, const aslam_gate_params* params) {
    if (!c) return ASLAM_E_INVALID;
    if (params)
        if (int r = check_gate_params(c, *params)) return r;
    // a batch still pending was submitted under the setting in force so far: its windows (or per-frame steps) are enqueued first
    if (int r = finalize_pending(c)) return r;
    if (!params) { c->slam_gate_on = false; return ASLAM_OK; }
    if (int r = alloc_health(c)) return r;
    if (!c->slam_gate.verdicts) {
        const size_t filters = (size_t)std::max(1, std::min(c->max_batch, ASLAM_MAX_ROBOTS));   // the single filter, or the robots of a round
        HIP_TRY(c, dalloc(&c->slam_gate.verdicts, filters * 2 * kMarkerMax));
        HIP_TRY(c, hipMemset(c->slam_gate.verdicts, 0, filters * 2 * kMarkerMax * sizeof(double)));
    }
    const aslam_gate_params& p = *params;
    c->slam_gate_prm = p;
    c->slam_gate_prm.pad = 0;
    c->slam_gate.g = c->gate;            // the records; the parameters are this gate's own
    c->slam_gate.g.gate_d2 = p.gate_d2;
    c->slam_gate.g.min_attempted = p.min_attempted;
    c->slam_gate.g.min_accept_percent = p.min_accept_percent;
    c->slam_gate.g.lost_after = p.lost_after;
    c->slam_gate_on = true;
    return ASLAM_OK;
}

// ---- the SLAM gate inside EKF windows (include/aruco_slam_hip.h) ------------------------------------------------------
int aslam_set_slam_gate_windows(aslam_ctx* c, int on) {
    if (!c) return ASLAM_E_INVALID;
    // a batch still pending was submitted under the setting in force so far: its windows (or per-frame steps) are enqueued first
    if (int r = finalize_pending(c)) return r;
    c->slam_gate_windows = on != 0;        // (the verdicts travel in the window's log header: nothing to allocate)
    return ASLAM_OK;
}

int aslam_get_slam_gate_windows(aslam_ctx* c, int* on) {
    if (!c || !on) return fail(c, ASLAM_E_INVALID, "null argument");
    *on = c->slam_gate_windows ? 1 : 0;
    return ASLAM_OK;
}

int aslam_get_slam_gate(aslam_ctx* c, int* on, aslam_gate_params* out) {
    if (!c || !on) return fail(c, ASLAM_E_INVALID, "null argument");
    *on = c->slam_gate_on ? 1 : 0;
    if (out) {
        if (c->slam_gate_on) *out = c->slam_gate_prm;
        else aslam_default_gate_params(out);
    }
    return ASLAM_OK;
}

// ---- landmark confirmation (include/aruco_slam_hip.h) ------------------------------------------------------------------
static_assert(kConfirmSingle == ASLAM_MAX_ROBOTS, "the single filter's table follows the robots'");
static_assert(sizeof(SlotConfirm) == sizeof(aslam_slot_confirm), "records are copied as they are");

void aslam_default_confirm_params(aslam_confirm_params* p) {
    if (!p) return;
    p->min_sightings = 3;
    p->max_gap = 10;
}

int aslam_set_landmark_confirmation(aslam_ctx* c, const aslam_confirm_params* params) {
    if (!c) return ASLAM_E_INVALID;
    if (params) {
        if (params->min_sightings < 2 || params->min_sightings > 127) return fail(c, ASLAM_E_INVALID, "min_sightings 2..127");
        if (params->max_gap < 1 || params->max_gap > 1000000) return fail(c, ASLAM_E_INVALID, "max_gap 1..1000000 frames");
    }
    // a batch still pending was submitted under the setting in force so far: it is enqueued first, and everything enqueued finishes
    if (int r = sync_streams(c)) return r;
    if (!params) { c->confirm_on = false; return ASLAM_OK; }
    if (!c->ev_confirm) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_confirm, hipEventDisableTiming));
    if (!c->d_confirm_rec) {
        const size_t ns = (size_t)c->ekf.max_slots;
        HIP_TRY(c, dalloc(&c->d_confirm_rec, ns));
        HIP_TRY(c, hipMemset(c->d_confirm_rec, 0, ns * sizeof(SlotConfirm)));
    }
    if (!c->h_confirm)
        HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_confirm), std::max(sizeof(ConfirmTable), (size_t)c->ekf.max_slots * sizeof(SlotConfirm)),
                                 hipHostMallocDefault));
    if (!c->d_confirm) {
        ConfirmTable* d = nullptr;
        HIP_TRY(c, dalloc(&d, (size_t)kConfirmSingle + 1));
        HIP_TRY(c, hipMemset(d, 0, ((size_t)kConfirmSingle + 1) * sizeof(ConfirmTable)));
        c->d_confirm = d;
    }
    c->confirm_prm = *params;
    c->confirm_on = true;
    // every SLAM filter present starts from its map as it stands (a frozen map's filter is reseeded by aslam_localize_end)
    if (c->mode == Mode::Slam) return confirm_reseed(c, 1, nullptr);
    if (c->mode == Mode::FleetSlam) return confirm_reseed_fleet(c);
    return ASLAM_OK;
}

int aslam_get_landmark_confirmation(aslam_ctx* c, int* on, aslam_confirm_params* out) {
    if (!c || !on) return fail(c, ASLAM_E_INVALID, "null argument");
    *on = c->confirm_on ? 1 : 0;
    if (out) {
        if (c->confirm_on) *out = c->confirm_prm;
        else aslam_default_confirm_params(out);
    }
    return ASLAM_OK;
}

int aslam_get_slot_confirm(aslam_ctx* c, int first, int count, aslam_slot_confirm* out) {
    if (!c || !out) return fail(c, ASLAM_E_INVALID, "null argument");
    if (!c->confirm_on) return fail(c, ASLAM_E_STATE, "landmark confirmation is off (aslam_set_landmark_confirmation first)");
    if (first < 0 || count < 1 || count > c->ekf.max_slots || first > c->ekf.max_slots - count)
        return fail(c, ASLAM_E_INVALID, "EKF slot range outside [0, 2 max_batch)");
    { int rs = sync_streams(c); if (rs) return rs; }
    HIP_TRY(c, hipMemcpyAsync(c->h_confirm, c->d_confirm_rec + first, sizeof(SlotConfirm) * count, hipMemcpyDeviceToHost, c->stream_ekf));
    HIP_TRY(c, hipStreamSynchronize(c->stream_ekf));
    std::memcpy(out, c->h_confirm, sizeof(SlotConfirm) * count);
    return ASLAM_OK;
}

namespace {
// the tentative ids of table `table`, ascending: count > 0 and last sighted at most max_gap frames ago
int read_tentative(aslam_ctx* c, int table, int max, int* n, int* ids, int* counts, int* ages) {
    if (max < 0 || (max > 0 && (!ids || !counts || !ages))) return fail(c, ASLAM_E_INVALID, "max entries need output arrays");
    { int rs = sync_streams(c); if (rs) return rs; }
    HIP_TRY(c, hipMemcpyAsync(c->h_confirm, c->d_confirm + table, sizeof(ConfirmTable), hipMemcpyDeviceToHost, c->stream_ekf));
    HIP_TRY(c, hipStreamSynchronize(c->stream_ekf));
    const ConfirmTable& T = *reinterpret_cast<const ConfirmTable*>(c->h_confirm);
    int k = 0;
    for (int id = 0; id < kIdTableSize; id++) {
        if (T.cnt[id] <= 0 || T.t - T.last[id] > c->confirm_prm.max_gap) continue;
        if (k < max) { ids[k] = id; counts[k] = T.cnt[id]; ages[k] = T.t - T.last[id]; }
        k++;
    }
    *n = k;
    return ASLAM_OK;
}
}  // namespace

int aslam_get_tentative(aslam_ctx* c, int max, int* n, int* ids, int* counts, int* ages) {
    if (!c || !n) return fail(c, ASLAM_E_INVALID, "null argument");
    if (!c->confirm_on) return fail(c, ASLAM_E_STATE, "landmark confirmation is off (aslam_set_landmark_confirmation first)");
    if (int r = allow(c, kSlam)) return r;
    return read_tentative(c, kConfirmSingle, max, n, ids, counts, ages);
}

int aslam_fleet_get_tentative(aslam_ctx* c, int robot, int max, int* n, int* ids, int* counts, int* ages) {
    if (!c || !n) return fail(c, ASLAM_E_INVALID, "null argument");
    if (!c->confirm_on) return fail(c, ASLAM_E_STATE, "landmark confirmation is off (aslam_set_landmark_confirmation first)");
    if (int r = allow(c, kFleetSlam)) return r;
    if (robot < 0 || robot >= c->fleet_n) return fail(c, ASLAM_E_INVALID, "robot index outside the fleet");
    return read_tentative(c, robot, max, n, ids, counts, ages);
}

// ---- pose ambiguity check (include/aruco_slam_hip.h) --------------------------------------------------------------------
static_assert(sizeof(PoseAmbiguity) == sizeof(aslam_pose_ambiguity), "records are copied as they are");
static_assert(sizeof(SlotPoseAmbiguity) == sizeof(aslam_slot_pose_ambiguity), "records are copied as they are");

void aslam_default_pose_ambiguity_params(aslam_pose_ambiguity_params* p) {
    if (!p) return;
    p->ratio = 1.5;
    p->floor_px = 0.5;
    p->min_dtheta = 0.05;
    p->reject = 1;
    p->pad = 0;
}

int aslam_set_pose_ambiguity(aslam_ctx* c, const aslam_pose_ambiguity_params* params) {
    if (!c) return ASLAM_E_INVALID;
    if (params) {
        if (!(std::isfinite(params->ratio) && params->ratio >= 1.0)) return fail(c, ASLAM_E_INVALID, "ratio >= 1, finite");
        if (!(std::isfinite(params->floor_px) && params->floor_px >= 0.0)) return fail(c, ASLAM_E_INVALID, "floor_px >= 0, finite");
        if (!(params->min_dtheta >= 0.0 && params->min_dtheta < 3.14159265358979323846)) return fail(c, ASLAM_E_INVALID, "min_dtheta in [0, pi)");
        if (params->reject != 0 && params->reject != 1) return fail(c, ASLAM_E_INVALID, "reject 0 or 1");
    }
    // a batch still pending was submitted under the setting in force so far: it is enqueued first, and everything enqueued finishes
    if (int r = sync_streams(c)) return r;
    if (!params) { c->pose_amb_on = false; return ASLAM_OK; }
    if (!c->d_pose_amb) {
        const size_t n = (size_t)c->max_batch * kMarkerMax;
        HIP_TRY(c, dalloc(&c->d_pose_amb, n));
        HIP_TRY(c, hipMemset(c->d_pose_amb, 0, n * sizeof(PoseAmbiguity)));
    }
    if (!c->d_pose_amb_sum) {
        HIP_TRY(c, dalloc(&c->d_pose_amb_sum, (size_t)c->max_batch));
        HIP_TRY(c, hipMemset(c->d_pose_amb_sum, 0, (size_t)c->max_batch * sizeof(SlotPoseAmbiguity)));
    }
    c->pose_amb_prm = *params;
    c->pose_amb_prm.pad = 0;
    c->pose_amb_on = true;
    return ASLAM_OK;
}

int aslam_get_pose_ambiguity(aslam_ctx* c, int* on, aslam_pose_ambiguity_params* out) {
    if (!c || !on) return fail(c, ASLAM_E_INVALID, "null argument");
    *on = c->pose_amb_on ? 1 : 0;
    if (out) {
        if (c->pose_amb_on) *out = c->pose_amb_prm;
        else aslam_default_pose_ambiguity_params(out);
    }
    return ASLAM_OK;
}

int aslam_get_slot_pose_ambiguity(aslam_ctx* c, int slot, int max, int* n, aslam_pose_ambiguity* out, aslam_slot_pose_ambiguity* sum) {
    if (!c || !n) return fail(c, ASLAM_E_INVALID, "null argument");
    if (!c->pose_amb_on) return fail(c, ASLAM_E_STATE, "the pose ambiguity check is off (aslam_set_pose_ambiguity first)");
    if (int r = check_slot_range(c, slot, 1)) return r;
    if (max < 0 || (max > 0 && !out)) return fail(c, ASLAM_E_INVALID, "max records need an output array");
    { int rs = sync_streams(c); if (rs) return rs; }
    SlotPoseAmbiguity s{};
    HIP_TRY(c, hipMemcpy(&s, c->d_pose_amb_sum + slot, sizeof(s), hipMemcpyDeviceToHost));
    const int m = std::min(std::max(s.checked, 0), kMarkerMax);
    *n = m;
    const int w = std::min(m, max);
    if (w > 0) HIP_TRY(c, hipMemcpy(out, c->d_pose_amb + (size_t)slot * kMarkerMax, (size_t)w * sizeof(PoseAmbiguity), hipMemcpyDeviceToHost));
    if (sum) std::memcpy(sum, &s, sizeof(s));
    return ASLAM_OK;
}

// ---- observation covariance (include/aruco_slam_hip.h) ------------------------------------------------------------------
static_assert(sizeof(ObsCovariance) == sizeof(aslam_obs_covariance), "records are copied as they are");
static_assert(sizeof(SlotObsCovariance) == sizeof(aslam_slot_obs_covariance), "records are copied as they are");

void aslam_default_obs_covariance_params(aslam_obs_covariance_params* p) {
    if (!p) return;
    p->sigma_px = 0.5;
    p->scale = 1.0;
    p->floor_xy = 1e-6;
    p->floor_th = 1e-6;
    p->gate_norm = 1.0;
    p->use_residual = 1;
    p->pad = 0;
}

int aslam_set_observation_covariance(aslam_ctx* c, const aslam_obs_covariance_params* params) {
    if (!c) return ASLAM_E_INVALID;
    if (params) {
        if (!(std::isfinite(params->sigma_px) && params->sigma_px > 0.0)) return fail(c, ASLAM_E_INVALID, "sigma_px > 0, finite");
        if (!(std::isfinite(params->scale) && params->scale > 0.0)) return fail(c, ASLAM_E_INVALID, "scale > 0, finite");
        if (!(std::isfinite(params->floor_xy) && params->floor_xy >= 0.0)) return fail(c, ASLAM_E_INVALID, "floor_xy >= 0, finite");
        if (!(std::isfinite(params->floor_th) && params->floor_th >= 0.0)) return fail(c, ASLAM_E_INVALID, "floor_th >= 0, finite");
        if (!(params->gate_norm > 0.0)) return fail(c, ASLAM_E_INVALID, "gate_norm > 0 (+inf allowed)");
        if (params->use_residual != 0 && params->use_residual != 1) return fail(c, ASLAM_E_INVALID, "use_residual 0 or 1");
    }
    // a batch still pending was submitted under the setting in force so far: it is enqueued first, and everything enqueued finishes
    if (int r = sync_streams(c)) return r;
    if (!params) { c->obs_cov_on = false; return ASLAM_OK; }
    if (!c->d_obs_cov) {
        const size_t n = (size_t)c->max_batch * kMarkerMax;
        HIP_TRY(c, dalloc(&c->d_obs_cov, n));
        HIP_TRY(c, hipMemset(c->d_obs_cov, 0, n * sizeof(ObsCovariance)));
    }
    if (!c->d_obs_cov_sum) {
        HIP_TRY(c, dalloc(&c->d_obs_cov_sum, (size_t)c->max_batch));
        HIP_TRY(c, hipMemset(c->d_obs_cov_sum, 0, (size_t)c->max_batch * sizeof(SlotObsCovariance)));
    }
    c->obs_cov_prm = *params;
    c->obs_cov_prm.pad = 0;
    c->obs_cov_on = true;
    return ASLAM_OK;
}

int aslam_get_observation_covariance(aslam_ctx* c, int* on, aslam_obs_covariance_params* out) {
    if (!c || !on) return fail(c, ASLAM_E_INVALID, "null argument");
    *on = c->obs_cov_on ? 1 : 0;
    if (out) {
        if (c->obs_cov_on) *out = c->obs_cov_prm;
        else aslam_default_obs_covariance_params(out);
    }
    return ASLAM_OK;
}

int aslam_get_slot_obs_covariance(aslam_ctx* c, int slot, int max, int* n, aslam_obs_covariance* out, aslam_slot_obs_covariance* sum) {
    if (!c || !n) return fail(c, ASLAM_E_INVALID, "null argument");
    if (!c->obs_cov_on) return fail(c, ASLAM_E_STATE, "the observation covariance is off (aslam_set_observation_covariance first)");
    if (int r = check_slot_range(c, slot, 1)) return r;
    if (max < 0 || (max > 0 && !out)) return fail(c, ASLAM_E_INVALID, "max records need an output array");
    { int rs = sync_streams(c); if (rs) return rs; }
    SlotObsCovariance s{};
    HIP_TRY(c, hipMemcpy(&s, c->d_obs_cov_sum + slot, sizeof(s), hipMemcpyDeviceToHost));
    const int m = std::min(std::max(s.checked, 0), kMarkerMax);
    *n = m;
    const int w = std::min(m, max);
    if (w > 0) HIP_TRY(c, hipMemcpy(out, c->d_obs_cov + (size_t)slot * kMarkerMax, (size_t)w * sizeof(ObsCovariance), hipMemcpyDeviceToHost));
    if (sum) std::memcpy(sum, &s, sizeof(s));
    return ASLAM_OK;
}

// Consistent innovations: one switch per context, in any mode, kept across mode changes
int aslam_set_consistent_innovations(aslam_ctx* c, int on) {
    if (!c) return ASLAM_E_INVALID;
    if (on != 0 && on != 1) return fail(c, ASLAM_E_INVALID, "on: 0 or 1");
    // a batch still pending was submitted under the setting in force so far: it is enqueued first, and everything enqueued finishes
    if (int r = sync_streams(c)) return r;
    c->consistent_on = on == 1;
    return ASLAM_OK;
}

int aslam_get_consistent_innovations(aslam_ctx* c, int* on) {
    if (!c || !on) return fail(c, ASLAM_E_INVALID, "null argument");
    *on = c->consistent_on ? 1 : 0;
    return ASLAM_OK;
}

// Consistent innovations inside EKF windows: one switch per context, in any mode, kept across mode changes
int aslam_set_consistent_windows(aslam_ctx* c, int on) {
    if (!c) return ASLAM_E_INVALID;
    if (on != 0 && on != 1) return fail(c, ASLAM_E_INVALID, "on: 0 or 1");
    // a batch still pending was submitted under the setting in force so far: it is enqueued first, and everything enqueued finishes
    if (int r = sync_streams(c)) return r;
    c->consistent_windows = on == 1;
    return ASLAM_OK;
}

int aslam_get_consistent_windows(aslam_ctx* c, int* on) {
    if (!c || !on) return fail(c, ASLAM_E_INVALID, "null argument");
    *on = c->consistent_windows ? 1 : 0;
    return ASLAM_OK;
}

// The SLAM gate on the running innovation inside EKF windows: one switch per context, in any mode, kept across mode changes
int aslam_set_gated_consistent_windows(aslam_ctx* c, int on) {
    if (!c) return ASLAM_E_INVALID;
    if (on != 0 && on != 1) return fail(c, ASLAM_E_INVALID, "on: 0 or 1");
    // a batch still pending was submitted under the setting in force so far: it is enqueued first, and everything enqueued finishes
    if (int r = sync_streams(c)) return r;
    c->gated_consistent_windows = on == 1;
    return ASLAM_OK;
}

int aslam_get_gated_consistent_windows(aslam_ctx* c, int* on) {
    if (!c || !on) return fail(c, ASLAM_E_INVALID, "null argument");
    *on = c->gated_consistent_windows ? 1 : 0;
    return ASLAM_OK;
}

namespace {
// what every health getter checks first.  In a SLAM mode (SLAM, fleet SLAM) the records are the SLAM gate's: readable while it is set
// and the getter serves that mode (slam_modes).  In the localization modes they are the innovation gate's, as before (loc_modes).
int gate_readable(aslam_ctx* c, unsigned loc_modes, unsigned slam_modes) {
    if (in(c->mode) & slam_modes) {
        if (c->slam_gate_on) return ASLAM_OK;
        return fail(c, ASLAM_E_STATE, "no SLAM gate set (aslam_set_slam_gate first; the innovation gate covers the localization modes only)");
    }
    if ((in(c->mode) & loc_modes) && !c->gate_on) return fail(c, ASLAM_E_STATE, "no innovation gate set (aslam_set_innovation_gate first)");
    return allow(c, loc_modes);
}

// bytes of records from the device array d into the page-locked h behind the EKF steps enqueued so far, then to out
int read_health(aslam_ctx* c, const void* d, void* h, size_t bytes, void* out) {
    { int rs = sync_streams(c); if (rs) return rs; }
    HIP_TRY(c, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream_ekf));
    HIP_TRY(c, hipStreamSynchronize(c->stream_ekf));
    std::memcpy(out, h, bytes);
    return ASLAM_OK;
}
}  // namespace

int aslam_get_slot_health(aslam_ctx* c, int first, int count, aslam_slot_health* out) {
    if (!c || !out) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = gate_readable(c, kLocalize | kFleetLocalize, kSlam | kFleetSlam)) return r;
    if (first < 0 || count < 1 || count > c->ekf.max_slots || first > c->ekf.max_slots - count)
        return fail(c, ASLAM_E_INVALID, "EKF slot range outside [0, 2 max_batch)");
    return read_health(c, c->gate.slot + first, c->h_slot_health, sizeof(SlotHealth) * count, out);
}

int aslam_get_track_health(aslam_ctx* c, aslam_track_health* out) {
    if (!c || !out) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = gate_readable(c, kLocalize, kSlam)) return r;
    return read_health(c, c->gate.track + kTrackSingle, c->h_track_health, sizeof(TrackHealth), out);
}

int aslam_fleet_get_health(aslam_ctx* c, int max, int* n_robots, aslam_track_health* out) {
    if (!c || !n_robots) return fail(c, ASLAM_E_INVALID, "null argument");
    if (max < 0 || (max > 0 && !out)) return fail(c, ASLAM_E_INVALID, "max records need an output array");
    if (int r = gate_readable(c, kFleetLocalize, kFleetSlam)) return r;
    *n_robots = c->fleet_n;
    const int n = std::min(max, c->fleet_n);
    if (n == 0) return ASLAM_OK;
    return read_health(c, c->gate.track, c->h_track_health, sizeof(TrackHealth) * n, out);
}

// MapLoader markers -> planar landmarks: heading of the marker's +z axis (third column of Matrix3x3(orientation)), which is what an
// observation's atan2(-R02, R22) measures (aruco_slam.cpp:361)
int aslam_landmarks_from_markers(int n, const aslam_marker_msg* in, int* ids, double* xyth) {
    if (n < 0 || (n > 0 && (!in || !ids || !xyth))) { host_err = "null argument"; return ASLAM_E_INVALID; }
    const double PI = 3.14159265358979323846;
    for (int i = 0; i < n; i++) {
        const double ez[3] = {0.0, 0.0, 1.0};
        double r[3];
        quat_rotate(in[i].orientation, ez, r);
        if (!(std::hypot(r[0], r[1]) >= 1e-6)) {
            host_err = "marker " + std::to_string(in[i].id) + ": its +z axis has no horizontal component (the marker lies flat), no heading";
            return ASLAM_E_INVALID;
        }
        double th = std::atan2(r[1], r[0]);
        if (th >= PI) th -= 2.0 * PI;                                   // normAngle (aruco_slam.cpp:412-421)
        if (th < -PI) th += 2.0 * PI;
        ids[i] = in[i].id;
        xyth[3 * i] = in[i].position[0]; xyth[3 * i + 1] = in[i].position[1]; xyth[3 * i + 2] = th;
    }
    return ASLAM_OK;
}

// ---- persistence (no counterpart in the reference: warm starts of large maps) ----------------------------
int aslam_save_state(aslam_ctx* c, const char* path) {
    if (!c || !path) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kSingle)) return r;
    int N = 0;
    int r = aslam_get_state(c, &N, nullptr, nullptr);
    if (r) return r;
    const int L = (N - 3) / 3;
    std::vector<double> mu(N), S((size_t)N * N);
    std::vector<int> ids(std::max(L, 1));
    r = aslam_get_state(c, &N, mu.data(), S.data());
    if (r) return r;
    int L2 = 0;
    r = aslam_get_landmark_ids(c, &L2, ids.data());
    if (r) return r;
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(c, ASLAM_E_INVALID, std::string("cannot write ") + path);
    const char magic[8] = {'A', 'S', 'L', 'A', 'M', 'S', 'T', '1'};
    const int hdr[2] = {N, c->is_init ? 1 : 0};
    bool ok = std::fwrite(magic, 1, 8, f) == 8 && std::fwrite(hdr, sizeof(int), 2, f) == 2 &&
              std::fwrite(mu.data(), sizeof(double), mu.size(), f) == mu.size() &&
              std::fwrite(S.data(), sizeof(double), S.size(), f) == S.size() &&
              std::fwrite(ids.data(), sizeof(int), (size_t)L, f) == (size_t)L;
    ok = (std::fclose(f) == 0) && ok;
    return ok ? ASLAM_OK : fail(c, ASLAM_E_INVALID, std::string("short write to ") + path);
}

int aslam_load_state(aslam_ctx* c, const char* path) {
    if (!c || !path) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kSlam)) return r;
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(c, ASLAM_E_INVALID, std::string("cannot read ") + path);
    char magic[8];
    int hdr[2] = {0, 0};
    bool ok = std::fread(magic, 1, 8, f) == 8 && std::memcmp(magic, "ASLAMST1", 8) == 0 && std::fread(hdr, sizeof(int), 2, f) == 2;
    const int N = hdr[0];
    ok = ok && N >= 3 && (N - 3) % 3 == 0 && (N - 3) / 3 <= c->ekf.max_landmarks;
    std::vector<double> mu, S;
    std::vector<int> ids;
    if (ok) {
        const int L = (N - 3) / 3;
        mu.resize(N); S.resize((size_t)N * N); ids.resize(std::max(L, 1));
        ok = std::fread(mu.data(), sizeof(double), mu.size(), f) == mu.size() && std::fread(S.data(), sizeof(double), S.size(), f) == S.size() &&
             std::fread(ids.data(), sizeof(int), (size_t)L, f) == (size_t)L;
    }
    std::fclose(f);
    if (!ok) return fail(c, ASLAM_E_INVALID, std::string("not a state file that fits this context: ") + path);
    int r = aslam_set_state(c, N, mu.data(), S.data(), ids.data());
    if (r) return r;
    c->is_init = hdr[1] != 0;
    return ASLAM_OK;
}

int aslam_get_slot_detections(aslam_ctx* c, int slot, int* M, int* ids, float* corners, double* rvecs, double* tvecs) {
    if (!c || !M) return fail(c, ASLAM_E_INVALID, "null argument");
    int r = check_slot_range(c, slot, 1);
    if (r) return r;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unsigned n = 0;
    HIP_TRY(c, hipMemcpy(&n, c->d_nmarkers + slot, sizeof(unsigned), hipMemcpyDeviceToHost));
    n = std::min(n, (unsigned)kMarkerMax);
    std::vector<Marker> h(n);
    if (n) HIP_TRY(c, hipMemcpy(h.data(), c->d_markers + (size_t)slot * kMarkerMax, n * sizeof(Marker), hipMemcpyDeviceToHost));
    *M = (int)n;
    for (unsigned i = 0; i < n; i++) {
        if (ids) ids[i] = h[i].id;
        if (corners) std::memcpy(corners + 8 * i, h[i].c, sizeof(float) * 8);
        if (rvecs) std::memcpy(rvecs + 3 * i, h[i].rvec, sizeof(double) * 3);
        if (tvecs) std::memcpy(tvecs + 3 * i, h[i].tvec, sizeof(double) * 3);
    }
    return ASLAM_OK;
}

int aslam_get_detections(aslam_ctx* c, int* M, int* ids, float* corners, double* rvecs, double* tvecs) {
    if (!c) return ASLAM_E_INVALID;
    return aslam_get_slot_detections(c, c->last_first + std::max(c->last_count, 1) - 1, M, ids, corners, rvecs, tvecs);
}

int aslam_get_slot_raw_observations(aslam_ctx* c, int slot, int* n_out, int* ids, int* valid, double* xyth, double* Rdiag) {
    if (!c || !n_out) return fail(c, ASLAM_E_INVALID, "null argument");
    int r = check_slot_range(c, slot, 1);
    if (r) return r;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->confirm_stream) HIP_TRY(c, hipStreamSynchronize(c->confirm_stream));   // landmark confirmation rewrites valid flags on the stream that carries the list
    unsigned n = 0;
    HIP_TRY(c, hipMemcpy(&n, c->d_nmarkers + slot, sizeof(unsigned), hipMemcpyDeviceToHost));
    n = std::min(n, (unsigned)kMarkerMax);
    std::vector<ObsRaw> h(n);
    if (n) HIP_TRY(c, hipMemcpy(h.data(), c->d_obs + (size_t)slot * kMarkerMax, n * sizeof(ObsRaw), hipMemcpyDeviceToHost));
    *n_out = (int)n;
    for (unsigned i = 0; i < n; i++) {
        if (ids) ids[i] = h[i].id;
        if (valid) valid[i] = h[i].valid;
        if (xyth) { xyth[3 * i] = h[i].x; xyth[3 * i + 1] = h[i].y; xyth[3 * i + 2] = h[i].th; }
        if (Rdiag) std::memcpy(Rdiag + 3 * i, h[i].r, sizeof(double) * 3);
    }
    return ASLAM_OK;
}

int aslam_get_observations(aslam_ctx* c, int* n_out, int* ids, int* idx, int* action, double* xyth, double* Rdiag) {
    if (!c || !n_out) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kSingle)) return r;
    { int rs = sync_streams(c); if (rs) return rs; }
    int n = 0;
    HIP_TRY(c, hipMemcpy(&n, c->ekf.d_npop, sizeof(int), hipMemcpyDeviceToHost));
    std::vector<PopRec> h(n);
    if (n) HIP_TRY(c, hipMemcpy(h.data(), c->ekf.d_pop, n * sizeof(PopRec), hipMemcpyDeviceToHost));
    *n_out = n;
    for (int i = 0; i < n; i++) {
        if (ids) ids[i] = h[i].id;
        if (idx) idx[i] = h[i].index;
        if (action) action[i] = h[i].action;
        if (xyth) { xyth[3 * i] = h[i].z[0]; xyth[3 * i + 1] = h[i].z[1]; xyth[3 * i + 2] = h[i].z[2]; }
        if (Rdiag) std::memcpy(Rdiag + 3 * i, h[i].r, sizeof(double) * 3);
    }
    return ASLAM_OK;
}

int aslam_get_slot_ekf_stats(aslam_ctx* c, int first, int count, int* stats) {
    if (!c || !stats) return fail(c, ASLAM_E_INVALID, "null argument");
    int r = check_slot_range(c, first, count);
    if (r) return r;
    return read_ekf_stats(c, first, count, stats);
}

int aslam_get_landmark_ids(aslam_ctx* c, int* L, int* ids) {
    if (!c || !L) return fail(c, ASLAM_E_INVALID, "null argument");
    { int rs = sync_streams(c); if (rs) return rs; }
    return read_landmark_ids(c, c->ekf, L, ids);
}

int aslam_detect_batch(aslam_ctx* c, const uint8_t* frames, int nframes, int rows, int cols, int channels, size_t step,
                       size_t frame_stride, int max_per_frame, int* counts, int* ids, float* corners, double* rvecs, double* tvecs) {
    if (!c || !frames || !counts || nframes <= 0 || max_per_frame <= 0) return fail(c, ASLAM_E_INVALID, "bad arguments");
    for (int f0 = 0; f0 < nframes; f0 += c->max_batch) {
        int nb = std::min(c->max_batch, nframes - f0);
        int r = aslam_stage_frames(c, 0, frames + (size_t)f0 * frame_stride, nb, rows, cols, channels, step, frame_stride);
        if (r) return r;
        r = run_detect(c, single_call(0, nb), false);
        if (r) return r;
        c->rig_last = false;
        r = sync_and_check(c);
        if (r) return r;
        for (int i = 0; i < nb; i++) {
            int M = 0;
            std::vector<int> hid(kMarkerMax);
            std::vector<float> hc((size_t)kMarkerMax * 8);
            std::vector<double> hr((size_t)kMarkerMax * 3), ht((size_t)kMarkerMax * 3);
            r = aslam_get_slot_detections(c, i, &M, hid.data(), hc.data(), hr.data(), ht.data());
            if (r) return r;
            const int f = f0 + i;
            counts[f] = M;
            const int m = std::min(M, max_per_frame);
            if (ids) std::memcpy(ids + (size_t)f * max_per_frame, hid.data(), sizeof(int) * m);
            if (corners) std::memcpy(corners + (size_t)f * max_per_frame * 8, hc.data(), sizeof(float) * 8 * m);
            if (rvecs) std::memcpy(rvecs + (size_t)f * max_per_frame * 3, hr.data(), sizeof(double) * 3 * m);
            if (tvecs) std::memcpy(tvecs + (size_t)f * max_per_frame * 3, ht.data(), sizeof(double) * 3 * m);
        }
    }
    return ASLAM_OK;
}

int aslam_export_map(aslam_ctx* c, void* dst, int dst_is_device) {
    if (!c || !dst) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kSingle)) return r;
    { int rp = finalize_pending(c); if (rp) return rp; }
    launch_ekf_export_map(c->stream_ekf, c->ekf);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(dst, c->ekf.d_maprec, (size_t)ASLAM_MAP_RECORD_BYTES * c->ekf.max_landmarks,
                              dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream_ekf));
    HIP_TRY(c, hipStreamSynchronize(c->stream_ekf));
    return ASLAM_OK;
}

int aslam_export_map_async(aslam_ctx* c, void* d_dst, int buffer) {
    if (!c || !d_dst || buffer < 0 || buffer > 1) return fail(c, ASLAM_E_INVALID, "bad arguments");
    if (int r = allow(c, kSingle)) return r;
    if (!c->ev_export[buffer]) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_export[buffer], hipEventDisableTiming));
    { int rp = finalize_pending(c); if (rp) return rp; }
    launch_ekf_export_map(c->stream_ekf, c->ekf);              // ordered after the EKF steps enqueued so far
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(d_dst, c->ekf.d_maprec, (size_t)ASLAM_MAP_RECORD_BYTES * c->ekf.max_landmarks, hipMemcpyDeviceToDevice, c->stream_ekf));
    HIP_TRY(c, hipEventRecord(c->ev_export[buffer], c->stream_ekf));
    return ASLAM_OK;
}

int aslam_export_wait(aslam_ctx* c, int buffer) {
    if (!c || buffer < 0 || buffer > 1) return fail(c, ASLAM_E_INVALID, "bad arguments");
    if (c->ev_export[buffer]) HIP_TRY(c, hipEventSynchronize(c->ev_export[buffer]));
    return ASLAM_OK;
}

// ---- landmark-map gather over RCCL, reachable from C / C++ (the Python side can use torch.distributed instead) ----
namespace {
struct NcclUid { char internal[128]; };                                    // ncclUniqueId (rccl.h): 128 opaque bytes
struct Rccl {
    void* h = nullptr;
    int (*GetUniqueId)(NcclUid*) = nullptr;
    int (*CommInitRank)(void**, int, NcclUid, int) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
Rccl* rccl() {
    static Rccl r;
    static bool tried = false;
    if (!tried) {
        tried = true;
        const char* names[] = {"librccl.so.1", "librccl.so"};
        for (const char* n : names) { r.h = dlopen(n, RTLD_NOW | RTLD_NOLOAD); if (r.h) break; }      // a copy the process already uses (torch's)
        if (!r.h) for (const char* n : names) { r.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (r.h) break; }
        if (r.h) {
            r.GetUniqueId = reinterpret_cast<int (*)(NcclUid*)>(dlsym(r.h, "ncclGetUniqueId"));
            r.CommInitRank = reinterpret_cast<int (*)(void**, int, NcclUid, int)>(dlsym(r.h, "ncclCommInitRank"));
            r.AllGather = reinterpret_cast<int (*)(const void*, void*, size_t, int, void*, hipStream_t)>(dlsym(r.h, "ncclAllGather"));
            r.CommDestroy = reinterpret_cast<int (*)(void*)>(dlsym(r.h, "ncclCommDestroy"));
            r.GetErrorString = reinterpret_cast<const char* (*)(int)>(dlsym(r.h, "ncclGetErrorString"));
            if (!r.GetUniqueId || !r.CommInitRank || !r.AllGather || !r.CommDestroy) r.h = nullptr;
        }
    }
    return r.h ? &r : nullptr;
}
int rccl_fail(aslam_ctx* c, const char* what, int rc) {
    Rccl* r = rccl();
    return fail(c, ASLAM_E_HIP, std::string(what) + ": " + (r && r->GetErrorString ? r->GetErrorString(rc) : "rccl error"));
}
}  // namespace

int aslam_comm_get_unique_id(void* id) {
    Rccl* r = rccl();
    if (!id) return ASLAM_E_INVALID;
    if (!r) return ASLAM_E_STATE;
    return r->GetUniqueId(static_cast<NcclUid*>(id)) == 0 ? ASLAM_OK : ASLAM_E_HIP;
}

int aslam_comm_create(aslam_ctx* c, const void* id, int world, int rank) {
    if (!c || !id || world < 1 || rank < 0 || rank >= world) return fail(c, ASLAM_E_INVALID, "bad arguments");
    Rccl* r = rccl();
    if (!r) return fail(c, ASLAM_E_STATE, "librccl.so not found (the map gather needs RCCL)");
    if (c->comm) return fail(c, ASLAM_E_STATE, "communicator already created");
    HIP_TRY(c, hipSetDevice(c->init.device_id));
    NcclUid uid;
    std::memcpy(&uid, id, sizeof(uid));
    int rc = r->CommInitRank(&c->comm, world, uid, rank);
    if (rc != 0) { c->comm = nullptr; return rccl_fail(c, "ncclCommInitRank", rc); }
    c->comm_world = world; c->comm_rank = rank;
    HIP_TRY(c, dalloc(&c->d_gather, (size_t)world * c->ekf.max_landmarks * ASLAM_MAP_RECORD_BYTES));
    return ASLAM_OK;
}

int aslam_comm_gather_maps(aslam_ctx* c, void* dst, int dst_is_device) {
    if (!c || !dst) return fail(c, ASLAM_E_INVALID, "null argument");
    if (int r = allow(c, kSingle)) return r;
    if (!c->comm) return fail(c, ASLAM_E_STATE, "aslam_comm_create first");
    Rccl* r = rccl();
    const size_t nb = (size_t)ASLAM_MAP_RECORD_BYTES * c->ekf.max_landmarks;
    { int rp = finalize_pending(c); if (rp) return rp; }
    launch_ekf_export_map(c->stream_ekf, c->ekf);                  // ordered after the EKF steps enqueued so far
    HIP_TRY(c, hipGetLastError());
    int rc = r->AllGather(c->ekf.d_maprec, c->d_gather, nb, /* ncclInt8 */ 0, c->comm, c->stream_ekf);
    if (rc != 0) return rccl_fail(c, "ncclAllGather", rc);
    HIP_TRY(c, hipMemcpyAsync(dst, c->d_gather, nb * c->comm_world, dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream_ekf));
    HIP_TRY(c, hipStreamSynchronize(c->stream_ekf));
    return ASLAM_OK;
}

int aslam_comm_destroy(aslam_ctx* c) {
    if (!c) return ASLAM_E_INVALID;
    if (c->comm) {
        hipStreamSynchronize(c->stream_ekf);
        Rccl* r = rccl();
        if (r) r->CommDestroy(c->comm);
        c->comm = nullptr;
    }
    if (c->d_gather) { hipFree(c->d_gather); c->d_gather = nullptr; }
    return ASLAM_OK;
}

// ---- instrumentation -----------------------------------------------------------------------------------
int aslam_debug_get_nbr(aslam_ctx* c, int slot, int scale, uint8_t* out) {
    if (!c || !out || scale < 0 || scale >= kScales) return fail(c, ASLAM_E_INVALID, "bad arguments");
    int r = check_slot_range(c, slot, 1);
    if (r) return r;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const DetectCfg& g = c->cfg;
    const size_t pb = nbr_plane_bytes(g.rows, g.pitch);
    std::vector<uint8_t> tiled(pb);
    HIP_TRY(c, hipMemcpy(tiled.data(), c->d_nbr + ((size_t)slot * kScales + scale) * pb, pb, hipMemcpyDeviceToHost));
    for (int y = 0; y < g.rows; y++)
        for (int x = 0; x < g.cols; x++) out[(size_t)y * g.cols + x] = tiled[nbr_index(x, y, g.pitch)];     // un-tile for the caller
    return ASLAM_OK;
}

// contours of one (slot, scale) of the last detection that covered the slot, sorted into OpenCV order (descending key)
int aslam_debug_get_contours(aslam_ctx* c, int slot, int scale, int max_contours, long long max_points, int* n_contours,
                             int* sizes, int* keys, int* points_xy, long long* n_points) {
    if (!c || !n_contours) return fail(c, ASLAM_E_INVALID, "bad arguments");
    int rr = check_slot_range(c, slot, 1);
    if (rr) return rr;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unsigned nc = 0;
    HIP_TRY(c, hipMemcpy(&nc, c->d_ncontours + slot, sizeof(unsigned), hipMemcpyDeviceToHost));
    nc = std::min(nc, c->cfg.cap_contours);
    std::vector<ContourRec> recs(nc);
    if (nc) HIP_TRY(c, hipMemcpy(recs.data(), c->d_contours + (size_t)slot * c->cfg.cap_contours, nc * sizeof(ContourRec), hipMemcpyDeviceToHost));
    std::vector<ContourRec> sel;
    for (auto& r : recs) if (r.scale == (unsigned)scale) sel.push_back(r);
    std::sort(sel.begin(), sel.end(), [](const ContourRec& a, const ContourRec& b) { return a.key > b.key; });
    long long tot = 0;
    int n = 0;
    std::vector<unsigned> pts;
    for (auto& r : sel) {
        if (n >= max_contours || tot + (long long)r.n > max_points) return fail(c, ASLAM_E_CAPACITY, "debug buffer too small");
        pts.resize(r.n);
        if (r.n) HIP_TRY(c, hipMemcpy(pts.data(), c->d_points + (size_t)slot * c->cfg.cap_points + r.off, r.n * sizeof(unsigned), hipMemcpyDeviceToHost));
        if (sizes) sizes[n] = (int)r.n;
        if (keys) keys[n] = (int)r.key;
        if (points_xy)
            for (unsigned i = 0; i < r.n; i++) {
                points_xy[2 * (tot + i)] = (int)(short)(pts[i] & 0xFFFFu);
                points_xy[2 * (tot + i) + 1] = (int)(short)(pts[i] >> 16);
            }
        tot += r.n;
        n++;
    }
    *n_contours = n;
    if (n_points) *n_points = tot;
    return ASLAM_OK;
}

int aslam_debug_get_candidates(aslam_ctx* c, int slot, int stage, int max, int* n_out, float* corners, int* sizes, int* ids) {
    if (!c || !n_out) return fail(c, ASLAM_E_INVALID, "bad arguments");
    int r = check_slot_range(c, slot, 1);
    if (r) return r;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (stage == 0) {
        unsigned n = 0;
        HIP_TRY(c, hipMemcpy(&n, c->d_ncand + slot, sizeof(unsigned), hipMemcpyDeviceToHost));
        n = std::min(n, (unsigned)kCandMax);
        std::vector<CandRec> h(n);
        if (n) HIP_TRY(c, hipMemcpy(h.data(), c->d_cands + (size_t)slot * kCandMax, n * sizeof(CandRec), hipMemcpyDeviceToHost));
        std::sort(h.begin(), h.end(), [](const CandRec& a, const CandRec& b) { return a.ordkey < b.ordkey; });
        *n_out = (int)n;
        for (unsigned i = 0; i < n && (int)i < max; i++) {
            if (corners) for (int k = 0; k < 4; k++) { corners[8 * i + 2 * k] = h[i].x[k]; corners[8 * i + 2 * k + 1] = h[i].y[k]; }
            if (sizes) sizes[i] = (int)h[i].n;
            if (ids) ids[i] = -1;
        }
    } else {
        unsigned n = 0;
        HIP_TRY(c, hipMemcpy(&n, c->d_nfinal + slot, sizeof(unsigned), hipMemcpyDeviceToHost));
        n = std::min(n, (unsigned)kCandMax);
        std::vector<FinalCand> h(n);
        if (n) HIP_TRY(c, hipMemcpy(h.data(), c->d_finals + (size_t)slot * kCandMax, n * sizeof(FinalCand), hipMemcpyDeviceToHost));
        *n_out = (int)n;
        for (unsigned i = 0; i < n && (int)i < max; i++) {
            if (corners) std::memcpy(corners + 8 * i, h[i].c, sizeof(float) * 8);
            if (sizes) sizes[i] = h[i].n;
            if (ids) ids[i] = h[i].id;
        }
    }
    return ASLAM_OK;
}

int aslam_debug_inject_observations(aslam_ctx* c, int slot, int n, const int* ids, const int* valid, const double* xyth,
                                    const double* Rdiag) {
    if (!c || n < 0 || n > kMarkerMax || (n && (!ids || !valid || !xyth || !Rdiag))) return fail(c, ASLAM_E_INVALID, "bad arguments");
    int r = check_slot_range(c, slot, 1);
    if (r) return r;
    r = sync_streams(c);
    if (r) return r;
    std::vector<ObsRaw> h(n);
    for (int i = 0; i < n; i++) {
        h[i].id = ids[i]; h[i].valid = valid[i];
        h[i].x = xyth[3 * i]; h[i].y = xyth[3 * i + 1]; h[i].th = xyth[3 * i + 2];
        h[i].r[0] = Rdiag[3 * i]; h[i].r[1] = Rdiag[3 * i + 1]; h[i].r[2] = Rdiag[3 * i + 2];
    }
    unsigned un = (unsigned)n;
    if (n) HIP_TRY(c, hipMemcpy(c->d_obs + (size_t)slot * kMarkerMax, h.data(), n * sizeof(ObsRaw), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_nmarkers + slot, &un, sizeof(unsigned), hipMemcpyHostToDevice));
    return ASLAM_OK;
}

int aslam_debug_inject_candidates(aslam_ctx* c, int slot, int n, const int* ids, const int* rots, const float* corners) {
    if (!c || n < 0 || n > kCandMax || (n && (!ids || !rots || !corners))) return fail(c, ASLAM_E_INVALID, "bad arguments");
    int r = check_slot_range(c, slot, 1);
    if (r) return r;
    std::vector<FinalCand> h(n);
    for (int i = 0; i < n; i++) {
        if (ids[i] < -1 || rots[i] < 0 || rots[i] > 3) return fail(c, ASLAM_E_INVALID, "candidate: id >= -1 and rotation 0..3");
        for (int k = 0; k < 8; k++) {
            if (!std::isfinite(corners[8 * i + k])) return fail(c, ASLAM_E_INVALID, "candidate: non-finite corner");
            h[i].c[k] = corners[8 * i + k];
        }
        h[i].n = 0;
        h[i].id = ids[i];
        h[i].pad[0] = rots[i];
        h[i].pad[1] = 0;
    }
    r = sync_streams(c);
    if (r) return r;
    unsigned un = (unsigned)n;
    if (n) HIP_TRY(c, hipMemcpy(c->d_finals + (size_t)slot * kCandMax, h.data(), n * sizeof(FinalCand), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_nfinal + slot, &un, sizeof(unsigned), hipMemcpyHostToDevice));
    return ASLAM_OK;
}

namespace {
// both pose hooks: what run_detect launches at P_POSE for the call's frames, chunk by chunk (slot first + i: camera i % n of a rig),
// without corner refinement (no grey frame is needed) or with the detection call's own (refine)
int debug_run_pose(aslam_ctx* c, int first, int count, const int* robot_of_slot, bool refine) {
    if (!c) return ASLAM_E_INVALID;
    int r = check_slot_range(c, first, count);
    if (r) return r;
    if ((c->fleet_n > 0) != (robot_of_slot != nullptr))
        return fail(c, ASLAM_E_INVALID, "robot_of_slot: given exactly when a fleet is active");
    if (robot_of_slot)
        for (int i = 0; i < count; i++)
            if (robot_of_slot[i] < 0 || robot_of_slot[i] >= c->fleet_n) return fail(c, ASLAM_E_INVALID, "robot index outside the fleet");
    if (!robot_of_slot && c->rig_n == 0 && !c->have_cam) return fail(c, ASLAM_E_STATE, "camera parameters not set (aslam_set_camera)");
    if (refine) {
        if (!c->dp.doCornerRefinement) return fail(c, ASLAM_E_STATE, "corner refinement is not enabled (aslam_set_detector_params)");
        if (c->rows == 0) return fail(c, ASLAM_E_STATE, "no frames staged");
        for (int i = first; i < first + count; i++)
            if ((int)c->slot_shape.size() <= i || c->slot_shape[i] != frame_shape(c))
                return fail(c, ASLAM_E_STATE, "slot has no frame of the current shape (stage one and run a detection pass on it first)");
    }
    r = sync_streams(c);
    if (r) return r;
    if (refine) {
        // cornerSubPix starts inside the image: a detection pass never hands it anything else, and the loop relies on it
        std::vector<FinalCand> h;
        for (int i = first; i < first + count; i++) {
            unsigned n = 0;
            HIP_TRY(c, hipMemcpy(&n, c->d_nfinal + i, sizeof(unsigned), hipMemcpyDeviceToHost));
            n = std::min(n, (unsigned)kCandMax);
            h.resize(n);
            if (n) HIP_TRY(c, hipMemcpy(h.data(), c->d_finals + (size_t)i * kCandMax, n * sizeof(FinalCand), hipMemcpyDeviceToHost));
            for (const FinalCand& f : h)
                for (int q = 0; q < 4 && f.id >= 0; q++)
                    if (!(f.c[2 * q] >= 0 && f.c[2 * q] < (float)c->cfg.cols && f.c[2 * q + 1] >= 0 && f.c[2 * q + 1] < (float)c->cfg.rows))
                        return fail(c, ASLAM_E_INVALID, "identified candidate with a corner outside the frame");
        }
    }
    const Call k{first, count, c->rig_n > 0 ? &c->rig : nullptr, robot_of_slot, first, count};
    hipStream_t st = c->stream;
    if (c->last_detect && c->last_detect != st) HIP_TRY(c, hipStreamWaitEvent(st, c->ev_detect, 0));
    c->last_detect = st;
    c->last_first = first;
    c->last_count = count;
    if (robot_of_slot) {
        r = pinned_upload(c, c->fleet_camidx_up, c->d_fleet_camidx + first, robot_of_slot, count, st);
        if (r) return r;
    }
    RefineCfg off{};
    off.on = 0;
    const int chunk = detect_chunk();
    for (int f0 = first; f0 < first + count; f0 += chunk)
        launch_pose_stage(c, k, st, f0, std::min(chunk, first + count - f0), refine ? refine_cfg(c, f0) : off);
    HIP_TRY(c, hipEventRecord(c->ev_detect, st));
    HIP_TRY(c, hipGetLastError());
    return ASLAM_OK;
}
} // namespace

int aslam_debug_run_pose(aslam_ctx* c, int first, int count, const int* robot_of_slot) {
    return debug_run_pose(c, first, count, robot_of_slot, false);
}

int aslam_debug_run_pose_refined(aslam_ctx* c, int first, int count, const int* robot_of_slot) {
    return debug_run_pose(c, first, count, robot_of_slot, true);
}

int aslam_debug_run_identify(aslam_ctx* c, int first, int count) {
    if (!c) return ASLAM_E_INVALID;
    int r = check_slot_range(c, first, count);
    if (r) return r;
    if (c->rows == 0) return fail(c, ASLAM_E_STATE, "no frames staged");
    for (int i = first; i < first + count; i++)
        if ((int)c->slot_shape.size() <= i || c->slot_shape[i] != frame_shape(c))
            return fail(c, ASLAM_E_STATE, "slot has no frame of the current shape (stage one and run a detection pass on it first)");
    r = sync_streams(c);
    if (r) return r;
    if (!c->d_ident_rec) HIP_TRY(c, dalloc(&c->d_ident_rec, (size_t)kCandMax * c->max_batch));
    std::vector<unsigned> nf(count);
    HIP_TRY(c, hipMemcpy(nf.data(), c->d_nfinal + first, count * sizeof(unsigned), hipMemcpyDeviceToHost));
    hipStream_t st = c->stream;
    if (c->last_detect && c->last_detect != st) HIP_TRY(c, hipStreamWaitEvent(st, c->ev_detect, 0));
    c->last_detect = st;
    c->last_first = first;
    c->last_count = count;
    // what run_detect launches at P_IDENTIFY, chunk by chunk: the work list k_assemble would have written (every candidate of
    // every frame, frame by frame, in candidate order) and its counters
    const int chunk = detect_chunk();
    std::vector<IdentWork> work;
    for (int f0 = first; f0 < first + count; f0 += chunk) {
        const int n = std::min(chunk, first + count - f0);
        work.clear();
        for (int f = 0; f < n; f++)
            for (unsigned i = 0; i < std::min(nf[f0 - first + f], (unsigned)kCandMax); i++) work.push_back(IdentWork{(unsigned)f, i});
        const unsigned heads[2] = {(unsigned)work.size(), 0u};     // n_ident, q_ident
        if (!work.empty()) HIP_TRY(c, hipMemcpyAsync(c->d_work, work.data(), work.size() * sizeof(IdentWork), hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(&c->d_ctr->n_ident, heads, sizeof(heads), hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipStreamSynchronize(st));                      // (the host vectors are reused)
        launch_identify_stage(c, st, c->cfg, f0, c->d_ident_rec);
    }
    HIP_TRY(c, hipEventRecord(c->ev_detect, st));
    HIP_TRY(c, hipGetLastError());
    return ASLAM_OK;
}

int aslam_debug_get_identified(aslam_ctx* c, int slot, int max, int* n_out, int* ids, int* rots, uint8_t* cells, long long* info) {
    if (!c || !n_out || max < 0) return fail(c, ASLAM_E_INVALID, "bad arguments");
    int r = check_slot_range(c, slot, 1);
    if (r) return r;
    if (!c->d_ident_rec) return fail(c, ASLAM_E_STATE, "no identification records (aslam_debug_run_identify)");
    r = sync_streams(c);
    if (r) return r;
    unsigned n = 0;
    HIP_TRY(c, hipMemcpy(&n, c->d_nfinal + slot, sizeof(unsigned), hipMemcpyDeviceToHost));
    n = std::min(n, (unsigned)kCandMax);
    *n_out = (int)n;
    const unsigned m = std::min(n, (unsigned)max);
    std::vector<FinalCand> h(m);
    std::vector<IdentRecord> rec(m);
    if (m) {
        HIP_TRY(c, hipMemcpy(h.data(), c->d_finals + (size_t)slot * kCandMax, m * sizeof(FinalCand), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(rec.data(), c->d_ident_rec + (size_t)slot * kCandMax, m * sizeof(IdentRecord), hipMemcpyDeviceToHost));
    }
    const int nc = c->cfg.marker_size + 2 * c->cfg.border_bits, ncell = nc * nc;
    for (unsigned i = 0; i < m; i++) {
        if (ids) ids[i] = h[i].id;
        if (rots) rots[i] = h[i].pad[0];
        if (cells)
            for (int k = 0; k < kDictMaxCells * kDictMaxCells; k++)
                cells[(size_t)i * kDictMaxCells * kDictMaxCells + k] = k < ncell ? (uint8_t)((rec[i].bits[k / 64] >> (k % 64)) & 1ull) : 0;
        if (info) {
            long long* o = info + (size_t)i * 8;
            o[0] = rec[i].branch; o[1] = rec[i].T; o[2] = rec[i].border_err; o[3] = rec[i].sum; o[4] = rec[i].sq;
            o[5] = rec[i].id; o[6] = rec[i].rot; o[7] = nc;
        }
    }
    return ASLAM_OK;
}

namespace {
// Injected coordinates: the 16-bit packing holds [-32768, 32767], but k_quads' wave reductions carry squared distances and cross
// products as 32-bit integers (wave_first_max_exact), which holds for differences below 2^15 (a detection pass: below 2^12)
constexpr int kInjectCoordMin = -16384, kInjectCoordMax = 16383;
// what both quad hooks ask of a slot: a frame of the current shape staged in it (its shape and DetectCfg are the launch's)
int check_slots_staged(aslam_ctx* c, int first, int count) {
    int r = check_slot_range(c, first, count);
    if (r) return r;
    if (c->rows == 0) return fail(c, ASLAM_E_STATE, "no frames staged");
    for (int i = first; i < first + count; i++)
        if ((int)c->slot_shape.size() <= i || c->slot_shape[i] != frame_shape(c))
            return fail(c, ASLAM_E_STATE, "slot has no frame of the current shape (stage one first)");
    return ASLAM_OK;
}
// a (scale, discovery key) list as k_link would have produced it: a window in force, a key of the frame, no pair twice
int check_scale_keys(aslam_ctx* c, int n, const int* scales, const int* keys) {
    std::vector<unsigned long long> seen(n);
    for (int i = 0; i < n; i++) {
        if (scales[i] < 0 || scales[i] >= c->cfg.n_scales) return fail(c, ASLAM_E_INVALID, "scale outside the threshold windows in force");
        if (keys[i] < 0 || (long long)keys[i] > (long long)c->rows * c->cols) return fail(c, ASLAM_E_INVALID, "key outside [0, rows * cols]");
        seen[i] = ((unsigned long long)scales[i] << 32) | (unsigned)keys[i];
    }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return fail(c, ASLAM_E_INVALID, "(scale, key) twice in one slot");
    return ASLAM_OK;
}
}

int aslam_debug_inject_contours(aslam_ctx* c, int slot, int n, const int* scales, const int* keys, const int* sizes, const int* points_xy) {
    if (!c || n < 0 || (n && (!scales || !keys || !sizes || !points_xy))) return fail(c, ASLAM_E_INVALID, "bad arguments");
    int r = check_slots_staged(c, slot, 1);
    if (r) return r;
    const DetectCfg& g = c->cfg;
    if ((unsigned)n > g.cap_contours) return fail(c, ASLAM_E_INVALID, "more contours than cap_contours_per_frame");
    r = check_scale_keys(c, n, scales, keys);
    if (r) return r;
    std::vector<ContourRec> recs(n);
    std::vector<unsigned> pts;
    size_t tot = 0;
    for (int i = 0; i < n; i++) {
        if (sizes[i] < 1 || sizes[i] > 65534) return fail(c, ASLAM_E_INVALID, "contour size outside [1, 65534]");
        if (tot + (size_t)sizes[i] > g.cap_points) return fail(c, ASLAM_E_INVALID, "more points than cap_points_per_frame");
        for (int k = 0; k < sizes[i]; k++) {
            const int x = points_xy[2 * (tot + k)], y = points_xy[2 * (tot + k) + 1];
            if (x < kInjectCoordMin || x > kInjectCoordMax || y < kInjectCoordMin || y > kInjectCoordMax)
                return fail(c, ASLAM_E_INVALID, "point coordinate outside [-16384, 16383]");
            pts.push_back((unsigned)(x & 0xFFFF) | ((unsigned)(y & 0xFFFF) << 16));
        }
        recs[i] = ContourRec{(unsigned)slot, (unsigned)scales[i], (unsigned)keys[i], (unsigned)sizes[i], (unsigned)tot,
                             (short)points_xy[2 * tot], (short)points_xy[2 * tot + 1], 0, {0u, 0u}};
        tot += (size_t)sizes[i];
    }
    r = sync_streams(c);
    if (r) return r;
    const unsigned un = (unsigned)n, up = (unsigned)tot;
    if (n) HIP_TRY(c, hipMemcpy(c->d_contours + (size_t)slot * g.cap_contours, recs.data(), n * sizeof(ContourRec), hipMemcpyHostToDevice));
    if (tot) HIP_TRY(c, hipMemcpy(c->d_points + (size_t)slot * g.cap_points, pts.data(), tot * sizeof(unsigned), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_ncontours + slot, &un, sizeof(unsigned), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_npoints + slot, &up, sizeof(unsigned), hipMemcpyHostToDevice));
    return ASLAM_OK;
}

int aslam_debug_inject_quads(aslam_ctx* c, int slot, int n, const int* corners, const int* sizes, const int* scales, const int* keys) {
    if (!c || n < 0 || n > kCandMax || (n && (!corners || !sizes || !scales || !keys))) return fail(c, ASLAM_E_INVALID, "bad arguments");
    int r = check_slots_staged(c, slot, 1);
    if (r) return r;
    r = check_scale_keys(c, n, scales, keys);
    if (r) return r;
    std::vector<CandRec> h(n);
    for (int i = 0; i < n; i++) {
        if (sizes[i] < 1 || sizes[i] > 65534) return fail(c, ASLAM_E_INVALID, "contour size outside [1, 65534]");
        for (int k = 0; k < 4; k++) {
            const int x = corners[8 * i + 2 * k], y = corners[8 * i + 2 * k + 1];
            if (x < kInjectCoordMin || x > kInjectCoordMax || y < kInjectCoordMin || y > kInjectCoordMax)
                return fail(c, ASLAM_E_INVALID, "corner coordinate outside [-16384, 16383]");
            h[i].x[k] = (short)x; h[i].y[k] = (short)y;
        }
        h[i].n = (unsigned)sizes[i];
        h[i].ordkey = cand_ordkey((unsigned)scales[i], (unsigned)keys[i]);
    }
    r = sync_streams(c);
    if (r) return r;
    const unsigned un = (unsigned)n;
    if (n) HIP_TRY(c, hipMemcpy(c->d_cands + (size_t)slot * kCandMax, h.data(), n * sizeof(CandRec), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_ncand + slot, &un, sizeof(unsigned), hipMemcpyHostToDevice));
    return ASLAM_OK;
}

int aslam_debug_run_quads(aslam_ctx* c, int first, int count, int stages) {
    if (!c) return ASLAM_E_INVALID;
    if (stages < 1 || stages > 3) return fail(c, ASLAM_E_INVALID, "stages: 1 quads, 2 assemble, 3 both");
    int r = check_slots_staged(c, first, count);
    if (r) return r;
    r = sync_streams(c);
    if (r) return r;
    hipStream_t st = c->stream;
    if (c->last_detect && c->last_detect != st) HIP_TRY(c, hipStreamWaitEvent(st, c->ev_detect, 0));
    c->last_detect = st;
    c->last_first = first;
    c->last_count = count;
    // what run_detect launches at P_QUADS and P_ASSEMBLE, chunk by chunk.  Of the counters a detection pass clears (k_clear_counts)
    // those these two stages use: the queue heads, and the candidate counts when k_quads is to fill them (the injected lists stay)
    const DetectCfg& g = c->cfg;
    const int chunk = detect_chunk();
    for (int f0 = first; f0 < first + count; f0 += chunk) {
        const int nf = std::min(chunk, first + count - f0);
        HIP_TRY(c, hipMemsetAsync(c->d_ctr, 0, sizeof(unsigned) * kCounterHeads, st));
        if (stages & 1) {
            HIP_TRY(c, hipMemsetAsync(c->d_ncand + f0, 0, sizeof(unsigned) * nf, st));
            prof_begin(c, P_QUADS, st);
            launch_prefix(st, nf, c->d_ncontours + f0, g.cap_contours, 1u, c->d_pre_quads);
            launch_quads(st, c->nwaves, g, nf, c->d_ctr, c->d_contours + (size_t)f0 * g.cap_contours, c->d_ncontours + f0, c->d_pre_quads,
                         c->d_points + (size_t)f0 * g.cap_points, c->d_cands + (size_t)f0 * kCandMax, c->d_ncand + f0);
            prof_end(c);
        }
        if (stages & 2) {
            prof_begin(c, P_ASSEMBLE, st);
            launch_assemble(st, nf, g, c->d_ctr, c->d_cands + (size_t)f0 * kCandMax, c->d_ncand + f0,
                            c->d_finals + (size_t)f0 * kCandMax, c->d_nfinal + f0, c->d_work);
            prof_end(c);
        }
    }
    HIP_TRY(c, hipEventRecord(c->ev_detect, st));
    HIP_TRY(c, hipGetLastError());
    return sync_and_check(c);             // a candidate or pair list that overflowed: ASLAM_E_CAPACITY, as aslam_sync reports it
}

int aslam_debug_run_contours(aslam_ctx* c, int first, int count, int cut_grid, int lds_nodes) {
    if (!c) return ASLAM_E_INVALID;
    if (cut_grid != 0 && cut_grid != kCutGridSingle && cut_grid != kCutGrid) return fail(c, ASLAM_E_INVALID, "cut_grid: 0 (the call's own), 32 or 64");
    int r = check_slots_staged(c, first, count);
    if (r) return r;
    r = sync_streams(c);
    if (r) return r;
    hipStream_t st = c->stream;
    if (c->last_detect && c->last_detect != st) HIP_TRY(c, hipStreamWaitEvent(st, c->ev_detect, 0));
    c->last_detect = st;
    c->last_first = first;
    c->last_count = count;
    DetectCfg g = c->cfg;
    g.cut_mask = (cut_grid ? cut_grid : cut_grid_of_call(g, count, count == 1)) - 1;
    // every ticket of these slots reads "unused" until a link kernel writes it: one it should have written and did not then shows in
    // the list, whatever an earlier call left there
    HIP_TRY(c, hipMemsetAsync(c->d_wlist + (size_t)first * g.cap_write, 0xFF, sizeof(WriteRec) * (size_t)count * g.cap_write, st));
    const int chunk = detect_chunk();
    for (int f0 = first; f0 < first + count; f0 += chunk) launch_contour_stage(c, st, g, f0, std::min(chunk, first + count - f0), lds_nodes);
    HIP_TRY(c, hipEventRecord(c->ev_detect, st));
    HIP_TRY(c, hipGetLastError());
    return sync_and_check(c);             // a node, contour or point list that overflowed: ASLAM_E_CAPACITY, as aslam_sync reports it
}

int aslam_debug_get_nodes(aslam_ctx* c, int slot, int max, int* n_out, unsigned* state, unsigned* next, unsigned* steps, int* area) {
    if (!c || !n_out || max < 0) return fail(c, ASLAM_E_INVALID, "bad arguments");
    int r = check_slot_range(c, slot, 1);
    if (r) return r;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unsigned n = 0;
    HIP_TRY(c, hipMemcpy(&n, c->d_nstarts + slot, sizeof(unsigned), hipMemcpyDeviceToHost));
    n = std::min(n, c->cfg.cap_starts);
    *n_out = (int)n;
    if (n > (unsigned)max) return fail(c, ASLAM_E_CAPACITY, "debug buffer too small");
    std::vector<unsigned> st(n);
    std::vector<NodeRec> rec(n);
    if (n) {
        HIP_TRY(c, hipMemcpy(st.data(), c->d_starts + (size_t)slot * c->cfg.cap_starts, n * sizeof(unsigned), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(rec.data(), c->d_nodes + (size_t)slot * c->cfg.cap_starts, n * sizeof(NodeRec), hipMemcpyDeviceToHost));
    }
    for (unsigned i = 0; i < n; i++) {
        if (state) state[i] = st[i];
        if (next) next[i] = rec[i].nxt;
        if (steps) steps[i] = rec[i].len;
        if (area) area[i] = rec[i].area;
    }
    return ASLAM_OK;
}

int aslam_debug_get_write_tickets(aslam_ctx* c, int slot, int max, int* n_out, unsigned* state, unsigned* contour, unsigned* rel, unsigned* cnt) {
    if (!c || !n_out || max < 0) return fail(c, ASLAM_E_INVALID, "bad arguments");
    int r = check_slot_range(c, slot, 1);
    if (r) return r;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unsigned n = 0;
    HIP_TRY(c, hipMemcpy(&n, c->d_nwrite + slot, sizeof(unsigned), hipMemcpyDeviceToHost));
    n = std::min(n, c->cfg.cap_write);
    *n_out = (int)n;
    if (n > (unsigned)max) return fail(c, ASLAM_E_CAPACITY, "debug buffer too small");
    std::vector<WriteRec> rec(n);
    if (n) HIP_TRY(c, hipMemcpy(rec.data(), c->d_wlist + (size_t)slot * c->cfg.cap_write, n * sizeof(WriteRec), hipMemcpyDeviceToHost));
    for (unsigned i = 0; i < n; i++) {
        if (state) state[i] = rec[i].state;
        if (contour) contour[i] = rec[i].ci;
        if (rel) rel[i] = rec[i].rel;
        if (cnt) cnt[i] = rec[i].cnt;
    }
    return ASLAM_OK;
}

int aslam_debug_get_link_todo(aslam_ctx* c, int slot, int* flag) {
    if (!c || !flag) return fail(c, ASLAM_E_INVALID, "bad arguments");
    int r = check_slot_range(c, slot, 1);
    if (r) return r;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unsigned v = 0;
    HIP_TRY(c, hipMemcpy(&v, c->d_link_todo + slot, sizeof(unsigned), hipMemcpyDeviceToHost));
    *flag = (int)v;
    return ASLAM_OK;
}

int aslam_debug_get_frame_counts(aslam_ctx* c, int slot, unsigned* out /* 6 */) {
    if (!c || !out || slot < 0 || slot >= c->max_batch) return ASLAM_E_INVALID;
    const unsigned* src[6] = {c->d_nstarts, c->d_ncontours, c->d_npoints, c->d_nwrite, c->d_ncand, c->d_link_todo};
    for (int i = 0; i < 6; i++)
        if (hipMemcpy(out + i, src[i] + slot, sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) return ASLAM_E_HIP;
    return ASLAM_OK;
}
int aslam_debug_get_counters(aslam_ctx* c, unsigned* out) {
    return hipMemcpy(out, c->d_ctr, 32, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}
int aslam_profile_enable(aslam_ctx* c, int on) {
    if (!c) return ASLAM_E_INVALID;
    c->prof_on = on != 0;
    if (c->prof_on && c->prof_empty_ms == 0.0) {
        // calibrate the event pair itself: 64 empty spans on the (idle) EKF stream, median
        int r = sync_streams(c);
        if (r) return r;
        std::vector<float> v;
        for (int k = 0; k < 64; k++) {
            hipEvent_t a, b;
            hipEventCreate(&a); hipEventCreate(&b);
            hipEventRecord(a, c->stream_ekf);
            hipEventRecord(b, c->stream_ekf);
            hipEventSynchronize(b);
            float ms = 0;
            if (hipEventElapsedTime(&ms, a, b) == hipSuccess) v.push_back(ms);
            hipEventDestroy(a); hipEventDestroy(b);
        }
        if (!v.empty()) { std::sort(v.begin(), v.end()); c->prof_empty_ms = v[v.size() / 2]; }
    }
    return ASLAM_OK;
}
int aslam_get_plan_stats(aslam_ctx* c, long long out[4]) {
    if (!c || !out) return ASLAM_E_INVALID;
    int r = finalize_pending(c);
    if (r) return r;
    for (int i = 0; i < 4; i++) out[i] = c->plan_stats[i];
    return ASLAM_OK;
}
int aslam_profile_reset(aslam_ctx* c) {
    if (!c) return ASLAM_E_INVALID;
    sync_streams(c);
    prof_collect(c);
    for (int i = 0; i < 4; i++) c->plan_stats[i] = 0;
    for (int i = 0; i < P_COUNT; i++) { c->prof_calls[i] = 0; c->prof_ms[i] = 0; }
    return ASLAM_OK;
}
int aslam_profile_get(aslam_ctx* c, int max, const char** names, int* calls, double* total_ms) {
    if (!c) return ASLAM_E_INVALID;
    sync_streams(c);
    prof_collect(c);
    int n = std::min(max, (int)P_COUNT);
    for (int i = 0; i < n; i++) {
        if (names) names[i] = kProfNames[i];
        if (calls) calls[i] = c->prof_calls[i];
        // a start/stop event pair measures a few microseconds even around nothing; that calibrated amount is taken off every
        // span so that the averages agree with rocprofv3's kernel durations
        if (total_ms) total_ms[i] = std::max(0.0, c->prof_ms[i] - c->prof_calls[i] * c->prof_empty_ms);
    }
    return P_COUNT;
}

int aslam_synth_render(aslam_ctx* c, int slot, int rows, int cols, const double K[9], int n_markers, const int* ids,
                       const double* poses, double marker_length, int background, int noise_amp, unsigned seed, int ss,
                       uint8_t* out_host) {
    if (!c || !K || n_markers < 0 || n_markers > 256 || (n_markers && (!ids || !poses)) || ss < 1 || ss > 8)
        return fail(c, ASLAM_E_INVALID, "bad arguments");
    int r = check_slot_range(c, slot, 1);
    if (r) return r;
    if (rows != c->rows || cols != c->cols || c->channels != 1) {
        r = configure_frames(c, rows, cols, 1);
        if (r) return r;
    }
    c->in_frame_bytes = (size_t)rows * cols;
    r = quiesce_slots(c, slot, 1);
    if (r) return r;
    note_slot_shape(c, slot, 1);
    const int nc = c->dict_ms + 2;
    std::vector<SynthMarker> mk(n_markers);
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    for (int m = 0; m < n_markers; m++) {
        if (ids[m] < 0 || ids[m] >= c->dict_n) return fail(c, ASLAM_E_INVALID, "marker id outside the dictionary");
        const double* P = poses + 12 * m;      // R row-major then t
        double H[9] = {P[0], P[1], P[9], P[3], P[4], P[10], P[6], P[7], P[11]};    // [r1 r2 t]
        double det = H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6]) + H[2] * (H[3] * H[7] - H[4] * H[6]);
        if (det == 0) return fail(c, ASLAM_E_INVALID, "degenerate marker pose");
        double d = 1.0 / det;
        SynthMarker& S = mk[m];
        S.Hinv[0] = (H[4] * H[8] - H[5] * H[7]) * d; S.Hinv[1] = (H[2] * H[7] - H[1] * H[8]) * d; S.Hinv[2] = (H[1] * H[5] - H[2] * H[4]) * d;
        S.Hinv[3] = (H[5] * H[6] - H[3] * H[8]) * d; S.Hinv[4] = (H[0] * H[8] - H[2] * H[6]) * d; S.Hinv[5] = (H[2] * H[3] - H[0] * H[5]) * d;
        S.Hinv[6] = (H[3] * H[7] - H[4] * H[6]) * d; S.Hinv[7] = (H[1] * H[6] - H[0] * H[7]) * d; S.Hinv[8] = (H[0] * H[4] - H[1] * H[3]) * d;
        const double ext = marker_length * 0.5 + marker_length / nc;
        double x0 = 1e30, y0 = 1e30, x1 = -1e30, y1 = -1e30;
        for (int k = 0; k < 4; k++) {
            double X = (k == 0 || k == 3) ? -ext : ext, Y = (k < 2) ? ext : -ext;
            double px = H[0] * X + H[1] * Y + H[2], py = H[3] * X + H[4] * Y + H[5], pw = H[6] * X + H[7] * Y + H[8];
            double u = fx * px / pw + cx, v = fy * py / pw + cy;
            x0 = std::min(x0, u); x1 = std::max(x1, u); y0 = std::min(y0, v); y1 = std::max(y1, v);
        }
        S.bbox[0] = (int)std::floor(x0) - 2; S.bbox[1] = (int)std::floor(y0) - 2;
        S.bbox[2] = (int)std::ceil(x1) + 2;  S.bbox[3] = (int)std::ceil(y1) + 2;
        S.bits[0] = c->dict_cells[(size_t)ids[m] * 2];
        S.bits[1] = c->dict_cells[(size_t)ids[m] * 2 + 1];
    }
    if (n_markers) HIP_TRY(c, hipMemcpyAsync(c->d_synth, mk.data(), mk.size() * sizeof(SynthMarker), hipMemcpyHostToDevice, c->stream));
    uint8_t* dst = c->d_in + (size_t)slot * c->in_frame_bytes;
    launch_render(c->stream, dst, rows, cols, fx, fy, cx, cy, n_markers, c->d_synth, nc, marker_length, background, noise_amp, seed, ss);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (out_host) HIP_TRY(c, hipMemcpy(out_host, dst, (size_t)rows * cols, hipMemcpyDeviceToHost));
    return ASLAM_OK;
}

} // extern "C"
