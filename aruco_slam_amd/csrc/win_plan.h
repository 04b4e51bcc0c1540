// The window planner of a staged batch ("Who forms the windows"): host arithmetic only, no HIP runtime call and no context.
// The host follows the reference's bookkeeping (checkLandmark, queue order, the "stationary" test, aruco_slam.cpp:92-95, 192-198,
// 423-435) on the observations read back from the device and cuts the batch into windows = runs of frames whose fused landmarks fit
// into one set S (ekf_window.hip); every other frame, and every frame the host cannot decide (a marker id it does not know: a new
// landmark; one id twice), takes the per-frame chain, planned on the device.  A window frame may fuse any subset of S and may drop
// "stationary" observations; S is the union over the window.
// Under the SLAM gate (gated windows) the host plans as if every prepared correction were accepted.  The verdicts
// matter to the plan in one place only: a "stationary" match against an entry of the mirror whose own correction may have been
// rejected.  Such a frame is undecidable on the host and goes to the device with the rest of its batch, like a frame with an unknown
// id; a match that fails needs no verdict (a rejected predecessor is absent from the list, an accepted one is too far away).
#pragma once
#include "ekf.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <queue>
#include <utility>
#include <vector>

namespace aslam {

constexpr int kWinWidenFrames = 16;     // a window of at least this many frames is not widened to the next image size (64 -> 128 -> 192)
constexpr int kWinChainFrames = 8;      // frames per chain kernel of a window (its log is replayed meanwhile); <= kWinPieceMax

// unconfirmed: the entry comes from an action-1 observation of a frame planned under the SLAM gate, whose verdict the host does
// not know (rejected: the device's list does not hold it).  Entries read back from the device are exact.
struct HostLast { int id; double z[3]; bool unconfirmed = false; };

struct PlanMirror {                     // the host's copy of the device's bookkeeping tables
    std::vector<int> id2idx;            // id -> landmark table (kIdTableSize entries, -1 = unknown)
    int L = 0;                          // landmarks in the map
    std::vector<HostLast> last;         // last_observed_marker_ (NaN z = unset)
};

struct PlanLimits {
    int max_landmarks, max_updates_per_frame;
    int s_cap;                          // largest set S: contexts configured for few corrections per frame keep SP <= 128 (their chain steps stay cheap)
    bool gate_on;                       // the SLAM gate is set: an update's entry of the mirror is unconfirmed
};
inline int win_s_cap(int win_sp_max) { return win_sp_max >= 192 ? kWinSMax : 41; }

struct WinOp { int frame; bool predict; int K; std::vector<int> S; };      // K == 0: per-frame chain for `frame`; else a window of K frames on S
struct BatchPlan {
    std::vector<WinOp> ops;             // the batch's frames, each once, in order
    bool any_window = false;
    int frames_left_to_device = 0;      // frames the host could not follow (the device plans them, and every later frame of the batch)
};

// addEncoder semantics (aruco_slam.cpp:24-29): the very first sample only arms the filter.  Returns whether this sample predicts.
inline bool arm_filter(bool& is_init) {
    const bool predict = is_init;
    is_init = true;
    return predict;
}

// Plans slots [first, first + count).  obs (kMarkerMax per slot), n_markers and frames are indexed by slot; the WinFrame rows of the
// frames inside windows are written (positions within the final S of their window), no others.  is_init is armed per frame;
// mirror_dirty is set when a frame is left to the device.
inline BatchPlan plan_batch(PlanMirror& M, bool& is_init, bool& mirror_dirty, const PlanLimits& lim, const ObsRaw* obs,
                            const unsigned* n_markers, int first, int count, WinFrame* frames) {
    struct FramePlan { std::vector<int> corr_idx, corr_det, pop_idx, pop_det, pop_act; int n_markers = 0; };
    BatchPlan plan;
    std::vector<WinOp>& ops = plan.ops;
    std::vector<FramePlan> plans(count);
    const bool debug = std::getenv("ASLAM_DEBUG_PLAN") != nullptr;
    int w_first = -1, w_K = 0;
    std::vector<int> w_S;                                                   // sorted landmark indices of the open window
    bool device_plans = false;
    auto close_window = [&]() {
        if (w_K == 0) return;
        if (w_K == 1) ops.push_back(WinOp{w_first, true, 0, {}});           // a lone frame: the per-frame chain is as good
        else ops.push_back(WinOp{w_first, true, w_K, w_S});
        w_K = 0; w_S.clear();
    };
    for (int f = first; f < first + count; f++) {
        const bool predict = arm_filter(is_init);
        const ObsRaw* ob = obs + (size_t)f * kMarkerMax;
        const int nM = (int)std::min(n_markers[f], (unsigned)kMarkerMax);
        bool clean = !device_plans;
        std::vector<std::pair<int, int>> pop;       // (landmark index, detection index) of the observations that pass the gates, pop order
        int n_new = 0;
        if (clean) {
            // obs_.push(ob) in detection order into the reference's own priority queue (aruco_slam.h:85-88, aruco_slam.cpp:369-373):
            // new markers (index -1) pop first, in libstdc++ heap order, and take the next landmark indices in that order (:256)
            struct QItem { int idx, det; bool operator<(const QItem& o) const { return idx > o.idx; } };
            std::priority_queue<QItem> q;
            std::vector<int> seen;
            for (int i = 0; i < nM && clean; i++) {
                if (!ob[i].valid) continue;
                const int id = ob[i].id;
                if (id < 0 || id >= kIdTableSize || std::find(seen.begin(), seen.end(), id) != seen.end()) { clean = false; break; }   // one id twice (Q10): device
                seen.push_back(id);
                q.push(QItem{M.id2idx[id], i});
            }
            while (clean && !q.empty()) {
                QItem it = q.top();
                q.pop();
                if (it.idx < 0) {
                    if (M.L >= lim.max_landmarks) { clean = false; break; }              // capacity: reported by the device
                    it.idx = M.L++;
                    M.id2idx[ob[it.det].id] = it.idx;
                    n_new++;
                }
                pop.push_back({it.idx, it.det});
            }
        }
        auto to_device = [&]() {
            if (debug) std::fprintf(stderr, "plan frame %d: nM %d left to the device\n", f, nM);
            close_window();
            device_plans = true;
            plan.frames_left_to_device++;
            mirror_dirty = true;
            ops.push_back(WinOp{f, predict, 0, {}});
        };
        if (!clean) { to_device(); continue; }
        // pop order = ascending landmark index (aruco_slam.h:85-88); "stationary" test against last frame's list (:192-198)
        FramePlan& fp = plans[f - first];
        fp.n_markers = nM;
        int n_stationary = 0;
        std::vector<HostLast> nlast(pop.size());
        bool undecidable = false;
        for (size_t j = 0; j < pop.size(); j++) {
            const ObsRaw& o = ob[pop[j].second];
            bool stationary = false;
            if ((int)j < n_new) {                                            // augment branch: last_observation_ stays unset (Q3)
                nlast[j].id = o.id;
                nlast[j].z[0] = nlast[j].z[1] = nlast[j].z[2] = std::nan("");
                continue;
            }
            for (const HostLast& l : M.last)
                if (l.id == o.id) {                                          // std::find: first with the same id
                    const double d0 = l.z[0] - o.x, d1 = l.z[1] - o.y, d2 = l.z[2] - o.th;
                    stationary = std::sqrt(d0 * d0 + d1 * d1 + d2 * d2) < 0.01;     // NaN compares false
                    undecidable = undecidable || (stationary && l.unconfirmed);     // the predecessor's verdict decides
                    break;
                }
            n_stationary += stationary ? 1 : 0;
            nlast[j].id = o.id;
            if (stationary) { nlast[j].z[0] = nlast[j].z[1] = nlast[j].z[2] = std::nan(""); }
            else { nlast[j].z[0] = o.x; nlast[j].z[1] = o.y; nlast[j].z[2] = o.th; nlast[j].unconfirmed = lim.gate_on; }
            fp.pop_idx.push_back(pop[j].first); fp.pop_det.push_back(pop[j].second); fp.pop_act.push_back(stationary ? 2 : 1);
            if (!stationary) { fp.corr_idx.push_back(pop[j].first); fp.corr_det.push_back(pop[j].second); }
        }
        if (undecidable) { to_device(); continue; }                            // (the mirror is read back before the next batch is planned)
        M.last.swap(nlast);
        const int m = (int)fp.corr_idx.size();
        const bool eligible = predict && n_new == 0 && m <= kWinCorrMax && (int)pop.size() <= 64 && m <= lim.s_cap && m <= lim.max_updates_per_frame;
        if (debug)
            std::fprintf(stderr, "plan frame %d: nM %d m %d new %d stationary %d predict %d eligible %d (window K %d, |S| %zu)\n", f, nM, m, n_new, n_stationary,
                         (int)predict, (int)eligible, w_K, w_S.size());
        if (!eligible) {
            close_window();
            ops.push_back(WinOp{f, predict, 0, {}});
            continue;
        }
        // does the frame fit into the open window?  (its landmarks are ascending, like S)
        std::vector<int> un;
        if (w_K > 0) std::set_union(w_S.begin(), w_S.end(), fp.corr_idx.begin(), fp.corr_idx.end(), std::back_inserter(un));
        // a wider image makes every step of the window dearer: a window that is already long is closed rather than widened
        const bool widens = w_K >= kWinWidenFrames && ekf_win_tiles((int)un.size()) > ekf_win_tiles((int)w_S.size());
        if (w_K == 0 || w_K >= kWinFrames || (int)un.size() > lim.s_cap || f != w_first + w_K || widens) {
            close_window();
            w_first = f; w_K = 0;
            un = fp.corr_idx;
        }
        w_S.swap(un);
        w_K++;
    }
    close_window();
    // the plan of every window frame in the device's format (positions within the final S of its window)
    for (const WinOp& o : ops) {
        if (o.K == 0) continue;
        plan.any_window = true;
        for (int k = 0; k < o.K; k++) {
            const FramePlan& fp = plans[o.frame + k - first];
            WinFrame& wf = frames[o.frame + k];
            wf.m = (int)fp.corr_idx.size(); wf.npop = (int)fp.pop_idx.size(); wf.n_markers = fp.n_markers; wf.pad = 0;
            for (int a = 0; a < wf.m; a++) {
                wf.cdet[a] = (unsigned char)fp.corr_det[a];
                wf.cpos[a] = (unsigned char)(std::lower_bound(o.S.begin(), o.S.end(), fp.corr_idx[a]) - o.S.begin());
            }
            for (int i = 0; i < wf.npop; i++) {
                wf.pdet[i] = (unsigned char)fp.pop_det[i]; wf.pact[i] = (unsigned char)fp.pop_act[i]; wf.pidx[i] = (short)fp.pop_idx[i];
            }
        }
    }
    return plan;
}

// Frames per chain piece of a window of K frames, first piece first, none longer than piece_cap.  The replay of piece i - 1 runs in
// the launch of piece i and takes about half as long per frame as the chain, so a piece may be at most twice as long as the one that
// follows it; what follows the window waits for the last replay, so the pieces shrink towards the end: .., 8, 4, 2, 1, 1.
inline std::vector<int> win_piece_sizes(int K, int piece_cap) {
    std::vector<int> sizes;
    int left = K, nxt = 1, count = 0;
    while (left > 0) {
        int kn = std::min(std::min(nxt, piece_cap), left);
        sizes.push_back(kn);
        left -= kn;
        if (++count >= 2) nxt = std::min(2 * nxt, piece_cap);               // 1, 1, 2, 4, ...
    }
    std::reverse(sizes.begin(), sizes.end());
    return sizes;
}

} // namespace aslam
