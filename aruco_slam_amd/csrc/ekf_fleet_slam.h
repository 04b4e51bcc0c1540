// Fleet SLAM: R robots, each a complete EKF-SLAM filter of its own (mu, Sigma, id tables, last-observed list, pop
// list), stepped by the per-frame chain kernels of ekf.hip.  Included by ekf.hip ahead of the kernels (the gfx950 build and the CPU
// emulation both see it).
//
// Every chain kernel is a template on where its filter comes from:
//   EkfSingle  the by-value EkfState and the frame's scalar arguments as the host passes them (every single-filter launch);
//   EkfFleet   robot blockIdx.z of a round's work list: the row {robot, slot, predict, 0} is one scalar load, the robot's EkfState is
//              robot 0's with every pointer moved by robot * stride, the frame's encoder sample is the context's d_enc[slot].
// The kernels' grids in x / y depend only on the capacity E.ld, which all robots share, and no kernel synchronises between
// workgroups, so a round of n robots is each kernel of the chain once with gridDim.z = n.
#pragma once
#include "ekf.h"

namespace aslam {

template <class T> __host__ __device__ __forceinline__ T* ekf_moved(T* p, size_t off) {
    return reinterpret_cast<T*>(reinterpret_cast<char*>(p) + off);
}

// robot `robot`'s filter: every per-robot pointer of robot 0's moved by robot * stride bytes (d_slot_stat stays the context's)
__host__ __device__ __forceinline__ EkfState ekf_robot_state(const EkfState& b, size_t stride, int robot) {
    const size_t off = stride * (size_t)robot;
    EkfState E = b;
    E.d_mu = ekf_moved(b.d_mu, off); E.d_sigma = ekf_moved(b.d_sigma, off); E.d_L = ekf_moved(b.d_L, off);
    E.d_id2idx = ekf_moved(b.d_id2idx, off); E.d_idx2id = ekf_moved(b.d_idx2id, off);
    E.d_last = ekf_moved(b.d_last, off); E.d_nlast = ekf_moved(b.d_nlast, off); E.d_pop = ekf_moved(b.d_pop, off);
    E.d_npop = ekf_moved(b.d_npop, off); E.d_upd = ekf_moved(b.d_upd, off); E.d_m = ekf_moved(b.d_m, off);
    E.d_V = ekf_moved(b.d_V, off); E.d_Wt = ekf_moved(b.d_Wt, off); E.d_T = ekf_moved(b.d_T, off);
    E.d_Sv = ekf_moved(b.d_Sv, off); E.d_Sw = ekf_moved(b.d_Sw, off); E.d_alpha = ekf_moved(b.d_alpha, off);
    E.d_gamma = ekf_moved(b.d_gamma, off); E.d_G = ekf_moved(b.d_G, off); E.d_g = ekf_moved(b.d_g, off);
    return E;
}

struct EkfSingle {
    EkfState E;
    __device__ __forceinline__ EkfState state() const { return E; }
    // the frame of k_ekf_plan: as passed
    __device__ __forceinline__ void frame(double&, double&, double&, int&, const ObsRaw* __restrict__&, const unsigned* __restrict__&, int&) const {}
};

struct EkfFleet {
    EkfState base;                     // robot 0's filter
    size_t stride;
    const int* work;                   // the round's rows {robot, slot, predict, 0}
    const double* enc;                 // per slot: wl, wr, dt
    __device__ __forceinline__ const int* row() const { return work + 4 * blockIdx.z; }          // wave-uniform: scalar loads
    __device__ __forceinline__ EkfState state() const { return ekf_robot_state(base, stride, row()[0]); }
    // the frame of k_ekf_plan: its slot's encoder sample, predict flag, observation list and count (obs / n_markers: the context's bases)
    __device__ __forceinline__ void frame(double& wl, double& wr, double& dt, int& do_predict, const ObsRaw* __restrict__& obs,
                                          const unsigned* __restrict__& n_markers, int& slot) const {
        const int* r = row();
        slot = r[1];
        do_predict = r[2];
        wl = enc[3 * slot]; wr = enc[3 * slot + 1]; dt = enc[3 * slot + 2];
        obs += (size_t)kMarkerMax * slot;
        n_markers += slot;
    }
};

} // namespace aslam
