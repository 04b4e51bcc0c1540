// Fleet localization: R robots, each with its own pose filter (mu_x, Sigma_xx) and last_observed_marker_ list, on
// one shared frozen map (the id table and the landmark rows of mu, as in localization, ekf_localize.h).  Included by ekf.hip
// (both the gfx950 build and the CPU emulation see it).
//
// k_fleet_steps<G, M, C> (the policies of ekf_localize.h) runs one 128-lane workgroup per robot present in a call: §11's per-slot
// body (loc_steps) over that robot's slots in ascending order, on the robot's own filter.  Robots never interact, so the workgroups
// are independent.  The host builds the work list below and keeps the armed flags.
#pragma once
#include "ekf_localize.h"

namespace aslam {

// Work list of one call, n groups (one per robot present):
//     int hdr[4 * n]: robot, predict_first, offset of its slots in slots[], number of slots
//     int slots[]:    the robots' slots, ascending within each robot
// The robots' filters are in FleetState (ekf.h).

// robot `robot`'s filter and its slots of the call
struct LocFleet {
    const FleetState& F;
    int robot;
    const int* slots;
    int count, predict_first;
    static constexpr bool kPopList = false;          // aslam_get_observations describes the single filter, not a robot
    __device__ __forceinline__ int track() const { return robot; }
    __device__ __forceinline__ int n() const { return count; }
    __device__ __forceinline__ int slot(int k) const { return slots[k]; }
    __device__ __forceinline__ bool predict(int k) const { return k > 0 || predict_first; }
    __device__ __forceinline__ void load(double& mx, double& my, double& mt, double* P) const {
        const double* s = F.pose + (size_t)kFleetState * robot;
        mx = s[0]; my = s[1]; mt = s[2];
#pragma unroll
        for (int i = 0; i < 9; i++) P[i] = s[3 + i];
    }
    __device__ __forceinline__ void store(double mx, double my, double mt, const double* P) const {
        double* s = F.pose + (size_t)kFleetState * robot;
        s[0] = mx; s[1] = my; s[2] = mt;
#pragma unroll
        for (int i = 0; i < 9; i++) s[3 + i] = P[i];
    }
    __device__ __forceinline__ LastObs* last() const { return F.last + (size_t)kMarkerMax * robot; }
    __device__ __forceinline__ int* nlast() const { return F.nlast + robot; }
    // uncertain map: the robot's own cross strip, 3 x W row-major, in LDS (sX) as in memory
    template <class M> __device__ __forceinline__ void load_cross(const M& um, double* sX) const {
        const int n = 9 * um.m.L;
        const double* g = um.m.cross + (size_t)n * robot;
        for (int j = threadIdx.x; j < n; j += kMarkerMax) sX[j] = g[j];
    }
    template <class M> __device__ __forceinline__ void store_cross(const M& um, const double* sX) const {
        const int n = 9 * um.m.L;
        double* g = um.m.cross + (size_t)n * robot;
        for (int j = threadIdx.x; j < n; j += kMarkerMax) g[j] = sX[j];
    }
};

// one instantiation per combination of policies, as k_loc_steps (ekf_localize.h): every robot's workgroup gates its own corrections
// and keeps its own records, carries its own Sigma_xl in dynamic LDS (§23), corrects from its own running mean (§32)
template <class G, class M, class C>
__global__ __launch_bounds__(kMarkerMax) void k_fleet_steps(EkfState E, FleetState F, SlamParams sp, const ObsRaw* __restrict__ obs,
                                                           const unsigned* __restrict__ n_markers, const double* __restrict__ enc,
                                                           const int* __restrict__ work, int n_groups, LocPolicy<G, M, C> p) {
    const int* h = work + 4 * blockIdx.x;            // wave-uniform: scalar loads
    loc_steps<LocFleet, G, M, C>(LocFleet{F, h[0], work + 4 * n_groups + h[2], h[3], h[1]}, E, sp, obs, n_markers, enc, G(p), M(p));
}

void launch_fleet_steps(hipStream_t st, const EkfState& E, const FleetState& F, const SlamParams& sp, const ObsRaw* obs,
                        const unsigned* n_markers, const double* enc, const int* work, int n_groups, const GateState* gate, const MapCov* umap,
                        bool consistent) {
    with_loc_policies(gate, umap, consistent, [&](auto g, auto m, auto c) {
        launch_steps_kernel<k_fleet_steps<decltype(g), decltype(m), decltype(c)>>(st, n_groups, g, m, c, E, F, sp, obs, n_markers, enc, work, n_groups);
    });
}

} // namespace aslam
