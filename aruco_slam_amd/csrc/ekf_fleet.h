// Fleet localization: R robots, each with its own pose filter (mu_x, Sigma_xx) and last_observed_marker_ list, on
// one shared frozen map (the id table and the landmark rows of mu, as in localization, ekf_localize.h).  Included by ekf.hip
// (both the gfx950 build and the CPU emulation see it).
//
// k_fleet_steps runs one 128-lane workgroup per robot present in a call: §11's per-slot body (loc_steps) over that robot's slots in
// ascending order, on the robot's own filter.  Robots never interact, so the workgroups are independent.  The host builds the work
// list below and keeps the armed flags.
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

__global__ __launch_bounds__(kMarkerMax) void k_fleet_steps(EkfState E, FleetState F, SlamParams sp, const ObsRaw* __restrict__ obs,
                                                           const unsigned* __restrict__ n_markers, const double* __restrict__ enc,
                                                           const int* __restrict__ work, int n_groups) {
    const int* h = work + 4 * blockIdx.x;            // wave-uniform: scalar loads
    loc_steps(LocFleet{F, h[0], work + 4 * n_groups + h[2], h[3], h[1]}, E, sp, obs, n_markers, enc);
}

// the same with the innovation gate: every robot's workgroup gates its own corrections and keeps its own records
__global__ __launch_bounds__(kMarkerMax) void k_fleet_steps_gated(EkfState E, FleetState F, SlamParams sp, const ObsRaw* __restrict__ obs,
                                                                 const unsigned* __restrict__ n_markers, const double* __restrict__ enc,
                                                                 const int* __restrict__ work, int n_groups, GateState g) {
    const int* h = work + 4 * blockIdx.x;
    loc_steps(LocFleet{F, h[0], work + 4 * n_groups + h[2], h[3], h[1]}, E, sp, obs, n_markers, enc, Gated{g});
}

// the same two on an uncertain map: every robot's workgroup carries its own Sigma_xl in dynamic LDS
__global__ __launch_bounds__(kMarkerMax) void k_fleet_steps_umap(EkfState E, FleetState F, SlamParams sp, const ObsRaw* __restrict__ obs,
                                                                const unsigned* __restrict__ n_markers, const double* __restrict__ enc,
                                                                const int* __restrict__ work, int n_groups, MapCov mc) {
    const int* h = work + 4 * blockIdx.x;
    loc_steps(LocFleet{F, h[0], work + 4 * n_groups + h[2], h[3], h[1]}, E, sp, obs, n_markers, enc, NoGate{}, UncertainMap{mc});
}

__global__ __launch_bounds__(kMarkerMax) void k_fleet_steps_umap_gated(EkfState E, FleetState F, SlamParams sp, const ObsRaw* __restrict__ obs,
                                                                      const unsigned* __restrict__ n_markers, const double* __restrict__ enc,
                                                                      const int* __restrict__ work, int n_groups, GateState g, MapCov mc) {
    const int* h = work + 4 * blockIdx.x;
    loc_steps(LocFleet{F, h[0], work + 4 * n_groups + h[2], h[3], h[1]}, E, sp, obs, n_markers, enc, Gated{g}, UncertainMap{mc});
}

// the same four with consistent innovations: a robot's workgroup is the single filter's RunningMean body
__global__ __launch_bounds__(kMarkerMax) void k_fleet_steps_ci(EkfState E, FleetState F, SlamParams sp, const ObsRaw* __restrict__ obs,
                                                              const unsigned* __restrict__ n_markers, const double* __restrict__ enc,
                                                              const int* __restrict__ work, int n_groups) {
    const int* h = work + 4 * blockIdx.x;
    loc_steps<LocFleet, NoGate, FixedMap, RunningMean>(LocFleet{F, h[0], work + 4 * n_groups + h[2], h[3], h[1]}, E, sp, obs, n_markers, enc);
}

__global__ __launch_bounds__(kMarkerMax) void k_fleet_steps_ci_gated(EkfState E, FleetState F, SlamParams sp, const ObsRaw* __restrict__ obs,
                                                                    const unsigned* __restrict__ n_markers, const double* __restrict__ enc,
                                                                    const int* __restrict__ work, int n_groups, GateState g) {
    const int* h = work + 4 * blockIdx.x;
    loc_steps<LocFleet, Gated, FixedMap, RunningMean>(LocFleet{F, h[0], work + 4 * n_groups + h[2], h[3], h[1]}, E, sp, obs, n_markers, enc, Gated{g});
}

__global__ __launch_bounds__(kMarkerMax) void k_fleet_steps_umap_ci(EkfState E, FleetState F, SlamParams sp, const ObsRaw* __restrict__ obs,
                                                                   const unsigned* __restrict__ n_markers, const double* __restrict__ enc,
                                                                   const int* __restrict__ work, int n_groups, MapCov mc) {
    const int* h = work + 4 * blockIdx.x;
    loc_steps<LocFleet, NoGate, UncertainMap, RunningMean>(LocFleet{F, h[0], work + 4 * n_groups + h[2], h[3], h[1]}, E, sp, obs, n_markers, enc, NoGate{},
                                                           UncertainMap{mc});
}

__global__ __launch_bounds__(kMarkerMax) void k_fleet_steps_umap_ci_gated(EkfState E, FleetState F, SlamParams sp, const ObsRaw* __restrict__ obs,
                                                                         const unsigned* __restrict__ n_markers, const double* __restrict__ enc,
                                                                         const int* __restrict__ work, int n_groups, GateState g, MapCov mc) {
    const int* h = work + 4 * blockIdx.x;
    loc_steps<LocFleet, Gated, UncertainMap, RunningMean>(LocFleet{F, h[0], work + 4 * n_groups + h[2], h[3], h[1]}, E, sp, obs, n_markers, enc, Gated{g},
                                                          UncertainMap{mc});
}

void launch_fleet_steps(hipStream_t st, const EkfState& E, const FleetState& F, const SlamParams& sp, const ObsRaw* obs,
                        const unsigned* n_markers, const double* enc, const int* work, int n_groups, const GateState* gate, const MapCov* umap,
                        bool consistent) {
    if (consistent) {                // the RunningMean kernels, the same launches otherwise
        if (umap) {
            static bool allowed[2] = {false, false};
            const size_t dyn = umap_lds_bytes(umap->L);
            if (gate) {
                umap_allow_lds(k_fleet_steps_umap_ci_gated, allowed[1]);
                hipLaunchKernelGGL(k_fleet_steps_umap_ci_gated, dim3(n_groups), dim3(kMarkerMax), dyn, st, E, F, sp, obs, n_markers, enc, work, n_groups, *gate, *umap);
            } else {
                umap_allow_lds(k_fleet_steps_umap_ci, allowed[0]);
                hipLaunchKernelGGL(k_fleet_steps_umap_ci, dim3(n_groups), dim3(kMarkerMax), dyn, st, E, F, sp, obs, n_markers, enc, work, n_groups, *umap);
            }
            return;
        }
        if (gate)
            hipLaunchKernelGGL(k_fleet_steps_ci_gated, dim3(n_groups), dim3(kMarkerMax), 0, st, E, F, sp, obs, n_markers, enc, work, n_groups, *gate);
        else
            hipLaunchKernelGGL(k_fleet_steps_ci, dim3(n_groups), dim3(kMarkerMax), 0, st, E, F, sp, obs, n_markers, enc, work, n_groups);
        return;
    }
    if (umap) {
        static bool allowed[2] = {false, false};
        const size_t dyn = umap_lds_bytes(umap->L);
        if (gate) {
            umap_allow_lds(k_fleet_steps_umap_gated, allowed[1]);
            hipLaunchKernelGGL(k_fleet_steps_umap_gated, dim3(n_groups), dim3(kMarkerMax), dyn, st, E, F, sp, obs, n_markers, enc, work, n_groups, *gate, *umap);
        } else {
            umap_allow_lds(k_fleet_steps_umap, allowed[0]);
            hipLaunchKernelGGL(k_fleet_steps_umap, dim3(n_groups), dim3(kMarkerMax), dyn, st, E, F, sp, obs, n_markers, enc, work, n_groups, *umap);
        }
        return;
    }
    if (gate)
        hipLaunchKernelGGL(k_fleet_steps_gated, dim3(n_groups), dim3(kMarkerMax), 0, st, E, F, sp, obs, n_markers, enc, work, n_groups, *gate);
    else
        hipLaunchKernelGGL(k_fleet_steps, dim3(n_groups), dim3(kMarkerMax), 0, st, E, F, sp, obs, n_markers, enc, work, n_groups);
}

} // namespace aslam
