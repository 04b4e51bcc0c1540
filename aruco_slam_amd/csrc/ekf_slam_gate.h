// Innovation gate of the SLAM chains (include/aruco_slam_hip.h).  Included by ekf.hip ahead of the kernels (the gfx950
// build and the CPU emulation both see it).
//
// The solve kernels of the per-frame chains (k_ekf_mid, k_ekf_mid64, k_ekf_small and its ekf_small_general) are templates on a gate
// policy beside their state source.  Pivot block ib of their block Gauss-Jordan sweep IS the reference's S_ib = H Sigma_{ib-1} H^T + R
// with the live Sigma (aruco_slam.cpp:146), so d2 = ze^T S_ib^-1 ze costs 15 flops where S_ib^-1 is formed.  A rejected correction is a
// pivot that is not eliminated: its block row and block column become zero and stay zero under every later pivot (a later pivot jb
// changes A(ib, .) by A(ib, jb) Y = 0 and A(., ib) by F Y(jb, ib) = F S^-1 A(jb, ib) = 0), the other blocks never see it.  The
// result G is the frame's G without that correction, with a zero block row and column in its place; everything behind the solve
// (k_ekf_apply, k_ekf_T, k_ekf_update_mfma, mu += W g) runs unchanged.
//   NoSlamGate  the default: every gated statement sits under `if constexpr`, the kernels are the ungated ones.
//   SlamGate    the threshold and where the solve leaves d2 and its verdict per correction, in update order; k_ekf_gate_finish turns
//               them into the pop list's actions, the compacted last-observed list, the slot record and the track record.
#pragma once
#include "ekf.h"
#include "ekf_dev.h"
#include "ekf_fleet_slam.h"
#include <cmath>

namespace aslam {

struct NoSlamGate { static constexpr bool kOn = false; };
struct SlamGate {
    static constexpr bool kOn = true;
    double gate_d2;                    // > 0, or +inf: monitor only
    double* out;                       // per filter of the launch (blockIdx.z) 2 kMarkerMax doubles: d2 per update position, then 1.0 = accepted / 0.0 = rejected
    __device__ __forceinline__ double* mine() const { return out + (size_t)2 * kMarkerMax * blockIdx.z; }
};

// What a solve kernel takes: its state source and its gate policy as the two bases of one struct.  NoSlamGate is an empty base, so an
// ungated kernel's argument has the bytes of Src alone (an empty struct passed beside Src would take a slot of its own and move the
// hidden arguments behind it: the kernels would no longer be instruction for instruction the ungated ones).
// The innovation policy C (FrozenMean / RunningMean, ekf_dev.h) is a third base, empty in both its forms: the argument
// bytes of every instantiation are those of Src and G.  With RunningMean the solve carries the running innovation e_r -= (H_r K_i) e_i
// through the sweep where the gate needs it (the multiplier is the block the sweep already forms), judges pivot i by e_i and emits
// g = G ze (rejected entries masked), which is sum_i gamma_i e_i: G, and with it Sigma, keep their bits.
template <class Src, class G, class C = FrozenMean> struct Solve : Src, G, C {};

__device__ __forceinline__ bool slam_gate_rejects(const SlamGate& g, double d2) {
    return g.gate_d2 < HUGE_VAL && !(d2 <= g.gate_d2);                         // a NaN d2 rejects
}
__device__ __forceinline__ double slam_gate_d2(const double* Si, double z0, double z1, double z2) {   // ze^T S^-1 ze, S^-1 row-major
    return z0 * (Si[0] * z0 + Si[1] * z1 + Si[2] * z2) + z1 * (Si[3] * z0 + Si[4] * z1 + Si[5] * z2) +
           z2 * (Si[6] * z0 + Si[7] * z1 + Si[8] * z2);
}
// the verdict on update `pos` from its S^-1 and frozen-mean innovation, by the one thread that formed S^-1: d2 and the verdict go to
// the filter's buffer; returns 1.0 = accepted, 0.0 = rejected (what the solve publishes beside S^-1)
__device__ __forceinline__ double slam_gate_verdict(const SlamGate& g, const double* Si, double z0, double z1, double z2, int pos) {
    const double d2 = slam_gate_d2(Si, z0, z1, z2);
    const double acc = slam_gate_rejects(g, d2) ? 0.0 : 1.0;
    double* o = g.mine();
    o[pos] = d2;
    o[kMarkerMax + pos] = acc;
    return acc;
}

// which slot record and which track record a filter's frame belongs to
__device__ __forceinline__ void slam_gate_where(const EkfSingle&, int slot_arg, int& slot, int& track) { slot = slot_arg; track = kTrackSingle; }
__device__ __forceinline__ void slam_gate_where(const EkfFleet& S, int, int& slot, int& track) { slot = S.row()[1]; track = S.row()[0]; }

// After the solve: one workgroup per filter (blockIdx.z = the robot of the round), thread q on popped observation q.  The update
// positions are the action-1 entries of d_pop in order (k_ekf_plan's own prefix).  Rejected observations get action 3 and leave
// d_last (two-wave ballots and a prefix, as the compaction of the localization steps, ekf_localize.h); lane 0 then walks the pop
// list once, in order: the slot record, entry [2] of the slot stats, the track record (the integer streak rule of §19).
template <class Src>
static __global__ __launch_bounds__(kMarkerMax) void k_ekf_gate_finish(Src S, SlamGate gate, GateState gs, int slot_arg) {
    const EkfState E = S.state();
    __shared__ double sD2[kMarkerMax], sZn[kMarkerMax];
    __shared__ int sKind[kMarkerMax], sId[kMarkerMax];        // 0: no correction, 1: accepted, 2: rejected
    __shared__ int sUpdCnt[2], sKeepCnt[2];
    const int tid = threadIdx.x;
    int slot, track;
    slam_gate_where(S, slot_arg, slot, track);
    const int np = min(*E.d_npop, kMarkerMax);
    const int m = *E.d_m;                                      // 0: nothing was solved (no correction, or more than the chain takes: reported by k_ekf_plan)
    const double* verdicts = gate.mine();
    PopRec pr{};
    LastObs lo{};
    if (tid < np) { pr = E.d_pop[tid]; lo = E.d_last[tid]; }
    const bool upd = tid < np && m > 0 && pr.action == 1;
    const unsigned long long bU = __ballot(upd);
    if ((tid & 63) == 0) sUpdCnt[tid >> 6] = __popcll(bU);
    __syncthreads();
    bool rej = false;
    int kind = 0;
    if (upd) {
        const int up = (tid >= 64 ? sUpdCnt[0] : 0) + __popcll(bU & ((1ull << (tid & 63)) - 1ull));   // < m <= kMarkerMax
        const double* ze = E.d_upd[up].ze;
        rej = verdicts[kMarkerMax + up] == 0.0;
        kind = rej ? 2 : 1;
        sD2[tid] = verdicts[up];
        sZn[tid] = sqrt(ze[0] * ze[0] + ze[1] * ze[1] + ze[2] * ze[2]);
        if (rej) E.d_pop[tid].action = 3;
    }
    sKind[tid] = kind;
    sId[tid] = pr.id;
    const bool keep = tid < np && !rej;
    const unsigned long long bK = __ballot(keep);
    if ((tid & 63) == 0) sKeepCnt[tid >> 6] = __popcll(bK);
    __syncthreads();                                           // every lane holds its entry of d_last
    if (keep) E.d_last[(tid >= 64 ? sKeepCnt[0] : 0) + __popcll(bK & ((1ull << (tid & 63)) - 1ull))] = lo;
    if (tid == 0) {
        *E.d_nlast = sKeepCnt[0] + sKeepCnt[1];
        int att = 0, acc = 0, nrej = 0, flag = 0, worst = -1;
        double nis = 0.0, mx = 0.0;
        bool have = false;
        for (int q = 0; q < np; q++) {                         // pop order
            const int k = sKind[q];
            if (k == 0) continue;
            const double d2 = sD2[q];
            att++;
            flag += sZn[q] >= 1.0 ? 1 : 0;                    // the ||ze|| half of aruco_slam.cpp:156 (the chains never form K)
            if (d2 == d2 && (!have || d2 > mx)) { have = true; mx = d2; worst = sId[q]; }
            if (k == 2) nrej++;
            else { acc++; nis += d2; }
        }
        if (slot >= 0 && slot < E.max_slots) {
            E.d_slot_stat[4 * slot + 2] = acc;                 // corrections fused: the accepted ones
            SlotHealth* h = gs.slot + slot;
            h->attempted = att; h->accepted = acc; h->rejected = nrej; h->ref_flagged = flag;
            h->nis_sum = nis; h->d2_max = mx; h->worst_id = worst; h->pad = 0;
        }
        TrackHealth* t = gs.track + track;
        int streak = t->bad_streak;
        if (att >= gs.min_attempted) streak = 100 * acc < gs.min_accept_percent * att ? streak + 1 : 0;
        t->frames = t->frames + 1;
        t->accepted_total = t->accepted_total + acc;
        t->rejected_total = t->rejected_total + nrej;
        t->bad_streak = streak;
        t->lost = streak >= gs.lost_after ? 1 : 0;
        t->pad[0] = t->pad[1] = t->pad[2] = 0;
    }
}

} // namespace aslam
