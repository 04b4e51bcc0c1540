// Landmark confirmation: a marker id that is new to a SLAM map enters it only after min_sightings judged frames have
// seen it without a gap of more than max_gap frames.  The stage is a filter on the observation list of an EKF slot and runs before
// anything reads that list (the per-frame chain's k_ekf_plan, the D2H copy the host's window planner works from): a withheld sighting
// gets valid = 0 in place and from there on looks exactly like one the range / covariance gates of k_pose dropped.  No EKF kernel knows
// of it.  Included by ekf.hip (both the gfx950 build and the CPU emulation see it).
//
//   k_confirm         1 workgroup per filter of the launch (blockIdx.z), one lane per observation; the filter's table (count and last
//                     sighting per id, its frame counter) sits in LDS while the workgroup walks the filter's slots in ascending order
//   k_confirm_reseed  1 workgroup per filter: confirmed := the ids of the filter's landmark id table, every count 0, t = 0
//
// One slot (t = the filter's frame counter, already advanced):
//   step A  every sighting with valid != 0 and 0 <= id < 1024 whose id is not confirmed bids for its id with atomicMax(&last[id], t):
//           last[id] < t before the slot, so exactly one lane per id reads back a value below t.  That lane owns the id for this slot:
//           it restarts a stale count (t - last > max_gap), counts the sighting, and promotes the id at min_sightings.
//   barrier
//   step B  every such sighting whose id is still not confirmed is withheld: valid = 0, its bit set in the slot's mask.
// All integer; the only atomic is the LDS atomicMax of step A.  Global memory is written with plain stores.
#pragma once
#include "ekf.h"
#include "ekf_fleet_slam.h"

namespace aslam {

constexpr int kConfirmT = kMarkerMax;          // lanes of a k_confirm workgroup: one per observation of a slot
constexpr int kConfirmReseedT = 256;
struct alignas(16) ConfirmQuad { int v[4]; };  // four table entries: one 16-byte load or store
static_assert(kConfirmT == 128 && sizeof(SlotConfirm) == 32, "two waves, one 64-bit ballot each, fill the four mask words");
static_assert(kIdTableSize % (4 * kConfirmT) == 0 && sizeof(ConfirmTable) % 16 == 0, "the table moves 16 bytes at a time");

__global__ __launch_bounds__(kConfirmT) void k_confirm(ConfirmArg A) {
    __shared__ __align__(16) int sCnt[kIdTableSize];
    __shared__ __align__(16) int sLast[kIdTableSize];
    __shared__ int sWave[kConfirmT / 64][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int table = kConfirmSingle, first = A.first, count = A.count;
    if (A.work) {                              // a fleet round: this workgroup's robot and its one slot (wave-uniform)
        const int* r = A.work + 4 * blockIdx.z;
        table = r[0]; first = r[1]; count = 1;
    }
    ConfirmTable* __restrict__ T = A.tables + table;
    for (int i = tid; i < kIdTableSize / 4; i += kConfirmT) {
        reinterpret_cast<ConfirmQuad*>(sCnt)[i] = reinterpret_cast<const ConfirmQuad*>(T->cnt)[i];
        reinterpret_cast<ConfirmQuad*>(sLast)[i] = reinterpret_cast<const ConfirmQuad*>(T->last)[i];
    }
    int t = T->t;
    // a lane's observation of the next slot is loaded while the current slot is judged: the walk over the table is serial, the list
    // loads are not (the barriers inside the loop order LDS only and leave these loads in flight)
    int n_next = 0, id_next = -1, valid_next = 0;
    auto fetch = [&](int s) {
        n_next = (int)min(A.n_markers[s], (unsigned)kMarkerMax);
        const ObsRaw* __restrict__ p = A.obs + (size_t)s * kMarkerMax + tid;
        id_next = tid < n_next ? p->id : -1;
        valid_next = tid < n_next ? p->valid : 0;
    };
    if (count > 0) fetch(first);
    __syncthreads();
    for (int s = first; s < first + count; s++) {
        t += 1;
        ObsRaw* __restrict__ o = A.obs + (size_t)s * kMarkerMax + tid;
        const int id = id_next;
        const bool judged = valid_next != 0 && id >= 0 && id < kIdTableSize;   // (a lane beyond the list has valid_next = 0)
        if (s + 1 < first + count) fetch(s + 1);
        // step A
        bool owner = false, promoted = false;
        if (judged && sCnt[id] >= 0) {
            const int before = atomicMax(&sLast[id], t);
            owner = before < t;
            if (owner) {                       // the only lane that touches sCnt[id] in this slot
                int cnt = sCnt[id];
                if (cnt > 0 && t - before > A.max_gap) cnt = 0;
                cnt += 1;
                promoted = cnt >= A.min_sightings;
                sCnt[id] = promoted ? -1 : cnt;
            }
        }
        const unsigned long long bj = __ballot(judged), bo = __ballot(owner), bp = __ballot(promoted);
        ASLAM_LDS_BARRIER();                   // every id's verdict of this slot is in
        // step B
        const bool withheld = judged && sCnt[id] >= 0;
        if (withheld) o->valid = 0;
        const unsigned long long bw = __ballot(withheld);
        SlotConfirm* __restrict__ rec = A.rec + s;
        if (lane == 0) {
            sWave[wv][0] = __popcll(bj); sWave[wv][1] = __popcll(bo); sWave[wv][2] = __popcll(bw); sWave[wv][3] = __popcll(bp);
            rec->withheld_mask[2 * wv] = (unsigned)bw;
            rec->withheld_mask[2 * wv + 1] = (unsigned)(bw >> 32);
        }
        ASLAM_LDS_BARRIER();                   // the waves' counts are in; step B has read the table before the next slot's step A
        if (tid < 4) {
            int v = 0;
            for (int w = 0; w < kConfirmT / 64; w++) v += sWave[w][tid];
            (tid == 0 ? rec->judged : tid == 1 ? rec->tentative : tid == 2 ? rec->withheld : rec->promoted) = v;
        }
    }
    __syncthreads();
    for (int i = tid; i < kIdTableSize / 4; i += kConfirmT) {
        reinterpret_cast<ConfirmQuad*>(T->cnt)[i] = reinterpret_cast<const ConfirmQuad*>(sCnt)[i];
        reinterpret_cast<ConfirmQuad*>(T->last)[i] = reinterpret_cast<const ConfirmQuad*>(sLast)[i];
    }
    if (tid == 0) T->t = t;
}

__global__ __launch_bounds__(kConfirmReseedT) void k_confirm_reseed(ConfirmReseed A) {
    __shared__ int sCnt[kIdTableSize];
    const int tid = threadIdx.x, k = blockIdx.z;
    const EkfState E = ekf_robot_state(A.base, A.stride, A.robot[k]);
    ConfirmTable* __restrict__ T = A.tables + (A.single ? kConfirmSingle : (int)A.robot[k]);
    const int L = min(max(*E.d_L, 0), E.max_landmarks);
    for (int id = tid; id < kIdTableSize; id += kConfirmReseedT) sCnt[id] = 0;
    __syncthreads();
    for (int i = tid; i < L; i += kConfirmReseedT) {
        const int id = E.d_idx2id[i];
        if (id >= 0 && id < kIdTableSize) sCnt[id] = -1;       // (lanes that meet on an id store the same value)
    }
    __syncthreads();
    for (int id = tid; id < kIdTableSize; id += kConfirmReseedT) {
        T->cnt[id] = sCnt[id];
        T->last[id] = 0;
    }
    if (tid == 0) T->t = 0;
}

void launch_confirm(hipStream_t st, const ConfirmArg& A, int filters) {
    hipLaunchKernelGGL(k_confirm, dim3(1, 1, filters), dim3(kConfirmT), 0, st, A);
}
void launch_confirm_reseed(hipStream_t st, const ConfirmReseed& A) {
    hipLaunchKernelGGL(k_confirm_reseed, dim3(1, 1, A.n), dim3(kConfirmReseedT), 0, st, A);
}

} // namespace aslam
