// Map edit: landmarks taken out of a SLAM filter on the device.  Marginalising a landmark out of a Gaussian is
// deleting its three rows and columns of mu and Sigma: no arithmetic, only data movement, in place.  Included by ekf.hip (both the
// gfx950 build and the CPU emulation see it).
//
// One removal on n filters (the single one, or the listed robots of a SLAM fleet: blockIdx.z = position in the list) is three
// launches on one stream:
//   k_map_plan  1 workgroup per filter: the kept flags of the landmarks prefix-scanned into src_of[] (new state index -> old state
//               index, strictly increasing, src_of[b] >= b); idx2id, id2idx, L and mu rewritten; the last-observed list compacted;
//               {N, N', removed} left in the filter's meta row for the two Sigma passes and the host
//   k_map_cols  columns compacted: a workgroup owns a strip of 16 rows, all columns
//   k_map_rows  rows compacted: a workgroup owns one new column, all rows
// Every kept entry moves towards lower addresses, so a pass must never read what it has already overwritten.  Both Sigma passes walk
// their index in ascending batches: a batch reads old indices src_of[i] >= i of its own range or beyond, passes one workgroup
// barrier, and writes new indices of its own range, all below everything a later batch reads.  Across workgroups there is nothing
// to order inside a launch: no workgroup of k_map_cols touches another's rows, none of k_map_rows another's column; the stream
// orders the launches.  Only the N x N corner of the ld x ld array is touched.
#pragma once
#include "ekf.h"
#include "ekf_fleet_slam.h"
#include <climits>

namespace aslam {

constexpr int kMapEditT = 256;         // lanes of a k_map_plan / k_map_rows workgroup
constexpr int kMapColsT = 1024;        // lanes of a k_map_cols workgroup
constexpr int kMapStrip = 16;          // rows of a k_map_cols strip: one 128-byte segment per column (ld / 16 workgroups fill the chip)
constexpr int kMapColsSlots = kMapColsT / kMapStrip;   // columns the workgroup's lanes stand on at a time
constexpr int kMapColsU = 8;           // columns a k_map_cols lane has in flight per batch (loads first, then their stores)
constexpr int kMapRowsU = 4;           // rows a k_map_rows lane has in flight per batch

__device__ __forceinline__ bool map_edit_listed(const MapEdit& J, int id) {
    return id >= 0 && id < kIdTableSize && ((J.ids[id >> 5] >> (id & 31)) & 1u);
}

// One workgroup per filter.  Landmarks and the last-observed list are compacted in place in ascending chunks of one entry per lane:
// a chunk is read, a barrier passed, and written at positions <= its own, which no later chunk reads.
__global__ __launch_bounds__(kMapEditT) void k_map_plan(MapEdit J) {
    __shared__ int sFirst[kIdTableSize];       // per id: lowest new index of a kept landmark with it
    __shared__ int sWave[kMapEditT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int k = blockIdx.z;
    const EkfState E = ekf_robot_state(J.base, J.stride, J.robot[k]);
    int* __restrict__ src_of = J.src_of + (size_t)k * E.ld;
    const int L = min(max(*E.d_L, 0), E.max_landmarks);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int id = tid; id < kIdTableSize; id += kMapEditT) sFirst[id] = INT_MAX;
    if (tid < 3) src_of[tid] = tid;
    __syncthreads();
    int kept = 0;                              // landmarks kept by the chunks so far (the same in every lane)
    for (int i0 = 0; i0 < L; i0 += kMapEditT) {
        const int i = i0 + tid;
        int id = -1;
        double m0 = 0.0, m1 = 0.0, m2 = 0.0;
        bool keep = false;
        if (i < L) {
            id = E.d_idx2id[i];
            m0 = E.d_mu[3 + 3 * i]; m1 = E.d_mu[4 + 3 * i]; m2 = E.d_mu[5 + 3 * i];
            keep = !map_edit_listed(J, id);
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) sWave[wv] = __popcll(bal);
        __syncthreads();                       // the chunk is read; the waves' counts are in
        int before = kept, total = 0;
        for (int w = 0; w < kMapEditT / 64; w++) {
            if (w < wv) before += sWave[w];
            total += sWave[w];
        }
        if (keep) {
            const int ni = before + __popcll(bal & below);
            E.d_idx2id[ni] = id;
            E.d_mu[3 + 3 * ni] = m0; E.d_mu[4 + 3 * ni] = m1; E.d_mu[5 + 3 * ni] = m2;
            for (int c = 0; c < 3; c++) src_of[3 + 3 * ni + c] = 3 + 3 * i + c;
            if (id >= 0 && id < kIdTableSize) atomicMin(&sFirst[id], ni);
        }
        kept += total;
        __syncthreads();                       // sWave is free again
    }
    for (int i = kept + tid; i < L; i += kMapEditT) {          // the vacated tail, as aslam_set_state leaves unused entries
        E.d_idx2id[i] = -1;
        E.d_mu[3 + 3 * i] = 0.0; E.d_mu[4 + 3 * i] = 0.0; E.d_mu[5 + 3 * i] = 0.0;
    }
    for (int id = tid; id < kIdTableSize; id += kMapEditT) E.d_id2idx[id] = sFirst[id] == INT_MAX ? -1 : sFirst[id];

    // last_observed_marker_: entries of removed ids go, the others stay in order (kMarkerMax <= kMapEditT: one chunk)
    const int nl = min(max(*E.d_nlast, 0), kMarkerMax);
    LastObs e{};
    bool keep_last = false;
    if (tid < nl) {
        e = E.d_last[tid];
        keep_last = !map_edit_listed(J, e.id);
    }
    const unsigned long long bal = __ballot(keep_last);
    if (lane == 0) sWave[wv] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kMapEditT / 64; w++) {
        if (w < wv) before += sWave[w];
        total += sWave[w];
    }
    if (keep_last) E.d_last[before + __popcll(bal & below)] = e;
    if (tid == 0) {
        *E.d_nlast = total;
        *E.d_L = kept;
        int* meta = J.meta + 4 * k;
        meta[0] = 3 + 3 * L; meta[1] = 3 + 3 * kept; meta[2] = L - kept; meta[3] = 0;
    }
}

// Columns: Sigma[r, b] := Sigma[r, src_of[b]] for b < N', then 0.0 for N' <= b < N, for the rows r < N of the strip.  The workgroup's
// lanes are kMapStrip rows x kMapColsSlots columns: 16 consecutive lanes on the 16 rows of one column (a 128-byte segment), a wave on
// four neighbouring columns, each lane kMapColsU columns of a batch of kMapColsSlots * kMapColsU new columns.  A batch reads old
// columns >= its first new column and, behind the barrier, writes new columns below the next batch's first.
__global__ __launch_bounds__(kMapColsT) void k_map_cols(MapEdit J) {
    const int k = blockIdx.z;
    const int N = J.meta[4 * k], Nk = J.meta[4 * k + 1];
    if (N == Nk || (int)blockIdx.x * kMapStrip >= N) return;   // nothing removed, or a strip beyond the state (whole workgroup)
    const EkfState E = ekf_robot_state(J.base, J.stride, J.robot[k]);
    const int* __restrict__ src_of = J.src_of + (size_t)k * E.ld;
    const int slot = threadIdx.x / kMapStrip;
    const int row = blockIdx.x * kMapStrip + threadIdx.x % kMapStrip;
    const bool live = row < N;
    const size_t ld = (size_t)E.ld;
    double* S = E.d_sigma + row;
    for (int b0 = 0; b0 < Nk; b0 += kMapColsSlots * kMapColsU) {
        double v[kMapColsU];
        int s[kMapColsU];
#pragma unroll
        for (int u = 0; u < kMapColsU; u++) {
            const int b = b0 + u * kMapColsSlots + slot;
            s[u] = b < Nk ? src_of[b] : b;                     // a column that stays where it is is not moved
            v[u] = 0.0;
            if (live && s[u] != b) v[u] = S[(size_t)s[u] * ld];
        }
        __syncthreads();                                       // every load of the batch is done
#pragma unroll
        for (int u = 0; u < kMapColsU; u++) {
            const int b = b0 + u * kMapColsSlots + slot;
            if (live && s[u] != b) S[(size_t)b * ld] = v[u];
        }
    }
    if (live)
        for (int b = Nk + slot; b < N; b += kMapColsSlots) S[(size_t)b * ld] = 0.0;
}

// Rows: Sigma[a, b] := Sigma[src_of[a], b] for a < N', then 0.0 for N' <= a < N, in new column b = blockIdx.x < N' (the columns
// [N', N) are zero since k_map_cols).  A batch is kMapRowsU rows per lane, consecutive lanes on consecutive rows.
__global__ __launch_bounds__(kMapEditT) void k_map_rows(MapEdit J) {
    const int k = blockIdx.z;
    const int N = J.meta[4 * k], Nk = J.meta[4 * k + 1];
    const int b = blockIdx.x;
    if (N == Nk || b >= Nk) return;
    const EkfState E = ekf_robot_state(J.base, J.stride, J.robot[k]);
    const int* __restrict__ src_of = J.src_of + (size_t)k * E.ld;
    double* col = E.d_sigma + (size_t)b * E.ld;
    const int tid = threadIdx.x;
    for (int a0 = 0; a0 < Nk; a0 += kMapEditT * kMapRowsU) {
        double v[kMapRowsU];
        int s[kMapRowsU];
#pragma unroll
        for (int u = 0; u < kMapRowsU; u++) {
            const int a = a0 + u * kMapEditT + tid;
            s[u] = a < Nk ? src_of[a] : a;
            v[u] = 0.0;
            if (s[u] != a) v[u] = col[s[u]];
        }
        __syncthreads();                                       // every load of the batch is done
#pragma unroll
        for (int u = 0; u < kMapRowsU; u++) {
            const int a = a0 + u * kMapEditT + tid;
            if (s[u] != a) col[a] = v[u];
        }
    }
    for (int a = Nk + tid; a < N; a += kMapEditT) col[a] = 0.0;
}

hipError_t map_edit_reserve(MapEditBufs& B, int filters, int ld) {
    if (filters <= B.cap) return hipSuccess;
    map_edit_free(B);
    MapEditBufs b{};
    hipError_t e;
    if ((e = hipMalloc(reinterpret_cast<void**>(&b.src_of), sizeof(int) * (size_t)filters * ld)) != hipSuccess ||
        (e = hipMalloc(reinterpret_cast<void**>(&b.meta), sizeof(int) * 4 * (size_t)filters)) != hipSuccess ||
        (e = hipHostMalloc(reinterpret_cast<void**>(&b.h_meta), sizeof(int) * 4 * (size_t)filters, hipHostMallocDefault)) != hipSuccess) {
        map_edit_free(b);
        return e;
    }
    b.cap = filters;
    B = b;
    return hipSuccess;
}

void map_edit_free(MapEditBufs& B) {
    if (B.src_of) hipFree(B.src_of);
    if (B.meta) hipFree(B.meta);
    if (B.h_meta) hipHostFree(B.h_meta);
    B = MapEditBufs{};
}

void launch_map_plan(hipStream_t st, const MapEdit& J) {
    hipLaunchKernelGGL(k_map_plan, dim3(1, 1, J.n), dim3(kMapEditT), 0, st, J);
}
void launch_map_cols(hipStream_t st, const MapEdit& J) {
    hipLaunchKernelGGL(k_map_cols, dim3((J.base.ld + kMapStrip - 1) / kMapStrip, 1, J.n), dim3(kMapColsT), 0, st, J);
}
void launch_map_rows(hipStream_t st, const MapEdit& J) {
    hipLaunchKernelGGL(k_map_rows, dim3(J.base.ld, 1, J.n), dim3(kMapEditT), 0, st, J);
}

} // namespace aslam
