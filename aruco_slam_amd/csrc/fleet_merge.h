// Map merge: N landmark maps given as MapRecord records, each in its own frame, aligned into one anchor map's frame
// from the marker ids they share and fused per marker id.  Included by ekf.hip (both the gfx950 build and the CPU emulation see it).
//
// Data flow of one merge of n_maps maps of per_map records (all tables in MergeBufs, ekf.h):
//   k_fleet_export_maps  (fleet source only) every robot's map as records, robot z into rows [z * max_landmarks, ...)
//   k_merge_index        id -> record position per map; the reference table := the anchor's records; rounds / transforms reset
//   per round k = 1, 2, ... (the host reads the aligned count back after each round and stops when it did not grow or is n_maps):
//     k_merge_align      every map not yet aligned against the table as k_merge_insert of round k - 1 left it
//     k_merge_insert     the ids the table lacks, from the lowest map aligned in round k that has them
//   k_merge_fuse         per id of the table: information-form fusion of the aligned maps' marginals, compacted in ascending id order
// No kernel waits for another workgroup, and there is no floating-point atomic: every sum has a fixed order, so the same input
// gives the same bits.
#pragma once
#include "ekf.h"
#include "ekf_dev.h"
#include "ekf_fleet_slam.h"

namespace aslam {

constexpr int kMergeAlignT = 256;      // lanes of a k_merge_align workgroup: 4 ids each
constexpr int kMergeFuseT = 64;        // lanes of a k_merge_fuse workgroup: one wave, one id per lane

// what k_ekf_export_map does, for robot blockIdx.z of a SLAM fleet: its landmarks as records, unused ones id = -1
__global__ __launch_bounds__(256) void k_fleet_export_maps(EkfState base, size_t stride, MapRecord* __restrict__ out) {
    const EkfState E = ekf_robot_state(base, stride, blockIdx.z);
    const int L = *E.d_L;
    const int ld = E.ld;
    MapRecord* dst = out + (size_t)blockIdx.z * E.max_landmarks;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < E.max_landmarks; i += gridDim.x * 256) {
        MapRecord r;
        if (i < L) {
            const int li = 3 + 3 * i;
            r.id = E.d_idx2id[i]; r.index = i;
            r.x = E.d_mu[li]; r.y = E.d_mu[li + 1]; r.theta = E.d_mu[li + 2];
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) r.S[a * 3 + b] = E.d_sigma[(size_t)(li + b) * ld + li + a];
        } else {
            r.id = -1; r.index = -1; r.x = r.y = r.theta = 0;
            for (int k = 0; k < 9; k++) r.S[k] = 0;
        }
        dst[i] = r;
    }
}

// One workgroup per map, one record per thread and pass.  The map's id -> position table is built in LDS: filled with -1 (as
// unsigned the largest value), then atomicMin of the position, so of two records with one id the lower position stays.  The anchor's
// workgroup also writes the reference table and the aligned count (1: the anchor).
__global__ __launch_bounds__(256) void k_merge_index(MergeBufs M, const MapRecord* __restrict__ rec, int per_map, int anchor) {
    __shared__ unsigned pos[kIdTableSize];
    const int m = blockIdx.x;
    const MapRecord* mine = rec + (size_t)m * per_map;
    for (int id = threadIdx.x; id < kIdTableSize; id += 256) pos[id] = 0xFFFFFFFFu;
    __syncthreads();
    for (int i = threadIdx.x; i < per_map; i += 256) {
        const int id = mine[i].id;
        if (id >= 0 && id < kIdTableSize) atomicMin(&pos[id], (unsigned)i);
    }
    __syncthreads();
    for (int id = threadIdx.x; id < kIdTableSize; id += 256) {
        const int p = (int)pos[id];
        M.index[(size_t)m * kIdTableSize + id] = p;
        if (m == anchor) {
            M.present[id] = p >= 0 ? 1 : 0;
            if (p >= 0) {
                M.mean[3 * id] = mine[p].x; M.mean[3 * id + 1] = mine[p].y; M.mean[3 * id + 2] = mine[p].theta;
            }
        }
    }
    if (threadIdx.x == 0) {
        M.round[m] = m == anchor ? 0 : -1;
        M.T[3 * m] = 0.0; M.T[3 * m + 1] = 0.0; M.T[3 * m + 2] = 0.0;
        if (m == anchor) *M.aligned = 1;
    }
}

// sum of one value per lane over the workgroup, in a fixed tree order; every lane gets it (s: kMergeAlignT doubles of LDS)
__device__ __forceinline__ double merge_block_sum(double v, double* s) {
    __syncthreads();                   // the previous sum has been read by every lane
    s[threadIdx.x] = v;
    __syncthreads();
    for (int h = kMergeAlignT / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) s[threadIdx.x] += s[threadIdx.x + h];
        __syncthreads();
    }
    return s[0];
}

// Round `round`, one workgroup per map: a map not aligned yet that shares at least min_common ids with the table, not all on one
// point, gets T = (t, phi): phi = atan2(sum (p - pm) x (q - qm), sum (p - pm) . (q - qm)), t = qm - R(phi) pm, over the common ids
// (p: the map's positions, q: the table's, pm / qm their centroids; headings do not enter).  The table is only read here.
__global__ __launch_bounds__(kMergeAlignT) void k_merge_align(MergeBufs M, const MapRecord* __restrict__ rec, int per_map, int min_common,
                                                             int round) {
    __shared__ double s[kMergeAlignT];
    const int m = blockIdx.x;
    if (M.round[m] != -1) return;      // workgroup-uniform
    const MapRecord* mine = rec + (size_t)m * per_map;
    constexpr int kPer = kIdTableSize / kMergeAlignT;
    double px[kPer], py[kPer], qx[kPer], qy[kPer];
    bool common[kPer];
    double n = 0.0, spx = 0.0, spy = 0.0, sqx = 0.0, sqy = 0.0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const int id = threadIdx.x + kMergeAlignT * k;
        const int p = M.index[(size_t)m * kIdTableSize + id];
        common[k] = p >= 0 && M.present[id] != 0;
        px[k] = py[k] = qx[k] = qy[k] = 0.0;
        if (common[k]) {
            px[k] = mine[p].x; py[k] = mine[p].y;
            qx[k] = M.mean[3 * id]; qy[k] = M.mean[3 * id + 1];
            n += 1.0; spx += px[k]; spy += py[k]; sqx += qx[k]; sqy += qy[k];
        }
    }
    n = merge_block_sum(n, s);
    if (n < (double)min_common) return;                // workgroup-uniform: the map waits for a later round
    const double pmx = merge_block_sum(spx, s) / n, pmy = merge_block_sum(spy, s) / n;
    const double qmx = merge_block_sum(sqx, s) / n, qmy = merge_block_sum(sqy, s) / n;
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int k = 0; k < kPer; k++)
        if (common[k]) {
            const double dpx = px[k] - pmx, dpy = py[k] - pmy, dqx = qx[k] - qmx, dqy = qy[k] - qmy;
            a += dpx * dqy - dpy * dqx;
            b += dpx * dqx + dpy * dqy;
        }
    a = merge_block_sum(a, s);
    b = merge_block_sum(b, s);
    if (a == 0.0 && b == 0.0) return;                  // every common landmark on one point: no rotation to be had
    if (threadIdx.x == 0) {
        const double phi = atan2(a, b);
        const double c = cos(phi), sn = sin(phi);
        M.T[3 * m] = qmx - (c * pmx - sn * pmy);
        M.T[3 * m + 1] = qmy - (sn * pmx + c * pmy);
        M.T[3 * m + 2] = phi;
        M.round[m] = round;
        atomicAdd(M.aligned, 1);
    }
}

// a map's mean moved into the anchor frame by the map's T = (tx, ty, phi)
__device__ __forceinline__ void merge_move(const MapRecord& r, double tx, double ty, double c, double sn, double phi, double* out) {
    out[0] = c * r.x - sn * r.y + tx;
    out[1] = sn * r.x + c * r.y + ty;
    double th = r.theta + phi;
    wrap1(th);
    out[2] = th;
}

// Round `round`, one thread per id: an id the table lacks is inserted from the lowest map aligned in this round that has it
__global__ __launch_bounds__(256) void k_merge_insert(MergeBufs M, const MapRecord* __restrict__ rec, int n_maps, int per_map, int round) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= kIdTableSize || M.present[id]) return;
    for (int m = 0; m < n_maps; m++) {
        if (M.round[m] != round) continue;
        const int p = M.index[(size_t)m * kIdTableSize + id];
        if (p < 0) continue;
        const double phi = M.T[3 * m + 2];
        double v[3];
        merge_move(rec[(size_t)m * per_map + p], M.T[3 * m], M.T[3 * m + 1], cos(phi), sin(phi), phi, v);
        M.mean[3 * id] = v[0]; M.mean[3 * id + 1] = v[1]; M.mean[3 * id + 2] = v[2];
        M.present[id] = 1;
        return;
    }
}

// One thread per id, one wave per workgroup.  For an id of the table, over the aligned maps that hold it in ascending map order:
// C = (S + S^T) / 2, C' = J C J^T (J = blockdiag(R(phi), 1)), skipped unless finite with positive leading minors; Lambda = sum C'^-1,
// m = m0 + Lambda^-1 sum C'^-1 (m' - m0) around the table's mean m0, covariance Lambda^-1.  The output position of an id is the number
// of table ids below it: those of earlier workgroups counted from the flags, those of this wave from a ballot.
__global__ __launch_bounds__(kMergeFuseT) void k_merge_fuse(MergeBufs M, const MapRecord* __restrict__ rec, int n_maps, int per_map) {
    const int lane = threadIdx.x, base = blockIdx.x * kMergeFuseT, id = base + lane;
    int below = 0;
    for (int j = lane; j < base; j += kMergeFuseT) below += M.present[j] ? 1 : 0;
    for (int h = kMergeFuseT / 2; h > 0; h >>= 1) below += __shfl_xor(below, h);
    const bool have = M.present[id] != 0;
    const unsigned long long mask = __ballot(have);
    const int at = below + __popcll(mask & ((1ull << lane) - 1ull));
    if (blockIdx.x == gridDim.x - 1 && lane == 0) *M.out_n = below + __popcll(mask);
    if (!have) return;
    const double m0[3] = {M.mean[3 * id], M.mean[3 * id + 1], M.mean[3 * id + 2]};
    double Lam[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, eta[3] = {0, 0, 0};
    int seen = 0;
    for (int m = 0; m < n_maps; m++) {
        if (M.round[m] < 0) continue;
        const int p = M.index[(size_t)m * kIdTableSize + id];
        if (p < 0) continue;
        const MapRecord& r = rec[(size_t)m * per_map + p];
        const double phi = M.T[3 * m + 2], c = cos(phi), sn = sin(phi);
        double C[9], Cp[9], W[9], v[3];
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) C[3 * i + j] = 0.5 * (r.S[3 * i + j] + r.S[3 * j + i]);
        // J C J^T: A = J C (rows 0, 1 rotated), then A J^T (columns 0, 1 rotated)
        double A[9];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            A[j] = c * C[j] - sn * C[3 + j];
            A[3 + j] = sn * C[j] + c * C[3 + j];
            A[6 + j] = C[6 + j];
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            Cp[3 * i] = A[3 * i] * c - A[3 * i + 1] * sn;
            Cp[3 * i + 1] = A[3 * i] * sn + A[3 * i + 1] * c;
            Cp[3 * i + 2] = A[3 * i + 2];
        }
#pragma unroll
        for (int i = 0; i < 9; i++) ok = ok && isfinite(Cp[i]);
        const double m2 = Cp[0] * Cp[4] - Cp[1] * Cp[3];
        const double m3 = Cp[0] * (Cp[4] * Cp[8] - Cp[5] * Cp[7]) - Cp[1] * (Cp[3] * Cp[8] - Cp[5] * Cp[6]) + Cp[2] * (Cp[3] * Cp[7] - Cp[4] * Cp[6]);
        ok = ok && Cp[0] > 0.0 && m2 > 0.0 && m3 > 0.0;
        if (!ok) continue;
        merge_move(r, M.T[3 * m], M.T[3 * m + 1], c, sn, phi, v);
        double d[3] = {v[0] - m0[0], v[1] - m0[1], v[2] - m0[2]};
        wrap1(d[2]);
        inv3_reg(Cp, W);
#pragma unroll
        for (int i = 0; i < 9; i++) Lam[i] += W[i];
#pragma unroll
        for (int i = 0; i < 3; i++) eta[i] += W[3 * i] * d[0] + W[3 * i + 1] * d[1] + W[3 * i + 2] * d[2];
        seen++;
    }
    double out[3] = {m0[0], m0[1], m0[2]}, P[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (seen > 0) {
        inv3_reg(Lam, P);
#pragma unroll
        for (int i = 0; i < 3; i++) out[i] += P[3 * i] * eta[0] + P[3 * i + 1] * eta[1] + P[3 * i + 2] * eta[2];
        wrap1(out[2]);
    }
    M.out_ids[at] = id;
    M.out_seen[at] = seen;
#pragma unroll
    for (int i = 0; i < 3; i++) M.out_xyth[3 * at + i] = out[i];
#pragma unroll
    for (int i = 0; i < 9; i++) M.out_sigma[9 * at + i] = P[i];
}

// ---- host side -------------------------------------------------------------------------------------------
hipError_t merge_alloc(MergeBufs& M) {
    if (M.mem) return hipSuccess;
    MergeBufs b{};
    size_t off = 0;
    auto take = [&off](auto*& p, size_t count) {
        p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(off);
        off += (count * sizeof(*p) + 255) / 256 * 256;
    };
    take(b.index, (size_t)kMergeMaxMaps * kIdTableSize);
    take(b.present, kIdTableSize);
    take(b.mean, 3 * (size_t)kIdTableSize);
    take(b.round, kMergeMaxMaps);
    take(b.T, 3 * (size_t)kMergeMaxMaps);
    take(b.aligned, 1);
    take(b.out_n, 1);
    take(b.out_ids, kIdTableSize);
    take(b.out_seen, kIdTableSize);
    take(b.out_xyth, 3 * (size_t)kIdTableSize);
    take(b.out_sigma, 9 * (size_t)kIdTableSize);
    hipError_t e = hipMalloc(&b.mem, off);
    if (e != hipSuccess) return e;
    const size_t at = reinterpret_cast<size_t>(b.mem);
    b.index = ekf_moved(b.index, at); b.present = ekf_moved(b.present, at); b.mean = ekf_moved(b.mean, at);
    b.round = ekf_moved(b.round, at); b.T = ekf_moved(b.T, at); b.aligned = ekf_moved(b.aligned, at);
    b.out_n = ekf_moved(b.out_n, at); b.out_ids = ekf_moved(b.out_ids, at); b.out_seen = ekf_moved(b.out_seen, at);
    b.out_xyth = ekf_moved(b.out_xyth, at); b.out_sigma = ekf_moved(b.out_sigma, at);
    b.mem_bytes = off;
    b.out_bytes = off - (reinterpret_cast<size_t>(b.round) - at);
    if ((e = hipHostMalloc(reinterpret_cast<void**>(&b.h_aligned), sizeof(int), hipHostMallocDefault)) != hipSuccess ||
        (e = hipHostMalloc(reinterpret_cast<void**>(&b.h_out), b.out_bytes, hipHostMallocDefault)) != hipSuccess) {
        if (b.h_aligned) hipHostFree(b.h_aligned);
        hipFree(b.mem);
        return e;
    }
    M = b;
    return hipSuccess;
}

void merge_free(MergeBufs& M) {
    if (M.mem) hipFree(M.mem);
    if (M.rec) hipFree(M.rec);
    if (M.h_aligned) hipHostFree(M.h_aligned);
    if (M.h_out) hipHostFree(M.h_out);
    M = MergeBufs{};
}

hipError_t merge_reserve_records(MergeBufs& M, size_t count) {
    if (count <= M.rec_cap) return hipSuccess;
    if (M.rec) hipFree(M.rec);
    M.rec = nullptr;
    M.rec_cap = 0;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&M.rec), count * sizeof(MapRecord));
    if (e == hipSuccess) M.rec_cap = count;
    return e;
}

void launch_fleet_export_maps(hipStream_t st, const FleetSlam& F, MapRecord* out) {
    hipLaunchKernelGGL(k_fleet_export_maps, dim3((F.base.max_landmarks + 255) / 256, 1, F.n), dim3(256), 0, st, F.base, F.stride, out);
}

hipError_t merge_run(hipStream_t st, const MergeBufs& M, const MapRecord* rec, int n_maps, int per_map, int anchor, int min_common,
                     int* rounds) {
    hipLaunchKernelGGL(k_merge_index, dim3(n_maps), dim3(256), 0, st, M, rec, per_map, anchor);
    int aligned = 1, k = 0;
    hipError_t e;
    while (aligned < n_maps) {
        k++;
        hipLaunchKernelGGL(k_merge_align, dim3(n_maps), dim3(kMergeAlignT), 0, st, M, rec, per_map, min_common, k);
        hipLaunchKernelGGL(k_merge_insert, dim3(kIdTableSize / 256), dim3(256), 0, st, M, rec, n_maps, per_map, k);
        if ((e = hipMemcpyAsync(M.h_aligned, M.aligned, sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
        if (*M.h_aligned == aligned) break;            // a round that aligned no map: the rest stays unaligned
        aligned = *M.h_aligned;
    }
    hipLaunchKernelGGL(k_merge_fuse, dim3(kIdTableSize / kMergeFuseT), dim3(kMergeFuseT), 0, st, M, rec, n_maps, per_map);
    if (rounds) *rounds = k;
    return hipGetLastError();
}

} // namespace aslam
