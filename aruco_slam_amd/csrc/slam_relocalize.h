// SLAM relocalization: a lost SLAM filter's pose from ONE frame's observations against its own, live map, with the
// covariance that follows to first order: Sigma_xx', and the pose <-> landmark strip Sigma_lx' that a pose derived from the map's
// own landmarks has with exactly those landmarks.  The inverse of the augment: there a landmark becomes a function of the pose and
// an observation, here the pose becomes a function of landmarks and observations.  Included by ekf.hip (both the gfx950 build and
// the CPU emulation see it).  The normative text is in include/aruco_slam_hip.h ("SLAM relocalization");
// tests/slam_relocalize_reference.py restates it in long double.
//
// Two launches per call on one stream, filter of slot i = the single filter, or robot robot_of_slot[i] of a SLAM fleet:
//   k_slam_reloc_solve  one 128-lane workgroup per slot, one lane per observation.  Candidates, hypotheses, consensus, winner and
//                       runner-up are phases 1-3 of k_relocalize (relocalize.h) with the filter's own id table and mu as the map; the
//                       phases are restated here because k_relocalize itself stays as it is.  The winner's supporters then form
//                       C = J R J^T + G P G^T (P: the landmark's own 3 x 3 block of Sigma), C^-1 and C^-1 d in LDS; lane 0 walks
//                       them in ascending list position, inverts Lambda and writes the record (status, counts, pose); the supporter
//                       lanes write the slot's seat table: per supporter, in list order, its landmark index and M = Lambda^-1 C^-1 G;
//                       lane 0 adds the measurement term sum A (J R J^T) A^T of Sigma_xx' and the pose.
//   k_slam_reloc_seat   grid x = tiles of kSlamRelocTile state indices, grid y = slots.  A workgroup of an unsolved slot exits at
//                       once, and so does every tile but the first without apply.  The seat table is staged in LDS (every lane reads
//                       the same entry: a broadcast); a lane owns one state index c >= 3 and accumulates Sigma_lx'(c, 0..2) =
//                       sum_j Sigma(c, l_j .. l_j + 2) M_j^T over the supporters from three loads per supporter that are coalesced
//                       across the lanes (column l_j + q of the column-major Sigma, consecutive rows), then writes Sigma(c, 0..2) and
//                       the mirror Sigma(0..2, c).  Tile 0 also forms Sigma_xx' = measurement term + sum_j M_j Sigma_lx'(l_j.., :):
//                       the strip rows it needs are recomputed by the same function, so no workgroup waits for another; it completes
//                       the record (sigma) and, with apply, writes Sigma_xx, mu_x and the last-observed length 0.
// Reads touch rows and columns >= 3 of Sigma only (Sigma_ll), writes rows and columns 0..2 only: in place without a hazard.  No
// floating-point atomic, every sum in ascending list position: the same input gives the same bits, whatever else the call carries.
#pragma once
#include "ekf.h"
#include "ekf_dev.h"
#include "ekf_fleet_slam.h"
#include "relocalize.h"

namespace aslam {

__global__ __launch_bounds__(kMarkerMax) void k_slam_reloc_solve(SlamReloc A) {
    __shared__ double sX[kMarkerMax], sY[kMarkerMax], sT[kMarkerMax];     // the hypotheses
    __shared__ double sW[9][kMarkerMax];                                  // per supporter: C^-1 (00 01 02 11 12 22), then C^-1 d; later A Cm A^T (6)
    __shared__ double sP[9];                                              // Lambda^-1
    __shared__ unsigned long long sCand[2], sSup[2];                      // per wave: candidate lanes, supporters of the winner
    __shared__ int sKey[2];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int slot = A.first + blockIdx.x;
    const EkfState E = ekf_robot_state(A.base, A.stride, A.robot_of_slot ? A.robot_of_slot[blockIdx.x] : 0);
    const RelocParams prm = A.prm;
    const int L = min(max(*E.d_L, 0), E.max_landmarks);
    const int nM = (int)min(A.n_markers[slot], (unsigned)kMarkerMax);
    RelocRecord* rec = A.out + blockIdx.x;
    SlamRelocSeat* seat = A.seat + blockIdx.x;

    // 1. candidates and their hypotheses: the map is the filter's own
    ObsRaw o{};
    bool cand = false;
    int ix = -1;
    double hx = 0.0, hy = 0.0, ht = 0.0, c = 1.0, s = 0.0;
    if (tid < nM) {
        o = A.obs[(size_t)slot * kMarkerMax + tid];
        if (o.valid && o.id >= 0 && o.id < kIdTableSize && isfinite(o.x) && isfinite(o.y) && isfinite(o.th) && isfinite(o.r[0]) &&
            isfinite(o.r[1]) && isfinite(o.r[2]) && o.r[0] > 0.0 && o.r[1] > 0.0 && o.r[2] > 0.0) {
            ix = E.d_id2idx[o.id];
            if (ix >= 0 && ix < L) {
                const double* lm = E.d_mu + 3 + 3 * ix;
                ht = lm[2] - o.th;
                wrap1(ht);
                sincos(ht, &s, &c);
                hx = lm[0] - (c * o.x - s * o.y);
                hy = lm[1] - (s * o.x + c * o.y);
                cand = true;
            }
        }
    }
    sX[tid] = hx; sY[tid] = hy; sT[tid] = ht;
    {
        const unsigned long long b = __ballot(cand);
        if ((tid & 63) == 0) sCand[wave] = b;
    }
    __syncthreads();

    // 2. consensus: the supporters of every candidate
    const unsigned long long cm[2] = {sCand[0], sCand[1]};
    int count = 0;
    if (cand)
        for (int k = 0; k < nM; k++)
            if ((cm[k >> 6] >> (k & 63)) & 1ull) count += reloc_supports(sX[k], sY[k], sT[k], hx, hy, ht, prm) ? 1 : 0;

    // 3. the winner: greatest count, then lowest list position; the runner-up among those that do not support it
    const int key = reloc_block_max(cand ? (count << 8) | (kMarkerMax - 1 - tid) : 0, sKey);
    const int n_cand = __popcll(cm[0]) + __popcll(cm[1]);
    if (key == 0) {                                                       // workgroup-uniform
        if (tid == 0) {
            RelocRecord r{};
            r.status = 1; r.best = -1;
            *rec = r;
            seat->n_sup = 0;
        }
        return;
    }
    const int best = kMarkerMax - 1 - (key & 0xFF), n_in = key >> 8;
    const double bx = sX[best], by = sY[best], bt = sT[best];
    const bool sup = cand && reloc_supports(hx, hy, ht, bx, by, bt, prm);
    const int runner_up = reloc_block_max(cand && !sup ? count : 0, sKey);
    if (n_in < prm.min_inliers) {                                         // workgroup-uniform
        if (tid == 0) {
            RelocRecord r{};
            r.status = 2; r.n_candidates = n_cand; r.n_inliers = n_in; r.runner_up = runner_up; r.best = best;
            *rec = r;
            seat->n_sup = 0;
        }
        return;
    }

    // 4. fusion weights: C = J diag(r) J^T + G P G^T per supporter (upper triangles, mirrored: exactly symmetric)
    double Cm[9] = {}, G[9] = {}, W[9] = {};
    if (sup) {
        const double J[9] = {-c, s, -(s * o.x + c * o.y), -s, -c, c * o.x - s * o.y, 0.0, 0.0, -1.0};
        G[0] = 1.0; G[1] = 0.0; G[2] = s * o.x + c * o.y;                 // d(hypothesis) / d(landmark)
        G[3] = 0.0; G[4] = 1.0; G[5] = -(c * o.x - s * o.y);
        G[6] = 0.0; G[7] = 0.0; G[8] = 1.0;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = i; j < 3; j++)
                Cm[3 * i + j] = Cm[3 * j + i] = J[3 * i] * o.r[0] * J[3 * j] + J[3 * i + 1] * o.r[1] * J[3 * j + 1] + J[3 * i + 2] * o.r[2] * J[3 * j + 2];
        const size_t ld = (size_t)E.ld, li = (size_t)(3 + 3 * ix);
        double P[9], GP[9], C[9];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = i; j < 3; j++) P[3 * i + j] = P[3 * j + i] = E.d_sigma[(li + j) * ld + li + i];   // Sigma(li + i, li + j), i <= j
        mul3(G, P, GP);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = i; j < 3; j++)
                C[3 * i + j] = C[3 * j + i] = Cm[3 * i + j] + (GP[3 * i] * G[3 * j] + GP[3 * i + 1] * G[3 * j + 1] + GP[3 * i + 2] * G[3 * j + 2]);
        inv3_reg(C, W);
        double d[3] = {hx - bx, hy - by, ht - bt};
        wrap1(d[2]);
        sW[0][tid] = W[0]; sW[1][tid] = W[1]; sW[2][tid] = W[2]; sW[3][tid] = W[4]; sW[4][tid] = W[5]; sW[5][tid] = W[8];
#pragma unroll
        for (int i = 0; i < 3; i++) sW[6 + i][tid] = W[3 * i] * d[0] + W[3 * i + 1] * d[1] + W[3 * i + 2] * d[2];
    }
    {
        const unsigned long long b = __ballot(sup);
        if ((tid & 63) == 0) sSup[wave] = b;
    }
    __syncthreads();
    const unsigned long long sm[2] = {sSup[0], sSup[1]};
    double pose[3] = {0.0, 0.0, 0.0};
    if (tid == 0) {
        double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int w = 0; w < 2; w++)
            for (unsigned long long m = sm[w]; m; m &= m - 1) {                // ascending list position
                const int k = 64 * w + __ffsll((long long)m) - 1;
#pragma unroll
                for (int i = 0; i < 9; i++) a[i] += sW[i][k];
            }
        const double Lam[9] = {a[0], a[1], a[2], a[1], a[3], a[4], a[2], a[4], a[5]};
        double Pm[9];
        inv3_reg(Lam, Pm);
        pose[0] = bx + (Pm[0] * a[6] + Pm[1] * a[7] + Pm[2] * a[8]);
        pose[1] = by + (Pm[3] * a[6] + Pm[4] * a[7] + Pm[5] * a[8]);
        pose[2] = bt + (Pm[6] * a[6] + Pm[7] * a[7] + Pm[8] * a[8]);
        wrap1(pose[2]);
#pragma unroll
        for (int i = 0; i < 9; i++) sP[i] = Pm[i];
    }
    __syncthreads();                                                          // Lambda^-1 is in; sW has been read

    // the seat table: A = Lambda^-1 C^-1 and M = A G per supporter, at its rank among the supporters (list order)
    if (sup) {
        double Pm[9], Aj[9], M[9], AC[9];
#pragma unroll
        for (int i = 0; i < 9; i++) Pm[i] = sP[i];
        mul3(Pm, W, Aj);
        mul3(Aj, G, M);
        mul3(Aj, Cm, AC);
        int q = 0;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = i; j < 3; j++) sW[q++][tid] = AC[3 * i] * Aj[3 * j] + AC[3 * i + 1] * Aj[3 * j + 1] + AC[3 * i + 2] * Aj[3 * j + 2];
        const int p = (wave ? __popcll(sm[0]) : 0) + __popcll(sm[wave] & ((1ull << (tid & 63)) - 1ull));
        seat->idx[p] = ix;
#pragma unroll
        for (int i = 0; i < 9; i++) seat->M[p][i] = M[i];
    }
    __syncthreads();
    if (tid != 0) return;
    double t[6] = {0, 0, 0, 0, 0, 0};
    for (int w = 0; w < 2; w++)
        for (unsigned long long m = sm[w]; m; m &= m - 1) {
            const int k = 64 * w + __ffsll((long long)m) - 1;
#pragma unroll
            for (int i = 0; i < 6; i++) t[i] += sW[i][k];
        }
    const double meas[9] = {t[0], t[1], t[2], t[1], t[3], t[4], t[2], t[4], t[5]};
    seat->n_sup = __popcll(sm[0]) + __popcll(sm[1]);
    seat->N = 3 + 3 * L;
#pragma unroll
    for (int i = 0; i < 3; i++) seat->m[i] = pose[i];
#pragma unroll
    for (int i = 0; i < 9; i++) seat->meas[i] = meas[i];
    RelocRecord r{};                                                          // sigma: k_slam_reloc_seat (it needs Sigma_ll B^T)
    r.status = 0; r.n_candidates = n_cand; r.n_inliers = n_in; r.runner_up = runner_up; r.best = best;
#pragma unroll
    for (int i = 0; i < 3; i++) r.pose[i] = pose[i];
    *rec = r;
}

// Sigma_lx'(c, 0..2) = sum over the supporters j, ascending, of Sigma(c, l_j + q) M_j[a][q]: the one order both uses below share
__device__ __forceinline__ void slam_reloc_strip_row(const double* __restrict__ Sg, size_t ld, int c, int n_sup, const int* sIdx,
                                                     const double* sM, double* acc) {
    acc[0] = acc[1] = acc[2] = 0.0;
#pragma unroll 4
    for (int j = 0; j < n_sup; j++) {
        const double* col = Sg + (size_t)(3 + 3 * sIdx[j]) * ld + c;
        const double v0 = col[0], v1 = col[ld], v2 = col[2 * ld];
        const double* M = sM + 9 * j;
#pragma unroll
        for (int a = 0; a < 3; a++) acc[a] += v0 * M[3 * a] + v1 * M[3 * a + 1] + v2 * M[3 * a + 2];
    }
}

__global__ __launch_bounds__(kSlamRelocTile) void k_slam_reloc_seat(SlamReloc A) {
    __shared__ int sIdx[kMarkerMax];
    __shared__ double sM[kMarkerMax * 9];                                 // the seat table's M_j
    __shared__ double sS[kMarkerMax * 9];                                 // tile 0: Sigma_lx' rows l_j .. l_j + 2 (3 x 3 per supporter)
    __shared__ double sXX[9];
    const SlamRelocSeat* __restrict__ seat = A.seat + blockIdx.y;
    const int n_sup = min(seat->n_sup, (int)kMarkerMax), tile = blockIdx.x, tid = threadIdx.x;
    if (n_sup <= 0 || (tile != 0 && !A.apply)) return;                    // unsolved, or nothing to seat (workgroup-uniform)
    const EkfState E = ekf_robot_state(A.base, A.stride, A.robot_of_slot ? A.robot_of_slot[blockIdx.y] : 0);
    const int N = min(seat->N, E.ld);
    if (tile * kSlamRelocTile >= N) return;
    for (int k = tid; k < n_sup; k += kSlamRelocTile) sIdx[k] = seat->idx[k];
    for (int k = tid; k < 9 * n_sup; k += kSlamRelocTile) sM[k] = (&seat->M[0][0])[k];
    __syncthreads();
    double* __restrict__ Sg = E.d_sigma;
    const size_t ld = (size_t)E.ld;
    if (A.apply) {
        const int c = tile * kSlamRelocTile + tid;
        if (c >= 3 && c < N) {
            double acc[3];
            slam_reloc_strip_row(Sg, ld, c, n_sup, sIdx, sM, acc);
#pragma unroll
            for (int a = 0; a < 3; a++) {
                Sg[(size_t)a * ld + c] = acc[a];                          // Sigma(c, a)
                Sg[(size_t)c * ld + a] = acc[a];                          // Sigma(a, c)
            }
        }
    }
    if (tile != 0) return;
    // Sigma_xx' = measurement term + sum_j M_j Sigma_lx'(l_j .. l_j + 2, :), upper triangle mirrored
    for (int k = tid; k < 3 * n_sup; k += kSlamRelocTile) {
        double acc[3];
        slam_reloc_strip_row(Sg, ld, 3 + 3 * sIdx[k / 3] + k % 3, n_sup, sIdx, sM, acc);
#pragma unroll
        for (int a = 0; a < 3; a++) sS[3 * k + a] = acc[a];
    }
    __syncthreads();
    if (tid < 9 && tid / 3 <= tid % 3) {
        const int i = tid / 3, j = tid % 3;
        double v = seat->meas[3 * i + j];
        for (int k = 0; k < n_sup; k++) {
            const double* M = sM + 9 * k;
            const double* S = sS + 9 * k;
            v += M[3 * i] * S[j] + M[3 * i + 1] * S[3 + j] + M[3 * i + 2] * S[6 + j];
        }
        sXX[3 * i + j] = sXX[3 * j + i] = v;
    }
    __syncthreads();
    if (tid < 9) {
        A.out[blockIdx.y].sigma[tid] = sXX[tid];
        if (A.apply) Sg[(size_t)(tid % 3) * ld + tid / 3] = sXX[tid];
    }
    if (A.apply && tid < 3) E.d_mu[tid] = seat->m[tid];
    if (A.apply && tid == 0) *E.d_nlast = 0;
}

// ---- host side -------------------------------------------------------------------------------------------
hipError_t slam_reloc_alloc(SlamRelocBufs& B, int slots) {
    if (B.seat) return hipSuccess;
    SlamRelocSeat* p = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), sizeof(SlamRelocSeat) * slots);
    if (e != hipSuccess) return e;
    B.seat = p;
    B.cap = slots;
    return hipSuccess;
}

void slam_reloc_free(SlamRelocBufs& B) {
    if (B.seat) hipFree(B.seat);
    B = SlamRelocBufs{};
}

void launch_slam_reloc_solve(hipStream_t st, const SlamReloc& A, int count) {
    hipLaunchKernelGGL(k_slam_reloc_solve, dim3(count), dim3(kMarkerMax), 0, st, A);
}

void launch_slam_reloc_seat(hipStream_t st, const SlamReloc& A, int count) {
    const int tiles = A.apply ? (A.base.ld + kSlamRelocTile - 1) / kSlamRelocTile : 1;
    hipLaunchKernelGGL(k_slam_reloc_seat, dim3(tiles, count), dim3(kSlamRelocTile), 0, st, A);
}

} // namespace aslam
