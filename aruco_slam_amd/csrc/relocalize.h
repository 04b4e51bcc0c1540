// Relocalization: a pose and its covariance from ONE frame's observations against the frozen map, with no prior pose.
// Included by ekf.hip (both the gfx950 build and the CPU emulation see it).  The normative text is in include/aruco_slam_hip.h
// ("relocalization"); tests/relocalize_reference.py restates it in numpy.
//
// k_relocalize runs one 128-lane workgroup per slot of the call, one lane per observation of the slot's ObsRaw list:
//   1. every lane tests its observation (valid, id in the map, finite, r > 0) and inverts z_hat of loc_steps into a pose hypothesis,
//      which goes into LDS;
//   2. every candidate lane counts the candidates whose hypothesis lies within (tol_xy, tol_th) of its own, itself included;
//   3. the winner is the greatest (count, -position): a wave reduction, then one LDS step across the two waves; a second reduction
//      of the same shape gives the runner-up, the greatest count among the candidates that do not support the winner;
//   4. the winner's supporters form C^-1 (6 numbers, symmetric) and C^-1 d (3 numbers) in LDS; lane 0 walks them in ascending list
//      position, inverts the sum and writes the slot's result record and, with apply, the pose block of the filter it belongs to.
// Nothing but the record and that pose block is written.  No floating-point atomic, every sum in a fixed order: the same input gives
// the same bits, and a slot's record does not depend on which other slots the call carries.
#pragma once
#include "ekf.h"
#include "ekf_dev.h"

namespace aslam {

// candidate k's hypothesis against candidate j's: within tol_xy and tol_th of each other (symmetric; a candidate supports itself)
__device__ __forceinline__ bool reloc_supports(double xk, double yk, double tk, double xj, double yj, double tj, const RelocParams& p) {
    const double dx = xk - xj, dy = yk - yj;
    double dt = tk - tj;
    wrap1(dt);
    return dx * dx + dy * dy <= p.tol_xy2 && fabs(dt) <= p.tol_th;
}

// greatest key of the workgroup in every lane (two waves: shuffles, then one LDS step); s: 2 ints of LDS
__device__ __forceinline__ int reloc_block_max(int key, int* s) {
    for (int h = 32; h > 0; h >>= 1) key = max(key, __shfl_xor(key, h));
    __syncthreads();                   // the previous reduction has been read by every lane
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = key;
    __syncthreads();
    return max(s[0], s[1]);
}

__global__ __launch_bounds__(kMarkerMax) void k_relocalize(EkfState E, FleetState F, RelocParams prm, const ObsRaw* __restrict__ obs,
                                                          const unsigned* __restrict__ n_markers, int first,
                                                          const int* __restrict__ robot_of_slot, int apply, RelocRecord* __restrict__ out) {
    __shared__ double sX[kMarkerMax], sY[kMarkerMax], sT[kMarkerMax];     // the hypotheses
    __shared__ double sW[9][kMarkerMax];                                  // per supporter: C^-1 (00 01 02 11 12 22), then C^-1 d
    __shared__ unsigned long long sCand[2], sSup[2];                      // per wave: candidate lanes, supporters of the winner
    __shared__ int sKey[2];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int slot = first + blockIdx.x;
    const int nM = (int)min(n_markers[slot], (unsigned)kMarkerMax);

    // 1. candidates and their hypotheses
    ObsRaw o{};
    bool cand = false;
    double hx = 0.0, hy = 0.0, ht = 0.0, c = 1.0, s = 0.0;
    if (tid < nM) {
        o = obs[(size_t)slot * kMarkerMax + tid];
        if (o.valid && o.id >= 0 && o.id < kIdTableSize && isfinite(o.x) && isfinite(o.y) && isfinite(o.th) && isfinite(o.r[0]) &&
            isfinite(o.r[1]) && isfinite(o.r[2]) && o.r[0] > 0.0 && o.r[1] > 0.0 && o.r[2] > 0.0) {
            const int ix = E.d_id2idx[o.id];
            if (ix >= 0) {
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

    // 3. the winner: greatest count, then lowest list position; count >= 1 for a candidate, so a key of 0 means there is none
    const int key = reloc_block_max(cand ? (count << 8) | (kMarkerMax - 1 - tid) : 0, sKey);
    RelocRecord* rec = out + blockIdx.x;
    const int n_cand = __popcll(cm[0]) + __popcll(cm[1]);
    if (key == 0) {                                                       // workgroup-uniform
        if (tid == 0) {
            RelocRecord r{};
            r.status = 1; r.best = -1;
            *rec = r;
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
        }
        return;
    }

    // 4. fusion in information form around the winner's hypothesis
    if (sup) {
        // J = d(hypothesis) / d(observation), C = J diag(r) J^T (upper triangle, mirrored: exactly symmetric)
        const double J[9] = {-c, s, -(s * o.x + c * o.y), -s, -c, c * o.x - s * o.y, 0.0, 0.0, -1.0};
        double C[9], W[9];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = i; j < 3; j++)
                C[3 * i + j] = C[3 * j + i] = J[3 * i] * o.r[0] * J[3 * j] + J[3 * i + 1] * o.r[1] * J[3 * j + 1] + J[3 * i + 2] * o.r[2] * J[3 * j + 2];
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
    if (tid != 0) return;
    double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int w = 0; w < 2; w++)
        for (unsigned long long m = sSup[w]; m; m &= m - 1) {              // ascending list position
            const int k = 64 * w + __ffsll((long long)m) - 1;
#pragma unroll
            for (int i = 0; i < 9; i++) a[i] += sW[i][k];
        }
    const double Lam[9] = {a[0], a[1], a[2], a[1], a[3], a[4], a[2], a[4], a[5]};
    double P[9];
    inv3_reg(Lam, P);
    RelocRecord r{};
    r.status = 0; r.n_candidates = n_cand; r.n_inliers = n_in; r.runner_up = runner_up; r.best = best;
    r.pose[0] = bx + (P[0] * a[6] + P[1] * a[7] + P[2] * a[8]);
    r.pose[1] = by + (P[3] * a[6] + P[4] * a[7] + P[5] * a[8]);
    double th = bt + (P[6] * a[6] + P[7] * a[7] + P[8] * a[8]);
    wrap1(th);
    r.pose[2] = th;
#pragma unroll
    for (int i = 0; i < 9; i++) r.sigma[i] = P[i];
    *rec = r;
    if (!apply) return;
    if (robot_of_slot) {                                                  // a fleet robot: what aslam_fleet_set_pose writes
        const int robot = robot_of_slot[blockIdx.x];
        double* st = F.pose + (size_t)kFleetState * robot;
#pragma unroll
        for (int i = 0; i < 3; i++) st[i] = r.pose[i];
#pragma unroll
        for (int i = 0; i < 9; i++) st[3 + i] = P[i];
        F.nlast[robot] = 0;
    } else {                                                              // the single filter: mu_x and the Sigma_xx block (column-major)
#pragma unroll
        for (int i = 0; i < 3; i++) E.d_mu[i] = r.pose[i];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) E.d_sigma[(size_t)j * E.ld + i] = P[i * 3 + j];
        *E.d_nlast = 0;
    }
}

// ---- host side -------------------------------------------------------------------------------------------
hipError_t reloc_alloc(RelocBufs& B, int slots) {
    if (B.d) return hipSuccess;
    RelocBufs b{};
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&b.d), sizeof(RelocRecord) * slots);
    if (e != hipSuccess) return e;
    if ((e = hipHostMalloc(reinterpret_cast<void**>(&b.h), sizeof(RelocRecord) * slots, hipHostMallocDefault)) != hipSuccess) {
        hipFree(b.d);
        return e;
    }
    b.cap = slots;
    B = b;
    return hipSuccess;
}

void reloc_free(RelocBufs& B) {
    if (B.d) hipFree(B.d);
    if (B.h) hipHostFree(B.h);
    B = RelocBufs{};
}

void launch_relocalize(hipStream_t st, const EkfState& E, const FleetState& F, const RelocParams& prm, const ObsRaw* obs,
                       const unsigned* n_markers, int first, int count, const int* robot_of_slot, int apply, RelocRecord* out) {
    hipLaunchKernelGGL(k_relocalize, dim3(count), dim3(kMarkerMax), 0, st, E, F, prm, obs, n_markers, first, robot_of_slot, apply, out);
}

} // namespace aslam
