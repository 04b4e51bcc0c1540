// Localization against a frozen map: the reference's addImage update (src/aruco_slam.cpp:88-207) on a state whose
// landmark blocks are fixed, mu_l frozen, Sigma_ll = 0, Sigma_xl = 0.  With those zero blocks K = Sigma Gx^T (Gx Sigma Gx^T + R)^-1
// has zero landmark rows, so every correction reduces to the 3 x 3 pose block:
//     S = H P H^T + R,   K = P H^T S^-1,   mu_x += K ze,   P <- (I - K H) P          (H = pose part of Gxm, P = Sigma_xx)
// and the landmark rows of mu / Sigma are never written.  Included by ekf.hip (both the gfx950 build and the CPU emulation see it).
//
// k_loc_steps runs the EKF steps of slots [first, first + count) in ONE launch of one workgroup (128 lanes = one per observation):
// per slot the lanes load the observations, look up the landmark index (unknown ids and gated observations are dropped before the
// queue), rank the pop order, test "stationary" against the previous step's list and prepare every correction's H, ze and R; lane 0
// keeps mu_x and P in registers across all slots and runs the predict and the dependent chain of 3 x 3 corrections.
//
// The body is loc_steps<Src>: Src says which slots the workgroup steps through and where the filter it corrects lives.  LocSingle
// is the context's one filter (k_loc_steps); a fleet's workgroup uses LocFleet, its robot's own filter (ekf_fleet.h).
// k_loc_steps<G, M, C> and k_fleet_steps<G, M, C> are kernel templates on the three policies below, one instantiation per combination a
// launch can ask for; with_loc_policies picks it and launch_steps_kernel launches it, for both.
//
// loc_steps<Src, G> takes a compile-time gate policy G (include/aruco_slam_hip.h).  NoGate, the default, is the
// chain above and nothing else: every gated statement sits under `if constexpr (G::kOn)`.  Gated (k_loc_steps<Gated, ..>,
// k_fleet_steps<Gated, ..>) adds on lane 0, per correction, d2 = ze^T S^-1 ze, the reference's logged test (aruco_slam.cpp:156), the
// skip of a correction whose d2 exceeds a finite gate, the slot's health sums in pop order and the filter's track record, which
// stays in registers across the slots of a launch; a rejected flag per popped observation lives in LDS, and after the chain all
// lanes compact the last-observed list with two ballots so that it holds the accepted updates and the no-ops only.
//
// loc_steps<Src, G, M> takes a compile-time map policy M (include/aruco_slam_hip.h).  FixedMap, the default, is the
// filter above: every new statement sits under `if constexpr (M::kOn)`.  UncertainMap (k_loc_steps<.., UncertainMap, ..>,
// k_fleet_steps<.., UncertainMap, ..>) is the Schmidt-Kalman filter on a map whose landmarks carry fixed covariance blocks C_i: the strip
// X = [Sigma_xx | Sigma_xl] replaces P.  Sigma_xl (3 x 3L) lives in dynamic LDS for the whole launch (Src says where it is loaded
// from and stored to), Sigma_xx stays in lane 0's registers.  The front half of the slot body is shared; per correction lane 0 forms
// S, K and the decision from the six columns it needs (pose block and block i), updates those six itself and publishes K and the
// fuse flag; behind one barrier every lane subtracts K (Hx X[:, j]) from its own columns, behind a second one the chain goes on.  A
// rejected correction costs the first barrier only.
//
// loc_steps<Src, G, M, C> takes a compile-time innovation policy C (include/aruco_slam_hip.h).  FrozenMean, the
// default, is the reference's chain (quirk Q1): every correction adds K ze with ze formed at the frame's predicted mean.
// RunningMean (k_loc_steps<.., RunningMean>, k_fleet_steps<.., RunningMean>) corrects from the mean the previous
// correction left: lane 0 forms e = ze - H (mu_x - sPose), a plain difference with no angle wrap, where H is the pose part of the
// Jacobian (on an uncertain map the landmarks are not estimated), judges the correction by e and adds K e.  S, K, the covariance
// update and ref_flagged (the reference's logged test on ze) are untouched.  Every new statement sits under `if constexpr (C::kOn)`.
#pragma once
#include "common.h"
#include "ekf.h"
#include "ekf_dev.h"

namespace aslam {

struct LocCorr {                     // one prepared correction: H (row-major 3 x 3), innovation, diag R
    double H[9];
    double ze[3];
    double r[3];
};

// the context's filter: slots first .. first + count - 1, pose in mu / Sigma, last_observed_marker_ in d_last; it also leaves the last
// slot's popped observations for aslam_get_observations
struct LocSingle {
    const EkfState& E;
    int first, count, predict_first;
    static constexpr bool kPopList = true;
    __device__ __forceinline__ int track() const { return kTrackSingle; }
    __device__ __forceinline__ int n() const { return count; }
    __device__ __forceinline__ int slot(int k) const { return first + k; }
    __device__ __forceinline__ bool predict(int k) const { return k > 0 || predict_first; }
    __device__ __forceinline__ void load(double& mx, double& my, double& mt, double* P) const {
        mx = E.d_mu[0]; my = E.d_mu[1]; mt = E.d_mu[2];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) P[i * 3 + j] = E.d_sigma[(size_t)j * E.ld + i];
    }
    __device__ __forceinline__ void store(double mx, double my, double mt, const double* P) const {
        E.d_mu[0] = mx; E.d_mu[1] = my; E.d_mu[2] = mt;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) E.d_sigma[(size_t)j * E.ld + i] = P[i * 3 + j];
    }
    __device__ __forceinline__ LastObs* last() const { return E.d_last; }
    __device__ __forceinline__ int* nlast() const { return E.d_nlast; }
    // uncertain map: the strip's landmark columns, 3 x W row-major in sX (LDS) <-> rows 0..2 of Sigma, mirrored into columns 0..2
    template <class M> __device__ __forceinline__ void load_cross(const M& um, double* sX) const {
        const int W = 3 * um.m.L;
        for (int j = threadIdx.x; j < W; j += kMarkerMax)
#pragma unroll
            for (int i = 0; i < 3; i++) sX[i * W + j] = E.d_sigma[(size_t)(3 + j) * E.ld + i];
    }
    template <class M> __device__ __forceinline__ void store_cross(const M& um, const double* sX) const {
        const int W = 3 * um.m.L;
        for (int j = threadIdx.x; j < W; j += kMarkerMax)
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const double v = sX[i * W + j];
                E.d_sigma[(size_t)(3 + j) * E.ld + i] = v;
                E.d_sigma[(size_t)i * E.ld + 3 + j] = v;
            }
    }
};

struct NoGate { static constexpr bool kOn = false; };
struct Gated {
    static constexpr bool kOn = true;
    GateState g;
};
struct FixedMap { static constexpr bool kOn = false; };
struct UncertainMap {
    static constexpr bool kOn = true;
    MapCov m;
};

template <class Src, class G = NoGate, class M = FixedMap, class C = FrozenMean>
__device__ __forceinline__ void loc_steps(const Src& src, const EkfState& E, const SlamParams& sp, const ObsRaw* obs, const unsigned* n_markers,
                                          const double* enc, const G& gate = G{}, const M& umap = M{}) {
    __shared__ LastObs sLast[kMarkerMax];       // last_observed_marker_ of the previous step
    __shared__ int sIndex[kMarkerMax];          // landmark index per observation slot (-2: dropped)
    __shared__ int sOrder[kMarkerMax];          // pop order
    __shared__ int sHeap[kMarkerMax];
    __shared__ LocCorr sCorr[kMarkerMax];       // the step's corrections in pop order
    __shared__ double sPose[3];                 // frame-start pose (after the predict)
    __shared__ int sDup, sNl, sCnt[2], sUpdCnt[2], sStatCnt[2];
    const int tid = threadIdx.x;
    const int count = src.n();
    int* sCorrPop = nullptr;                    // gated: pop position of every correction, rejected flag of every popped observation
    int* sRej = nullptr;
    int* sKeepCnt = nullptr;
    if constexpr (G::kOn) {
        __shared__ int sGateCorrPop[kMarkerMax], sGateRej[kMarkerMax], sGateKeepCnt[2];
        sCorrPop = sGateCorrPop; sRej = sGateRej; sKeepCnt = sGateKeepCnt;
    }
    // uncertain map: Sigma_xl (3 x W row-major, W = 3 L) for the whole launch, every prepared correction's C_i and landmark block,
    // and lane 0's verdict per correction (gain and fuse flag, two copies used alternately)
    double* sX = nullptr;
    double* sMapC = nullptr;
    double* sGain = nullptr;
    double* sPred = nullptr;
    int* sBlock = nullptr;
    int* sFuse = nullptr;
    int W = 0;
    if constexpr (M::kOn) {
        ASLAM_DYN_LDS(umap_lds);
        __shared__ double sUmapC[kMarkerMax * 9], sUmapGain[2 * 9], sUmapPred[2];
        __shared__ int sUmapBlock[kMarkerMax], sUmapFuse[2];
        sX = reinterpret_cast<double*>(umap_lds);
        sMapC = sUmapC; sGain = sUmapGain; sPred = sUmapPred; sBlock = sUmapBlock; sFuse = sUmapFuse;
        W = 3 * umap.m.L;
        src.load_cross(umap, sX);
    }

    double mx = 0, my = 0, mt = 0, P[9];        // lane 0: the pose and Sigma_xx, in registers for the whole launch
    int trFrames = 0, trAcc = 0, trRej = 0, trStreak = 0, trLost = 0;   // gated, lane 0: the filter's track record, likewise
    if (tid == 0) {
        src.load(mx, my, mt, P);
        sNl = min(*src.nlast(), kMarkerMax);
        if constexpr (G::kOn) {
            const TrackHealth* t = gate.g.track + src.track();
            trFrames = t->frames; trAcc = t->accepted_total; trRej = t->rejected_total; trStreak = t->bad_streak;
        }
    }
    sLast[tid] = src.last()[tid];               // entries beyond the list length are never read
    __syncthreads();

    for (int k = 0; k < count; k++) {
        const int slot = src.slot(k);
        const int nM = (int)min(n_markers[slot], (unsigned)kMarkerMax);
        // checkLandmark (aruco_slam.cpp:423-435): an id outside the map is dropped like a gated observation (never augmented)
        ObsRaw o{};
        int myIndex = -2;
        if (tid < nM) {
            o = obs[(size_t)slot * kMarkerMax + tid];
            if (o.valid && o.id >= 0 && o.id < kIdTableSize) {
                const int ix = E.d_id2idx[o.id];
                if (ix >= 0) myIndex = ix;
            }
        }
        sIndex[tid] = myIndex;
        if (tid == 0) {
            sDup = 0;
            if (src.predict(k)) {
                // addEncoder (aruco_slam.cpp:35-73) on the pose block, the arithmetic of predict_block (ekf.hip) in the same order:
                // with Sigma_xl = 0 the landmark rows and columns stay zero
                const double* e = enc + (size_t)3 * slot;
                const double wl = e[0], wr = e[1], dt = e[2];
                double delta_enl = dt * wl, delta_enr = dt * wr;
                double delta_sl = sp.kl * delta_enl, delta_sr = sp.kr * delta_enr;
                double l_ = 2 * sp.b;
                double delta_theta = (delta_sr - delta_sl) / l_;
                double delta_s = 0.5 * (delta_sr + delta_sl);
                double tmp_th = mt + 0.5 * delta_theta;
                double c, s;
                sincos(tmp_th, &s, &c);
                double th = mt + delta_theta;
                wrap1(th);
                const double Hp[9] = {1.0, 0.0, -delta_s * s, 0.0, 1.0, delta_s * c, 0.0, 0.0, 1.0};
                mx = mx + delta_s * c; my = my + delta_s * s; mt = th;
                const double f = 0.5 * sp.kl * dt;                       // kl for BOTH wheels (quirk Q7)
                double wkh[6] = {f * c, f * c, f * s, f * s, f * (1 / sp.b), f * (-1 / sp.b)};
                double su0 = sp.Q_k * fabs(wl), su1 = sp.Q_k * fabs(wr);
                double Q[9], T[9];
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < 3; j++) Q[i * 3 + j] = wkh[i * 2] * su0 * wkh[j * 2] + wkh[i * 2 + 1] * su1 * wkh[j * 2 + 1];
                for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) T[i * 3 + j] = Hp[i * 3] * P[j] + Hp[i * 3 + 1] * P[3 + j] + Hp[i * 3 + 2] * P[6 + j];
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < 3; j++)
                        P[i * 3 + j] = (T[i * 3] * Hp[j * 3] + T[i * 3 + 1] * Hp[j * 3 + 1] + T[i * 3 + 2] * Hp[j * 3 + 2]) + Q[i * 3 + j];
                if constexpr (M::kOn) { sPred[0] = Hp[2]; sPred[1] = Hp[5]; }
            }
            sPose[0] = mx; sPose[1] = my; sPose[2] = mt;
        }
        {
            const unsigned long long b = __ballot(myIndex >= 0);
            if ((tid & 63) == 0) sCnt[tid >> 6] = __popcll(b);
        }
        __syncthreads();
        if constexpr (M::kOn) {
            // Sigma_xl <- D Sigma_xl, every lane its own columns: D = Hp differs from I in (0,2) and (1,2) only
            if (src.predict(k)) {
                const double d0 = sPred[0], d1 = sPred[1];
                for (int j = tid; j < W; j += kMarkerMax) {
                    const double x2 = sX[2 * W + j];
                    sX[j] = sX[j] + d0 * x2;
                    sX[W + j] = sX[W + j] + d1 * x2;
                }
            }
        }
        // pop order: every key is a landmark index >= 0, so unless one id was detected twice it is ascending index -> rank in parallel
        if (myIndex >= 0) {
            int rank = 0;
            for (int j = 0; j < nM; j++) {
                const int kj = sIndex[j];
                rank += (kj >= 0 && kj < myIndex);
                if (j != tid && kj == myIndex) sDup = 1;
            }
            sOrder[rank] = tid;
        }
        __syncthreads();
        if (tid == 0 && sDup) {
            // one id twice: libstdc++ push_heap / pop_heap on the same keys (k_ekf_plan, oracle/ekf_literal.py::_Heap)
            int len = 0;
            for (int i = 0; i < nM; i++) {
                if (sIndex[i] < 0) continue;
                int hole = len++, value = i;
                int parent = (hole - 1) / 2;
                while (hole > 0 && sIndex[sHeap[parent]] > sIndex[value]) {
                    sHeap[hole] = sHeap[parent];
                    hole = parent;
                    parent = (hole - 1) / 2;
                }
                sHeap[hole] = value;
            }
            int np = 0;
            while (len > 0) {
                sOrder[np++] = sHeap[0];
                if (len > 1) {
                    int value = sHeap[len - 1];
                    sHeap[len - 1] = sHeap[0];
                    int n = len - 1, hole = 0, second = 0;
                    while (second < (n - 1) / 2) {
                        second = 2 * (second + 1);
                        if (sIndex[sHeap[second]] > sIndex[sHeap[second - 1]]) second--;
                        sHeap[hole] = sHeap[second];
                        hole = second;
                    }
                    if ((n & 1) == 0 && second == (n - 2) / 2) {
                        second = 2 * (second + 1);
                        sHeap[hole] = sHeap[second - 1];
                        hole = second - 1;
                    }
                    int parent = (hole - 1) / 2;
                    while (hole > 0 && sIndex[sHeap[parent]] > sIndex[value]) {
                        sHeap[hole] = sHeap[parent];
                        hole = parent;
                        parent = (hole - 1) / 2;
                    }
                    sHeap[hole] = value;
                }
                len--;
            }
        }
        __syncthreads();
        const int np = sCnt[0] + sCnt[1];
        const int nl = sNl;
        // popped observation q = tid: "stationary" test against the previous step's list (aruco_slam.cpp:192-198), then the
        // correction's operands from the frame-start pose (aruco_slam.cpp:116-143)
        ObsRaw po{};
        int pidx = -1, act = 0;
        double pl[3] = {0, 0, 0};
        if (tid < np) {
            const int det = sOrder[tid];
            pidx = sIndex[det];
            po = obs[(size_t)slot * kMarkerMax + det];
            bool stationary = false;
            for (int j = 0; j < nl; j++)
                if (sLast[j].id == po.id) {                              // std::find: first with the same id
                    double d0 = sLast[j].z[0] - po.x, d1 = sLast[j].z[1] - po.y, d2 = sLast[j].z[2] - po.th;
                    stationary = sqrt(d0 * d0 + d1 * d1 + d2 * d2) < 0.01;   // NaN compares false (Q2/Q3)
                    break;
                }
            act = stationary ? 2 : 1;
            const double* lm = E.d_mu + 3 + 3 * pidx;
            pl[0] = lm[0]; pl[1] = lm[1]; pl[2] = lm[2];
            PopRec pr;
            pr.id = po.id; pr.index = pidx; pr.action = act; pr.det = det;
            pr.z[0] = po.x; pr.z[1] = po.y; pr.z[2] = po.th;
            pr.r[0] = po.r[0]; pr.r[1] = po.r[1]; pr.r[2] = po.r[2];
            if (Src::kPopList && k == count - 1) E.d_pop[tid] = pr;
        }
        const unsigned long long bU = __ballot(act == 1), bS = __ballot(act == 2);
        if ((tid & 63) == 0) { sUpdCnt[tid >> 6] = __popcll(bU); sStatCnt[tid >> 6] = __popcll(bS); }
        __syncthreads();                                                 // every lane finished reading sLast / sOrder
        const int m = sUpdCnt[0] + sUpdCnt[1];
        if (act == 1) {
            const int up = (tid >= 64 ? sUpdCnt[0] : 0) + __popcll(bU & ((1ull << (tid & 63)) - 1ull));
            const double x = sPose[0], y = sPose[1], theta = sPose[2];
            double sintheta, costheta;
            sincos(theta, &sintheta, &costheta);
            double gdx = pl[0] - x, gdy = pl[1] - y, gdth = pl[2] - theta;
            wrap1(gdth);
            const double zh0 = gdx * costheta + gdy * sintheta, zh1 = -gdx * sintheta + gdy * costheta;
            LocCorr cr;
            cr.ze[0] = po.x - zh0; cr.ze[1] = po.y - zh1; cr.ze[2] = po.th - gdth;
            wrap1(cr.ze[2]);
            cr.H[0] = -costheta; cr.H[1] = -sintheta; cr.H[2] = -gdx * sintheta + gdy * costheta;
            cr.H[3] = sintheta;  cr.H[4] = -costheta; cr.H[5] = -gdx * costheta - gdy * sintheta;
            cr.H[6] = 0.0;       cr.H[7] = 0.0;       cr.H[8] = -1.0;
            cr.r[0] = po.r[0]; cr.r[1] = po.r[1]; cr.r[2] = po.r[2];
            sCorr[up] = cr;
            if constexpr (G::kOn) sCorrPop[up] = tid;
            if constexpr (M::kOn) {                                      // its landmark's block and C_i: loaded off the chain
                sBlock[up] = 3 * pidx;
                const double* cg = umap.m.C + (size_t)9 * pidx;
#pragma unroll
                for (int i = 0; i < 9; i++) sMapC[9 * up + i] = cg[i];
            }
        }
        // last_observed_marker_ = observed_marker (aruco_slam.cpp:263); last_observation_ is set in the update branch only
        if (tid < np) {
            LastObs lo;
            lo.id = po.id; lo.pad = 0;
            if (act == 1) { lo.z[0] = po.x; lo.z[1] = po.y; lo.z[2] = po.th; }
            else { lo.z[0] = lo.z[1] = lo.z[2] = nan(""); }
            sLast[tid] = lo;
            if constexpr (G::kOn) sRej[tid] = 0;
        }
        __syncthreads();
        if (tid == 0 || M::kOn) {                                        // uncertain map: every lane walks the chain, lane 0 decides
            // gated: the slot's health record, summed in pop order
            int hAcc = 0, hRej = 0, hFlag = 0, hWorst = -1;
            bool hHave = false;
            double hNis = 0.0, hMax = 0.0;
            // the dependent chain: m sequential corrections of the pose block (aruco_slam.cpp:145-205 with zero landmark blocks)
            for (int q = 0; q < m; q++) {
                const LocCorr& cr = sCorr[q];
                if (!M::kOn || tid == 0) {
                    double H[9], HP[9], PHt[9], S[9], Si[9], K[9], A[9], Pn[9];
#pragma unroll
                    for (int i = 0; i < 9; i++) H[i] = cr.H[i];
                    if constexpr (M::kOn) {
                        // Schmidt-Kalman: cst = Gxm Sigma on the pose columns (HP) and on block i (A), Gxm = [Hx | Hl at block i];
                        // Hl = [[c, s, 0], [-s, c, 0], [0, 0, 1]] is Hx's rotation part negated
                        const double Hl[9] = {-H[0], -H[1], 0.0, -H[3], -H[4], 0.0, 0.0, 0.0, 1.0};
                        const double* Ci = sMapC + 9 * q;
                        const double* Xb = sX + sBlock[q];
                        double B[9];
#pragma unroll
                        for (int i = 0; i < 3; i++)
#pragma unroll
                            for (int j = 0; j < 3; j++) B[i * 3 + j] = Xb[i * W + j];
#pragma unroll
                        for (int i = 0; i < 3; i++)
#pragma unroll
                            for (int j = 0; j < 3; j++) {
                                HP[i * 3 + j] = (H[i * 3] * P[j] + H[i * 3 + 1] * P[3 + j] + H[i * 3 + 2] * P[6 + j]) +
                                                (Hl[i * 3] * B[j * 3] + Hl[i * 3 + 1] * B[j * 3 + 1] + Hl[i * 3 + 2] * B[j * 3 + 2]);
                                A[i * 3 + j] = (H[i * 3] * B[j] + H[i * 3 + 1] * B[3 + j] + H[i * 3 + 2] * B[6 + j]) +
                                               (Hl[i * 3] * Ci[j] + Hl[i * 3 + 1] * Ci[3 + j] + Hl[i * 3 + 2] * Ci[6 + j]);
                            }
#pragma unroll
                        for (int i = 0; i < 3; i++)
#pragma unroll
                            for (int j = 0; j < 3; j++) {
                                PHt[i * 3 + j] = HP[j * 3 + i];                  // (cst's pose columns)^T
                                S[i * 3 + j] = (HP[i * 3] * H[j * 3] + HP[i * 3 + 1] * H[j * 3 + 1] + HP[i * 3 + 2] * H[j * 3 + 2]) +
                                               (A[i * 3] * Hl[j * 3] + A[i * 3 + 1] * Hl[j * 3 + 1] + A[i * 3 + 2] * Hl[j * 3 + 2]) +
                                               (i == j ? cr.r[i] : 0.0);
                            }
                    } else {
                        mul3(H, P, HP);                                          // H P
#pragma unroll
                        for (int i = 0; i < 3; i++)
#pragma unroll
                            for (int j = 0; j < 3; j++) {
                                PHt[i * 3 + j] = P[i * 3] * H[j * 3] + P[i * 3 + 1] * H[j * 3 + 1] + P[i * 3 + 2] * H[j * 3 + 2];   // P H^T
                                S[i * 3 + j] = HP[i * 3] * H[j * 3] + HP[i * 3 + 1] * H[j * 3 + 1] + HP[i * 3 + 2] * H[j * 3 + 2]       // H P H^T
                                               + (i == j ? cr.r[i] : 0.0);
                            }
                    }
                    inv3_reg(S, Si);
                    mul3(PHt, Si, K);                                        // K_x = P H^T S^-1
                    // the innovation the correction is judged by and applied with: ze, or e = ze - H (mu_x - mu_0) at the running mean
                    [[maybe_unused]] double e0, e1, e2;
                    if constexpr (C::kOn) {
                        const double dx = mx - sPose[0], dy = my - sPose[1], dth = mt - sPose[2];
                        e0 = cr.ze[0] - (H[0] * dx + H[1] * dy + H[2] * dth);
                        e1 = cr.ze[1] - (H[3] * dx + H[4] * dy + H[5] * dth);
                        e2 = cr.ze[2] - (H[6] * dx + H[7] * dy + H[8] * dth);
                    }
                    bool fuse = true;
                    if constexpr (G::kOn) {
                        const double z0 = C::kOn ? e0 : cr.ze[0], z1 = C::kOn ? e1 : cr.ze[1], z2 = C::kOn ? e2 : cr.ze[2];
                        const double d2 = z0 * (Si[0] * z0 + Si[1] * z1 + Si[2] * z2) + z1 * (Si[3] * z0 + Si[4] * z1 + Si[5] * z2) +
                                          z2 * (Si[6] * z0 + Si[7] * z1 + Si[8] * z2);            // ze^T S^-1 ze
                        double kk = 0.0;
#pragma unroll
                        for (int i = 0; i < 9; i++) kk += K[i] * K[i];
                        if constexpr (C::kOn)                                    // the reference's logged test stays on ze
                            hFlag += (sqrt(cr.ze[0] * cr.ze[0] + cr.ze[1] * cr.ze[1] + cr.ze[2] * cr.ze[2]) >= 1.0 || sqrt(kk) >= 10.0) ? 1 : 0;
                        else
                            hFlag += (sqrt(z0 * z0 + z1 * z1 + z2 * z2) >= 1.0 || sqrt(kk) >= 10.0) ? 1 : 0;   // aruco_slam.cpp:156
                        const int pop = sCorrPop[q];
                        if (d2 == d2 && (!hHave || d2 > hMax)) { hHave = true; hMax = d2; hWorst = sLast[pop].id; }
                        if (gate.g.gate_d2 < HUGE_VAL && !(d2 <= gate.g.gate_d2)) {       // a NaN d2 rejects
                            fuse = false;
                            hRej++;
                            sRej[pop] = 1;
                        } else {
                            hAcc++;
                            hNis += d2;
                        }
                    }
                    if (fuse) {
                        if constexpr (C::kOn) {
                            mx += K[0] * e0 + K[1] * e1 + K[2] * e2;
                            my += K[3] * e0 + K[4] * e1 + K[5] * e2;
                            mt += K[6] * e0 + K[7] * e1 + K[8] * e2;
                        } else {
                            mx += K[0] * cr.ze[0] + K[1] * cr.ze[1] + K[2] * cr.ze[2];
                            my += K[3] * cr.ze[0] + K[4] * cr.ze[1] + K[5] * cr.ze[2];
                            mt += K[6] * cr.ze[0] + K[7] * cr.ze[1] + K[8] * cr.ze[2];
                        }
                        if constexpr (M::kOn) {
                            // X <- X - K cst on the six columns lane 0 holds: Sigma_xx in registers, block i in place (no other
                            // lane reads or writes block i's columns during this correction)
                            double* Xw = sX + sBlock[q];
#pragma unroll
                            for (int i = 0; i < 3; i++)
#pragma unroll
                                for (int j = 0; j < 3; j++) {
                                    P[i * 3 + j] = P[i * 3 + j] - (K[i * 3] * HP[j] + K[i * 3 + 1] * HP[3 + j] + K[i * 3 + 2] * HP[6 + j]);
                                    Xw[i * W + j] = Xw[i * W + j] - (K[i * 3] * A[j] + K[i * 3 + 1] * A[3 + j] + K[i * 3 + 2] * A[6 + j]);
                                }
#pragma unroll
                            for (int i = 0; i < 9; i++) sGain[9 * (q & 1) + i] = K[i];
                        } else {
                            mul3(K, H, A);                                       // I - K H
#pragma unroll
                            for (int i = 0; i < 9; i++) A[i] = ((i % 4) == 0 ? 1.0 : 0.0) - A[i];
                            mul3(A, P, Pn);
#pragma unroll
                            for (int i = 0; i < 9; i++) P[i] = Pn[i];
                        }
                    }
                    if constexpr (M::kOn) sFuse[q & 1] = fuse ? 1 : 0;
                }
                if constexpr (M::kOn) {
                    // the strip pass of a fused correction: X[:, j] -= K (Hx X[:, j]) on every landmark column outside block i.
                    // A rejected correction costs the one barrier and no pass.
                    __syncthreads();                                         // lane 0's verdict is out
                    if (sFuse[q & 1]) {
                        double K[9], H[9];
#pragma unroll
                        for (int i = 0; i < 9; i++) { K[i] = sGain[9 * (q & 1) + i]; H[i] = cr.H[i]; }
                        const int b = sBlock[q];
                        for (int j = tid; j < W; j += kMarkerMax) {
                            if (j >= b && j < b + 3) continue;
                            const double x0 = sX[j], x1 = sX[W + j], x2 = sX[2 * W + j];
                            const double c0 = H[0] * x0 + H[1] * x1 + H[2] * x2, c1 = H[3] * x0 + H[4] * x1 + H[5] * x2,
                                         c2 = H[6] * x0 + H[7] * x1 + H[8] * x2;
                            sX[j] = x0 - (K[0] * c0 + K[1] * c1 + K[2] * c2);
                            sX[W + j] = x1 - (K[3] * c0 + K[4] * c1 + K[5] * c2);
                            sX[2 * W + j] = x2 - (K[6] * c0 + K[7] * c1 + K[8] * c2);
                        }
                        __syncthreads();                                     // the strip is whole again before lane 0 reads the next block
                    }
                }
            }
            if (!M::kOn || tid == 0) {
                const int fused = G::kOn ? hAcc : m;
                if constexpr (!G::kOn) sNl = np;
                if (slot < E.max_slots) {                                    // detections, appended (never), corrections, no-ops
                    int* st = E.d_slot_stat + 4 * slot;
                    st[0] = nM; st[1] = 0; st[2] = fused; st[3] = sStatCnt[0] + sStatCnt[1];
                }
                if (Src::kPopList && k == count - 1) { *E.d_npop = np; *E.d_m = fused; }
                if constexpr (G::kOn) {
                    if (slot < E.max_slots) {
                        SlotHealth* h = gate.g.slot + slot;
                        h->attempted = m; h->accepted = hAcc; h->rejected = hRej; h->ref_flagged = hFlag;
                        h->nis_sum = hNis; h->d2_max = hMax; h->worst_id = hWorst; h->pad = 0;
                    }
                    trFrames++;
                    trAcc += hAcc;
                    trRej += hRej;
                    if (m >= gate.g.min_attempted) trStreak = 100 * hAcc < gate.g.min_accept_percent * m ? trStreak + 1 : 0;
                    trLost = trStreak >= gate.g.lost_after ? 1 : 0;
                }
            }
        }
        if constexpr (G::kOn) {
            // the rejected observations leave the list (the reference's commented-out `continue` before aruco_slam.cpp:261): the kept
            // entries move up in pop order, placed by the two-wave prefix that places sCorr[up]
            __syncthreads();                                             // lane 0's chain wrote sRej
            int loId = 0;
            double lz0 = 0.0, lz1 = 0.0, lz2 = 0.0;
            bool keep = false, rej = false;
            if (tid < np) {
                rej = sRej[tid] != 0;
                keep = !rej;
                loId = sLast[tid].id; lz0 = sLast[tid].z[0]; lz1 = sLast[tid].z[1]; lz2 = sLast[tid].z[2];
            }
            const unsigned long long bK = __ballot(keep);
            if ((tid & 63) == 0) sKeepCnt[tid >> 6] = __popcll(bK);
            if (Src::kPopList && k == count - 1 && rej) E.d_pop[tid].action = 3;
            __syncthreads();                                             // every lane holds its entry
            if (keep) {
                LastObs& lo = sLast[(tid >= 64 ? sKeepCnt[0] : 0) + __popcll(bK & ((1ull << (tid & 63)) - 1ull))];
                lo.id = loId; lo.pad = 0; lo.z[0] = lz0; lo.z[1] = lz1; lo.z[2] = lz2;
            }
            if (tid == 0) sNl = sKeepCnt[0] + sKeepCnt[1];
        }
        __syncthreads();
    }
    if (tid < sNl) src.last()[tid] = sLast[tid];
    if constexpr (M::kOn) src.store_cross(umap, sX);
    if (tid == 0) {
        *src.nlast() = sNl;
        src.store(mx, my, mt, P);
        if constexpr (G::kOn) {
            TrackHealth* t = gate.g.track + src.track();
            t->frames = trFrames; t->accepted_total = trAcc; t->rejected_total = trRej; t->bad_streak = trStreak; t->lost = trLost;
            t->pad[0] = t->pad[1] = t->pad[2] = 0;
        }
    }
}

// What a step kernel takes behind its own arguments: its three policies as the bases of one struct, as Solve<Src, G, C> does for the
// SLAM solves (ekf_slam_gate.h).  Empty bases take no room, so GateState and MapCov lie where two arguments of their own would.
// The kernels hand loc_steps copies of the bases, G(p) and M(p): the payloads are then read at the kernel's top, as arguments of their
// own are (with references into p the compiler orders the first scalar loads of the fleet's uncertain-map kernels differently).
template <class G, class M, class C> struct LocPolicy : G, M, C {};

// the single filter's kernel, one instantiation per combination of policies (DESIGN.md §35 lists them); on an uncertain map Sigma_xl
// is in dynamic LDS, 24 * 3 L bytes
template <class G, class M, class C>
__global__ __launch_bounds__(kMarkerMax) void k_loc_steps(EkfState E, SlamParams sp, const ObsRaw* __restrict__ obs,
                                                         const unsigned* __restrict__ n_markers, const double* __restrict__ enc,
                                                         int first, int count, int predict_first, LocPolicy<G, M, C> p) {
    loc_steps<LocSingle, G, M, C>(LocSingle{E, first, count, predict_first}, E, sp, obs, n_markers, enc, G(p), M(p));
}

// Sigma_xl := 0 of the single filter (rows 0..2 and their mirror in columns 0..2): what a seat of its pose does on an uncertain map
__global__ void k_umap_clear_cross(EkfState E, int L) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= 3 * L) return;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        E.d_sigma[(size_t)(3 + j) * E.ld + i] = 0.0;
        E.d_sigma[(size_t)i * E.ld + 3 + j] = 0.0;
    }
}

void launch_umap_clear_cross(hipStream_t st, const EkfState& E, int L) {
    hipLaunchKernelGGL(k_umap_clear_cross, dim3((3 * L + 255) / 256), dim3(256), 0, st, E, L);
}

// what a launch asks for -> the policies of its kernel instantiation: f(G, M, C) gets the three policy objects, filled in
template <class F> void with_loc_policies(const GateState* gate, const MapCov* umap, bool consistent, F&& f) {
    auto innovation = [&](auto g, auto m) { consistent ? f(g, m, RunningMean{}) : f(g, m, FrozenMean{}); };
    auto map = [&](auto g) { umap ? innovation(g, UncertainMap{*umap}) : innovation(g, FixedMap{}); };
    gate ? map(Gated{*gate}) : map(NoGate{});
}

// one launch of the step kernel Kernel (k_loc_steps<G, M, C> or k_fleet_steps<G, M, C>) with n_groups workgroups: a... are the kernel's
// own arguments, the policies follow them.  Dynamic LDS of an uncertain-map kernel: the strip's landmark columns; above 64 KB a kernel
// has to be told once, and Kernel being a template argument makes `allowed` one flag per kernel, not one per signature.
inline size_t umap_lds_bytes(int L) { return sizeof(double) * 9 * (size_t)L; }
template <auto Kernel, class G, class M, class C, class... A>
void launch_steps_kernel(hipStream_t st, int n_groups, const G& g, const M& m, const C& c, const A&... a) {
    size_t dyn = 0;
    if constexpr (M::kOn) {
        static bool allowed = false;
        if (!allowed) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)umap_lds_bytes(kIdTableSize));
            allowed = true;
        }
        dyn = umap_lds_bytes(m.m.L);
    }
    hipLaunchKernelGGL(Kernel, dim3(n_groups), dim3(kMarkerMax), dyn, st, a..., LocPolicy<G, M, C>{g, m, c});
}

void launch_loc_steps(hipStream_t st, const EkfState& E, const SlamParams& sp, const ObsRaw* obs, const unsigned* n_markers,
                      const double* enc, int first, int count, int predict_first, const GateState* gate, const MapCov* umap, bool consistent) {
    with_loc_policies(gate, umap, consistent, [&](auto g, auto m, auto c) {
        launch_steps_kernel<k_loc_steps<decltype(g), decltype(m), decltype(c)>>(st, 1, g, m, c, E, sp, obs, n_markers, enc, first, count, predict_first);
    });
}

} // namespace aslam
