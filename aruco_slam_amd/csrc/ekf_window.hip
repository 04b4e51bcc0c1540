// Windowed EKF: a run of consecutive frames whose fused landmarks all lie in one set S (no new landmark; at most kWinSMax
// landmarks in the union) is processed on the S x S block of the covariance only; the rest of Sigma follows ONCE per window.
//
// Split the state into S (robot pose + the landmarks of the set, s = 3 + 3 nS, padded to SP = 16 T) and R (everything else):
//     Sigma = [ P   Y ]      P = Sigma[S,S]   Y = Sigma[S,R]   Z = Sigma[R,R]      (Sigma is symmetric to rounding: aruco_slam.cpp:73, 204)
//             [ Y^T Z ]
// The reference's filter is sequential: one predict per encoder sample (aruco_slam.cpp:21-74: Sigma <- D Sigma D^T + Q, D = identity
// except its pose block) and, per popped observation j of a frame, K_j = Sigma H_j^T (H_j Sigma H_j^T + R_j)^-1 with the LIVE Sigma
// and the innovation at the frame's FROZEN mean, mu += K_j ze_j, Sigma <- (I - K_j H_j) Sigma (aruco_slam.cpp:88, 108-207).  H_j has
// only the pose block and the block of landmark j, so restricted to S every one of these steps is a rank-3 (predict: rank-4)
// correction of P,
//     correction:  c = H_j P (3 x s),  S_j = c H_j^T + R_j,  Kt = S_j^-1 c (= K_j^T),  P <- P - Kt^T c,  mu_S += Kt^T ze_j
//     predict:     P <- P + u r2 + (r2^T + P22 u) u^T + Q     (u = the third column of D - I, r2 = row 2 of P; Q = F Qk F^T has rank 2)
// and touches R only linearly through Y:  Y <- D Y,  Y <- Y - Kt^T (H_j Y),  Z <- Z - (H_j Y)^T S_j^-1 (H_j Y),
// mu_R <- mu_R + (H_j Y)^T S_j^-1 ze_j.  Hence, over the whole window, with an s x s accumulator Lambda (= I at the start),
//     Y_K = Lambda Y_0      Z_K = Z_0 - Y_0^T Psi Y_0      mu_R,K = mu_R,0 + Y_0^T psi
//     per step:  t = H_j Lambda,  u = S_j^-1 t,  Lambda <- Lambda - Kt^T t  (predict: Lambda <- D Lambda),  Psi += t^T u,  psi += t^T S_j^-1 ze_j
// This is the reference's own arithmetic, step for step, on the rows and columns it can change; nothing is approximated.  The one
// property used is the symmetry of Sigma (H P read as (P H^T)^T, X = Y^T).  Frames of a window may fuse ANY subset of S, in the
// reference's pop order (ascending landmark index = ascending position in S), and may drop "stationary" observations
// (aruco_slam.cpp:192-198: a no-op): a window ends only when a frame brings a landmark that does not fit into S, or a new one.
//
// Kernels (per window; a window's frames are cut into pieces of a few frames):
//   k_ekf_win_step    one launch per piece, three roles by workgroup:
//     chain   (workgroup 0) walks the steps of piece i.  P lives in the f64 matrix-core accumulators of the worker waves for the
//             whole piece (wave w: RW tile rows of T 16 x 16 tiles); a step is one v_mfma_f64_16x16x4_f64 per tile (depth 3 or 4).
//             A separate "prepare" wave (lane = column) runs one step AHEAD: the workers publish the three landmark rows of step
//             j + 2 as they stand after step j, the prepare wave applies step j + 1's correction to them and to the pose rows it
//             carries in its own registers, forms c, S, S^-1, Kt and hands the operands to the workers: one barrier per step.  The
//             workers log -Kt (the A operand they read) and worker wave 0 the header, composed from what the prepare wave leaves in
//             LDS (S^-1 per step; ze and the Jacobian scalars once per frame); in the one-launch window a logger wave of its own
//             copies both from LDS to the log;
//     replay  (SP / 8 workgroups) replays the log of piece i - 1, each on its own 8 columns of Lambda (all rows; in LDS) and its
//             part of psi, and logs t and u;
//     Psi     (T workgroups) adds the t^T u of piece i - 2 to Psi on the matrix cores.
//             The three depend on each other only through the previous launch: the stream orders them, no events between pieces.
//   k_ekf_win_gather  Y_0 = rows S of Sigma (second stream, behind the previous window's flush)
//   k_ekf_win_thin    [Psi; Lambda] Y_0 as one tiled product (U = Psi Y_0, Y_K = Lambda Y_0), mu_R += Y_0^T psi;
//   k_ekf_update_mfma (ekf.hip) Sigma -= Y_0^T U: the ONE pass over Sigma per window;  k_ekf_win_fix writes rows / columns S and P_K.
//   k_ekf_win_next    the next window's P and mu_S from this window's small results, before its flush has run.
#include "common.h"
#include "ekf.h"
#include "ekf_dev.h"
#include "ekf_slam_gate.h"
#include <cmath>
#include <cstdlib>
#include <algorithm>
#include <type_traits>

namespace aslam {

constexpr int WBW = 8;                        // columns of Lambda per scan workgroup
// one-launch window: the chain publishes its step count every kWinPubEvery steps, for the steps kWinPubLag or more behind
constexpr int kWinPubEvery = 4, kWinPubLag = 4;
#if defined(__HIP__)
constexpr unsigned long long kWinSpinTicks = 2000000;   // a wait gives up after 20 ms without progress (wall clock: 100 MHz)
#else
constexpr unsigned long long kWinSpinTicks = 6000000000ull;   // (the CPU emulation of the tests runs a step in about a millisecond)
#endif
// a wait that gave up: the FIRST code stays (a replay that stalls makes its Psi workgroups give up after it)
__device__ __forceinline__ void win_fail(const EkfState& E, unsigned code) { atomicCAS(E.d_win_err, 0u, code); }
// at the end of a publication step: the logger wave's stores of every step but the last kWinPubLag complete.  The logger wave
// issues 3 NC + 1 log stores per step (the three operand rows in NC chunks of 64 columns, the header), its count stores and no
// load: all but the newest (3 NC + 1) kWinPubLag store instructions are older than those steps' stores
template <int NC> __device__ __forceinline__ void win_vmcnt_lag() {
    static_assert(kWinPubLag == 4 && NC >= 1 && NC <= 3, "the counts below are (3 NC + 1) kWinPubLag");
    static_assert((3 * NC + 1) * kWinPubLag <= 63, "vmcnt has six bits");
    if constexpr (NC == 1) ASLAM_VMCNT(16);
    else if constexpr (NC == 2) ASLAM_VMCNT(28);
    else ASLAM_VMCNT(40);
}

// development aid (make FLAGS+=-DASLAM_WIN_STAMPS): cycle stamps of the prepare wave's step phases, of the workers and of the logger wave, summed over a piece
#ifdef ASLAM_WIN_STAMPS
#define WSTAMP(i) do { const long long t_ = clock64(); stamp_acc[i] += t_ - stamp_last; stamp_last = t_; } while (0)
// (a stamp orders nothing but volatile statements: a bucket of arithmetic is held between its stamps by its inputs and its result)
#define WSTAMP_AFTER(x) asm volatile("" : "+v"(x))
#define WSTAMP_BEFORE(x) asm volatile("" :: "v"(x))
// a stamp behind the matrix-core result x: a real instruction reads it, so the wave stands until the MFMA that writes it has ended
#define WSTAMP_RESULT(x) do { const int r_ = __builtin_amdgcn_readfirstlane(__double2hiint(x)); asm volatile("" :: "s"(r_)); } while (0)
// two stamps around the drain of the LDS queue: the clock is read (in issue order) behind the last LDS instruction, then again once
// that reading and every LDS operation in front of it have returned.  Bucket i ends at the first reading, bucket k holds the drain,
// which is never shorter than the first reading's own way back
#define WSTAMP_DRAIN(i, k) do { long long a_, b_; \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)\n\ts_memtime %1\n\ts_waitcnt lgkmcnt(0)" : "=&s"(a_), "=&s"(b_) :: "memory"); \
        stamp_acc[i] += a_ - stamp_last; stamp_acc[k] += b_ - a_; stamp_last = b_; } while (0)
#else
#define WSTAMP(i) do { } while (0)
#define WSTAMP_AFTER(x) do { } while (0)
#define WSTAMP_BEFORE(x) do { } while (0)
#endif

__host__ __device__ inline int win_log_stride(int T) { return 3 * 16 * T + kWinHdr; }
__host__ __device__ inline int win_tlog_stride(int T) { return 8 * 16 * T; }
// header of a logged step (doubles after the three operand rows)
enum { WH_TYPE = 0, WH_POS = 1, WH_SI = 2, WH_ZE = 11, WH_C = 14, WH_S = 15, WH_G02 = 16, WH_G12 = 17, WH_A = 18, WH_B = 19, WH_D2 = 20, WH_ACC = 21,
       WH_ZN = 22 };   // WH_ZN: the gated consistent window only (below): ||ze|| at the frozen mean, while WH_ZE carries e
// Gated window (aslam_set_slam_gate_windows): the one-launch step kernel is a template on a gate policy, as the solve
// kernels of the per-frame chains are (ekf_slam_gate.h).  NoSlamGate is the default: every gated statement sits under `if constexpr`
// and the policy is an empty base of the kernel's window argument, so the ungated kernels keep their arguments and their code.
// WinGate carries the threshold.  The prepare wave judges correction j where it forms S_j^-1 from the live P: d2 = ze^T S_j^-1 ze with
// the frame's frozen-mean ze.  A rejected step stays a step (the host planned the step count) with zero A operand rows, no mean
// update and step type 2 in its log header, which the replay role skips: P, mu_S, Lambda, Psi and psi do not see it, whatever its ze
// holds.  d2 and the verdict travel in the header (WH_D2; WH_ACC: 1.0 = accepted, 0.0 = rejected) to k_ekf_win_gate_finish.
struct WinGate { static constexpr bool kOn = true; double gate_d2; };
template <class G> struct WinArg : WinDesc, G {};
static_assert(sizeof(WinArg<NoSlamGate>) == sizeof(WinDesc), "the ungated window argument is the window descriptor alone");
// Consistent window (aslam_set_consistent_windows): the one-launch step kernel is also a template on the innovation
// policy of ekf_dev.h.  FrozenMean is the default; every RunningMean statement sits under `if constexpr`.  RunningMean corrects the
// mean with e = ze - H (mu_{j-1} - mu_0), mu_0 the frame's predicted mean, H as the chain writes it (Gxm below), no angle wrap.  The
// two waves that carry a copy of the mean (logger: every step; prepare: a frame's last correction, at the next predict) form e with
// this one function from the same six differences, so that both copies keep the same bits.  d: mu_{j-1} - mu_0 at columns 0, 1, 2 and
// lrow .. lrow + 2; ze comes in and e goes out in e0, e1, e2.
// Gated consistent window (aslam_set_gated_consistent_windows): RunningMean with WinGate, in the LG = 1 form, where the
// prepare wave carries the mean itself (lane = column) and so forms e in the step it judges: d2 = e^T S^-1 e, the selected mean update
// adds K e, and lane 0 leaves e (WH_ZE) and ||ze|| of the frozen-mean ze (WH_ZN, for ref_flagged) in the step's header.
__device__ __forceinline__ void win_running_innovation(double cth, double sth, double g02, double g12, const double (&d)[6], double& e0, double& e1,
                                                       double& e2) {
    e0 = e0 - ((-cth * d[0] - sth * d[1] + g02 * d[2]) + (cth * d[3] + sth * d[4]));
    e1 = e1 - ((sth * d[0] - cth * d[1] + g12 * d[2]) + (-sth * d[3] + cth * d[4]));
    e2 = e2 - (d[5] - d[2]);
}
// d_win_small: images of the window, each SPm x SPm at most (SPm = E.win_sp_max), stored with the window's own row stride SP
__host__ __device__ inline size_t wsm_P(int SPm, int par) { return (size_t)par * SPm * SPm; }             // P image of window parity par
__host__ __device__ inline size_t wsm_LAM(int SPm, int par) { return (size_t)(2 + par) * SPm * SPm; }      // Lambda / Psi / psi: also per parity (the flush of a
__host__ __device__ inline size_t wsm_PSI(int SPm, int par) { return (size_t)(4 + par) * SPm * SPm; }      // window reads them while the next window's replay writes its own)
__host__ __device__ inline size_t wsm_psi(int SPm, int par) { return (size_t)6 * SPm * SPm + (size_t)par * SPm; }
__host__ __device__ inline size_t wsm_MU(int SPm, int par) { return (size_t)6 * SPm * SPm + (size_t)(2 + par) * SPm; }   // mu_S image
__host__ __device__ inline size_t wsm_doubles(int SPm) { return (size_t)6 * SPm * SPm + (size_t)4 * SPm; }

__device__ __forceinline__ int win_state_index(const WinDesc& wd, int p) {      // state offset of position p of S
    return p < 3 ? p : wd.li[(p - 3) / 3] + (p - 3) % 3;
}

// value of element `idx` (0 .. 64 NC - 1) of a per-lane array v[NC] (element idx lives in lane idx & 63 of v[idx >> 6]); idx is
// wave-uniform.  Every lane of the wave must call it.
template <int NC> __device__ __forceinline__ double bcast_at(const double (&v)[NC], int idx) {
    const int ch = idx >> 6, ln = idx & 63;
    double r = ASLAM_WAVE_BCAST(v[0], ln);
    if (NC > 1) { const double r1 = ASLAM_WAVE_BCAST(v[NC > 1 ? 1 : 0], ln); r = ch == 1 ? r1 : r; }
    if (NC > 2) { const double r2 = ASLAM_WAVE_BCAST(v[NC > 2 ? 2 : 0], ln); r = ch == 2 ? r2 : r; }
    return r;
}

// the same with the chunk selected by uniform conditional moves in front of ONE cross-lane read (idx wave-uniform, every lane calls)
template <int NC> __device__ __forceinline__ double bcast_sel(const double (&v)[NC], int idx) {
    const int ch = idx >> 6;
    double x = v[0];
    if (NC > 1) x = ch == 1 ? v[NC > 1 ? 1 : 0] : x;
    if (NC > 2) x = ch == 2 ? v[NC > 2 ? 2 : 0] : x;
    return ASLAM_WAVE_BCAST(x, idx & 63);
}

// Rows p .. p + 2 of the image leave the accumulators of the worker wave(s) that own them (row r = 16 g + lk + 4 reg of tile row
// g): lanes with lk == r & 3 write their register reg = (r >> 2) & 3 of each of the T column tiles.  The register number must
// be static (a select chain over the accumulators costs more than the rest of the step): one instance per p mod 16.
//
// PK, the packed row: a publishing lane holds columns li + 16 t of its row, T values that lie 16 doubles apart, and writes them with
// T ds_write_b64.  The packed row keeps column c = 16 t + li at element
//     win_pub_slot(c) = 32 (t >> 1) + 2 li + (t & 1)
// so that a lane's values of tiles 2 h and 2 h + 1 are one aligned 16-byte chunk (chunk 16 h + li of the row) and leave as T / 2
// ds_write_b128.  It is a permutation of each 64-column chunk in itself (tiles 4 c .. 4 c + 3 go to elements 64 c .. 64 c + 63), so
// the row needs no padding and the prepare wave reads column lane + 64 c with the same ds_read_b64 at win_pub_slot(lane) + 64 c.  Banks
// (64 of 4 bytes; where a row starts, a multiple of 16 bytes, shifts every lane of an access alike and changes nothing below):
//   the read  (ds_read_b64, bank = dword mod 64, the two 32-lane halves apart): lanes 0 .. 31 are li = 0 .. 15 with t & 3 = 0, 1 and
//             read elements 64 c + 2 li + {0, 1}, 32 consecutive doubles = each of the 64 banks once; lanes 32 .. 63 (t & 3 = 2, 3)
//             the 32 doubles behind them;
//   the write (ds_write_b128, bank = dword mod 32, groups of 8 consecutive lanes): the 16 publishing lanes of a row are two such
//             groups, li = 0 .. 7 and 8 .. 15, and a group writes chunks 16 h + li of 4 dwords each, 8 consecutive chunks = each of
//             the 32 banks once.
// (The order T li + t, a lane's T values in one piece, cannot do both: its chunks start at even chunk numbers, a half-wave read
// touches 16 of them, and only 8 even numbers differ modulo the 16 chunks of a bank row.)  win_pub_slot_ok checks both claims.
typedef double v2d __attribute__((vector_size(2 * sizeof(double))));
__host__ __device__ constexpr int win_pub_slot(int c) { return (c & ~63) + 32 * ((c >> 5) & 1) + 2 * (c & 15) + ((c >> 4) & 1); }
template <int T> constexpr bool win_pub_slot_ok() {
    static_assert(T % 2 == 0, "tiles are packed in pairs");
    for (int c = 0; c < T / 4 + (T % 4 != 0); c++)
        for (int half = 0; half < 2; half++) {                     // the read: 32 lanes, 64 banks, every bank once
            unsigned long long banks = 0;
            for (int l = 32 * half; l < 32 * half + 32; l++) {
                const int dw = 2 * win_pub_slot(l + 64 * c);
                banks |= 3ull << (dw & 63);
            }
            if (banks != ~0ull) return false;
        }
    for (int h = 0; h < T / 2; h++)
        for (int grp = 0; grp < 2; grp++) {                        // the write: 8 lanes, 32 banks, every bank once; 16-byte aligned
            unsigned banks = 0;
            for (int li = 8 * grp; li < 8 * grp + 8; li++) {
                const int e = win_pub_slot(16 * (2 * h) + li);
                if (e % 2 != 0 || win_pub_slot(16 * (2 * h + 1) + li) != e + 1) return false;
                banks |= 15u << ((2 * e) & 31);
            }
            if (banks != ~0u) return false;
        }
    return true;
}
static_assert(win_pub_slot_ok<4>() && win_pub_slot_ok<8>() && win_pub_slot_ok<12>(), "the packed row's reads and writes are free of bank conflicts");
template <int P16, int T, int RW, bool PK>
__device__ __forceinline__ void win_publish_at(const v4d (&acc)[RW][T], int p, int wv, int lk, int li, double* rows, int spp) {
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const int rl = (P16 + q) & 15;
        const int g = (p + q) >> 4;
        double* d = rows + q * spp + (PK ? 2 * li : li);
#pragma unroll
        for (int rr = 0; rr < RW; rr++)
            if (g == wv * RW + rr && lk == (rl & 3)) {
                if constexpr (PK) {
#pragma unroll
                    for (int h = 0; h < T / 2; h++) *reinterpret_cast<v2d*>(d + 32 * h) = v2d{acc[rr][2 * h][rl >> 2], acc[rr][2 * h + 1][rl >> 2]};
                } else {
#pragma unroll
                    for (int t = 0; t < T; t++) d[16 * t] = acc[rr][t][rl >> 2];
                }
            }
    }
}
template <int T, int RW, bool PK>
__device__ __forceinline__ void win_publish(const v4d (&acc)[RW][T], int p, int wv, int lk, int li, double* rows, int spp) {
    switch (p & 15) {
#define ASLAM_WP_CASE(i) case i: win_publish_at<i, T, RW, PK>(acc, p, wv, lk, li, rows, spp); break;
        ASLAM_WP_CASE(0) ASLAM_WP_CASE(1) ASLAM_WP_CASE(2) ASLAM_WP_CASE(3) ASLAM_WP_CASE(4) ASLAM_WP_CASE(5) ASLAM_WP_CASE(6) ASLAM_WP_CASE(7)
        ASLAM_WP_CASE(8) ASLAM_WP_CASE(9) ASLAM_WP_CASE(10) ASLAM_WP_CASE(11) ASLAM_WP_CASE(12) ASLAM_WP_CASE(13) ASLAM_WP_CASE(14) ASLAM_WP_CASE(15)
#undef ASLAM_WP_CASE
    }
}

// What a window's last frame leaves behind for whatever follows: pop list, last_observed_marker_ (aruco_slam.cpp:202, 263).
// One wave, lane = popped observation; fm = corrections of the frame.
__device__ __forceinline__ void win_last_frame(const EkfState& E, const WinFrame& fr, const ObsRaw* __restrict__ fobs, int fm, int lane) {
    const int npop = fr.npop;
    if (lane < npop) {
        const ObsRaw o = fobs[fr.pdet[lane]];
        const bool upd = fr.pact[lane] == 1;
        PopRec pr;
        pr.id = o.id; pr.index = fr.pidx[lane]; pr.action = upd ? 1 : 2; pr.det = fr.pdet[lane];
        pr.z[0] = o.x; pr.z[1] = o.y; pr.z[2] = o.th;
        pr.r[0] = o.r[0]; pr.r[1] = o.r[1]; pr.r[2] = o.r[2];
        E.d_pop[lane] = pr;
        LastObs lo;
        lo.id = o.id; lo.pad = 0;
        const double nanv = __builtin_nan("");
        lo.z[0] = upd ? o.x : nanv; lo.z[1] = upd ? o.y : nanv; lo.z[2] = upd ? o.th : nanv;   // stationary: last_observation_ stays unset
        E.d_last[lane] = lo;
    }
    if (lane == 0) { *E.d_nlast = npop; *E.d_npop = npop; *E.d_m = fm; }
}

// ---------------------------------------------------------------------------------------------------------------------
// T tiles per side, RW tile rows per worker wave: ceil(T / RW) worker waves + 1 prepare wave (+ 1 logger wave in the one-launch
// window: it stores the step log and publishes the step count, so that neither lies on the workers' path).  With T = 4 (2 x 2 rows on two
// workers) the prepare wave - the kernel's critical path - has a SIMD to itself (measured: -11 % per step); at T = 8 the same idea
// (3 + 3 + 2 rows on three workers) makes the workers the bottleneck (measured: +12 %), so it keeps one worker per SIMD.
template <int T, bool ONE> struct WinChainLds {
    static constexpr int SP = 16 * T, SPP = SP + 16, KMAX = ONE ? kWinFrames : kWinPieceMax, NSMAX = KMAX * 64;
    double sA[2][4][SPP];                  // a step's A operand rows  Aop[k][row]   (P += Aop^T Bop)
    double sB[2][4][SPP];                  // ... and B operand rows   Bop[k][column]
    double sPub[2][3][SPP];                // the landmark rows of the step after next
    double sHdr[2][kWinHdr];               // what a step newly brings to its log header (correction: S^-1, unless the logger wave forms it
                                           // itself; predict: its six values), from the prepare wave to the wave that stores the header
                                           // (logger; pieces: worker wave 0)
    // a frame's records (ze0, ze1, ze2, g02, g12 of correction a; one launch: also R0, R1, R2, for the logger wave's S^-1), by frame
    // parity: see win_header_entry
    static constexpr int kRecRows = ONE ? 8 : 5;
    double sRec[2][kRecRows][64];
    // one launch, the mean on the logger wave: its mu_S for the prepare wave's next predict, by the parity of the phase it is written
    // in, and the pose that predict leaves, by frame parity (two predicts can follow each other)
    double sMuL[2][ONE ? SPP : 1];
    double sPose[2][4];
#ifdef ASLAM_WIN_POSE_CHECK
    double sDbg[2][3][SPP];                // the accumulators' pose rows, to compare with the prepare wave's own
#endif
    double sMu[SPP];                       // prepare wave's scratch: mu_S by position
    int sS[SP];
    int sOff[KMAX + 1];
    // per step: landmark position (255 = predict) and correction index, for the workers and the wave that stores the header (the
    // prepare wave counts its steps in scalar registers); the correction's detection in its frame's observation list
    unsigned char sPos[NSMAX], sIdx[NSMAX];
    unsigned char sDet[NSMAX];
    // what the block gained over the size the launch's LDS claim was measured at (launch_step_kernel): sRec and the logger wave's
    // mean hand-overs, less a per-step frame table
    static constexpr int kGrown = (int)sizeof(sRec) + (int)sizeof(sMuL) + (int)sizeof(sPose) - NSMAX;
};
// Entry `lane` (< kWinHdr) of step j's log header, composed by the wave that stores it.  A predict's header is what the prepare
// wave left in sHdr.  A correction's is S^-1 from sHdr, type and position from the step tables, and ze, g02, g12 from the records
// of the step's frame: the prepare wave writes them ONCE per frame, at the frame's predict, into sRec[frame parity].  Two parities
// suffice: the prepare wave prepares step j + 1 while step j is stored, and the step in front of frame k's predict belongs to
// frame k - 1 whatever the frames fuse (a frame without corrections is a lone predict, which reads no record).
// GATED: the prepare wave also left the step's type there (1.0, or 2.0 = rejected) with d2 and the verdict (WH_D2, WH_ACC).
template <bool GATED, class LDS> __device__ __forceinline__ double win_header_entry(const LDS& L, int j, int cb, int fpar, int lane) {
    double v = L.sHdr[cb][lane];
    const int pos = L.sPos[j];
    if (pos != 255) {
        const int a = L.sIdx[j];
        const int q = lane >= WH_ZE && lane < WH_ZE + 3 ? lane - WH_ZE : lane == WH_G02 ? 3 : lane == WH_G12 ? 4 : -1;
        if (q >= 0) v = L.sRec[fpar][q][a];
        if (!GATED && lane == WH_TYPE) v = 1.0;
        if (lane == WH_POS) v = (double)pos;
    }
    return v;
}
// LG (one launch only): what the logger wave takes over from the prepare wave.  Bit 0: it forms the log header's S^-1 itself, from
// the step's c rows in sB and the frame's records; bit 1: it carries mu_S.  0 is the comparison path (ASLAM_WIN_LOGGER_PARTS).
// WP: how the worker waves publish the landmark rows of the step after next (ASLAM_WIN_WORKER_PUBLISH; 0 is the comparison path).
//   bit 0  packed row: T / 2 ds_write_b128 per row instead of T ds_write_b64 (win_publish_at); the prepare wave reads the same rows
//          with the same three reads per chunk at a lane offset it forms once, in front of its loop.
//   bit 1  the step table's entry a phase ahead: sPos[j + 3] is read with phase j's B operand and kept in a register, so that no
//          LDS round trip stands between the MFMAs and the publication's switch (the step tables never change inside a window).
// The prepare wave's steps and the values it reads do not depend on WP, and no floating-point operation moves.
// IN: the innovation policy (FrozenMean, or RunningMean: the consistent window of DESIGN.md §33, ungated beside LG = 3, or the gated
// consistent window of DESIGN.md §37, WinGate beside LG = 1).
template <int T, int RW, bool ONE, class G, int LG, int WP, class IN = FrozenMean>
__device__ void win_chain_role(const EkfState& E, const SlamParams& sp, const WinDesc& wd, const G& gate, const ObsRaw* __restrict__ obs,
                               const double* __restrict__ enc, unsigned char* smem) {
    static_assert(ONE || !G::kOn, "only the one-launch window is gated");
    static_assert(ONE || LG == 0, "the piece schedule has no logger wave");
    static_assert(!IN::kOn || (ONE && ((LG == 3 && !G::kOn) || (LG == 1 && G::kOn))),
                  "the consistent window: one launch; ungated with the mean on the logger wave, gated with the mean on the prepare wave");
    constexpr bool LSI = (LG & 1) != 0, LMU = (LG & 2) != 0;
    constexpr bool PK = (WP & 1) != 0, AHEAD = (WP & 2) != 0;
    constexpr int SP = 16 * T, SPP = SP + 16, NC = SP / 64;       // SPP: operand rows lk and lk + 1 fall on opposite halves of the bank row
    constexpr int NWK = (T + RW - 1) / RW, NT = (NWK + (ONE ? 2 : 1)) * 64;   // workers, prepare wave, one launch: logger wave
    WinChainLds<T, ONE>& L = *reinterpret_cast<WinChainLds<T, ONE>*>(smem);
    auto& sA = L.sA; auto& sB = L.sB; auto& sPub = L.sPub; auto& sMu = L.sMu; auto& sS = L.sS; auto& sOff = L.sOff;
    auto& sPos = L.sPos; auto& sIdx = L.sIdx; auto& sDet = L.sDet;
    if (threadIdx.x >= NT) return;                                  // (the launch's block is sized for its widest role)
    const int tid = threadIdx.x;
    const int nS = wd.nS, s = 3 + 3 * nS;
    const int ld = E.ld;
    const WinFrame* __restrict__ frames = E.d_win_frames;

    const int wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    for (int e = tid; e < SP; e += NT) sS[e] = e < s ? win_state_index(wd, e) : 0;
    for (int e = tid; e < 2 * 4 * SPP; e += NT) { (&sA[0][0][0])[e] = 0.0; (&sB[0][0][0])[e] = 0.0; }
    for (int e = tid; e < 2 * 3 * SPP; e += NT) (&sPub[0][0][0])[e] = 0.0;
    for (int e = tid; e < 2 * kWinHdr; e += NT) (&L.sHdr[0][0])[e] = 0.0;
    if constexpr (ONE) {
        // the step tables of the whole window (K <= 64 frames): thread k loads frame k's head, its 64 landmark positions and its 64
        // detection indices at once, wave 0 forms the running sum with a lane scan, thread k writes its frame's steps.  The head
        // is all the frame's slot statistics need: thread k stores them here, off the chain
        int cnt = 0;
        unsigned cp[16], cd[16];
        if (tid < wd.K) {
            const int slot = wd.first_slot + tid;
            const WinFrame& fr = frames[slot];
            const int fm = fr.m, fnpop = fr.npop, fnm = fr.n_markers;
            cnt = 1 + fm;
            const unsigned* c4 = reinterpret_cast<const unsigned*>(fr.cpos);
            const unsigned* d4 = reinterpret_cast<const unsigned*>(fr.cdet);
#pragma unroll
            for (int q = 0; q < 16; q++) { cp[q] = c4[q]; cd[q] = d4[q]; }
            if (slot < E.max_slots) {
                int* st = E.d_slot_stat + 4 * slot;
                st[0] = fnm; st[1] = 0; st[2] = fm; st[3] = fnpop - fm;
            }
        }
        if (wave == 0) {
            int inc = cnt;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(inc, d); if (lane >= d) inc += y; }
            sOff[lane + 1] = inc;
            if (lane == 0) sOff[0] = 0;
        }
        __syncthreads();
        if (tid < wd.K) {
            const int o = sOff[tid], m = cnt - 1;
            sPos[o] = 255; sIdx[o] = 0; sDet[o] = 0;
#pragma unroll
            for (int a = 0; a < 63; a++)
                if (a < m) {
                    sPos[o + 1 + a] = (unsigned char)(cp[a >> 2] >> (8 * (a & 3))); sDet[o + 1 + a] = (unsigned char)(cd[a >> 2] >> (8 * (a & 3)));
                    sIdx[o + 1 + a] = (unsigned char)a;
                }
        }
        __syncthreads();
    } else {
        // steps per frame (1 predict + m corrections), every frame's count loaded by its own thread (one thread walking the plan would
        // pay one dependent global load per frame), then the running sum
        if (tid < wd.K) {
            const int slot = wd.first_slot + tid;
            const WinFrame& fr = frames[slot];
            const int fm = fr.m, fnpop = fr.npop, fnm = fr.n_markers;
            sOff[tid + 1] = 1 + fm;
            if (slot < E.max_slots) {                               // the frame's slot statistics
                int* st = E.d_slot_stat + 4 * slot;
                st[0] = fnm; st[1] = 0; st[2] = fm; st[3] = fnpop - fm;
            }
        }
        if (tid == 0) sOff[0] = 0;
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < wd.K; k++) sOff[k + 1] += sOff[k];
        __syncthreads();
        for (int k = 0; k < wd.K; k++) {
            const WinFrame& fr = frames[wd.first_slot + k];
            for (int a = tid; a <= fr.m; a += NT) {
                const int st = sOff[k] + a;
                sPos[st] = a == 0 ? 255 : fr.cpos[a - 1];
                sIdx[st] = a == 0 ? 0 : (unsigned char)(a - 1);
                sDet[st] = a == 0 ? 0 : fr.cdet[a - 1];
            }
        }
        __syncthreads();
    }
    const int NS = sOff[wd.K];                                    // steps of the piece: per frame one predict + m corrections

    const double* Pimg = E.d_win_small + wsm_P(E.win_sp_max, wd.wpar);
    const bool from_img = wd.piece != 0 || wd.from_image != 0;
    double* const logbase = E.d_win_log + (size_t)wd.log0 * win_log_stride(T);
    if (wave < NWK) {
        // =================================== worker waves: P in the accumulators ===================================
        v4d acc[RW][T];
#pragma unroll
        for (int rr = 0; rr < RW; rr++)
#pragma unroll
            for (int t = 0; t < T; t++)
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    const int r = 16 * (wave * RW + rr) + lk + 4 * reg, c = 16 * t + li;
                    double v = 0.0;
                    if (r < SP) {                                                  // (the last worker may own fewer than RW tile rows)
                        if (from_img) v = Pimg[(size_t)r * SP + c];                // the window goes on (or was prepared ahead): P from the image
                        else if (r < s && c < s) v = E.d_sigma[(size_t)sS[c] * ld + sS[r]];
                    }
                    acc[rr][t][reg] = v;
                }
        // landmark rows of step 1 as they stand before any step (step 0 is a predict; the prepare wave carries the pose rows itself)
#ifdef ASLAM_WIN_POSE_CHECK
        if (wave == 0 && lk < 3) {
#pragma unroll
            for (int t = 0; t < T; t++) { L.sDbg[0][lk][16 * t + li] = acc[0][t][0]; L.sDbg[1][lk][16 * t + li] = acc[0][t][0]; }
        }
#endif
        if (NS > 1 && sPos[1] != 255) win_publish<T, RW, PK>(acc, 3 + 3 * sPos[1], wave, lk, li, &sPub[1][0][0], SPP);
        ASLAM_LDS_BARRIER();
#ifdef ASLAM_WIN_STAMPS
        long long stamp_acc[6] = {0, 0, 0, 0, 0, 0}, stamp_last = clock64();
        int st_pn = 255;                                           // (stamps only) sPos[j + 2], read a phase ahead: which accumulator the wait's stamp reads
#endif
        int fpar = 1;                                              // (pieces, wave 0) parity of step j's frame: the first predict makes it 0
        int pn_ahead = 255;                                        // AHEAD: sPos[j + 2], read in phase j - 1
        for (int j = -1; j < NS; j++) {
            WSTAMP(0);
            int pn_next = 255;
            if constexpr (AHEAD) pn_next = sPos[j + 3 < NS ? j + 3 : NS - 1];     // (issued with the B operand's reads; used a phase later)
#ifdef ASLAM_WIN_STAMPS
            const int st_next = sPos[j + 3 < NS ? j + 3 : NS - 1];
#endif
            if (j >= 0) {
                const int cb = j & 1;
                double* const log = logbase + (size_t)j * win_log_stride(T);
                double b[T];
#pragma unroll
                for (int t = 0; t < T; t++) b[t] = sB[cb][lk][16 * t + li];
#ifdef ASLAM_WIN_STAMPS
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (stamps only: the B operand's reads apart from the products)
                WSTAMP(1);
#endif
#pragma unroll
                for (int rr = 0; rr < RW; rr++) {
                    if (T % RW != 0 && wave * RW + rr >= T) break;
                    const double a = sA[cb][lk][16 * (wave * RW + rr) + li];
#pragma unroll
                    for (int t = 0; t < T; t++) acc[rr][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[t], acc[rr][t], 0, 0, 0);
                    // pieces: the step's log rows, -Kt (predict: its rows 0..2).  One launch: the logger wave stores the log
                    if (!ONE && lk < 3) log[lk * SP + 16 * (wave * RW + rr) + li] = a;
                }
                if (!ONE && wave == 0) {
                    if (sPos[j] == 255) fpar ^= 1;
                    if (lane < kWinHdr) log[3 * SP + lane] = win_header_entry<false>(L, j, cb, fpar, lane);
                }
                WSTAMP(2);
#ifdef ASLAM_WIN_STAMPS
                // (stamps only) the wait for the products the publication reads.  The matrix core ends the MFMAs in issue order, so
                // the last accumulator of the last-issued tile row that holds a published row stands for all of them
                if (j + 2 < NS && st_pn != 255) {
                    const int g0 = (3 + 3 * st_pn) >> 4, g1 = (5 + 3 * st_pn) >> 4;
                    const int r_last = g1 - wave * RW >= 0 && g1 - wave * RW < RW ? g1 - wave * RW : g0 - wave * RW;
                    if (r_last == 0) WSTAMP_RESULT(acc[0][T - 1][0]);
                    else if (r_last == 1) WSTAMP_RESULT(acc[RW > 1 ? 1 : 0][T - 1][0]);
                }
                WSTAMP(3);
#endif
                if (j + 2 < NS) {                                   // landmark rows of step j + 2 as they stand after step j
#ifdef ASLAM_WIN_POSE_CHECK
                    if (wave == 0 && lk < 3) {
#pragma unroll
                        for (int t = 0; t < T; t++) L.sDbg[cb][lk][16 * t + li] = acc[0][t][0];
                    }
#endif
                    const int pn = AHEAD ? pn_ahead : sPos[j + 2];
                    if (pn != 255) win_publish<T, RW, PK>(acc, 3 + 3 * pn, wave, lk, li, &sPub[cb][0][0], SPP);
                }
            }
            pn_ahead = pn_next;
#ifdef ASLAM_WIN_STAMPS
            st_pn = st_next;
            WSTAMP_DRAIN(4, 5);
#endif
            ASLAM_LDS_BARRIER();
        }
#ifdef ASLAM_WIN_STAMPS
        if (lane == 0 && (ONE || wd.piece == 1))
            printf("worker %d T %d steps %d form %d: barrier-wait %lld | B reads %lld A reads + products%s %lld publish: wait for the products %lld look-up + switch + writes %lld drain %lld cycles per step\n",
                   wave, T, NS, WP, stamp_acc[0] / (NS + 1), stamp_acc[1] / (NS + 1), ONE ? "" : " + log", stamp_acc[2] / (NS + 1), stamp_acc[3] / (NS + 1),
                   stamp_acc[4] / (NS + 1), stamp_acc[5] / (NS + 1));
#endif
        // P_K for the next piece / the flush
        double* Pout = E.d_win_small + wsm_P(E.win_sp_max, wd.wpar);
#pragma unroll
        for (int rr = 0; rr < RW; rr++)
#pragma unroll
            for (int t = 0; t < T; t++)
#pragma unroll
                for (int reg = 0; reg < 4; reg++)
                    if (T % RW == 0 || wave * RW + rr < T) Pout[(size_t)(16 * (wave * RW + rr) + lk + 4 * reg) * SP + 16 * t + li] = acc[rr][t][reg];
        return;
    }

    if (ONE && wave == NWK + 1) {
        // ============================ logger wave (one-launch window): the step log and its publication ============================
        // In phase j the operand rows and the header of step j lie in the parity buffers sA[j & 1], sHdr[j & 1], which nobody writes
        // before the phase's barrier: this wave copies them to the log (write-through) and is the only wave of the role that stores
        // to the log in the loop, so the publication needs this wave's store counter alone.  Steps 0 .. j - 1 - kWinPubLag are complete
        // when it has waited for them at the end of step j - 1; it then passes the barrier (as every wave that read or wrote those
        // steps' operands has) and one of its lanes publishes their count for the replay workgroups.
        //
        // What the prepare wave does in a correction for this wave's sake alone is done here instead, off the critical path, with
        // the prepare wave's expressions on the prepare wave's inputs (every bit stays what it was):
        //   LSI  S^-1 of the header.  c of step j still lies in sB[j & 1][0..2] (the prepare wave wrote it a phase earlier and now
        //        writes the other parity only); cos / sin of the frame are kept from its predict's header, g02, g12 and R come from
        //        the frame's records.
        //   LMU  mu_S.  Kt is the negated A operand (exactly), ze comes from the records; a predict's pose arrives in sPose[frame
        //        parity].  The prepare wave needs the mean at a predict only, which it prepares in phase j for step j + 1: in
        //        phase j - 1 this wave leaves its mean (steps <= j - 1 applied) in sMuL[(j - 1) & 1] and the prepare wave adds step
        //        j's update itself.  Two parities: with two predicts in a row this wave writes in the phase the prepare wave reads in.
        double* const muimg = E.d_win_small + wsm_MU(E.win_sp_max, wd.wpar);
        double lmu[NC];
        double lmu0[IN::kOn ? NC : 1];                             // RunningMean: the frame's predicted mean mu_0, snapshot at its predict
        if constexpr (IN::kOn) {
#pragma unroll
            for (int c = 0; c < NC; c++) lmu0[c] = 0.0;
        }
        ASLAM_LDS_BARRIER();                                       // (pairs with the workers' barrier after their first publish)
        if constexpr (LMU) {
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const int col = lane + 64 * c;
                lmu[c] = col >= s ? 0.0 : from_img ? muimg[col] : E.d_mu[sS[col]];   // (as the prepare wave loads it)
            }
        }
        // What the window's last frame leaves behind for whatever follows: pop list, last_observed_marker_ (aruco_slam.cpp:202,
        // 263).  Nothing of it depends on the chain, and this wave has no log to store while the first predict is prepared: it
        // does the two-level load here.  The stores need the loaded values, so no load is in flight when the loop begins.
        win_last_frame(E, frames[wd.first_slot + wd.K - 1], obs + (size_t)(wd.first_slot + wd.K - 1) * kMarkerMax, sOff[wd.K] - sOff[wd.K - 1] - 1, lane);
        if constexpr (LMU) ASLAM_VMCNT(0);                         // (the mean's loads too: win_vmcnt_lag counts stores)
#ifdef ASLAM_WIN_STAMPS
        long long stamp_acc[4] = {0, 0, 0, 0}, stamp_last = clock64();
#endif
        int fpar = 1;                                              // parity of step j's frame: the first predict makes it 0
        double lcth = 1.0, lsth = 0.0;                             // cos / sin of step j's frame
        // The step tables never change: position and correction index of the steps ahead are read a phase or more before they are
        // needed, so that in a phase every LDS address is known at its start and all its reads are issued together, in front of any
        // use: one round trip through LDS instead of one per dependent read (the wave's time goes to LDS latency, not to arithmetic).
        // A predict takes the correction's path with harmless addresses (row 0, record 0) and its results are selected away.
        int p_cur = 255, a_cur = 0;                                // step j
        int p_n1 = sPos[0], a_n1 = sIdx[0];                        // step j + 1
        int p_n2 = sPos[NS > 1 ? 1 : 0];                           // step j + 2
        for (int j = -1; j < NS; j++) {
            WSTAMP(0);
            if (j > kWinPubLag && j % kWinPubEvery == 0 && lane == 0) win_signal(E.d_win_sync, wd.epoch, j - kWinPubLag);
            const int p_n3 = sPos[j + 3 < NS ? j + 3 : NS - 1], a_n2 = sIdx[j + 2 < NS ? j + 2 : NS - 1];
            if (j >= 0) {
                const int cb = j & 1;
                double* const log = logbase + (size_t)j * win_log_stride(T);
                const int pos = p_cur, a = a_cur;
                const bool corr = pos != 255;
                if (!corr) fpar ^= 1;
                const int lrow = corr ? 3 + 3 * pos : 0;
                const auto& rec = L.sRec[fpar];
                // ---- every read of the phase ----
                double av[3][NC];
#pragma unroll
                for (int k = 0; k < 3; k++)
#pragma unroll
                    for (int c = 0; c < NC; c++) av[k][c] = sA[cb][k][lane + 64 * c];
                // the header: what the prepare wave left, and the entry of the frame's records this lane stores (win_header_entry)
                const int hq = lane >= WH_ZE && lane < WH_ZE + 3 ? lane - WH_ZE : lane == WH_G02 ? 3 : lane == WH_G12 ? 4 : -1;
                const double hb = L.sHdr[cb][lane < kWinHdr ? lane : 0], hr = rec[hq >= 0 ? hq : 0][a];
                const double hC = L.sHdr[cb][WH_C], hS = L.sHdr[cb][WH_S], hT = L.sHdr[cb][WH_TYPE];
                const double pose = L.sPose[fpar][lane < 3 ? lane : 3];
                double ze0 = rec[0][a], ze1 = rec[1][a], ze2 = rec[2][a];
                const double g02 = rec[3][a], g12 = rec[4][a];
                double R0 = 0.0, R1 = 0.0, R2 = 0.0;
                double cB[3][6];
                if constexpr (LSI) {
                    R0 = rec[5][a]; R1 = rec[6][a]; R2 = rec[7][a];
#pragma unroll
                    for (int kk = 0; kk < 3; kk++) {
                        cB[kk][0] = sB[cb][kk][0]; cB[kk][1] = sB[cb][kk][1]; cB[kk][2] = sB[cb][kk][2];
                        cB[kk][3] = sB[cb][kk][lrow]; cB[kk][4] = sB[cb][kk][lrow + 1]; cB[kk][5] = sB[cb][kk][lrow + 2];
                    }
                }
                // ---- the operand rows to the log ----
#pragma unroll
                for (int k = 0; k < 3; k++)
#pragma unroll
                    for (int c = 0; c < NC; c++) st_wt(log + k * SP + lane + 64 * c, av[k][c]);
                if (!corr) { lcth = hC; lsth = hS; }
                if constexpr (IN::kOn && LMU) {
                    // ---- e = ze - H (mu_{j-1} - mu_0): six columns of this wave's own mean, by wave-uniform cross-lane reads ----
                    double dl[NC], d[6];
#pragma unroll
                    for (int c = 0; c < NC; c++) dl[c] = lmu[c] - lmu0[c];
#pragma unroll
                    for (int q = 0; q < 3; q++) { d[q] = bcast_sel<NC>(dl, q); d[3 + q] = bcast_sel<NC>(dl, lrow + q); }
                    win_running_innovation(lcth, lsth, g02, g12, d, ze0, ze1, ze2);
                }
                // ---- the header entry of this lane (win_header_entry) ----
                double hv = hb;
                if (corr) {
                    if (hq >= 0) hv = hr;
                    if constexpr (IN::kOn && LMU) hv = hq == 0 ? ze0 : hq == 1 ? ze1 : hq == 2 ? ze2 : hv;   // WH_ZE carries e: the replay's psi follows
                    if constexpr (IN::kOn && !LMU) hv = hq >= 0 && hq < 3 ? hb : hv;   // ... formed by the prepare wave, which left it (and WH_ZN) in sHdr
                    if (!G::kOn && lane == WH_TYPE) hv = 1.0;
                    if (lane == WH_POS) hv = (double)pos;
                }
                WSTAMP_BEFORE(hv);
                WSTAMP(1);
                if constexpr (LSI) {
                    // ---- S = c H^T + R and its inverse, as the prepare wave forms them (below) ----
                    double cth = lcth, sth = lsth;
                    WSTAMP_AFTER(cth); WSTAMP_AFTER(sth);
                    double Sm[9], Si[9];
#pragma unroll
                    for (int kk = 0; kk < 3; kk++) {
                        const double p0 = cB[kk][0], p1 = cB[kk][1], p2 = cB[kk][2];
                        const double l0 = cB[kk][3], l1 = cB[kk][4], l2 = cB[kk][5];
                        Sm[kk * 3 + 0] = (-cth * p0 - sth * p1 + g02 * p2) + (cth * l0 + sth * l1);
                        Sm[kk * 3 + 1] = (sth * p0 - cth * p1 + g12 * p2) + (-sth * l0 + cth * l1);
                        Sm[kk * 3 + 2] = l2 - p2;
                    }
                    Sm[0] += R0; Sm[4] += R1; Sm[8] += R2;
                    Sm[3] = Sm[1]; Sm[6] = Sm[2]; Sm[7] = Sm[5];    // one triangle of S, as the prepare wave inverts it (below)
                    inv3_fast(Sm, Si);
#pragma unroll
                    for (int q = 0; q < 9; q++) hv = corr && lane == WH_SI + q ? Si[q] : hv;
                }
                WSTAMP_BEFORE(hv);
                WSTAMP(2);
                if (lane < kWinHdr) st_wt(log + 3 * SP + lane, hv);
                // a publication follows the next barrier: this wave's stores of the steps before the last kWinPubLag are complete
                if ((j + 1) % kWinPubEvery == 0) win_vmcnt_lag<NC>();
                WSTAMP(1);
                if constexpr (LMU) {
                    WSTAMP_AFTER(ze0); WSTAMP_AFTER(ze1); WSTAMP_AFTER(ze2);
                    // ---- mu_ += K ze (aruco_slam.cpp:203), by selection: a rejected step's ze may be NaN (type 2), a predict has none ----
                    const bool upd = corr && !(G::kOn && hT == 2.0);
#pragma unroll
                    for (int c = 0; c < NC; c++) {
                        const double k0 = -av[0][c], k1 = -av[1][c], k2 = -av[2][c];
                        const double dm = k0 * ze0 + k1 * ze1 + k2 * ze2;
                        lmu[c] = upd ? lmu[c] + dm : lmu[c];
                    }
                    if (!corr && lane < 3) lmu[0] = pose;              // a predict: the pose it leaves
                    if constexpr (IN::kOn) {
                        if (!corr) {
#pragma unroll
                            for (int c = 0; c < NC; c++) lmu0[c] = lmu[c];
                        }
                    }
                }
            }
            if constexpr (LMU) {
                // step j + 2 is a predict: the prepare wave prepares it in the next phase, from this mean (steps <= j applied)
                if (j + 2 < NS && p_n2 == 255) {
#pragma unroll
                    for (int c = 0; c < NC; c++) L.sMuL[j & 1][lane + 64 * c] = lmu[c];
                }
            }
            p_cur = p_n1; a_cur = a_n1; p_n1 = p_n2; a_n1 = a_n2; p_n2 = p_n3;
            WSTAMP(3);
            ASLAM_LDS_BARRIER();
        }
        if constexpr (LMU) {
            // ---- mu_S for the window's flush and the next window; back into the state where the window asks for it ----
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const int col = lane + 64 * c;
                if (col < s) { muimg[col] = lmu[c]; if (wd.mu_out) E.d_mu[sS[col]] = lmu[c]; }
            }
        }
        ASLAM_VMCNT(0);                                            // the whole log: after this wave's last stores
        if (lane == 0) win_signal(E.d_win_sync, wd.epoch, NS);
#ifdef ASLAM_WIN_STAMPS
        if (lane == 0) printf("logger T %d steps %d: barrier-wait %lld copy + header %lld S^-1 %lld mu %lld cycles per step\n", T, NS, stamp_acc[0] / (NS + 1),
                              stamp_acc[1] / (NS + 1), stamp_acc[2] / (NS + 1), stamp_acc[3] / (NS + 1));
#endif
        return;
    }

    // ======================================= prepare wave: lane = column (NC chunks of 64) =======================================
    // What a step needs from another column (the previous step's A operand at the six row indices, c at the six special columns)
    // is wave-uniform and is read back from LDS as a broadcast - the operands live there anyway (measured: cheaper than v_readlane
    // plus chunk selection).
#ifndef ASLAM_NO_SETPRIO
    __builtin_amdgcn_s_setprio(3);                                  // the critical path of the kernel: wins the issue slot over the worker wave it shares a SIMD with
#endif
    const double kl = sp.kl, kr = sp.kr, inv2b = 1.0 / (2 * sp.b), invb = 1 / sp.b, Qk = sp.Q_k;
    double* const muimg = E.d_win_small + wsm_MU(E.win_sp_max, wd.wpar);
    const int pcol = PK ? win_pub_slot(lane) : lane;               // where column `lane` of a published row's chunk lies (win_publish_at)
    double mu[NC], pB[4][NC];
    double rp[3][NC];                                              // the pose rows of P, carried here (the workers publish landmark rows only)
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const int col = lane + 64 * c;
        // mu_S travels between the pieces of a window in its image; only the window's last piece puts it back into the state
        mu[c] = col >= s ? 0.0 : from_img ? muimg[col] : E.d_mu[sS[col]];
#pragma unroll
        for (int k = 0; k < 4; k++) pB[k][c] = 0.0;
#pragma unroll
        for (int q = 0; q < 3; q++) rp[q][c] = from_img ? Pimg[(size_t)q * SP + col] : col < s ? E.d_sigma[(size_t)sS[col] * ld + sS[q]] : 0.0;   // (as the workers load them)
    }
#ifdef ASLAM_WIN_POSE_CHECK
    double dmax = 0.0, dend = 0.0;
#endif
    // per-frame records, lane a = correction a of the frame (aruco_slam.cpp:119-143 at the frozen mean)
    double rze0 = 0, rze1 = 0, rze2 = 0, rR0 = 0, rR1 = 0, rR2 = 0, rg02 = 0, rg12 = 0;
    double cth = 1.0, sth = 0.0;
    // Step control in wave-uniform (scalar) registers: the frame fk, its corrections fm and the next correction fa.  A step is
    // a predict when the frame's corrections are exhausted (every piece and every window starts with a predict), and lane a keeps
    // the position of correction a from the predict on (vpos): no step waits for a look-up in the step tables
    int fk = -1, fm = 0, fa = 0, vpos = 0;
    bool prev_predict = false;
    bool dirty0 = false, dirty1 = false;                           // operand buffer 0 / 1 holds a predict's fourth depth row
    // LMU (the logger wave carries the mean): what the previous step did to it, which this wave adds at a predict to the mean the
    // logger left a phase earlier: K ze of an accepted correction (Kt is the negated A operand, which still lies in LDS: keeping
    // it in registers would cost every correction moves), or the pose a predict left
    double pn0 = 0.0, pn1 = 0.0, pth = 0.0;
    bool prev_rejected = false;
    if constexpr (LMU) {
#pragma unroll
        for (int c = 0; c < NC; c++) L.sMuL[0][lane + 64 * c] = mu[c];   // the first predict reads its mean where every later one does
    }
    // the first frame's inputs
    ObsRaw nObs{};
    if (lane < sOff[1] - 1) nObs = obs[(size_t)wd.first_slot * kMarkerMax + sDet[1 + lane]];
    double e_wl, e_wr, e_dt;
    { const double* e = enc + (size_t)3 * wd.first_slot; e_wl = e[0]; e_wr = e[1]; e_dt = e[2]; }
    ASLAM_LDS_BARRIER();                                           // (pairs with the workers' barrier after their first publish)
#ifdef ASLAM_WIN_STAMPS
    long long stamp_acc[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, stamp_last = clock64();
    int n_pred = 0;
#endif
    for (int j = -1; j < NS; j++) {
        const int n = j + 1;                                       // the step prepared in this phase
        WSTAMP(0);
        if (n < NS) {
            const int nb = n & 1, pb = j & 1;
            const bool is_predict = fa == fm;
            // first landmark row (a predict has none: copies of the pose rows)
            const int lrow = is_predict ? 0 : 3 + 3 * ASLAM_WAVE_BCAST(vpos, fa & 63);
            double r[6][NC];
#pragma unroll
            for (int c = 0; c < NC; c++) {
                r[0][c] = rp[0][c]; r[1][c] = rp[1][c]; r[2][c] = rp[2][c];
                r[3][c] = sPub[nb][0][pcol + 64 * c]; r[4][c] = sPub[nb][1][pcol + 64 * c]; r[5][c] = sPub[nb][2][pcol + 64 * c];
            }
#ifdef ASLAM_WIN_POSE_CHECK
            dend = 0.0;
#pragma unroll
            for (int q = 0; q < 3; q++)
#pragma unroll
                for (int c = 0; c < NC; c++) dend = fmax(dend, fabs(r[q][c] - L.sDbg[nb][q][lane + 64 * c]));
            dmax = fmax(dmax, dend);
#endif
            if (j >= 0) {
                // step j's correction of these rows: P[R][col] += sum_k Aop_j[k][R] Bop_j[k][col]
                const int kd = prev_predict ? 4 : 3;                // a correction has depth 3
                double f[4][6];
#pragma unroll
                for (int kk = 0; kk < 4; kk++) {
                    if (kk >= kd) break;
                    f[kk][0] = sA[pb][kk][0]; f[kk][1] = sA[pb][kk][1]; f[kk][2] = sA[pb][kk][2];      // (LDS broadcast reads: measured faster than v_readlane)
                    f[kk][3] = sA[pb][kk][lrow]; f[kk][4] = sA[pb][kk][lrow + 1]; f[kk][5] = sA[pb][kk][lrow + 2];
                }
#ifdef ASLAM_WIN_STAMPS
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (stamps only: the reads' wait apart from the FMAs)
                WSTAMP(7);
#endif
#pragma unroll
                for (int kk = 0; kk < 4; kk++) {
                    if (kk >= kd) break;
#pragma unroll
                    for (int c = 0; c < NC; c++) {
                        r[0][c] = fma(f[kk][0], pB[kk][c], r[0][c]); r[1][c] = fma(f[kk][1], pB[kk][c], r[1][c]); r[2][c] = fma(f[kk][2], pB[kk][c], r[2][c]);
                        r[3][c] = fma(f[kk][3], pB[kk][c], r[3][c]); r[4][c] = fma(f[kk][4], pB[kk][c], r[4][c]); r[5][c] = fma(f[kk][5], pB[kk][c], r[5][c]);
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < NC; c++) { rp[0][c] = r[0][c]; rp[1][c] = r[1][c]; rp[2][c] = r[2][c]; }
            WSTAMP(1);
            double* const hdr = L.sHdr[nb];
            double A[4][NC], B[4][NC];
            if (is_predict) {
#ifdef ASLAM_WIN_STAMPS
                n_pred++;
#endif
                if constexpr (LMU) {
                    // the mean after step j: the logger's (steps <= j - 1) and step j's update, with the expression of mu_ += K ze
#pragma unroll
                    for (int c = 0; c < NC; c++) mu[c] = L.sMuL[nb][lane + 64 * c];
                    if (j >= 0) {
                        if (prev_predict) {
                            if (lane == 0) mu[0] = pn0;
                            if (lane == 1) mu[0] = pn1;
                            if (lane == 2) mu[0] = pth;
                        } else if (!prev_rejected) {                // (step j was the last correction of its frame: fm - 1)
                            double ze0 = ASLAM_WAVE_BCAST(rze0, fm - 1), ze1 = ASLAM_WAVE_BCAST(rze1, fm - 1), ze2 = ASLAM_WAVE_BCAST(rze2, fm - 1);
                            if constexpr (IN::kOn) {
                                // e of that correction, as the logger wave forms it: mu_{j-1} is the row the logger left (loaded above),
                                // mu_0 the pose this wave predicted for the frame and the landmark means it left in sMu at that predict
                                const int lr = 3 + 3 * ASLAM_WAVE_BCAST(vpos, (fm - 1) & 63);
                                const double* ml = L.sMuL[nb];
                                const double d[6] = {ml[0] - pn0, ml[1] - pn1, ml[2] - pth, ml[lr] - sMu[lr], ml[lr + 1] - sMu[lr + 1], ml[lr + 2] - sMu[lr + 2]};
                                win_running_innovation(cth, sth, ASLAM_WAVE_BCAST(rg02, fm - 1), ASLAM_WAVE_BCAST(rg12, fm - 1), d, ze0, ze1, ze2);
                            }
#pragma unroll
                            for (int c = 0; c < NC; c++) {
                                const double k0 = -sA[pb][0][lane + 64 * c], k1 = -sA[pb][1][lane + 64 * c], k2 = -sA[pb][2][lane + 64 * c];
                                mu[c] += k0 * ze0 + k1 * ze1 + k2 * ze2;
                            }
                        }
                    }
                }
                const int k = ++fk;
                const int slot = wd.first_slot + k;
                fm = ASLAM_WAVE_BCAST(sOff[k + 1] - sOff[k] - 1, 0); fa = 0;     // corrections of the frame
                // ---- predict (aruco_slam.cpp:35-73) with the final mean of the previous frame ----
                const double delta_sl = kl * (e_dt * e_wl), delta_sr = kr * (e_dt * e_wr);
                const double delta_theta = (delta_sr - delta_sl) * inv2b;
                const double delta_s = 0.5 * (delta_sr + delta_sl);
#pragma unroll
                for (int c = 0; c < NC; c++) sMu[lane + 64 * c] = mu[c];
                __builtin_amdgcn_wave_barrier();
                const double m0 = sMu[0], m1 = sMu[1], m2 = sMu[2];
#ifdef ASLAM_WIN_STAMPS
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (stamps only: the mean's round trip through LDS apart from the sincos)
                WSTAMP(8);
#endif
                double th = m2 + delta_theta;
                wrap1(th);
                // the two sincos of the frame in one call: even lanes the mid-step heading, odd lanes the new heading
                double sv, cv;
                sincos((lane & 1) ? th : m2 + 0.5 * delta_theta, &sv, &cv);
                const double cm = ASLAM_WAVE_BCAST(cv, 0), sm = ASLAM_WAVE_BCAST(sv, 0);
                cth = ASLAM_WAVE_BCAST(cv, 1); sth = ASLAM_WAVE_BCAST(sv, 1);
                WSTAMP(9);
                const double ua = -delta_s * sm, ub = delta_s * cm;                 // H3 = I + [ua ub 0]^T e2^T
                const double f = 0.5 * kl * e_dt;                                    // kl for BOTH wheels (quirk Q7)
                const double su0 = Qk * fabs(e_wl), su1 = Qk * fabs(e_wr);
                const double P22 = ASLAM_WAVE_BCAST(r[2][0], 2);
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    const int col = lane + 64 * c;
                    const double u = col == 0 ? ua : col == 1 ? ub : 0.0;
                    const double w0 = col == 0 ? f * cm : col == 1 ? f * sm : col == 2 ? f * invb : 0.0;        // wkh column 0
                    const double w1 = col == 0 ? f * cm : col == 1 ? f * sm : col == 2 ? f * -invb : 0.0;       // wkh column 1
                    A[0][c] = u;                       B[0][c] = r[2][c];
                    A[1][c] = fma(P22, u, r[2][c]);    B[1][c] = u;
                    A[2][c] = su0 * w0;                B[2][c] = w0;
                    A[3][c] = su1 * w1;                B[3][c] = w1;
                    sA[nb][3][col] = A[3][c]; sB[nb][3][col] = B[3][c];
                }
                if (nb) dirty1 = true; else dirty0 = true;
                const double np0 = m0 + delta_s * cm, np1 = m1 + delta_s * sm;
                if constexpr (LMU) {
                    // the predicted pose: to the logger's mean, by frame parity, and kept for a predict that follows at once
                    if (lane < 3) L.sPose[k & 1][lane] = lane == 0 ? np0 : lane == 1 ? np1 : th;
                    pn0 = np0; pn1 = np1; pth = th;
                } else {
                    if (lane == 0) mu[0] = np0;
                    if (lane == 1) mu[0] = np1;
                    if (lane == 2) mu[0] = th;
                    // RunningMean on this wave: mu_0 of the frame is this pose and the landmark means in sMu, which stays as it is
                    // until the next predict
                    if constexpr (IN::kOn) { pn0 = np0; pn1 = np1; pth = th; }
                }
                // ---- the frame's records at the frozen mean (pose just predicted, landmarks as the previous frame left them) ----
                if (lane < fm) {
                    vpos = sPos[sOff[k] + 1 + lane];
                    const int q = 3 + 3 * vpos;
                    const double mx = sMu[q], my = sMu[q + 1], mth = sMu[q + 2];
                    const double gdx = mx - np0, gdy = my - np1;
                    double gdth = mth - th;
                    wrap1(gdth);
                    const double zh0 = gdx * cth + gdy * sth, zh1 = -gdx * sth + gdy * cth;
                    double z2 = nObs.th - gdth;
                    wrap1(z2);
                    rze0 = nObs.x - zh0; rze1 = nObs.y - zh1; rze2 = z2;
                    rg02 = -gdx * sth + gdy * cth; rg12 = -gdx * cth - gdy * sth;
                    rR0 = nObs.r[0]; rR1 = nObs.r[1]; rR2 = nObs.r[2];
                    // what of them the log header carries, for the wave that stores it
                    auto& rec = L.sRec[k & 1];
                    rec[0][lane] = rze0; rec[1][lane] = rze1; rec[2][lane] = rze2; rec[3][lane] = rg02; rec[4][lane] = rg12;
                    if constexpr (LSI) { rec[5][lane] = rR0; rec[6][lane] = rR1; rec[7][lane] = rR2; }
                }
                __builtin_amdgcn_wave_barrier();
                WSTAMP(10);
                if constexpr (!ONE) {
                    // piece schedule: the window's last frame leaves its pop list behind here (one launch: the logger wave does)
                    if (wd.last && k == wd.K - 1) win_last_frame(E, frames[slot], obs + (size_t)slot * kMarkerMax, fm, lane);
                }
                // the next frame's inputs are fetched while this one is solved
                if (k + 1 < wd.K) {
                    const int fmn = sOff[k + 2] - sOff[k + 1] - 1;
                    if (lane < fmn) nObs = obs[(size_t)(slot + 1) * kMarkerMax + sDet[sOff[k + 1] + 1 + lane]];      // (index from LDS: one load level)
                    const double* e = enc + (size_t)3 * (slot + 1);
                    e_wl = e[0]; e_wr = e[1]; e_dt = e[2];
                }
                // header of the logged step: type 0, D's two entries, the frame's cos / sin (the corrections of the frame use them)
                if (lane == 0) { hdr[WH_TYPE] = 0.0; hdr[WH_POS] = -1.0; hdr[WH_A] = ua; hdr[WH_B] = ub; hdr[WH_C] = cth; hdr[WH_S] = sth; }
                WSTAMP(2);
            } else {
                // ---- correction a of the frame: c = H P, S = c H^T + R, Kt = S^-1 c ----
                const int a = fa++;
                double ze0 = ASLAM_WAVE_BCAST(rze0, a), ze1 = ASLAM_WAVE_BCAST(rze1, a), ze2 = ASLAM_WAVE_BCAST(rze2, a);   // (RunningMean on this wave: e from the verdict on)
                const double R0 = ASLAM_WAVE_BCAST(rR0, a), R1 = ASLAM_WAVE_BCAST(rR1, a), R2 = ASLAM_WAVE_BCAST(rR2, a);
                const double g02 = ASLAM_WAVE_BCAST(rg02, a), g12 = ASLAM_WAVE_BCAST(rg12, a);
                // Gxm = [ -c -s g02  c  s 0 ;  s -c g12 -s  c 0 ;  0 0 -1  0 0 1 ]   (aruco_slam.cpp:140-143)
                double cc[3][NC];
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    cc[0][c] = (-cth * r[0][c] - sth * r[1][c] + g02 * r[2][c]) + (cth * r[3][c] + sth * r[4][c]);
                    cc[1][c] = (sth * r[0][c] - cth * r[1][c] + g12 * r[2][c]) + (-sth * r[3][c] + cth * r[4][c]);
                    cc[2][c] = r[5][c] - r[2][c];
                    sB[nb][0][lane + 64 * c] = cc[0][c]; sB[nb][1][lane + 64 * c] = cc[1][c]; sB[nb][2][lane + 64 * c] = cc[2][c];   // (the B operand, in place)
                }
                __builtin_amdgcn_wave_barrier();
                WSTAMP(3);
                double Sm[9], Si[9];
#pragma unroll
                for (int kk = 0; kk < 3; kk++) {
                    const double p0 = sB[nb][kk][0], p1 = sB[nb][kk][1], p2 = sB[nb][kk][2];
                    const double l0 = sB[nb][kk][lrow], l1 = sB[nb][kk][lrow + 1], l2 = sB[nb][kk][lrow + 2];
                    Sm[kk * 3 + 0] = (-cth * p0 - sth * p1 + g02 * p2) + (cth * l0 + sth * l1);
                    Sm[kk * 3 + 1] = (sth * p0 - cth * p1 + g12 * p2) + (-sth * l0 + cth * l1);
                    Sm[kk * 3 + 2] = l2 - p2;
                }
                Sm[0] += R0; Sm[4] += R1; Sm[8] += R2;
                // S is inverted from one triangle.  P <- P - c^T S^-1 c keeps the antisymmetric part A of P only while S^-1 is symmetric: S
                // formed from the rows c = H P carries H A H^T, and through S^-1 every correction would add (K H) A (K H)^T to A.  With
                // gains of order one (R as small as the predicted H P H^T) that doubles A per correction in the observed directions: from
                // rounding to 1e-9 of max|P| within 150 frames.  inv3_fast of a symmetric S is symmetric bit for bit
                Sm[3] = Sm[1]; Sm[6] = Sm[2]; Sm[7] = Sm[5];
                inv3_fast(Sm, Si);
                // RunningMean on this wave: from here on the correction is judged by and applied with e = ze - H (mu_{a-1} - mu_0),
                // formed in place from this wave's own mean: six columns by wave-uniform cross-lane reads, less the frame's predicted pose
                // and the landmark means its predict left in sMu.  A rejected step left mu alone, so the next e does not see it.  ||ze||,
                // k_ekf_win_gate_finish's expression on the frozen-mean ze, is kept for the header
                if constexpr (IN::kOn && !LMU) {
                    const double d[6] = {ASLAM_WAVE_BCAST(mu[0], 0) - pn0, ASLAM_WAVE_BCAST(mu[0], 1) - pn1, ASLAM_WAVE_BCAST(mu[0], 2) - pth,
                                         bcast_sel<NC>(mu, lrow) - sMu[lrow], bcast_sel<NC>(mu, lrow + 1) - sMu[lrow + 1], bcast_sel<NC>(mu, lrow + 2) - sMu[lrow + 2]};
                    const double zn = sqrt(ze0 * ze0 + ze1 * ze1 + ze2 * ze2);
                    win_running_innovation(cth, sth, g02, g12, d, ze0, ze1, ze2);
                    if (lane == 0) { hdr[WH_ZE] = ze0; hdr[WH_ZE + 1] = ze1; hdr[WH_ZE + 2] = ze2; hdr[WH_ZN] = zn; }   // WH_ZE carries e: the replay's psi follows
                }
                // gated: the verdict on this correction, from the S^-1 just formed and the frame's frozen-mean innovation, or e (a NaN d2 rejects)
                double d2 = 0.0;
                bool rejected = false;
                if constexpr (G::kOn) {
                    d2 = slam_gate_d2(Si, ze0, ze1, ze2);
                    rejected = gate.gate_d2 < HUGE_VAL && !(d2 <= gate.gate_d2);
                }
                WSTAMP(4);
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    // K = (P H^T) S^-1, (P H^T) = c^T:  Kt[k][col] = sum_k' c[k'][col] Si[k'][k];  the A operand is -Kt
                    const double k0 = cc[0][c] * Si[0] + cc[1][c] * Si[3] + cc[2][c] * Si[6];
                    const double k1 = cc[0][c] * Si[1] + cc[1][c] * Si[4] + cc[2][c] * Si[7];
                    const double k2 = cc[0][c] * Si[2] + cc[1][c] * Si[5] + cc[2][c] * Si[8];
                    if constexpr (G::kOn) {
                        // a rejected step: no mean update (selected, not multiplied: its ze may be NaN) and zero A rows, so that the
                        // workers, the pose rows carried here and the logged operands all see a zero update
                        if constexpr (!LMU) {
                            const double dm = k0 * ze0 + k1 * ze1 + k2 * ze2;
                            mu[c] = rejected ? mu[c] : mu[c] + dm;
                        }
                        A[0][c] = rejected ? 0.0 : -k0; A[1][c] = rejected ? 0.0 : -k1; A[2][c] = rejected ? 0.0 : -k2; A[3][c] = 0.0;
                    } else {
                        if constexpr (!LMU) mu[c] += k0 * ze0 + k1 * ze1 + k2 * ze2;   // mu_ += K ze (aruco_slam.cpp:203)
                        A[0][c] = -k0; A[1][c] = -k1; A[2][c] = -k2; A[3][c] = 0.0;
                    }
                    B[0][c] = cc[0][c]; B[1][c] = cc[1][c]; B[2][c] = cc[2][c]; B[3][c] = 0.0;
                }
                if (nb ? dirty1 : dirty0) {                         // the buffer last held a predict's fourth depth row
#pragma unroll
                    for (int c = 0; c < NC; c++) { sA[nb][3][lane + 64 * c] = 0.0; sB[nb][3][lane + 64 * c] = 0.0; }
                    if (nb) dirty1 = false; else dirty0 = false;
                }
                // what the step brings to its log header: S^-1 (the wave that stores the header composes the rest: win_header_entry)
                // (LSI: the logger wave forms S^-1 itself; the gate's verdict needs it here all the same)
                if (lane == 0) {
                    if constexpr (!LSI) {
#pragma unroll
                        for (int q = 0; q < 9; q++) hdr[WH_SI + q] = Si[q];
                    }
                    if constexpr (G::kOn) { hdr[WH_TYPE] = rejected ? 2.0 : 1.0; hdr[WH_D2] = d2; hdr[WH_ACC] = rejected ? 0.0 : 1.0; }
                }
                prev_rejected = rejected;
                WSTAMP(5);
            }
            // operands to the workers and the logger wave (pieces: to the workers, who also log them), and this wave's own copy
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const int col = lane + 64 * c;
                sA[nb][0][col] = A[0][c]; sA[nb][1][col] = A[1][c]; sA[nb][2][col] = A[2][c];
                if (is_predict) { sB[nb][0][col] = B[0][c]; sB[nb][1][col] = B[1][c]; sB[nb][2][col] = B[2][c]; }
#pragma unroll
                for (int kk = 0; kk < 4; kk++) pB[kk][c] = B[kk][c];
            }
            prev_predict = is_predict;
            WSTAMP(6);
        }
        ASLAM_LDS_BARRIER();
    }
#ifdef ASLAM_WIN_STAMPS
    if (lane == 0 && (ONE || wd.piece == 1)) {
        const int nc = NS - n_pred;
        printf("prepare T %d steps %d (%d predict): barrier %lld | rows wait %lld correct %lld | predict path %lld (mean through LDS %lld sincos %lld operands + records %lld global loads, bookkeeping, header %lld) per predict | c %lld S+inv %lld Kt+hdr %lld per correction | operands+log %lld per step\n",
               T, NS, n_pred, stamp_acc[0] / (NS + 1), stamp_acc[7] / NS, stamp_acc[1] / NS, (stamp_acc[2] + stamp_acc[8] + stamp_acc[9] + stamp_acc[10]) / (n_pred ? n_pred : 1), stamp_acc[8] / (n_pred ? n_pred : 1),
               stamp_acc[9] / (n_pred ? n_pred : 1), stamp_acc[10] / (n_pred ? n_pred : 1), stamp_acc[2] / (n_pred ? n_pred : 1), stamp_acc[3] / (nc ? nc : 1), stamp_acc[4] / (nc ? nc : 1),
               stamp_acc[5] / (nc ? nc : 1), stamp_acc[6] / NS);
    }
#endif
#ifdef ASLAM_WIN_POSE_CHECK
    // the last comparison is of the rows as they stand after step NS - 2: the step before the piece's last
    if (lane == 0) printf("pose-check T %d piece %d steps %d: max |prepare - accumulator| pose rows %.3e over the piece, %.3e at its end\n", T, wd.piece, NS, dmax, dend);
#endif
    // ---- mu_S for the next piece; back into the state at the window's end (one-launch window: by k_ekf_win_fix) ----
    if constexpr (!LMU) {                                           // (LMU: the logger wave has it)
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const int col = lane + 64 * c;
            if (col < s) { muimg[col] = mu[c]; if (wd.mu_out) E.d_mu[sS[col]] = mu[c]; }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Replay of a piece's log on Lambda: workgroup b carries columns WBW b .. WBW b + WBW - 1 (all SP rows; in LDS) and its entries of psi.
// Per step: t = H Lambda (3 x WBW), Lambda += Aop^T t, psi += t^T (S^-1 ze); t and u = S^-1 t are logged for the Psi product.
// Two LDS barriers per step.  Wave 0 forms t (and then u, for the log) and is the only wave that stores, waves 1..3 are the only
// ones that load (the next step's record, one step ahead): no wave ever waits for its own stores to be acknowledged.
struct WinReplay { int piece, log0, nsteps, wpar; };              // the piece a replay role works on
template <int T> struct WinScanLds {
    static constexpr int SP = 16 * T, REC = 3 * SP + kWinHdr;
    double sLam[SP][WBW + 1];
    double sRec[2][REC];
    double sT[2][4][WBW];                  // t (row 3 stays zero)
};
// GATED: a step of type 2 (a correction the gate rejected) leaves Lambda and psi alone and logs t = u = 0, which adds nothing to Psi.
template <int T, bool ONE, bool GATED>
__device__ void win_scan_role(const EkfState& E, const WinReplay& wd, int b, unsigned epoch, int* sAvail, unsigned char* smem) {
    constexpr int SP = 16 * T, EPT = SP * WBW / 256, REC = 3 * SP + kWinHdr;
    constexpr int RPT = (REC + 191) / 192;                         // record doubles per loading thread
    WinScanLds<T>& L = *reinterpret_cast<WinScanLds<T>*>(smem);
    auto& sLam = L.sLam; auto& sRec = L.sRec; auto& sT = L.sT;
    if (threadIdx.x >= 256) return;
    const int nsteps = wd.nsteps;
    const int tid = threadIdx.x;
    const int ls = win_log_stride(T), ts = win_tlog_stride(T);
    double* Lam = E.d_win_small + wsm_LAM(E.win_sp_max, wd.wpar);
    double* psi = E.d_win_small + wsm_psi(E.win_sp_max, wd.wpar);
    for (int e = tid; e < SP * WBW; e += 256) {
        const int r = e / WBW, c = e % WBW;
        sLam[r][c] = wd.piece ? Lam[(size_t)r * SP + WBW * b + c] : (r == WBW * b + c ? 1.0 : 0.0);
    }
    double ps = (tid >= 4 * WBW && tid < 5 * WBW && wd.piece) ? psi[WBW * b + tid - 4 * WBW] : 0.0;     // (the thread that accumulates entry c: below)
    double cth = 1.0, sth = 0.0;
    const double* logp = E.d_win_log + (size_t)wd.log0 * ls;
    double* tlog = E.d_win_tlog + (size_t)wd.log0 * ts + WBW * b;
    const int lt = tid - 64;                                       // loading thread index (waves 1..3)
    // the log was written moments ago by another CU: a record takes longer to arrive than a step lasts, so the loading waves keep
    // PFD records in flight (registers), one per step of the unrolled loop
    constexpr int PFD = 3;
    double pf[PFD][RPT];
    for (int e = tid; e < 2 * 4 * WBW; e += 256) (&sT[0][0][0])[e] = 0.0;
    // one-launch window: the steps arrive in batches, as the chain publishes them (the piece schedule: one batch, the whole log)
    for (int done = 0; done < nsteps;) {
      int avail = nsteps;
      if constexpr (ONE) {
        if (tid == 0) {                                             // ONE lane polls, relaxed; ONE acquire per batch
            int got = win_count(E.d_win_sync, epoch);
            const unsigned long long t0 = wall_clock64();
            while (got <= done) {
                __builtin_amdgcn_s_sleep(2);
                got = win_count(E.d_win_sync, epoch);
                if (got <= done && wall_clock64() - t0 > kWinSpinTicks) { win_fail(E, 1u); got = -1; break; }
            }
            *sAvail = got;
            ASLAM_ACQUIRE_AGENT();
            ASLAM_VMCNT(0);                                         // (holds the barrier until the invalidate is done)
        }
        __syncthreads();
        avail = *sAvail;
        if (avail < 0) return;
      }
#pragma unroll
      for (int u = 0; u < PFD; u++)
#pragma unroll
        for (int q = 0; q < RPT; q++) { const int e = lt + 192 * q; pf[u][q] = (lt >= 0 && e < REC && done + u < avail) ? logp[(size_t)(done + u) * ls + e] : 0.0; }
      __syncthreads();
      for (int n0 = done; n0 < avail; n0 += PFD) {
#pragma unroll
      for (int u = 0; u < PFD; u++) {
        const int n = n0 + u;
        if (n >= avail) break;
        double* rec = sRec[n & 1];
        double (*tt)[WBW] = sT[n & 1];
        if (lt >= 0) {
#pragma unroll
            for (int q = 0; q < RPT; q++) { const int e = lt + 192 * q; if (e < REC) rec[e] = pf[u][q]; }
            if (n + PFD < avail) {                                  // in flight while the next PFD steps are applied
                const double* nx = logp + (size_t)(n + PFD) * ls;
#pragma unroll
                for (int q = 0; q < RPT; q++) { const int e = lt + 192 * q; pf[u][q] = e < REC ? nx[e] : 0.0; }
            }
        }
        ASLAM_LDS_BARRIER();
        const double* hd = rec + 3 * SP;
        const bool is_predict = hd[WH_TYPE] == 0.0;
        const bool skipped = GATED && hd[WH_TYPE] == 2.0;
        if (tid < WBW) {
            const int c = tid;
            if (GATED && skipped) { tt[0][c] = 0.0; tt[1][c] = 0.0; tt[2][c] = 0.0; }
            else if (is_predict) {
                // Lambda <- D Lambda (rows 0, 1 += (a, b) row 2); nothing for Psi / psi
                cth = hd[WH_C]; sth = hd[WH_S];                     // the frame's cos / sin (every piece starts with a predict)
                const double r2 = sLam[2][c];
                sLam[0][c] += hd[WH_A] * r2; sLam[1][c] += hd[WH_B] * r2;
                tt[0][c] = 0.0; tt[1][c] = 0.0; tt[2][c] = 0.0;
            } else {
                const int lrow = 3 + 3 * (int)hd[WH_POS];
                const double g02 = hd[WH_G02], g12 = hd[WH_G12];
                const double r0 = sLam[0][c], r1 = sLam[1][c], r2 = sLam[2][c], l0 = sLam[lrow][c], l1 = sLam[lrow + 1][c], l2 = sLam[lrow + 2][c];
                tt[0][c] = (-cth * r0 - sth * r1 + g02 * r2) + (cth * l0 + sth * l1);
                tt[1][c] = (sth * r0 - cth * r1 + g12 * r2) + (-sth * l0 + cth * l1);
                tt[2][c] = l2 - r2;
            }
        }
        ASLAM_LDS_BARRIER();
        if (tid < 8 * WBW) {
            // the step's log rows of this block (wave 0): t (rows 0..2, row 3 zero), u = S^-1 t (rows 4..6, row 7 zero); psi += t^T (S^-1 ze)
            const int row = tid / WBW, c = tid % WBW, k = row & 3;
            const double t0 = tt[0][c], t1 = tt[1][c], t2 = tt[2][c];
            double v = 0.0;
            if (!is_predict && !skipped && k < 3) {
                const double* Si = hd + WH_SI + 3 * k;
                v = row < 4 ? tt[k][c] : Si[0] * t0 + Si[1] * t1 + Si[2] * t2;     // (Z <- Z - (H Y)^T S^-1 (H Y))
                if (row == 4) {                                     // thread (4, c): the whole of psi's entry c
                    const double* S9 = hd + WH_SI;
                    const double z0 = hd[WH_ZE], z1 = hd[WH_ZE + 1], z2 = hd[WH_ZE + 2];
                    const double w0 = S9[0] * z0 + S9[1] * z1 + S9[2] * z2, w1 = S9[3] * z0 + S9[4] * z1 + S9[5] * z2, w2 = S9[6] * z0 + S9[7] * z1 + S9[8] * z2;
                    ps += t0 * w0 + t1 * w1 + t2 * w2;
                }
            }
            if (ONE) st_wt(tlog + (size_t)n * ts + row * SP + c, v);
            else tlog[(size_t)n * ts + row * SP + c] = v;
        }
        if (!is_predict && !skipped) {
            // Lambda[r][c] += sum_k Aop[k][r] t[k][c]      (c is the same for all of a thread's entries)
            const int c = tid % WBW;
            const double t0 = tt[0][c], t1 = tt[1][c], t2 = tt[2][c];
#pragma unroll
            for (int q = 0; q < EPT; q++) {
                const int r = (tid + 256 * q) / WBW;
                sLam[r][c] += rec[r] * t0 + rec[SP + r] * t1 + rec[2 * SP + r] * t2;
            }
        }
      }
      }
      if (ONE && tid < 64) {                                        // wave 0, the only one that stores t / u: its stores, then the count
          ASLAM_WAVE_LOCKSTEP();                                    // (every lane's stores of the batch, not only lane 0's)
          ASLAM_VMCNT(0);
          if (tid == 0) win_signal(E.d_win_sync + kWinSyncLine * (1 + b), epoch, avail);
      }
      done = avail;
    }
    __syncthreads();
    for (int e = tid; e < SP * WBW; e += 256) { const int r = e / WBW, c = e % WBW; Lam[(size_t)r * SP + WBW * b + c] = sLam[r][c]; }
    // psi's entry c was accumulated by thread (row 4, c) = tid 4 WBW + c
    if (tid >= 4 * WBW && tid < 5 * WBW) psi[WBW * b + tid - 4 * WBW] = ps;
}

// Psi (+)= sum over the piece's steps of t^T u on the f64 matrix cores: workgroup = tile row, wave w = tile columns w, w + 4, ...
// The operands come straight from the t / u log (L2): four steps are fetched ahead of the four products.
// (GATED only names the kernel the role belongs to: where the compiler keeps a role out of line, every step kernel has its own copy,
// and the ungated kernels' code does not depend on the gated instantiations beside them)
template <int T, bool ONE, bool GATED>
__device__ void win_psi_role(const EkfState& E, const WinReplay& wd, int tr, unsigned epoch, int* sAvail) {
    constexpr int SP = 16 * T, TW = (T + 3) / 4, UN = 4, NSCAN = SP / WBW;
    if (threadIdx.x >= 256) return;
    const int nsteps = wd.nsteps;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int ts = win_tlog_stride(T);
    double* Psi = E.d_win_small + wsm_PSI(E.win_sp_max, wd.wpar);
    const double* tlog = E.d_win_tlog + (size_t)wd.log0 * ts;
    v4d acc[TW];
#pragma unroll
    for (int q = 0; q < TW; q++) {
        const int tc = wave + 4 * q;
#pragma unroll
        for (int reg = 0; reg < 4; reg++)
            acc[q][reg] = (wd.piece && tc < T) ? Psi[(size_t)(16 * tr + lk + 4 * reg) * SP + 16 * tc + li] : 0.0;
    }
    // A[i][k] = t[k][16 tr + i] (lane k * 16 + i), B[k][j] = u[k][16 tc + j]
    for (int done = 0; done < nsteps;) {
      int avail = nsteps;
      if constexpr (ONE) {
        // one-launch window: wave 0 polls the replay workgroups' counts (lane b: workgroup b), relaxed; ONE acquire per batch
        if (wave == 0) {
            const unsigned long long t0 = wall_clock64();
            int got;
            for (;;) {
                got = lane < NSCAN ? win_count(E.d_win_sync + kWinSyncLine * (1 + lane), epoch) : nsteps;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) got = min(got, __shfl_xor(got, d));
                if (got > done) break;
                const int late = __shfl(wall_clock64() - t0 > kWinSpinTicks ? 1 : 0, 0);      // (lane 0 decides for the wave)
                if (late) { if (lane == 0) win_fail(E, 2u); got = -1; break; }
                __builtin_amdgcn_s_sleep(2);
            }
            if (lane == 0) { *sAvail = got; ASLAM_ACQUIRE_AGENT(); ASLAM_VMCNT(0); }
        }
        __syncthreads();
        avail = *sAvail;
        __syncthreads();                                            // (every wave has read it before wave 0 polls again)
        if (avail < 0) return;
      }
    for (int n0 = done; n0 < avail; n0 += UN) {
        double a[UN], bv[UN][TW];
#pragma unroll
        for (int u = 0; u < UN; u++) {
            const bool ok = n0 + u < avail;
            const double* st = tlog + (size_t)(ok ? n0 + u : n0) * ts;
            a[u] = ok ? st[lk * SP + 16 * tr + li] : 0.0;
#pragma unroll
            for (int q = 0; q < TW; q++) { const int tc = wave + 4 * q; bv[u][q] = tc < T ? st[(4 + lk) * SP + 16 * tc + li] : 0.0; }
        }
#pragma unroll
        for (int u = 0; u < UN; u++)
#pragma unroll
            for (int q = 0; q < TW; q++) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], bv[u][q], acc[q], 0, 0, 0);
    }
      done = avail;
    }
#pragma unroll
    for (int q = 0; q < TW; q++) {
        const int tc = wave + 4 * q;
        if (tc < T) {
#pragma unroll
            for (int reg = 0; reg < 4; reg++) Psi[(size_t)(16 * tr + lk + 4 * reg) * SP + 16 * tc + li] = acc[q][reg];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// One launch = the chain of piece i (workgroup 0), the replay of piece i - 1 on Lambda (the next SP / 8 workgroups) and the Psi
// product of piece i - 2 (the last T workgroups).  The three depend on each other only through the PREVIOUS launch (the log of
// piece i - 1 is complete when this launch starts: same stream), so no events are needed between the pieces of a window and the
// replay is hidden behind the chain: with one event per piece the EKF alone ran 14 % slower (cfg2).
//
// ONE = true: one launch = a whole window (wd.K frames, wd.nsteps steps), the same three roles running side by side.  The chain
// publishes its step count every kWinPubEvery steps; each replay workgroup replays the published steps in batches and publishes
// its own count; each Psi workgroup takes the steps every replay workgroup has published.  Publication: the log and the t / u log
// are stored write-through (sc1); each storing wave waits for its stores of the published steps (a counted vmcnt: the chain's
// logger wave, the only wave of the chain that stores to the log, issues no global load in the step loop, so the count is static
// and covers only the newest steps, which are not waited for), then passes the step's barrier, and one of its lanes stores
// {epoch, count} with a relaxed agent-scope store.  A
// consumer polls with one lane (relaxed sc1 loads, s_sleep between polls), then makes ONE agent acquire, waits for it and passes
// a barrier before its waves load the batch.  The counters carry the window's epoch (an older window's count reads as 0), so
// nothing is reset between windows.  Forward progress: roles go by a ticket each workgroup takes when it starts (a CAS on an
// epoch-tagged word: first = chain, then the replay workgroups, then Psi), not by blockIdx, and every wait is on a role with a
// smaller ticket, i.e. on a workgroup that is already running.  Neither dispatch order nor co-residency of the whole grid is
// assumed (at T = 12 the 37 workgroups need not all be resident).  Every spin gives up after kWinSpinTicks without progress:
// the workgroup writes a code into E.d_win_err (the first code stays; read back with the call's counters) and leaves.
__device__ __forceinline__ int win_ticket(unsigned long long* w, unsigned epoch) {
    unsigned long long old = __hip_atomic_load((aslam_gu64*)w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        const bool cur = (unsigned)(old >> 32) == epoch;
        const unsigned long long nw = cur ? old + 1 : ((unsigned long long)epoch << 32) | 1u;
        const unsigned long long prev = atomicCAS(w, old, nw);
        if (prev == old) return cur ? (int)(unsigned)old : 0;
        old = prev;
    }
}
// the step kernel's block: the chain role's waves (ceil(T / RW) workers, the prepare wave, in a one-launch window the logger wave), and
// no fewer than the 256 threads the replay roles use
constexpr int win_step_threads(int T, int RW, bool ONE) {
    const int chain = ((T + RW - 1) / RW + (ONE ? 2 : 1)) * 64;
    return chain > 256 ? chain : 256;
}
template <int T, int RW, bool ONE, class G = NoSlamGate, int LG = 0, int WP = 0, class IN = FrozenMean>
__global__ __launch_bounds__(win_step_threads(T, RW, ONE))
void k_ekf_win_step(EkfState E, SlamParams sp, WinArg<G> wa, WinReplay rs, WinReplay rq, const ObsRaw* __restrict__ obs, const double* __restrict__ enc) {
    const WinDesc& wd = wa;
    constexpr size_t kLds = sizeof(WinChainLds<T, ONE>) > sizeof(WinScanLds<T>) ? sizeof(WinChainLds<T, ONE>) : sizeof(WinScanLds<T>);
    __shared__ __align__(16) unsigned char smem[kLds];
    __shared__ int sTicket, sAvail;
    constexpr int NSCAN = 16 * T / WBW;
    int bx = blockIdx.x;
    if constexpr (ONE) {
        if (threadIdx.x == 0) sTicket = win_ticket(E.d_win_sync + (size_t)kWinSyncLine * (kWinSyncCounters - 1), wd.epoch);
        __syncthreads();
        bx = sTicket;
    }
    if (bx == 0) { if (wd.K > 0) win_chain_role<T, RW, ONE, G, LG, WP, IN>(E, sp, wd, static_cast<const G&>(wa), obs, enc, smem); }
    else if (bx <= NSCAN) { if (rs.nsteps > 0) win_scan_role<T, ONE, G::kOn>(E, rs, bx - 1, wd.epoch, &sAvail, smem); }
    else if (rq.nsteps > 0) win_psi_role<T, ONE, G::kOn>(E, rq, bx - 1 - NSCAN, wd.epoch, &sAvail);
}

// ---------------------------------------------------------------------------------------------------------------------
// Behind a gated window's step launch, on the same stream: the bookkeeping k_ekf_gate_finish does behind a gated per-frame solve,
// for all K frames of the window at once.  One workgroup; wave w takes frames w, w + 16, ..., lane a = correction a of the frame
// (the corrections are the frame's action-1 pops, in pop order).  d2, the verdict and ze of correction a are in the header of step
// off_k + 1 + a of the window's log, which nothing overwrites before the next window's launch on this stream.  Per frame: lane 0 walks
// the corrections once in pop order (the slot record of §19 / §24, entry [2] of the slot stats = the accepted count).  Then thread 0
// carries the filter's track record through the K frames in order (the integer streak rule), and wave 0 turns the rejected pops of
// the window's LAST frame into action 3 and takes them out of the last-observed list the chain left behind (win_last_frame), so
// that a device-planned frame that follows sees the exact list.  Fixed orders throughout, no floating-point atomics.
// ZN (the gated consistent window): WH_ZE carries e there, which d2 and the verdict were formed from, and ref_flagged stays
// the reference's test on the frozen-mean ze: its norm, formed by the prepare wave with the expression below, is read from WH_ZN.
constexpr int kWinFinishThreads = 1024;
template <bool ZN>
__device__ __forceinline__ void win_gate_finish(const EkfState& E, const WinDesc& wd, const GateState& gs, const ObsRaw* __restrict__ obs) {
    constexpr int NW = kWinFinishThreads / 64;
    __shared__ double sD2[NW][64];
    __shared__ int sKind[NW][64], sFlag[NW][64], sId[NW][64];   // kind 1: accepted, 2: rejected
    __shared__ int sOff[kWinFrames + 1], sAtt[kWinFrames], sAcc[kWinFrames];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int K = min(wd.K, kWinFrames);
    const WinFrame* __restrict__ frames = E.d_win_frames + wd.first_slot;
    const int ls = win_log_stride(wd.T), SP = 16 * wd.T;
    const double* __restrict__ hdr0 = E.d_win_log + (size_t)wd.log0 * ls + 3 * SP;   // header of the window's step 0
    if (wave == 0) {                                                // step offset of every frame: 1 predict + m corrections each
        int inc = lane < K ? 1 + frames[lane].m : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(inc, d); if (lane >= d) inc += y; }
        sOff[lane + 1] = inc;
        if (lane == 0) sOff[0] = 0;
    }
    __syncthreads();
    for (int k = wave; k < K; k += NW) {
        const int slot = wd.first_slot + k;
        const WinFrame& fr = frames[k];
        const int m = min(fr.m, kWinCorrMax);
        if (lane < m) {
            const double* hd = hdr0 + (size_t)(sOff[k] + 1 + lane) * ls;
            sD2[wave][lane] = hd[WH_D2];
            sKind[wave][lane] = hd[WH_ACC] == 0.0 ? 2 : 1;
            if constexpr (ZN) sFlag[wave][lane] = hd[WH_ZN] >= 1.0 ? 1 : 0;
            else {
                const double z0 = hd[WH_ZE], z1 = hd[WH_ZE + 1], z2 = hd[WH_ZE + 2];
                sFlag[wave][lane] = sqrt(z0 * z0 + z1 * z1 + z2 * z2) >= 1.0 ? 1 : 0;   // the ||ze|| half of aruco_slam.cpp:156 (the chains never form K)
            }
            sId[wave][lane] = obs[(size_t)slot * kMarkerMax + fr.cdet[lane]].id;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            int acc = 0, nrej = 0, flag = 0, worst = -1;
            double nis = 0.0, mx = 0.0;
            bool have = false;
            for (int a = 0; a < m; a++) {                           // pop order
                const double d2 = sD2[wave][a];
                flag += sFlag[wave][a];
                if (d2 == d2 && (!have || d2 > mx)) { have = true; mx = d2; worst = sId[wave][a]; }
                if (sKind[wave][a] == 2) nrej++;
                else { acc++; nis += d2; }
            }
            if (slot >= 0 && slot < E.max_slots) {
                E.d_slot_stat[4 * slot + 2] = acc;                  // corrections fused: the accepted ones (the chain wrote the planned count)
                SlotHealth* h = gs.slot + slot;
                h->attempted = m; h->accepted = acc; h->rejected = nrej; h->ref_flagged = flag;
                h->nis_sum = nis; h->d2_max = mx; h->worst_id = worst; h->pad = 0;
            }
            sAtt[k] = m; sAcc[k] = acc;
        }
        __builtin_amdgcn_wave_barrier();                            // (the wave's next frame rewrites the arrays)
    }
    __syncthreads();
    if (tid == 0 && K > 0) {                                        // the track record, frame by frame
        TrackHealth* t = gs.track + kTrackSingle;
        int streak = t->bad_streak, acc_total = t->accepted_total, rej_total = t->rejected_total;
        for (int k = 0; k < K; k++) {
            const int att = sAtt[k], acc = sAcc[k];
            if (att >= gs.min_attempted) streak = 100 * acc < gs.min_accept_percent * att ? streak + 1 : 0;
            acc_total += acc; rej_total += att - acc;
        }
        t->frames = t->frames + K;
        t->accepted_total = acc_total;
        t->rejected_total = rej_total;
        t->bad_streak = streak;
        t->lost = streak >= gs.lost_after ? 1 : 0;
        t->pad[0] = t->pad[1] = t->pad[2] = 0;
    }
    if (wave == 1 && K > 0) {                                       // the last frame's pop list and last-observed list (npop <= 64: one wave)
        const WinFrame& fr = frames[K - 1];
        const int np = min(fr.npop, 64);
        const bool upd = lane < np && fr.pact[lane] == 1;
        const unsigned long long bU = __ballot(upd);
        bool rej = false;
        if (upd) {
            const int a = __popcll(bU & ((1ull << lane) - 1ull));   // the correction this pop is
            rej = a < kWinCorrMax && hdr0[(size_t)(sOff[K - 1] + 1 + a) * ls + WH_ACC] == 0.0;
        }
        LastObs lo{};
        if (lane < np) lo = E.d_last[lane];
        const bool keep = lane < np && !rej;
        const unsigned long long bK = __ballot(keep);               // (every lane holds its entry of d_last before any is rewritten)
        if (rej) E.d_pop[lane].action = 3;
        if (keep) E.d_last[__popcll(bK & ((1ull << lane) - 1ull))] = lo;
        if (lane == 0) *E.d_nlast = __popcll(bK);
    }
}
__global__ __launch_bounds__(kWinFinishThreads) void k_ekf_win_gate_finish(EkfState E, WinDesc wd, GateState gs, const ObsRaw* __restrict__ obs) {
    win_gate_finish<false>(E, wd, gs, obs);
}
__global__ __launch_bounds__(kWinFinishThreads) void k_ekf_win_gate_finish_zn(EkfState E, WinDesc wd, GateState gs, const ObsRaw* __restrict__ obs) {
    win_gate_finish<true>(E, wd, gs, obs);
}

// ---------------------------------------------------------------------------------------------------------------------
// U = Psi Y_0 -> d_T and Y_K = Lambda Y_0 -> d_V (both SP x N) as ONE product [Psi; Lambda] (2 SP x SP) . Y_0 (SP x N) on the matrix
// cores: workgroup (x, y) = 64 columns of Sigma x 64 rows of the stacked matrix, depth in chunks of 64 staged through LDS (both
// operands, coalesced), wave w = 16 of the columns x all 64 rows.  Workgroups with y = 0 also add Y_0^T psi to their 64 entries
// of mu_R.
template <int T>
__global__ __launch_bounds__(256) void k_ekf_win_thin(EkfState E, WinDesc wd) {
    constexpr int SP = 16 * T, YS = 66;
    __shared__ double sY[64 * YS];                                  // Y_0 chunk: [depth][column]
    __shared__ double sM[64 * YS];                                  // Psi / Lambda chunk: [row][depth]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int ld = E.ld;
    const int N = 3 + 3 * (*E.d_L);
    const int c0 = blockIdx.x * 64;
    if (c0 >= N) return;
    const int r0 = blockIdx.y * 64;                                 // row of the stacked matrix
    const bool lam = r0 >= SP;
    const int s = 3 + 3 * wd.nS;
    const double* M = E.d_win_small + (lam ? wsm_LAM(E.win_sp_max, wd.wpar) : wsm_PSI(E.win_sp_max, wd.wpar)) + (size_t)(lam ? r0 - SP : r0) * SP;
    const double* psi = E.d_win_small + wsm_psi(E.win_sp_max, wd.wpar);
    double* out = lam ? E.d_V : E.d_T;
    const int orow = lam ? r0 - SP : r0;
    v4d acc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) acc[q] = v4d{0.0, 0.0, 0.0, 0.0};
    double macc = 0.0;
    for (int ch = 0; ch < SP / 64; ch++) {
        if (ch) __syncthreads();
        for (int e = tid; e < 64 * 64; e += 256) {
            const int p = e >> 6, x = e & 63;
            sY[p * YS + x] = c0 + x < N ? E.d_Wt[(size_t)(64 * ch + p) * ld + c0 + x] : 0.0;
            sM[p * YS + x] = M[(size_t)p * SP + 64 * ch + x];
        }
        __syncthreads();
        for (int p0 = 0; p0 < 64; p0 += 4) {
            const double bv = sY[(p0 + lk) * YS + 16 * wave + li];
#pragma unroll
            for (int q = 0; q < 4; q++) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(sM[(16 * q + li) * YS + p0 + lk], bv, acc[q], 0, 0, 0);
        }
        if (blockIdx.y == 0 && tid < 64)
            for (int p = 0; p < 64 && 64 * ch + p < s; p++) macc += sY[p * YS + tid] * psi[64 * ch + p];
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int p = orow + 16 * q + lk + 4 * reg, c = c0 + 16 * wave + li;
            if (c < N) out[(size_t)p * ld + c] = acc[q][reg];
        }
    if (blockIdx.y == 0 && tid < 64 && c0 + tid < N && E.d_win_sidx[c0 + tid] < 0) E.d_mu[c0 + tid] += macc;      // mu_R += Y_0^T psi
}

// Rows and columns S of Sigma after the Z pass: row S_p <- Y_K[p][:], column S_p <- the same (symmetry), (S_p, S_q) <- P_K[p][q];
// mu_S back into the state (behind the previous window's flush: same stream).
__global__ __launch_bounds__(256) void k_ekf_win_fix(EkfState E, WinDesc wd, int SP) {
    const int ld = E.ld;
    const int N = 3 + 3 * (*E.d_L);
    const int s = 3 + 3 * wd.nS;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= N) return;
    const int tp = E.d_win_sidx[t];
    const double* Pimg = E.d_win_small + wsm_P(E.win_sp_max, wd.wpar);
    if (blockIdx.y == 0 && t < s) E.d_mu[win_state_index(wd, t)] = E.d_win_small[wsm_MU(E.win_sp_max, wd.wpar) + t];   // mu_S as the chain left it
    for (int p = blockIdx.y; p < s; p += gridDim.y) {
        const int Sp = win_state_index(wd, p);
        const double v = tp >= 0 ? Pimg[(size_t)p * SP + tp] : E.d_V[(size_t)p * ld + t];
        E.d_sigma[(size_t)Sp * ld + t] = v;                        // column S_p, row t (coalesced)
        if (tp < 0) E.d_sigma[(size_t)t * ld + Sp] = v;            // row S_p, column t
    }
}

// Y_0 (row p = row S_p of Sigma = its column S_p) -> d_Wt (rows s .. SP - 1 zero), position table of S.
__global__ __launch_bounds__(256) void k_ekf_win_gather(EkfState E, WinDesc wd) {
    const int ld = E.ld, nS = wd.nS, s = 3 + 3 * nS, SP = 16 * wd.T;
    const int N = 3 + 3 * (*E.d_L);
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= N) return;
    int pos = -1;
    if (t < 3) pos = t;
    else {
        const int base = (t - 3) / 3 * 3 + 3;
        for (int a = 0; a < nS; a++) if (wd.li[a] == base) pos = 3 + 3 * a + (t - base);
    }
    if (blockIdx.y == 0) E.d_win_sidx[t] = pos;
    for (int p = blockIdx.y; p < SP; p += gridDim.y) E.d_Wt[(size_t)p * ld + t] = p < s ? E.d_sigma[(size_t)win_state_index(wd, p) * ld + t] : 0.0;
}

// ---- early start of the next window -----------------------------------------------------------------------------------
// The chain of the window that follows needs only P' = Sigma[S', S'] and mu_S' as they will stand AFTER the previous window's
// flush; both follow from the previous window's small results without the pass over Sigma:
//     (a, b in S)      P_K                 (a in S, b not)   (Lambda Y_0)[a][b]            (neither)   Sigma_old[a][b] - (Y_0^T Psi Y_0)[a][b]
//     mu: in S as the chain left it, otherwise mu_old + Y_0^T psi.
// The flush of the previous window runs meanwhile.  k_ekf_win_next (below) does it in one launch.  The four-launch form it replaced
// stays as the comparison path (ASLAM_WIN_NEXT_SPLIT): k_ekf_win_next_gather collects Y_0's columns S' (Vg, zero where the entry
// is in S), Sigma_old[S', S'] and mu_old[S'] into small dense buffers with the index tables a miniature EkfState view needs;
// k_ekf_win_thin and k_ekf_update_mfma then run on that view (N := s'), and k_ekf_win_next_fix assembles the image the chain loads.
__global__ __launch_bounds__(256) void k_ekf_win_next_gather(EkfState E, WinDesc pv, WinDesc nx) {
    const int ld = E.ld, SPm = E.win_sp_max;
    const int s2 = 3 + 3 * nx.nS, SPp = 16 * pv.T;
    double* Vg = E.d_win_next;                                      // [p][a'] row stride SPm
    double* Ptmp = E.d_win_next + (size_t)3 * SPm * SPm;            // column-major, ld SPm
    double* mu2 = E.d_win_small + wsm_MU(SPm, nx.wpar);
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= s2) return;
    const int ia = win_state_index(nx, a);
    const int pa = E.d_win_sidx[ia];
    if (blockIdx.y == 0) {
        E.d_win_next_idx[a] = pa;
        if (a == 0) E.d_win_next_idx[SPm] = nx.nS;
        mu2[a] = pa >= 0 ? E.d_win_small[wsm_MU(SPm, pv.wpar) + pa] : E.d_mu[ia];     // in S: as the chain left it (its image)
    }
    for (int p = blockIdx.y; p < SPp; p += gridDim.y) Vg[(size_t)p * SPm + a] = pa < 0 ? E.d_Wt[(size_t)p * ld + ia] : 0.0;
    for (int b = blockIdx.y; b < s2; b += gridDim.y) Ptmp[(size_t)b * SPm + a] = E.d_sigma[(size_t)win_state_index(nx, b) * ld + ia];
}
__global__ __launch_bounds__(256) void k_ekf_win_next_fix(EkfState E, WinDesc pv, WinDesc nx) {
    const int SPm = E.win_sp_max, SPp = 16 * pv.T, SPn = 16 * nx.T;
    const int s2 = 3 + 3 * nx.nS;
    const double* Lg = E.d_win_next + (size_t)2 * SPm * SPm;        // (Lambda Vg)[p][a']
    const double* Ptmp = E.d_win_next + (size_t)3 * SPm * SPm;
    const double* Pprev = E.d_win_small + wsm_P(SPm, pv.wpar);
    double* Pout = E.d_win_small + wsm_P(SPm, nx.wpar);
    const int b = blockIdx.x * 256 + threadIdx.x;                   // column of the image (fastest)
    if (b >= SPn) return;
    const int pb = b < s2 ? E.d_win_next_idx[b] : -1;
    for (int a = blockIdx.y; a < SPn; a += gridDim.y) {
        double v = 0.0;
        if (a < s2 && b < s2) {
            const int pa = E.d_win_next_idx[a];
            v = pa >= 0 && pb >= 0 ? Pprev[(size_t)pa * SPp + pb] : pa >= 0 ? Lg[(size_t)pa * SPm + b] : pb >= 0 ? Lg[(size_t)pb * SPm + a] : Ptmp[(size_t)b * SPm + a];
        }
        Pout[(size_t)a * SPn + b] = v;
    }
}

// The same in ONE launch (the default; the four launches above stay behind ASLAM_WIN_NEXT_SPLIT for comparison): their 40 us were
// launch floor and the gaps between dependent kernels, not work.  Workgroup t owns columns 16 t .. 16 t + 15 of S' and depends on
// no other workgroup: it gathers its columns of Vg into LDS, forms (Psi Vg) and (Lambda Vg) for them, then
// Sigma_old[S', tile] - Vg^T (Psi Vg)[:, tile] with the whole of Vg as the other operand, and writes
//     every entry of its image columns but those with the row outside S and the column inside: such an entry is the mirror of
//     (Lambda Vg)[a][b], a in S, b outside, and is written with it by the tile that owns b.
// Every entry goes through the matrix-core sequence it had in the four launches (k_ekf_win_thin: accumulator from zero, depth
// ascending in fours; k_ekf_update_mfma: accumulator from Sigma_old, the (Psi Vg) operand negated; mu: multiply, then add, by
// ascending depth), so the image is the same to the bit.  The operands that come from global memory (Psi, Lambda; Vg's other
// columns) are read by the lane that feeds them to the matrix core: at 16 columns per workgroup a staging pass through LDS would
// only add barriers, and with none in the depth loops the compiler keeps several groups of loads in flight.
constexpr int kWinNextSP = 16 * 12;                                 // the widest window
__global__ __launch_bounds__(256) void k_ekf_win_next(EkfState E, WinDesc pv, WinDesc nx) {
    __shared__ double sVt[kWinNextSP][16];                          // Vg[:, tile]
    __shared__ double sTt[kWinNextSP][16];                          // (Psi Vg)[:, tile]
    __shared__ int sIa[kWinNextSP], sPa[kWinNextSP], sInv[kWinNextSP];   // of position a of S': state offset; position in S, -1 outside, -2 padding; of position p of S: its position in S' or -1
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int ld = E.ld, SPm = E.win_sp_max;
    const int Tp = pv.T, Tn = nx.T, SPp = 16 * Tp, SPn = 16 * Tn;
    const int s1 = 3 + 3 * pv.nS, s2 = 3 + 3 * nx.nS;
    const int c0 = 16 * blockIdx.x;
    const double* Pprev = E.d_win_small + wsm_P(SPm, pv.wpar);
    double* Pout = E.d_win_small + wsm_P(SPm, nx.wpar);
    if (tid < kWinNextSP) sInv[tid] = -1;
    __syncthreads();
    if (tid < SPn) {
        const int ia = tid < s2 ? win_state_index(nx, tid) : 0;
        const int pa = tid < s2 ? E.d_win_sidx[ia] : -2;
        sIa[tid] = ia; sPa[tid] = pa;
        if (pa >= 0) sInv[pa] = tid;
    }
    __syncthreads();
    for (int e = tid; e < 16 * SPp; e += 256) {
        const int p = e >> 4, a = c0 + (e & 15);
        sVt[p][e & 15] = sPa[a] == -1 ? E.d_Wt[(size_t)p * ld + sIa[a]] : 0.0;
    }
    // the image columns' entries that need no product: zero in the padding, P_K where row and column are both in S
    for (int e = tid; e < 16 * SPn; e += 256) {
        const int a = e >> 4, b = c0 + (e & 15);
        const int pa = sPa[a], pb = sPa[b];
        if (pa == -2 || pb == -2) Pout[(size_t)a * SPn + b] = 0.0;
        else if (pa >= 0 && pb >= 0) Pout[(size_t)a * SPn + b] = Pprev[(size_t)pa * SPp + pb];
    }
    __syncthreads();
    // [Psi; Lambda] Vg[:, tile]: the 2 Tp row tiles in turn over the waves
    for (int rt = wave; rt < 2 * Tp; rt += 4) {
        const bool lam = rt >= Tp;
        const int q = lam ? rt - Tp : rt;
        const double* M = E.d_win_small + (lam ? wsm_LAM(SPm, pv.wpar) : wsm_PSI(SPm, pv.wpar)) + (size_t)(16 * q + li) * SPp + lk;
        v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
        for (int pc = 0; pc < SPp; pc += 64) {                      // (SPp is a multiple of 64: sixteen groups' loads in flight at once)
            double av[16];
#pragma unroll
            for (int g = 0; g < 16; g++) av[g] = M[pc + 4 * g];
#pragma unroll
            for (int g = 0; g < 16; g++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[g], sVt[pc + 4 * g + lk][li], acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int p = 16 * q + lk + 4 * reg;
            if (!lam) sTt[p][li] = acc[reg];
            else {
                const int a = sInv[p], b = c0 + li;                 // (Lambda Vg)[p][b]: image entry (a, b) and its mirror
                if (a >= 0 && sPa[b] == -1) { Pout[(size_t)a * SPn + b] = acc[reg]; Pout[(size_t)b * SPn + a] = acc[reg]; }
            }
        }
    }
    // mu_S': in S as the chain left it (its image), otherwise mu_old + Y_0^T psi
    if (wave == 3 && lane < 16 && c0 + lane < s2) {
        const int a = c0 + lane, pa = sPa[a];
        double v;
        if (pa >= 0) v = E.d_win_small[wsm_MU(SPm, pv.wpar) + pa];
        else {
            const double* psi = E.d_win_small + wsm_psi(SPm, pv.wpar);
            double macc = 0.0;
            for (int p = 0; p < s1; p++) macc += sVt[p][lane] * psi[p];
            v = E.d_mu[sIa[a]] + macc;
        }
        E.d_win_small[wsm_MU(SPm, nx.wpar) + a] = v;
    }
    __syncthreads();
    // Sigma_old[S', tile] - Vg^T (Psi Vg)[:, tile], formed transposed as k_ekf_update_mfma does: D'[c][r], c in the tile
    for (int ri = wave; ri < Tn; ri += 4) {
        const int r = 16 * ri + li;
        const int pr = sPa[r];
        const double* W = E.d_Wt + (size_t)lk * ld + sIa[r];
        v4d acc;
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int c = c0 + lk + 4 * reg;
            acc[reg] = (c < s2 && r < s2) ? E.d_sigma[(size_t)sIa[c] * ld + sIa[r]] : 0.0;
        }
        for (int pc = 0; pc < SPp; pc += 64) {
            double bv[16];
#pragma unroll
            for (int g = 0; g < 16; g++) bv[g] = W[(size_t)(pc + 4 * g) * ld];     // (a valid address whatever r is; used where r lies outside S)
#pragma unroll
            for (int g = 0; g < 16; g++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-sTt[pc + 4 * g + lk][li], pr == -1 ? bv[g] : 0.0, acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int c = c0 + lk + 4 * reg;
            if (pr == -1 && sPa[c] == -1) Pout[(size_t)r * SPn + c] = acc[reg];
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
// a window's run-time width (4, 8 or 12 blocks of 16 columns) as a compile-time one: f(std::integral_constant<int, T>{})
template <class F> static void with_win_width(int T, F&& f) {
    if (T == 4) f(std::integral_constant<int, 4>{});
    else if (T == 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 12>{});
}
// Every workgroup of a step launch asks for more than half of a CU's LDS (an unused dynamic allocation on top of the static one), so
// that no second workgroup - a replay workgroup of the same launch, or anything else - is placed on the chain workgroup's CU and
// competes with the prepare wave for issue slots and LDS bandwidth (ASLAM_WIN_SHARE_CU: off, for comparison).  The claim is no
// larger than that needs: at SP = 64 the one-launch window leaves 70 388 of the CU's 163 840 bytes, which a k_ekf_win_thin workgroup
// of the previous window's flush (67 584 bytes) still finds when detection fills every other CU; with 4 KB less room the flush
// waited for up to a whole window (measured: DESIGN.md).  The chain role's block has grown by kGrown bytes since (the header records);
// the dynamic part gives them back, so that static + dynamic is what it was measured at.
template <int T, bool ONE, int LG = 0, int WP = 0, class IN = FrozenMean, class K, class W> static void launch_step_kernel(K kernel, hipStream_t st, int nb, int nt, size_t static_lds, const EkfState& E, const SlamParams& sp,
                                                const W& wd, const WinReplay& rs, const WinReplay& rq, const ObsRaw* obs, const double* enc) {
    static const bool share = std::getenv("ASLAM_WIN_SHARE_CU") != nullptr;
    constexpr size_t cap = (size_t)24 * 1024 + WinChainLds<T, ONE>::kGrown;
    const size_t dyn = share ? 0 : (size_t)84 * 1024 - std::min(static_lds, cap);                    // static + dynamic > 80 KB of the 160 KB
    static bool attr_done = false;                                 // (per instantiation: LG, WP and IN tell kernels of one signature apart)
    if (!attr_done && dyn > 0) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
        attr_done = true;
    }
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(nt), dyn, st, E, sp, wd, rs, rq, obs, enc);
}
// wp: how the workers publish (win_chain_role's WP, bits of kWinWorkerPublishAll; 0 = the comparison path; negative: the width's default)
#define ASLAM_WP_FORMS(F) F(0) F(1) F(2) F(3)
template <int T> static void launch_win_pieces_wp(hipStream_t st, int nb, int wp, const EkfState& E, const SlamParams& sp, const WinArg<NoSlamGate>& wa, const WinReplay& rs,
                                                          const WinReplay& rq, const ObsRaw* obs, const double* enc) {
    constexpr size_t lds = sizeof(WinChainLds<T, false>);
    switch (wp < 0 ? win_worker_publish_default(T) : wp & kWinWorkerPublishAll) {
#define ASLAM_WP_LAUNCH(i) case i: launch_step_kernel<T, false, 0, i>(k_ekf_win_step<T, 2, false, NoSlamGate, 0, i>, st, nb, win_step_threads(T, 2, false), lds, E, sp, wa, rs, rq, obs, enc); break;
        ASLAM_WP_FORMS(ASLAM_WP_LAUNCH)
#undef ASLAM_WP_LAUNCH
    }
}
void launch_ekf_win_step(hipStream_t st, const EkfState& E, const SlamParams& sp, const WinDesc& wd, const ObsRaw* obs, const double* enc,
                         int s_piece, int s_log0, int s_nsteps, int q_piece, int q_log0, int q_nsteps, int worker_publish) {
    const WinReplay rs{s_piece, s_log0, s_nsteps, wd.wpar}, rq{q_piece, q_log0, q_nsteps, wd.wpar};
    const int nb = 1 + 16 * wd.T / WBW + wd.T;
    const WinArg<NoSlamGate> wa{wd, {}};
    // (T = 8: 3 + 3 + 2 rows on three workers measured slower than RW = 2)
    with_win_width(wd.T, [&](auto T) { launch_win_pieces_wp<T()>(st, nb, worker_publish, E, sp, wa, rs, rq, obs, enc); });
}
// lg: what the logger wave takes over from the prepare wave (win_chain_role's LG; 0 = the comparison path).  The workers' forms are
// built beside the default logger only: with another lg the workers publish in their default form
template <int T, class G, class W> static void launch_win_one_lg(hipStream_t st, int nb, int lg, int wp, const EkfState& E, const SlamParams& sp, const W& wa, const WinReplay& r,
                                                                          const ObsRaw* obs, const double* enc, bool consistent = false) {
    constexpr size_t lds = sizeof(WinChainLds<T, true>);
    constexpr int WD = win_worker_publish_default(T), NT = win_step_threads(T, 2, true);
    if (consistent) {
        // the consistent window: one form per width, the width's default publication.  Ungated beside logger_parts = 3, the
        // mean on the logger wave; gated beside logger_parts = 1, the mean on the prepare wave, which judges e
        constexpr int LGC = G::kOn ? 1 : 3;
        launch_step_kernel<T, true, LGC, WD, RunningMean>(k_ekf_win_step<T, 2, true, G, LGC, WD, RunningMean>, st, nb, NT, lds, E, sp, wa, r, r, obs, enc);
        return;
    }
    if (lg == 3) {
        switch (wp < 0 ? WD : wp & kWinWorkerPublishAll) {
#define ASLAM_WP_LAUNCH(i) case i: launch_step_kernel<T, true, 3, i>(k_ekf_win_step<T, 2, true, G, 3, i>, st, nb, NT, lds, E, sp, wa, r, r, obs, enc); break;
            ASLAM_WP_FORMS(ASLAM_WP_LAUNCH)
#undef ASLAM_WP_LAUNCH
        }
    }
    else if (lg == 2) launch_step_kernel<T, true, 2, WD>(k_ekf_win_step<T, 2, true, G, 2, WD>, st, nb, NT, lds, E, sp, wa, r, r, obs, enc);
    else if (lg == 1) launch_step_kernel<T, true, 1, WD>(k_ekf_win_step<T, 2, true, G, 1, WD>, st, nb, NT, lds, E, sp, wa, r, r, obs, enc);
    else launch_step_kernel<T, true, 0, WD>(k_ekf_win_step<T, 2, true, G, 0, WD>, st, nb, NT, lds, E, sp, wa, r, r, obs, enc);
}
#undef ASLAM_WP_FORMS
void launch_ekf_win_one(hipStream_t st, const EkfState& E, const SlamParams& sp, const WinDesc& wd, const ObsRaw* obs, const double* enc, const SlamGateArg* gate,
                        int logger_parts, int worker_publish, bool consistent) {
    const WinReplay r{0, 0, wd.nsteps, wd.wpar};
    const int nb = 1 + 16 * wd.T / WBW + wd.T;
    // (the chain role's waves: ceil(T / 2) workers, the prepare wave, the logger wave)
    if (gate) {                                                     // the gated instantiations: same grids, same blocks
        const WinArg<WinGate> wa{wd, WinGate{gate->g.gate_d2}};
        with_win_width(wd.T, [&](auto T) { launch_win_one_lg<T(), WinGate>(st, nb, logger_parts, worker_publish, E, sp, wa, r, obs, enc, consistent); });
        return;
    }
    const WinArg<NoSlamGate> wa{wd, {}};
    with_win_width(wd.T, [&](auto T) { launch_win_one_lg<T(), NoSlamGate>(st, nb, logger_parts, worker_publish, E, sp, wa, r, obs, enc, consistent); });
}
void launch_ekf_win_gate_finish(hipStream_t st, const EkfState& E, const WinDesc& wd, const SlamGateArg& gate, const ObsRaw* obs, bool consistent) {
    if (consistent) hipLaunchKernelGGL(k_ekf_win_gate_finish_zn, dim3(1), dim3(kWinFinishThreads), 0, st, E, wd, gate.g, obs);
    else hipLaunchKernelGGL(k_ekf_win_gate_finish, dim3(1), dim3(kWinFinishThreads), 0, st, E, wd, gate.g, obs);
}
void launch_ekf_win_gather(hipStream_t st, const EkfState& E, const WinDesc& wd) {
    hipLaunchKernelGGL(k_ekf_win_gather, dim3((E.ld + 255) / 256, 16), dim3(256), 0, st, E, wd);       // y: rows of Y_0 in turn (one load in flight per thread otherwise)
}
static void launch_thin(hipStream_t st, const EkfState& E, const WinDesc& wd, int ncols) {
    const int SP = 16 * wd.T, nb = (ncols + 63) / 64;
    with_win_width(wd.T, [&](auto T) { hipLaunchKernelGGL(k_ekf_win_thin<T()>, dim3(nb, 2 * SP / 64), dim3(256), 0, st, E, wd); });
}
void launch_ekf_win_next(hipStream_t st, const EkfState& E, const WinDesc& pv, const WinDesc& nx, bool split) {
    if (!split) {
        hipLaunchKernelGGL(k_ekf_win_next, dim3(nx.T), dim3(256), 0, st, E, pv, nx);
        return;
    }
    const int SPm = E.win_sp_max, s2 = 3 + 3 * nx.nS, SPn = 16 * nx.T;
    hipLaunchKernelGGL(k_ekf_win_next_gather, dim3((s2 + 255) / 256, 64), dim3(256), 0, st, E, pv, nx);
    // the miniature state the previous window's thin products and the Sigma pass run on: N := s', Sigma := Sigma_old[S', S']
    EkfState E2 = E;
    E2.ld = SPm;
    E2.d_sigma = E.d_win_next + (size_t)3 * SPm * SPm;
    E2.d_Wt = E.d_win_next;                                         // Vg
    E2.d_T = E.d_win_next + (size_t)1 * SPm * SPm;                  // Psi Vg
    E2.d_V = E.d_win_next + (size_t)2 * SPm * SPm;                  // Lambda Vg
    E2.d_mu = E.d_win_small + wsm_MU(SPm, nx.wpar);
    E2.d_win_sidx = E.d_win_next_idx;
    E2.d_L = E.d_win_next_idx + SPm;
    launch_thin(st, E2, pv, s2);
    launch_ekf_update_mfma(st, E2, 16 * pv.T);
    hipLaunchKernelGGL(k_ekf_win_next_fix, dim3((SPn + 255) / 256, 16), dim3(256), 0, st, E, pv, nx);
}
void launch_ekf_win_flush(hipStream_t st, const EkfState& E, const WinDesc& wd) {
    const int SP = 16 * wd.T;
    launch_thin(st, E, wd, E.ld);
    launch_ekf_update_mfma(st, E, SP);                            // Sigma -= Y_0^T U (d_Wt = Y_0, d_T = U), rows / columns S included
    hipLaunchKernelGGL(k_ekf_win_fix, dim3((E.ld + 255) / 256, 16), dim3(256), 0, st, E, wd, SP);
}

} // namespace aslam
