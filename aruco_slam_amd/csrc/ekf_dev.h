// Small device helpers shared by the EKF kernels (ekf.hip, ekf_window.hip).
#pragma once
#include "common.h"
#include <cmath>

// hardware reciprocal estimate (v_rcp_f64); the CPU emulation of the tests defines it as a plain division
#ifndef ASLAM_RCP_ESTIMATE
#define ASLAM_RCP_ESTIMATE(x) __builtin_amdgcn_rcp(x)
#endif

// In-launch hand-offs between workgroups (ekf_window.hip, one-launch window): an agent-scope acquire, a wait for this wave's older
// vector-memory operations, and global-address-space 64-bit words for write-through (sc1) stores and counters.  The CPU emulation
// of the tests has sequentially consistent atomics and no memory counters.  ASLAM_WAVE_LOCKSTEP marks a place where one lane acts on
// what the other lanes of its wave did before it in program order: nothing on the device, where a wave executes in lockstep; the
// emulation runs the lanes of a wave one after the other between barriers and has to bring them together there.
#if defined(__HIP__)
#define ASLAM_ACQUIRE_AGENT() __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent")
#define ASLAM_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define ASLAM_WAVE_LOCKSTEP() do { } while (0)
typedef __attribute__((address_space(1))) unsigned long long aslam_gu64;
#else
#define ASLAM_ACQUIRE_AGENT() __threadfence()
#define ASLAM_VMCNT(n) do { } while (0)
#define ASLAM_WAVE_LOCKSTEP() hipemu::wave_sync()
typedef unsigned long long aslam_gu64;
#endif

namespace aslam {

// write-through store of one double (global_store_dwordx2 sc1): visible to another XCD once this wave's vmcnt covers it
__device__ __forceinline__ void st_wt(double* p, double v) {
    unsigned long long b;
    __builtin_memcpy(&b, &v, sizeof(b));
    __hip_atomic_store((aslam_gu64*)p, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void win_signal(unsigned long long* w, unsigned epoch, int count) {          // relaxed agent store, sc1
    __hip_atomic_store((aslam_gu64*)w, ((unsigned long long)epoch << 32) | (unsigned)count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int win_count(const unsigned long long* w, unsigned epoch) {              // relaxed agent load, sc1
    const unsigned long long v = __hip_atomic_load((const aslam_gu64*)w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (unsigned)(v >> 32) == epoch ? (int)(unsigned)v : 0;                                  // an older window's count reads as 0
}

// value of lane `src` (wave-uniform) in every lane, through two v_readlane - no LDS traffic, unlike __shfl's ds_bpermute
#ifndef ASLAM_WAVE_BCAST
#define ASLAM_WAVE_BCAST(v, src) aslam_wave_bcast(v, src)
__device__ __forceinline__ double aslam_wave_bcast(double v, int src) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}
__device__ __forceinline__ int aslam_wave_bcast(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
#endif
__device__ __forceinline__ double aslam_rcp_estimate(double x) { return ASLAM_RCP_ESTIMATE(x); }

typedef double v4d __attribute__((vector_size(4 * sizeof(double))));   // accumulator of v_mfma_f64_16x16x4_f64

// Innovation policy of the per-frame chains and the localization steps (include/aruco_slam_hip.h).  FrozenMean, the
// default, is the reference (quirk Q1): every correction of a frame adds K ze with ze formed at the frame's predicted mean.  RunningMean
// corrects from the mean the previous correction left, e_i = ze_i - H_i (mu_{i-1} - mu_0): the exact linear sequential update.
struct FrozenMean { static constexpr bool kOn = false; };
struct RunningMean { static constexpr bool kOn = true; };

__device__ __forceinline__ void wrap1(double& a) {      // ArucoSlam::normAngle (aruco_slam.cpp:412-421): wraps once
    const double PI = 3.14159265358979323846;
    if (a >= PI) a -= 2.0 * PI;
    if (a < -PI) a += 2.0 * PI;
}

__device__ __forceinline__ void inv3_reg(const double* P, double* o) {   // 3x3 inverse (cofactors), row-major
    const double a = P[0], b = P[1], c = P[2], d = P[3], e = P[4], f = P[5], g = P[6], h = P[7], i = P[8];
    const double A = e * i - f * h, B = f * g - d * i, C = d * h - e * g;
    const double id = 1.0 / (a * A + b * B + c * C);
    o[0] = A * id; o[1] = (c * h - b * i) * id; o[2] = (b * f - c * e) * id;
    o[3] = B * id; o[4] = (a * i - c * g) * id; o[5] = (c * d - a * f) * id;
    o[6] = C * id; o[7] = (b * g - a * h) * id; o[8] = (a * e - b * d) * id;
}
// the same with the reciprocal of the determinant by Newton's iteration on a hardware estimate (full double precision to a
// couple of ulps; the IEEE division sequence is four times as long and sits on the Gauss-Jordan sweep's critical path)
__device__ __forceinline__ void inv3_fast(const double* P, double* o) {
    const double a = P[0], b = P[1], c = P[2], d = P[3], e = P[4], f = P[5], g = P[6], h = P[7], i = P[8];
    const double A = fma(e, i, -f * h), B = fma(f, g, -d * i), C = fma(d, h, -e * g);
    const double det = fma(a, A, fma(b, B, c * C));
    double id = aslam_rcp_estimate(det);
    id = fma(fma(-det, id, 1.0), id, id);
    id = fma(fma(-det, id, 1.0), id, id);
    o[0] = A * id; o[1] = fma(c, h, -b * i) * id; o[2] = fma(b, f, -c * e) * id;
    o[3] = B * id; o[4] = fma(a, i, -c * g) * id; o[5] = fma(c, d, -a * f) * id;
    o[6] = C * id; o[7] = fma(b, g, -a * h) * id; o[8] = fma(a, e, -b * d) * id;
}
__device__ __forceinline__ void mul3(const double* X, const double* Y, double* Z) {   // Z = X * Y (3x3 row-major)
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Z[i * 3 + j] = X[i * 3] * Y[j] + X[i * 3 + 1] * Y[3 + j] + X[i * 3 + 2] * Y[6 + j];
}

} // namespace aslam
