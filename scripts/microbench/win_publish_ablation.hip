// Development microbenchmark (not part of the library or the tests): the window chain's step (ekf_window.hip, win_chain_role at
// SP = 64) as one workgroup of its four waves, with the workers' publication of the landmark rows in several forms, to see what the
// step pays for the write instructions and what for the rest of the workers' phase.
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o win_publish_ablation win_publish_ablation.hip
// Waves 0 and 1 are the workers (two tile rows of four 16 x 16 tiles each in the accumulators: B reads, eight
// v_mfma_f64_16x16x4_f64, the 16-way switch on the published position, the predicated row writes), wave 2 stands for the prepare
// wave (reads the three published rows, a dependent chain of `chain` f64 FMAs in place of its step, writes the six operand rows,
// raised priority), wave 3 for the logger wave (copies the three A rows to global memory).  One barrier per step, as in the kernel.
// The arithmetic is a stand-in (the operands are small constants, the accumulators stay finite); only the cycle counts matter.
//   PUB 0  as it is: T ds_write_b64 per published row (12 per step)
//   PUB 1  half the write instructions, same width: tiles 0 and 2 only (6 ds_write_b64; the rows are incomplete)
//   PUB 2  half the write instructions, the same data: the packed row, T / 2 ds_write_b128 per row
//   PUB 3  no write (the switch and the wait for the products stay: one lane group reads the registers into a dead store's place)
//   PUB 4  no publication at all
//   OWN 1  the tile row that holds the published rows is issued first
// chain = 0 shows the workers' phase alone, chain = 190 makes the stand-in about as long as the prepare wave's correction.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <type_traits>
typedef double v4d __attribute__((vector_size(32)));
typedef double v2d __attribute__((vector_size(16)));
#define LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
constexpr int T = 4, RW = 2, SP = 64, SPP = SP + 16;

template <int P16, int PUB>
__device__ __forceinline__ void publish_at(const v4d (&acc)[RW][T], int p, int wv, int lk, int li, double* rows) {
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const int rl = (P16 + q) & 15, g = (p + q) >> 4;
#pragma unroll
        for (int rr = 0; rr < RW; rr++)
            if (g == wv * RW + rr && lk == (rl & 3)) {
                if constexpr (PUB == 0) {
#pragma unroll
                    for (int t = 0; t < T; t++) rows[q * SPP + li + 16 * t] = acc[rr][t][rl >> 2];
                } else if constexpr (PUB == 1) {
#pragma unroll
                    for (int t = 0; t < T; t += 2) rows[q * SPP + li + 16 * t] = acc[rr][t][rl >> 2];
                } else if constexpr (PUB == 2) {
#pragma unroll
                    for (int h = 0; h < T / 2; h++) *reinterpret_cast<v2d*>(rows + q * SPP + 2 * li + 32 * h) = v2d{acc[rr][2 * h][rl >> 2], acc[rr][2 * h + 1][rl >> 2]};
                } else {
#pragma unroll
                    for (int t = 0; t < T; t++) asm volatile("" :: "v"(acc[rr][t][rl >> 2]));
                }
            }
    }
}
template <int PUB> __device__ __forceinline__ void publish(const v4d (&acc)[RW][T], int p, int wv, int lk, int li, double* rows) {
    switch (p & 15) {
#define C(i) case i: publish_at<i, PUB>(acc, p, wv, lk, li, rows); break;
        C(0) C(1) C(2) C(3) C(4) C(5) C(6) C(7) C(8) C(9) C(10) C(11) C(12) C(13) C(14) C(15)
#undef C
    }
}

template <int PUB, int OWN>
__global__ __launch_bounds__(256) void k_step(const unsigned char* pos, int ns, int chain, double* log, double* out, long long* cycles) {
    __shared__ __align__(16) double sA[2][4][SPP], sB[2][4][SPP], sPub[2][3][SPP];
    __shared__ unsigned char sPos[4096];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    for (int e = tid; e < 2 * 4 * SPP; e += 256) { (&sA[0][0][0])[e] = 1e-3 * ((e % 7) - 3); (&sB[0][0][0])[e] = 1e-3 * ((e % 5) - 2); }
    for (int e = tid; e < 2 * 3 * SPP; e += 256) (&sPub[0][0][0])[e] = 0.0;
    for (int e = tid; e < ns; e += 256) sPos[e] = pos[e];
    __syncthreads();
    long long t0 = 0;
    if (wave < 2) {
        v4d acc[RW][T];
#pragma unroll
        for (int rr = 0; rr < RW; rr++)
#pragma unroll
            for (int t = 0; t < T; t++) acc[rr][t] = v4d{1.0, 1.0, 1.0, 1.0};
        auto tile_row = [&](auto RR, int cb, const double (&b)[T]) {
            constexpr int rr = decltype(RR)::value;
            const double a = sA[cb][lk][16 * (wave * RW + rr) + li];
#pragma unroll
            for (int t = 0; t < T; t++) acc[rr][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[t], acc[rr][t], 0, 0, 0);
        };
        LDS_BARRIER();
        int pn_ahead = 255;
        for (int j = -1; j < ns; j++) {
            const int pn_next = sPos[j + 3 < ns ? j + 3 : ns - 1];
            if (j >= 0) {
                const int cb = j & 1;
                double b[T];
#pragma unroll
                for (int t = 0; t < T; t++) b[t] = sB[cb][lk][16 * t + li];
                const int pn = OWN ? pn_ahead : 255;
                if (OWN && ((3 + 3 * pn) >> 4) == wave * RW + 1) { tile_row(std::integral_constant<int, 1>{}, cb, b); tile_row(std::integral_constant<int, 0>{}, cb, b); }
                else { tile_row(std::integral_constant<int, 0>{}, cb, b); tile_row(std::integral_constant<int, 1>{}, cb, b); }
                if (PUB != 4 && j + 2 < ns) publish<PUB>(acc, 3 + 3 * (OWN ? pn : sPos[j + 2]), wave, lk, li, &sPub[cb][0][0]);
            }
            pn_ahead = pn_next;
            LDS_BARRIER();
        }
#pragma unroll
        for (int rr = 0; rr < RW; rr++)
#pragma unroll
            for (int t = 0; t < T; t++)
#pragma unroll
                for (int reg = 0; reg < 4; reg++) out[(size_t)(16 * (wave * RW + rr) + lk + 4 * reg) * SP + 16 * t + li] = acc[rr][t][reg];
    } else if (wave == 2) {
        __builtin_amdgcn_s_setprio(3);
        const int pcol = PUB == 2 ? 32 * ((lane >> 5) & 1) + 2 * (lane & 15) + ((lane >> 4) & 1) : lane;
        double keep = 0.0;
        LDS_BARRIER();
        t0 = clock64();
        for (int j = -1; j < ns; j++) {
            const int nb = (j + 1) & 1;
            if (j + 1 < ns) {
                double x = sPub[nb][0][pcol] + sPub[nb][1][pcol] + sPub[nb][2][pcol];
                for (int i = 0; i < chain; i++) x = fma(x, 0.999, 1e-6);
                keep += x;
                const double v = 1e-3 + 1e-9 * x;
#pragma unroll
                for (int k = 0; k < 3; k++) { sA[nb][k][lane] = -v; sB[nb][k][lane] = v; }
            }
            LDS_BARRIER();
        }
        if (lane == 0) cycles[0] = clock64() - t0;
        out[SP * SP + lane] = keep;
    } else {
        LDS_BARRIER();
        for (int j = -1; j < ns; j++) {
            if (j >= 0) {
#pragma unroll
                for (int k = 0; k < 3; k++) log[(size_t)j * 3 * SP + k * SP + lane] = sA[j & 1][k][lane];
            }
            LDS_BARRIER();
        }
    }
}

template <int PUB, int OWN> static void run(const unsigned char* dpos, int ns, int chain, double* dlog, double* dout, long long* dcyc) {
    long long best = 0;
    for (int rep = 0; rep < 5; rep++) {
        hipLaunchKernelGGL((k_step<PUB, OWN>), dim3(1), dim3(256), 0, 0, dpos, ns, chain, dlog, dout, dcyc);
        if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return; }
        long long c = 0;
        hipMemcpy(&c, dcyc, 8, hipMemcpyDeviceToHost);
        if (rep == 0 || c < best) best = c;
    }
    printf("publication form %d, owner tile row first %d, stand-in chain %3d: %6.0f cycles per step (best of 5 launches of %d steps)\n", PUB, OWN, chain,
           (double)best / (ns + 1), ns);
}

int main() {
    const int ns = 2100;                               // a hundred frames of twenty corrections and a predict (published as position 0: the ablation has no predict)
    unsigned char hpos[4096];
    for (int j = 0; j < ns; j++) hpos[j] = (unsigned char)(j % 21 == 0 ? 0 : j % 21 - 1);
    unsigned char* dpos; double *dlog, *dout; long long* dcyc;
    hipMalloc(&dpos, 4096); hipMalloc(&dlog, (size_t)ns * 3 * SP * 8); hipMalloc(&dout, (SP * SP + 64) * 8); hipMalloc(&dcyc, 64);
    hipMemcpy(dpos, hpos, ns, hipMemcpyHostToDevice);
    for (int chain : {0, 190}) {
        run<0, 0>(dpos, ns, chain, dlog, dout, dcyc);
        run<1, 0>(dpos, ns, chain, dlog, dout, dcyc);
        run<2, 0>(dpos, ns, chain, dlog, dout, dcyc);
        run<3, 0>(dpos, ns, chain, dlog, dout, dcyc);
        run<4, 0>(dpos, ns, chain, dlog, dout, dcyc);
        run<0, 1>(dpos, ns, chain, dlog, dout, dcyc);
        run<2, 1>(dpos, ns, chain, dlog, dout, dcyc);
    }
    return 0;
}
