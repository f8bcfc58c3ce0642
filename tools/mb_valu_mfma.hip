// mb_valu_mfma.hip -- does VALU work of a SIMD take time from its fp64 matrix pipe?
// Four waves per SIMD keep v_mfma_f64_16x16x4_f64 issued back to back on independent accumulators; per matrix instruction
// r = 0, 1, 2, 4, 8 VALU instructions (v_fma_f64, or v_add_u32 for comparison) are issued as well,
//   same:       by the wave that issues the matrix instruction, behind it (4 waves per SIMD, each both kinds), or
//   neighbour:  by other waves of the same SIMD (2 waves per SIMD issue matrix instructions only, 2 issue VALU only; the
//               matrix waves run twice the trips, so a SIMD executes the same instruction counts as in `same`).
// Printed: cycles per matrix instruction per SIMD (whole kernel, events, nominal clock), and for `neighbour` the run time of
// the slowest matrix wave and of the slowest VALU wave (s_memrealtime), which tells a slowed matrix pipe from a kernel that
// merely waits for its VALU waves.  A 16x16x4 fp64 matrix instruction is 64 cycles of the pipe when nothing disturbs it
// (2048 flop at 32 flop per cycle and SIMD; r = 0 measures 65).
// Build: hipcc --offload-arch=gfx950 -O3 tools/mb_valu_mfma.hip -o tools/mb_valu_mfma
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
typedef double double4_t __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

constexpr int NACC = 4;

// OP 0: v_fma_f64, 1: v_add_u32.  The VALU chains are 8 independent registers, used round robin.
template <int OP>
__device__ __forceinline__ void valu_one(double (&f)[8], unsigned (&u)[8], int idx, double b0, unsigned x) {
    if (OP == 0) asm volatile("v_fma_f64 %0, %0, %1, %0" : "+v"(f[idx & 7]) : "v"(b0));
    else asm volatile("v_add_u32 %0, %0, %1" : "+v"(u[idx & 7]) : "v"(x));
}

template <int OP, int R, bool NEIGHBOUR>
__global__ __launch_bounds__(1024, 1) void k_mix(double *out, long long *ticks, int iters, double a0, double b0, unsigned x) {
    const int wave = threadIdx.x >> 6;
    // waves go to the SIMDs round robin: the waves w, w + 4, w + 8, w + 12 share one
    const bool does_mfma = !NEIGHBOUR || ((wave >> 2) & 1) == 0, does_valu = !NEIGHBOUR || !does_mfma;
    double4_t acc[NACC];
    for (int i = 0; i < NACC; ++i) acc[i] = (double4_t){0, 0, 0, 0};
    const double a = a0 + threadIdx.x * 1e-3, b = b0 - threadIdx.x * 1e-3;
    double f[8];
    unsigned u[8];
    for (int j = 0; j < 8; ++j) { f[j] = a0 + j; u[j] = threadIdx.x + j; }
    const int trips = NEIGHBOUR ? 2 * iters : iters;
    __syncthreads();
    const long long t0 = wall_clock64();
    if (does_mfma && does_valu) {
        for (int it = 0; it < trips; ++it) {
#pragma unroll
            for (int i = 0; i < NACC; ++i) {
                acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int r = 0; r < R; ++r) valu_one<OP>(f, u, i * R + r, b0, x);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    } else if (does_mfma) {
        for (int it = 0; it < trips; ++it) {
#pragma unroll
            for (int i = 0; i < NACC; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
        }
    } else {
        for (int it = 0; it < trips; ++it) {
#pragma unroll
            for (int i = 0; i < NACC; ++i)
#pragma unroll
                for (int r = 0; r < R; ++r) valu_one<OP>(f, u, i * R + r, b0, x);
        }
    }
    const long long t1 = wall_clock64();
    double s = 0;
    for (int i = 0; i < NACC; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    for (int j = 0; j < 8; ++j) s += f[j] + u[j];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if ((threadIdx.x & 63) == 0) ticks[blockIdx.x * 16 + wave] = t1 - t0;
}

struct Dev { hipDeviceProp_t prop; int wall_khz; double *out; long long *ticks; hipEvent_t e0, e1; };

template <int OP, int R, bool NEIGHBOUR>
int run(Dev &d) {
    const int blocks = d.prop.multiProcessorCount, iters = 20000;
    for (int rep = 0; rep < 2; ++rep) { // the first launch warms up
        CK(hipEventRecord(d.e0));
        hipLaunchKernelGGL((k_mix<OP, R, NEIGHBOUR>), dim3(blocks), dim3(1024), 0, 0, d.out, d.ticks, iters, 1.0, 0.9999999, 3u);
        CK(hipEventRecord(d.e1));
        CK(hipEventSynchronize(d.e1));
    }
    float ms;
    CK(hipEventElapsedTime(&ms, d.e0, d.e1));
    std::vector<long long> t(blocks * 16);
    CK(hipMemcpy(t.data(), d.ticks, t.size() * sizeof(long long), hipMemcpyDeviceToHost));
    long long tm = 0, tv = 0;
    for (int i = 0; i < blocks * 16; ++i) {
        const bool m = !NEIGHBOUR || (((i & 15) >> 2) & 1) == 0;
        if (m) tm = tm > t[i] ? tm : t[i];
        else tv = tv > t[i] ? tv : t[i];
    }
    const double mfma_per_simd = 4.0 * iters * NACC; // in both placements
    const double cyc = ms * 1e-3 * (d.prop.clockRate * 1e3) / mfma_per_simd;
    printf("%-9s %-9s r=%d  %7.3f ms  %6.2f cycles per matrix instruction per SIMD", OP == 0 ? "v_fma_f64" : "v_add_u32",
           NEIGHBOUR ? "neighbour" : "same", R, ms, cyc);
    if (NEIGHBOUR) printf("   slowest matrix wave %.3f ms, slowest VALU wave %.3f ms", tm / (double)d.wall_khz, tv / (double)d.wall_khz);
    printf("\n");
    return 0;
}

template <int OP, bool NEIGHBOUR>
int sweep(Dev &d) {
    return run<OP, 0, NEIGHBOUR>(d) || run<OP, 1, NEIGHBOUR>(d) || run<OP, 2, NEIGHBOUR>(d) || run<OP, 4, NEIGHBOUR>(d) || run<OP, 8, NEIGHBOUR>(d);
}

int main() {
    Dev d;
    CK(hipGetDeviceProperties(&d.prop, 0));
    CK(hipDeviceGetAttribute(&d.wall_khz, hipDeviceAttributeWallClockRate, 0));
    printf("device %s, %d CUs, clock %d kHz, wall clock %d kHz\n", d.prop.gcnArchName, d.prop.multiProcessorCount, d.prop.clockRate, d.wall_khz);
    CK(hipMalloc(&d.out, sizeof(double) * 1024 * d.prop.multiProcessorCount));
    CK(hipMalloc(&d.ticks, sizeof(long long) * 16 * d.prop.multiProcessorCount));
    CK(hipEventCreate(&d.e0)); CK(hipEventCreate(&d.e1));
    if (sweep<0, false>(d) || sweep<0, true>(d) || sweep<1, false>(d) || sweep<1, true>(d)) return 1;
    return 0;
}
