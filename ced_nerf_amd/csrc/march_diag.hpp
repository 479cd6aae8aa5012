// The -DCED_MARCH_DIAG build of the frame loop's marching kernel (tools/march_diag.py; nothing in the shipped library):
// the tick behind CED_DIAG_TICK (march_accel.hpp), its per-wave accumulators and log, and the two readers.  Included, at
// global scope, by the unit that holds march_frame_kernel (frame.hip).
#pragma once
#include <hip/hip_runtime.h>

#ifdef CED_MARCH_DIAG
// [phase][0] passes of a wave through the phase, [1] lanes active in those passes, [2] cycles of the wave between this
// tick and its next one.  Phases: 0 ray set-up, 1 segment set-up, 2 distance-field probe, 3 closed-form re-entry,
// 4 exact walk (one look-ahead batch), 5 emission at an occupied cell, 6 reservation + regeneration, 7 idle tail.
__device__ unsigned long long g_march_diag[8][3];
// per-wave accumulators in LDS (a tick costs a handful of instructions of one lane), flushed once per wave
__device__ __forceinline__ unsigned long long (*ced_diag_acc())[8][3]
{
    __shared__ unsigned long long acc[16][8][3];
    return acc;
}
__device__ __forceinline__ unsigned long long *ced_diag_state()
{
    __shared__ unsigned long long st[16][2];        // last tick's time and phase
    return &st[0][0];
}
__device__ void ced_diag_tick(int phase)
{
    const unsigned long long m = __ballot(1);
    const int wave = threadIdx.x >> 6;
    if ((int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) {
        unsigned long long(*acc)[8][3] = ced_diag_acc();
        unsigned long long *st = ced_diag_state() + 2 * wave;
        const unsigned long long now = __builtin_readcyclecounter();
        if (st[1] != 0x1234) {                         // first tick of the wave: clear
            for (int p = 0; p < 8; ++p) for (int k = 0; k < 3; ++k) acc[wave][p][k] = 0;
            st[1] = 0x1234;
        } else {
            acc[wave][(int)(st[0] >> 60) & 7][2] += (now - st[0]) & 0x0fffffffffffffffull;
        }
        st[0] = (now & 0x0fffffffffffffffull) | ((unsigned long long)phase << 60);
        acc[wave][phase][0] += 1;
        acc[wave][phase][1] += (unsigned long long)__popcll(m);
    }
}
// per-wave log: passes through phases 0..7, lanes in them, cycles in them (one row per wave and launch)
constexpr int kDiagWaves = 1 << 17;
__device__ unsigned int g_march_wave_log[kDiagWaves][24];
__device__ unsigned int g_march_wave_n;
__device__ void ced_diag_flush()
{
    const int wave = threadIdx.x >> 6;
    unsigned long long(*acc)[8][3] = ced_diag_acc();
    unsigned long long *st = ced_diag_state() + 2 * wave;
    if ((threadIdx.x & 63) == 0 && st[1] == 0x1234) {
        for (int p = 0; p < 8; ++p) for (int k = 0; k < 3; ++k) if (acc[wave][p][k]) atomicAdd(&g_march_diag[p][k], acc[wave][p][k]);
        const unsigned int row = atomicAdd(&g_march_wave_n, 1u);
        if (row < (unsigned)kDiagWaves)
            for (int p = 0; p < 8; ++p) for (int k = 0; k < 3; ++k) g_march_wave_log[row][3 * p + k] = (unsigned int)acc[wave][p][k];
        st[1] = 0;
    }
}

extern "C" int ced_diag_march_read(unsigned long long *out, int reset)
{
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_march_diag), sizeof(unsigned long long) * 24) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[24] = { 0 };
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_march_diag), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
// rows of the per-wave log since the last reset (out: [max_rows][24] uint32); returns the number of rows
extern "C" int ced_diag_march_waves(unsigned int *out, int max_rows, int reset)
{
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    unsigned int n = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_march_wave_n), 4) != hipSuccess) return -1;
    if (n > (unsigned)kDiagWaves) n = kDiagWaves;
    if ((int)n > max_rows) n = max_rows;
    if (out && n && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_march_wave_log), (size_t)n * 96) != hipSuccess) return -1;
    if (reset) {
        unsigned int z = 0;
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_march_wave_n), &z, 4) != hipSuccess) return -1;
    }
    return (int)n;
}
#endif
