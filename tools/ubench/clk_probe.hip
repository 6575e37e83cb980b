// clk_probe.hip -- what does s_memtime count, and what clock does a busy SIMD run at?
#include <hip/hip_runtime.h>
#include <stdio.h>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
__global__ void k_valu(long long *out, int n, float s)
{
    const long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    float a = s;
    for (int i = 0; i < n; ++i) {
#pragma unroll
        for (int j = 0; j < 64; ++j) a = a * 1.0001f + 0.5f;       // 64 dependent v_fma per iteration
    }
    const long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0 && blockIdx.x == 0) { out[0] = t1 - t0; out[1] = r1 - r0; }
    if (a == 12345.0f) out[2] = 1;
}
__global__ void k_mfma(long long *out, int n, float s)
{
    const long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    f16x8 a, b;
    for (int q = 0; q < 8; ++q) { a[q] = (_Float16)(s + q); b[q] = (_Float16)(s - q); }
    f32x16 acc = {0};
    for (int i = 0; i < n; ++i) {
#pragma unroll
        for (int j = 0; j < 32; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
    }
    const long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0 && blockIdx.x == 0) { out[0] = t1 - t0; out[1] = r1 - r0; }
    if (acc[0] == 12345.0f) out[2] = 1;
}
__global__ void k_mfma_rand(long long *out, int n, float s)
{
    // two operand sets with lane-dependent pseudo-random bit patterns, alternated: every MFMA sees fresh data
    const unsigned l = threadIdx.x * 2654435761u + blockIdx.x * 40503u;
    f16x8 a1, b1, a2, b2;
    for (int q = 0; q < 8; ++q) {
        a1[q] = (_Float16)(s * (float)((l >> (q + 3)) & 1023u) * 0.001f - 0.5f);
        b1[q] = (_Float16)(s * (float)((l >> (q + 7)) & 1023u) * 0.001f - 0.5f);
        a2[q] = (_Float16)(s * (float)((l >> (q + 11)) & 1023u) * 0.001f - 0.5f);
        b2[q] = (_Float16)(s * (float)((l >> (q + 13)) & 1023u) * 0.001f - 0.5f);
    }
    const long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    f32x16 acc = {0};
    for (int i = 0; i < n; ++i) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a2, b2, acc, 0, 0, 0);
        }
    }
    const long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0 && blockIdx.x == 0) { out[0] = t1 - t0; out[1] = r1 - r0; }
    if (acc[0] == 12345.0f) out[2] = 1;
}
// The tile-shape gate of k_kp_gemm_w (LABBOOK R17.1): the same 32 x 32 fp32 output tile per wave and the same K = 64 per iteration, once as
// four v_mfma_f32_32x32x16_f16 and once as 2 x 2 tiles x two v_mfma_f32_16x16x32_f16 -- equal FLOPs, equal cycles per FLOP, and equal LDS
// traffic: every operand is read again from LDS (ds_read_b128, 8 per iteration either way; random non-zero fp16 bit patterns, a region per
// wave, lane-linear = conflict free), one or two workgroups of four waves per CU.  Reported: FLOP/s over the whole grid and the clock block
// 0 ran at (core ticks of s_memtime per 10 ns tick of s_memrealtime).
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <int TILE>
__global__ void __launch_bounds__(256, 2) k_mfma_lds(long long *out, int n, float s)
{
    __shared__ __attribute__((aligned(16))) f16x8 ops[4][8][64];      // [wave][operand of the iteration][lane]: 32 KB
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned l = threadIdx.x * 2654435761u + blockIdx.x * 40503u;
    for (int o = 0; o < 8; ++o) {
        f16x8 v;
        for (int q = 0; q < 8; ++q) v[q] = (_Float16)(s * (float)(((l * (2 * o + 3)) >> (q + 5)) & 1023u) * 0.001f - 0.5117f);      // never 0
        ops[wave][o][lane] = v;
    }
    __syncthreads();
    const long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    f32x16 acc = {0};
    f32x4 c[2][2] = {};
    for (int i = 0; i < n; ++i) {
        asm volatile("" ::: "memory");      // the operands come out of LDS again in every iteration
        if constexpr (TILE == 32) {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ops[wave][2 * k][lane], ops[wave][2 * k + 1][lane], acc, 0, 0, 0);
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const f16x8 a0 = ops[wave][4 * k][lane], a1 = ops[wave][4 * k + 1][lane], b0 = ops[wave][4 * k + 2][lane], b1 = ops[wave][4 * k + 3][lane];
                c[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, b0, c[0][0], 0, 0, 0);
                c[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, b1, c[0][1], 0, 0, 0);
                c[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b0, c[1][0], 0, 0, 0);
                c[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b1, c[1][1], 0, 0, 0);
            }
        }
    }
    const long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0 && blockIdx.x == 0) { out[0] = t1 - t0; out[1] = r1 - r0; }
    if (acc[0] + c[0][0][0] + c[0][1][1] + c[1][0][2] + c[1][1][3] == 12345.0f) out[2] = 1;
}
template <int TILE>
static void tile_gate(long long *d, int grid, int n)
{
    long long h[3];
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    float ms = 0.f;
    for (int rep = 0; rep < 2; ++rep) {      // the second launch is the measurement (clock and caches settled)
        hipEventRecord(e0, 0);
        hipLaunchKernelGGL(k_mfma_lds<TILE>, dim3(grid), dim3(256), 0, 0, d, n, 1.0f);
        hipEventRecord(e1, 0); hipEventSynchronize(e1); hipEventElapsedTime(&ms, e0, e1);
    }
    hipMemcpy(h, d, 24, hipMemcpyDeviceToHost);
    const double flop = 2.0 * 32 * 32 * 64 * (double)n * 4 * grid;
    printf("tile gate %2dx%2dx%2d f16, operands from LDS, grid %4d: %.3f ms, %.1f TFLOP/s, block 0 ran at %.0f MHz\n", TILE, TILE, TILE == 32 ? 16 : 32,
           grid, ms, flop / (ms * 1e9), (double)h[0] / h[1] * 100.0);
    hipEventDestroy(e0); hipEventDestroy(e1);
}
int main()
{
    long long *d, h[3];
    hipMalloc(&d, 24);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    for (int mode = 0; mode < 4; ++mode) {
        const int grid = (mode & 1) ? 2048 : 1, n = 20000;
        float ms;
        hipEventRecord(e0, 0);
        if (mode < 2) hipLaunchKernelGGL(k_valu, dim3(grid), dim3(256), 0, 0, d, n, 1.0f);
        else hipLaunchKernelGGL(k_mfma, dim3(grid), dim3(256), 0, 0, d, n, 1.0f);
        hipEventRecord(e1, 0); hipEventSynchronize(e1); hipEventElapsedTime(&ms, e0, e1);
        hipMemcpy(h, d, 24, hipMemcpyDeviceToHost);
        const double ops = (mode < 2) ? 64.0 * n : 32.0 * n;
        printf("%s grid %4d: wall %.3f ms | s_memtime %lld ticks (%.2f per op) | s_memrealtime %lld ticks -> %.1f MHz realtime, memtime %.1f MHz\n",
               mode < 2 ? "valu chain" : "mfma chain", grid, ms, h[0], h[0] / ops, h[1], h[1] / (ms * 1e3), h[0] / (ms * 1e3));
    }
    for (int grid = 1; grid <= 2048; grid *= 2048) {
        const int n = 20000;
        hipLaunchKernelGGL(k_mfma_rand, dim3(grid), dim3(256), 0, 0, d, n, 1.0f);
        hipDeviceSynchronize();
        hipMemcpy(h, d, 24, hipMemcpyDeviceToHost);
        printf("mfma chain, alternating random operands, grid %4d: block 0 ran at %.0f MHz (%lld core ticks / %lld x 10 ns)\n", grid, (double)h[0] / h[1] * 100.0, h[0], h[1]);
    }
    for (int grid = 1; grid <= 2048; grid *= 2048) {
        hipLaunchKernelGGL(k_mfma, dim3(grid), dim3(256), 0, 0, d, 20000, 1.0f);
        hipDeviceSynchronize();
        hipMemcpy(h, d, 24, hipMemcpyDeviceToHost);
        printf("mfma chain, constant operands,           grid %4d: block 0 ran at %.0f MHz\n", grid, (double)h[0] / h[1] * 100.0);
    }
    hipDeviceProp_t prop;
    hipGetDeviceProperties(&prop, 0);
    for (int per_cu = 1; per_cu <= 2; ++per_cu)
        for (int rep = 0; rep < 3; ++rep) {      // alternating: both shapes see the same thermal state
            tile_gate<32>(d, per_cu * prop.multiProcessorCount, 200000);
            tile_gate<16>(d, per_cu * prop.multiProcessorCount, 200000);
        }
    return 0;
}
