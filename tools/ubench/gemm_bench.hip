// gemm_bench.hip -- standalone timing harness for k_kp_gemm, and (third argument w16 | w32) for k_h_wino + k_kp_gemm_w<16 | 32>, the two bodies
// of the Winograd form side by side: gemm_bench 8 864 w32; gemm_bench 8 864 w16.  Built with -DFD_GW_CLOCK it also prints the clock the
// workgroups of k_kp_gemm_w ran at (core ticks of s_memtime per 10 ns tick of s_memrealtime, summed over the workgroups' item loops).
#include "../../fastdiff_amd/csrc/fd_kernels_kp.hip"
#include <stdio.h>
#include <stdlib.h>
#include <vector>
bool fd_prof_stamps(const fdk::Launch &, const char *, hipEvent_t *, hipEvent_t *) { return false; }
void fd_prof_begin(const fdk::Launch &, const char *) {}
void fd_prof_end(const fdk::Launch &) {}
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)
int main(int argc, char **argv)
{
    const int B = argc > 1 ? atoi(argv[1]) : 8, T = argc > 2 ? atoi(argv[2]) : 864;
    const size_t nh = (size_t)3 * B * 64 * T, nk = (size_t)3 * B * T * fd::KREC, ng = (size_t)776 * 24 * 256;
    float *h, *kp, *g, *gb;
    CK(hipMalloc(&h, nh * 4)); CK(hipMalloc(&kp, nk * 4)); CK(hipMalloc(&g, ng * 4)); CK(hipMalloc(&gb, fd::KREC * 4));
    std::vector<float> v(ng);
    for (size_t i = 0; i < ng; ++i) v[i] = (float)((i * 2654435761u) % 2001) * 1e-3f - 1.0f;
    CK(hipMemcpy(g, v.data(), ng * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(h, v.data(), nh * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(gb, v.data(), fd::KREC * 4, hipMemcpyHostToDevice));
    if (argc > 3 && argv[3][0] == 'w') {
        const bool t16 = atoi(argv[3] + 1) == 16;
        const int P = fdk_fast::gw_pairs(T), wchunks = P / fdk_fast::GW_PAIRS, items = 3 * (fd::KREC / 128) * B * wchunks, G = argc > 4 ? atoi(argv[4]) : 512;
        const size_t nw = (size_t)776 * 2 * 16 * 64 * 4;      // floats of a block's fp16 piece pack
        float *wx, *gw;
        int *flag;
        CK(hipMalloc(&flag, 256)); CK(hipMemset(flag, 0, 256));
        CK(hipMalloc(&wx, (size_t)3 * B * P * fdk_fast::GW_ROWB)); CK(hipMalloc(&gw, nw * 4));
        {   // fp16 weight pieces of plausible magnitude (2^-7 .. 2^-2), random sign and mantissa (as gemm_h2_bench.hip)
            std::vector<unsigned short> w16(nw * 2);
            unsigned x = 12345u;
            for (auto &b : w16) { x = x * 1664525u + 1013904223u; b = (unsigned short)(((x >> 16) & 0x8000u) | ((8u + ((x >> 8) % 6u)) << 10) | ((x >> 20) & 0x3FFu)); }
            CK(hipMemcpy(gw, w16.data(), nw * 4, hipMemcpyHostToDevice));
        }
        auto run = [&]() {
            hipLaunchKernelGGL(fdk_fast::k_h_wino, dim3((8 * P + 255) / 256, 3 * B), dim3(256), 0, 0, (const float *)h, (char *)wx, flag, B, T, P, (const int *)nullptr);
            if (t16) hipLaunchKernelGGL(fdk_fast::k_kp_gemm_w<16>, dim3(G), dim3(256), 0, 0, (const char *)wx, kp, (const float4 *)gw, (const float4 *)gw,
                                        (const float4 *)gw, gb, gb, gb, (const int *)flag, B, T, P, wchunks, items, (const int *)nullptr);
            else hipLaunchKernelGGL(fdk_fast::k_kp_gemm_w<32>, dim3(G), dim3(256), 0, 0, (const char *)wx, kp, (const float4 *)gw, (const float4 *)gw,
                                    (const float4 *)gw, gb, gb, gb, (const int *)flag, B, T, P, wchunks, items, (const int *)nullptr);
        };
        hipEvent_t w0, w1; CK(hipEventCreate(&w0)); CK(hipEventCreate(&w1));
        for (int i = 0; i < 2; ++i) run();
        CK(hipDeviceSynchronize());
#ifdef FD_GW_CLOCK
        { long long z[2] = {0, 0}; CK(hipMemcpyToSymbol(HIP_SYMBOL(fdk_fast::fd_gwclk), z, sizeof(z))); }
#endif
        const int wreps = 5;
        CK(hipEventRecord(w0, 0));
        for (int i = 0; i < wreps; ++i) run();
        CK(hipEventRecord(w1, 0)); CK(hipEventSynchronize(w1));
        float wms = 0; CK(hipEventElapsedTime(&wms, w0, w1));
        int raised = 0; CK(hipMemcpy(&raised, flag, 4, hipMemcpyDeviceToHost));
        printf("h_wino+kp_gemm_w<%d> B=%d T=%d grid=%d items=%d: %.1f us  (range flag %d)\n", t16 ? 16 : 32, B, T, G, items, wms * 1e3 / wreps, raised);
#ifdef FD_GW_CLOCK
        long long clk[2]; CK(hipMemcpyFromSymbol(clk, HIP_SYMBOL(fdk_fast::fd_gwclk), sizeof(clk)));
        printf("   item loops ran at %.0f MHz (%lld core ticks / %lld x 10 ns)\n", (double)clk[0] / clk[1] * 100.0, clk[0], clk[1]);
#endif
        return 0;
    }
    const int tiles_per_utt = (T + 31) / 32, chunks = (tiles_per_utt + fdk_fast::GEMM_CT - 1) / fdk_fast::GEMM_CT;
    const int chunk_tiles = (tiles_per_utt + chunks - 1) / chunks;
    const int n_items = 3 * (fd::KREC / 128) * B * chunks;
    dim3 grid(512, 1, 1);
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int i = 0; i < 2; ++i) hipLaunchKernelGGL(fdk_fast::k_kp_gemm, grid, dim3(256), 0, 0, h, kp, g, g, g, gb, gb, gb, B, T, chunks, chunk_tiles, n_items, (const int *)nullptr, (const int *)nullptr);
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0, 0));
    const int reps = 5;
    for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(fdk_fast::k_kp_gemm, grid, dim3(256), 0, 0, h, kp, g, g, g, gb, gb, gb, B, T, chunks, chunk_tiles, n_items, (const int *)nullptr, (const int *)nullptr);
    CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
    float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
    const double us = ms * 1e3 / reps, flops = 3 * 2.0 * 24832 * 192 * (double)B * T;
    printf("kp_gemm B=%d T=%d chunk_tiles=%d grid=(%d,%d): %.1f us  %.1f TFLOP/s\n", B, T, chunk_tiles, grid.x, grid.y, us, flops / us / 1e6);
#ifdef FD_GEMM_TIMING
    std::vector<long long> d(64 * 4 * 4);
    CK(hipMemcpyFromSymbol(d.data(), HIP_SYMBOL(fdk_fast::fd_gdbg), d.size() * 8));
    double a[4] = {0};
    for (int w = 0; w < 256; ++w) for (int i = 1; i < 4; ++i) a[i] += (double)(d[w * 4 + i] - d[w * 4 + i - 1]);
    printf("   prologue (weights + stage + barrier) %8.0f\n   first tile %8.0f\n   remaining %d tiles %8.0f (%.0f per tile)\n", a[1] / 256, a[2] / 256, chunk_tiles - 1, a[3] / 256, a[3] / 256 / (chunk_tiles - 1));
#endif
    return 0;
}
