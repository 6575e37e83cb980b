// fd_bins.h -- host side of the k-means bin pass (include/fastdiff_hip_ext.h: fd_bins_pass, which defines the computation): the argument
// refusals, the kernel's LDS layout and the scratch layout.  Plain C++ without the HIP runtime.  tests/diversity_ref.py is the float64
// oracle.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/fastdiff_hip_ext.h"

namespace fdb {

constexpr int CHUNK = FD_BINS_CHUNK, MAX_K = FD_BINS_MAX_K, MAX_D = FD_BINS_MAX_D, THREADS = 256, WAVES = THREADS / 64;
constexpr int BLOCK = 32 * WAVES;                             // rows staged in LDS together: one 32-column matrix tile per wave
constexpr int64_t MAX_N = (int64_t)1 << 40;
constexpr int MSG = 200;                                      // room for a refusal's text
static_assert(CHUNK % BLOCK == 0 && MAX_K == 128 && MAX_D == 128 && WAVES == 4, "the kernel is written for four waves and at most 4 x 4 matrix tiles");

// null = accepted, else what is wrong, with the value, in msg (null pointers are the caller's to check)
inline const char *refusal(const void *x, int64_t N, int D, int64_t ld, bool has_shift, bool has_scale, int K, const float *cent,
                           const float *cent_out, char (&msg)[MSG])
{
    if (N < 1 || N > MAX_N) { snprintf(msg, MSG, "N = %lld rows outside 1 .. 2^40", (long long)N); return msg; }
    if (D < 4 || D > MAX_D || D % 4) { snprintf(msg, MSG, "D = %d features: a multiple of 4 in 4 .. %d is expected", D, MAX_D); return msg; }
    if (K < 1 || K > MAX_K) { snprintf(msg, MSG, "K = %d bins outside 1 .. %d", K, MAX_K); return msg; }
    if (ld < D) { snprintf(msg, MSG, "ld = %lld is shorter than a row of D = %d", (long long)ld, D); return msg; }
    if (ld > ((int64_t)1 << 21)) { snprintf(msg, MSG, "ld = %lld above 2^21", (long long)ld); return msg; }
    if ((uintptr_t)x % 4) { snprintf(msg, MSG, "x is not aligned to 4 bytes"); return msg; }
    if (has_shift != has_scale) { snprintf(msg, MSG, "shift and scale come together: %s is null", has_shift ? "scale" : "shift"); return msg; }
    if (cent_out && cent_out < cent + (size_t)K * D && cent < cent_out + (size_t)K * D) { snprintf(msg, MSG, "centroids_out overlaps centroids"); return msg; }
    return nullptr;
}

constexpr int64_t chunks(int64_t N) { return (N + CHUNK - 1) / CHUNK; }
constexpr int tiles(int n) { return (n + 31) / 32; }
constexpr int zstride(int D) { return D + 2; }                // floats between rows in LDS: 2 * odd, so the two halves of a wavefront's operand read take the even and the odd banks

// LDS of the pass kernel, bytes: 256 doubles (the inertia's reduction), h [128], shift [128], scale [128], then the ints assign [BLOCK],
// bad [BLOCK], counts [128] and four words, then the centroids [32 * tiles(K)][zstride] and the rows [BLOCK][zstride] + 32 floats (the
// last matrix tile of the update reads up to 31 floats past a row's D)
constexpr size_t lds_bytes(int K, int D)
{
    return sizeof(double) * 256 + 4 * ((size_t)3 * 128 + 2 * BLOCK + 128 + 4 + (size_t)(32 * tiles(K) + BLOCK) * zstride(D) + 32);
}
static_assert(lds_bytes(MAX_K, MAX_D) <= 160 * 1024, "the largest problem fits the LDS of one CU");

// The scratch buffer, slots on 256-byte borders, per chunk c: counts [c][128] int32, inertia [c] double, moved [c] int32, nonfinite
// [c] int32, and with an update the sums [c][K][D] float
struct Layout { size_t counts, inertia, moved, nonfinite, sums, total; };
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline Layout layout(int64_t N, int K, int D, bool update)
{
    const size_t nc = (size_t)chunks(N);
    Layout o{};
    o.counts = 0;
    o.inertia = o.counts + align256(sizeof(int32_t) * nc * 128);
    o.moved = o.inertia + align256(sizeof(double) * nc);
    o.nonfinite = o.moved + align256(sizeof(int32_t) * nc);
    o.sums = o.nonfinite + align256(sizeof(int32_t) * nc);
    o.total = o.sums + (update ? align256(sizeof(float) * nc * (size_t)K * D) : 0);
    return o;
}

}  // namespace fdb
