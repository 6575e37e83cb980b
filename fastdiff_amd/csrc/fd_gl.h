// fd_gl.h -- host side of Griffin-Lim (include/fastdiff_hip_ext.h: "Griffin-Lim", which defines the computation): the lengths, the
// overlap-add envelope and the range it covers, the Philox counter layout of the random start, the argument refusals and the scratch
// layout.  The transform itself is described by fd_dft.h and fd_kernels_dft.h.  Plain C++ without the HIP runtime, so a stand-alone host
// program can include it (tools/gl_host_check.cpp).  tests/gl_ref.py is the float64 oracle.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/fastdiff_hip_ext.h"
#include "fd_dft.h"

namespace fdgl {

constexpr int N = FD_GL_NFFT, HOP = FD_GL_HOP, BINS = FD_GL_BINS, PAD = N / 2;
constexpr int FRAME_TILE = FD_GL_FRAME_TILE, SUM_CHUNK = FD_GL_SUM_CHUNK, THREADS = fdt::THREADS;
constexpr int COVER = N / HOP;                                // frames over a sample in full overlap
constexpr int SEG = N + HOP * (FRAME_TILE - 1);               // padded samples under one workgroup's frames
constexpr int AMP_PITCH = 516;                                // floats per frame of the transposed amplitudes [B][T][AMP_PITCH]: 513, rounded up to 16 bytes
constexpr int MAX_B = 4096, MAX_T = FD_GL_MAX_FRAMES, MAX_ITERS = FD_GL_MAX_ITERS, DEFAULT_ITERS = 60;
constexpr int MELS = 80;
constexpr int MSG = 200;                                      // room for a refusal's text
static_assert(N == 4 * HOP && PAD == 2 * HOP && fdt::split_n1(N) == 32 && fdt::split_n2(N) == 32, "the kernels are written for 1024 / 256");

// samples of `frames` frames: the front-end's T = 1 + len / 256 read backwards; -1 below 2 frames
inline int64_t samples(int64_t frames) { return frames < 2 ? -1 : (int64_t)HOP * (frames - 1); }

// the frames t < frames that cover padded position m: [lo, hi]
inline void cover(int64_t m, int64_t frames, int64_t *lo, int64_t *hi)
{
    *lo = m < N ? 0 : (m - N) / HOP + 1;
    *hi = m / HOP < frames - 1 ? m / HOP : frames - 1;
}

inline double window(int n) { return 0.5 - 0.5 * cos(2.0 * 3.14159265358979323846 * n / N); }

// sum_t w^2[m - 256 t] over those frames, in double (the kernels add the float32 squares of the float32 table in the same order)
inline double envelope(int64_t m, int64_t frames)
{
    int64_t lo, hi;
    cover(m, frames, &lo, &hi);
    double e = 0.0;
    for (int64_t t = lo; t <= hi; ++t) { const double w = window((int)(m - HOP * t)); e += w * w; }
    return e;
}

// the random start's draw of (frame t, bin k): generator call `pos`, output word `word` (stream FD_GL_PHILOX_STREAM, id = the item's)
constexpr int CALLS_PER_FRAME = (BINS + 3) / 4;               // 129
inline uint64_t philox_pos(int64_t t, int k) { return (uint64_t)t * CALLS_PER_FRAME + (uint64_t)(k >> 2); }
inline int philox_word(int k) { return k & 3; }
// ... and the counter and key words the generator sees
inline void philox_counter(uint64_t seed, uint64_t id, int64_t t, int k, uint32_t ctr[4], uint32_t key[2])
{
    const uint64_t pos = philox_pos(t, k);
    ctr[0] = (uint32_t)pos; ctr[1] = (uint32_t)(pos >> 32) ^ (uint32_t)id; ctr[2] = FD_GL_PHILOX_STREAM; ctr[3] = 0x5EEDu ^ (uint32_t)(id >> 32);
    key[0] = (uint32_t)seed; key[1] = (uint32_t)(seed >> 32);
}

// null = accepted, else what is wrong, with the value, in msg (the pointers are the caller's to check)
inline const char *refusal(int B, int T, int n_iters, int64_t wav_pitch, char (&msg)[MSG])
{
    if (B < 1 || B > MAX_B) { snprintf(msg, MSG, "B = %d items outside 1 .. %d", B, MAX_B); return msg; }
    if (T < 2 || T > MAX_T) { snprintf(msg, MSG, "T = %d frames outside 2 .. %d", T, MAX_T); return msg; }
    if (n_iters < 0 || n_iters > MAX_ITERS) { snprintf(msg, MSG, "n_iters = %d outside 0 .. %d", n_iters, MAX_ITERS); return msg; }
    if (wav_pitch < samples(T)) {
        snprintf(msg, MSG, "wav_pitch = %lld is less than the %lld samples of T = %d frames", (long long)wav_pitch, (long long)samples(T), T);
        return msg;
    }
    return nullptr;
}

// The scratch buffer, slots one after the other, each starting on a 256-byte border: lens [B] int64, ids [B] uint64, the amplitudes
// transposed [B][T][AMP_PITCH] float, two frame buffers [B][T][N] float, the per-frame sums [B][T][4] double
struct Layout { size_t lens, ids, amp, frames[2], part, total; };
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline Layout layout(int B, int T)
{
    Layout o{};
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t p = at; at = align256(at + bytes); return p; };
    const size_t bt = (size_t)B * (size_t)T;
    o.lens = take(sizeof(int64_t) * (size_t)B);
    o.ids = take(sizeof(uint64_t) * (size_t)B);
    o.amp = take(sizeof(float) * bt * AMP_PITCH);
    o.frames[0] = take(sizeof(float) * bt * N);
    o.frames[1] = take(sizeof(float) * bt * N);
    o.part = take(sizeof(double) * bt * 4);
    o.total = at;
    return o;
}

}  // namespace fdgl
