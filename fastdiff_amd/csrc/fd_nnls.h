// fd_nnls.h -- host side of the non-negative mel inversion (include/fastdiff_hip_ext.h: fd_mel_to_linear_nnls, which defines the
// computation): the argument refusals, the step bound L, the momentum table, the zero-padded images of the bank that the kernel streams,
// the split of its work over the waves and the scratch layout.  Plain C++ without the HIP runtime, so a stand-alone host program can
// include it (tools/nnls_host_check.cpp).  tests/nnls_ref.py is the float64 oracle.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/fastdiff_hip_ext.h"

namespace fdn {

constexpr int MELS = 80, BINS = FD_GL_BINS, TILE = FD_NNLS_FRAME_TILE, THREADS = 256, WAVES = THREADS / 64;
constexpr int MAX_B = 4096, MAX_T = FD_GL_MAX_FRAMES, MAX_ITERS = FD_NNLS_MAX_ITERS, DEFAULT_ITERS = 128;
constexpr int POWER_ITERS = 200;
constexpr double MARGIN = 1.01;
constexpr int MSG = 200;                                      // room for a refusal's text
// The images of the bank: AT [KPAIRS * 2][MPAD] (AT[k][m] = A[m][k], zero for k >= 513 and m >= 80) feeds A y, 32 mels per matrix
// tile; AP [MELS][BPAD] (zero for k >= 513) feeds A^T r, 32 bins per tile.
constexpr int CHUNK = 4;                                      // bin or mel pairs whose A operands are fetched together, one chunk ahead
constexpr int KPAIRS = ((BINS + 1) / 2 + CHUNK - 1) / CHUNK * CHUNK;      // 260 bin pairs (257, rounded up to whole chunks), one matrix instruction each per mel tile
constexpr int MTILES = (MELS + 31) / 32, MPAD = 32 * MTILES;  // 3, 96
constexpr int BTILES = (BINS + 31) / 32, BPAD = 32 * BTILES;  // 17, 544
constexpr int YROWS = 2 * KPAIRS;                             // rows of y in LDS: 513 bins and seven zero rows
constexpr int MAX_BT = (BTILES + WAVES - 1) / WAVES;          // bin tiles of the busiest wave (wave 0: 5)
static_assert(TILE == 32 && WAVES == 4 && MTILES == 3 && BTILES == 17 && KPAIRS == 260, "the kernel is written for 32-column matrix tiles and four waves");

// Bin tiles w, w + 4, ... belong to wave w, so wave 0 has five and the others four.  The bin pairs of A y are dealt out in whole
// chunks to even that: with 3 instructions per pair and 40 per bin tile, [pair_begin(w), pair_begin(w + 1)) gives 356, 364, 364, 376
// instructions (the last three pairs of wave 3 are the zero padding).
constexpr int pair_begin(int w) { return w <= 0 ? 0 : (w == 1 ? 52 : (w == 2 ? 120 : (w == 3 ? 188 : KPAIRS))); }
static_assert(pair_begin(1) % CHUNK == 0 && pair_begin(2) % CHUNK == 0 && pair_begin(3) % CHUNK == 0 && KPAIRS % CHUNK == 0 && (MELS / 2) % CHUNK == 0, "whole chunks");
constexpr int bin_tiles(int wave) { return (BTILES - wave + WAVES - 1) / WAVES; }

inline bool finite_bits(float v)
{
    uint32_t u;
    memcpy(&u, &v, sizeof(u));                                // (on the bit pattern: the library is built with -fno-honor-nans)
    return (u & 0x7F800000u) != 0x7F800000u;
}

// null = accepted, else what is wrong, with the value, in msg (the pointers and lens are the caller's to check)
inline const char *refusal(int B, int T, int n_iters, int variant, char (&msg)[MSG])
{
    if (B < 1 || B > MAX_B) { snprintf(msg, MSG, "B = %d items outside 1 .. %d", B, MAX_B); return msg; }
    if (T < 1 || T > MAX_T) { snprintf(msg, MSG, "T = %d frames outside 1 .. %d", T, MAX_T); return msg; }
    if (n_iters < 0 || n_iters > MAX_ITERS) { snprintf(msg, MSG, "n_iters = %d outside 0 .. %d", n_iters, MAX_ITERS); return msg; }
    if (variant != FD_GL_PWG && variant != FD_GL_TACOTRON) { snprintf(msg, MSG, "unknown variant %d (FD_GL_PWG / FD_GL_TACOTRON)", variant); return msg; }
    return nullptr;
}

// the first element of a [n] that is not finite, or -1
inline long first_nonfinite(const float *a, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!finite_bits(a[i])) return (long)i;
    return -1;
}

// L >= lambda_max(A A^T): POWER_ITERS power iterations on the Gram matrix in double from v_j = 1 + j / 80, then MARGIN times the
// Rayleigh quotient.  Deterministic: plain loops in a fixed order.  A zero bank gives the smallest positive normal double, so that
// 1 / L stays finite in float32's reach only after the caller's clamp (step()).
inline double step_bound(const float *bank)
{
    static_assert(MELS == 80, "the start vector is stated for 80 filters");
    double G[MELS][MELS];
    for (int i = 0; i < MELS; ++i)
        for (int j = i; j < MELS; ++j) {
            double s = 0.0;
            for (int k = 0; k < BINS; ++k) s += (double)bank[(size_t)i * BINS + k] * (double)bank[(size_t)j * BINS + k];
            G[i][j] = G[j][i] = s;
        }
    double v[MELS], w[MELS];
    for (int j = 0; j < MELS; ++j) v[j] = 1.0 + (double)j / MELS;
    double q = 0.0;
    for (int it = 0; it <= POWER_ITERS; ++it) {
        double nn = 0.0, vw = 0.0;
        for (int i = 0; i < MELS; ++i) {
            double s = 0.0;
            for (int j = 0; j < MELS; ++j) s += G[i][j] * v[j];
            w[i] = s;
            nn += v[i] * v[i];
            vw += v[i] * s;
        }
        q = nn > 0.0 ? vw / nn : 0.0;                         // the Rayleigh quotient of the current vector
        if (it == POWER_ITERS) break;
        double wn = 0.0;
        for (int i = 0; i < MELS; ++i) wn += w[i] * w[i];
        if (!(wn > 0.0)) break;                               // G v = 0: a zero bank (or a start vector in its null space)
        wn = sqrt(wn);
        for (int i = 0; i < MELS; ++i) v[i] = w[i] / wn;
    }
    const double L = MARGIN * q;
    return L > 2.2250738585072014e-308 ? L : 2.2250738585072014e-308;
}

// the kernel's step: float32(1 / L), kept finite (a bank of tiny values would give inf, and inf * 0 = NaN in the update)
inline float step(double L)
{
    const double s = 1.0 / L;
    return s > 3.0e38 ? 3.0e38f : (float)s;
}

// beta_k, k < n, in double, rounded to float32 once
inline void betas(int n, float *out)
{
    double t = 1.0;
    for (int k = 0; k < n; ++k) {
        const double t1 = (1.0 + sqrt(1.0 + 4.0 * t * t)) / 2.0;
        out[k] = (float)((t - 1.0) / t1);
        t = t1;
    }
}

// The device table of one variant, floats: AT, AP, the betas
struct Table { size_t at, ap, beta, total; };
constexpr Table table()
{
    Table t{};
    t.at = 0;
    t.ap = t.at + (size_t)YROWS * MPAD;
    t.beta = t.ap + (size_t)MELS * BPAD;
    t.total = t.beta + MAX_ITERS;
    return t;
}
inline void fill_table(const float *bank, float *out)
{
    const Table t = table();
    for (size_t i = 0; i < t.total; ++i) out[i] = 0.0f;
    for (int m = 0; m < MELS; ++m)
        for (int k = 0; k < BINS; ++k) {
            out[t.at + (size_t)k * MPAD + m] = bank[(size_t)m * BINS + k];
            out[t.ap + (size_t)m * BPAD + k] = bank[(size_t)m * BINS + k];
        }
    betas(MAX_ITERS, out + t.beta);
}

// LDS of the solve kernel, floats: y [YROWS][TILE], the waves' partial sums of A y [WAVES][MELS][TILE] (the record pass keeps its
// [MELS][TILE] doubles there), r [MELS][TILE], g [MELS][TILE]
struct Lds { size_t y, part, r, g, total; };
constexpr Lds lds()
{
    Lds o{};
    o.y = 0;
    o.part = o.y + (size_t)YROWS * TILE;
    o.r = o.part + (size_t)WAVES * MELS * TILE;
    o.g = o.r + (size_t)MELS * TILE;
    o.total = o.g + (size_t)MELS * TILE;
    return o;
}
static_assert(sizeof(double) * MELS * TILE <= sizeof(float) * WAVES * MELS * TILE, "the record pass's squares fit in the partial sums' slot");

// The scratch buffer, slots on 256-byte borders: lens [B] int64, the per-frame sums [B][T][4] double
struct Layout { size_t lens, part, total; };
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline Layout layout(int B, int T)
{
    Layout o{};
    o.lens = 0;
    o.part = align256(sizeof(int64_t) * (size_t)B);
    o.total = o.part + align256(sizeof(double) * (size_t)B * (size_t)T * 4);
    return o;
}

}  // namespace fdn
