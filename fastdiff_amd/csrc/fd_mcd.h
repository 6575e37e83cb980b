// fd_mcd.h -- host side of the mel-cepstral distortion (include/fastdiff_hip_ext.h: "Mel-cepstral distortion with time alignment"): the
// constants that decide which thread is at which cell of the alignment in which step, the refusals, the frame counts, the DCT table the
// cepstrum kernel reads, the index ranges of the skewed sweep and the LDS and scratch sizing.  Plain C++ without the HIP runtime, so a
// stand-alone host program can include it (tools/mcd_host_check.cpp).  tests/mcd_ref.py is the float64 oracle.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/fastdiff_hip_ext.h"

namespace fdm {

constexpr int MELS = 80, HOP = 256;
constexpr int MAX_COEF = 40;                                  // FD_MCD_MAX_COEF
constexpr int DEFAULT_COEF = 13;
constexpr int ROWS = 256;                                     // FD_DTW_ROWS: rows of one block = threads of the workgroup
constexpr int COLS = 64;                                      // FD_DTW_COLS: columns staged together
constexpr int RING = ROWS + COLS;                             // columns of b (and of the row above the block) that LDS holds
constexpr int WAVE = 64, WAVES = ROWS / WAVE;
constexpr int MAX_B = 4096;
constexpr int64_t MAX_FRAMES = (int64_t)1 << 22;              // FD_MCD_MAX_FRAMES
constexpr int64_t MAX_ALIGN_CELLS = (int64_t)1 << 26;         // FD_DTW_MAX_ALIGN_CELLS
constexpr int64_t MAX_LD = (int64_t)1 << 21;
constexpr int TACO_SHORT = 512;                               // tacotron: n <= 512 is FD_MCD_SHORT (the reflection is undefined)
constexpr double K_DB = 6.141851463713754;                    // 10 sqrt(2) / ln 10
constexpr int MSG = 200;                                      // room for a refusal's text
static_assert(ROWS % WAVE == 0 && COLS <= ROWS && RING == 320, "the sweep's geometry");

inline void defaults(fd_mcd_config *c) { c->n_coef = DEFAULT_COEF; c->reserved = 0; }

// null = accepted, else what is wrong, with the value, in msg
inline const char *coef_refusal(int n_coef, char (&msg)[MSG])
{
    if (n_coef < 1 || n_coef > MAX_COEF) { snprintf(msg, MSG, "n_coef = %d outside 1 .. %d", n_coef, MAX_COEF); return msg; }
    return nullptr;
}

inline const char *refusal(const fd_mcd_config &c, char (&msg)[MSG])
{
    if (c.reserved != 0) { snprintf(msg, MSG, "reserved = %d is not 0", (int)c.reserved); return msg; }
    return coef_refusal(c.n_coef, msg);
}

inline int64_t frames(int64_t n) { return 1 + n / HOP; }

// B and L of a waveform batch
inline const char *wave_refusal(int B, int64_t L, const char *what, char (&msg)[MSG])
{
    if (B < 1 || B > MAX_B) { snprintf(msg, MSG, "B = %d outside 1 .. %d", B, MAX_B); return msg; }
    if (L < 1 || frames(L) > MAX_FRAMES) {
        snprintf(msg, MSG, "%s = %lld samples outside 1 .. %lld (%lld frames)", what, (long long)L, (long long)(MAX_FRAMES * HOP - 1), (long long)MAX_FRAMES);
        return msg;
    }
    return nullptr;
}

// the shape of an alignment call (the counts themselves are checked with the other tools' check_counts)
inline const char *dtw_refusal(int B, int D, int64_t ld, int64_t pitch_a, int64_t pitch_b, bool align, int64_t align_pitch, char (&msg)[MSG])
{
    if (B < 1 || B > MAX_B) { snprintf(msg, MSG, "B = %d outside 1 .. %d", B, MAX_B); return msg; }
    if (D < 1 || D > MAX_COEF) { snprintf(msg, MSG, "D = %d outside 1 .. %d", D, MAX_COEF); return msg; }
    if (ld < D || ld > MAX_LD) { snprintf(msg, MSG, "ld = %lld outside D = %d .. %lld", (long long)ld, D, (long long)MAX_LD); return msg; }
    if (pitch_a < 1 || pitch_a > MAX_FRAMES) { snprintf(msg, MSG, "pitch_a = %lld outside 1 .. %lld", (long long)pitch_a, (long long)MAX_FRAMES); return msg; }
    if (pitch_b < 1 || pitch_b > MAX_FRAMES) { snprintf(msg, MSG, "pitch_b = %lld outside 1 .. %lld", (long long)pitch_b, (long long)MAX_FRAMES); return msg; }
    if (align && align_pitch < pitch_a) { snprintf(msg, MSG, "align_pitch = %lld is less than pitch_a = %lld", (long long)align_pitch, (long long)pitch_a); return msg; }
    return nullptr;
}

// with align_out: a pair of more cells than MAX_ALIGN_CELLS is refused
inline const char *align_refusal(int b, int64_t Ta, int64_t Tb, char (&msg)[MSG])
{
    if (Ta * Tb > MAX_ALIGN_CELLS) {
        snprintf(msg, MSG, "pair %d has %lld x %lld = %lld cells, with align_out at most %lld are kept", b, (long long)Ta, (long long)Tb, (long long)(Ta * Tb),
                 (long long)MAX_ALIGN_CELLS);
        return msg;
    }
    return nullptr;
}

// The DCT table [MAX_COEF][MELS]: row d - 1 = sqrt(2 / 80) cos(pi d (j + 1/2) / 80), d = 1 .. MAX_COEF, rounded once from double
inline void dct_table(float *tab)
{
    const double pi = 3.14159265358979323846, s = sqrt(2.0 / MELS);
    for (int d = 1; d <= MAX_COEF; ++d)
        for (int j = 0; j < MELS; ++j) tab[(d - 1) * MELS + j] = (float)(s * cos(pi * d * (j + 0.5) / MELS));
}
inline double dct_entry(int d, int j)      // the same in double, d = 0 .. MELS - 1 (d = 0: 1 / sqrt(80)), for the check of orthonormality
{
    const double pi = 3.14159265358979323846;
    return d == 0 ? sqrt(1.0 / MELS) : sqrt(2.0 / MELS) * cos(pi * d * (j + 0.5) / MELS);
}

// The sweep.  Rows are cut into blocks of ROWS; block k has rows(k) rows and runs steps(k) steps; in step s thread r is at column s - r.
inline int64_t blocks(int64_t Ta) { return (Ta + ROWS - 1) / ROWS; }
inline int block_rows(int64_t Ta, int64_t k) { const int64_t left = Ta - k * ROWS; return (int)(left < ROWS ? left : ROWS); }
inline int64_t block_steps(int64_t Ta, int64_t Tb, int64_t k) { return Tb + block_rows(Ta, k) - 1; }
// the ring slot of column j
inline int slot(int64_t j) { return (int)(j % RING); }
// the column tile [lo, hi) loaded in the phase of step s (s = -1: before the first step): columns s + 1 .. s + COLS when COLS divides s + 1
inline bool tile_at(int64_t s, int64_t Tb, int64_t *lo, int64_t *hi)
{
    if ((s + 1) % COLS != 0 || s + 1 >= Tb) return false;
    *lo = s + 1;
    *hi = s + 1 + COLS < Tb ? s + 1 + COLS : Tb;
    return true;
}
// the padded width of the feature rows in registers and LDS: the kernel is compiled for 16 and MAX_COEF (a zero difference adds nothing)
inline int padded_d(int D) { return D <= 16 ? 16 : MAX_COEF; }

// LDS of the alignment workgroup: b's ring, the row above the block (D, cells, diagonal steps), the values between wavefronts (two
// buffers), one flag
constexpr size_t dtw_lds_bytes(int DP) { return sizeof(float) * DP * RING + (sizeof(double) + 2 * sizeof(int)) * (RING + 2 * WAVES) + sizeof(int); }
constexpr size_t LDS_WORKGROUP_MAX = 64 * 1024;
static_assert(dtw_lds_bytes(MAX_COEF) <= LDS_WORKGROUP_MAX, "the alignment workgroup's LDS");

// bytes of direction codes of one pair: two bits per cell, four cells of a row to a byte
inline int64_t code_pitch(int64_t Tb) { return (Tb + 3) / 4; }
inline int64_t code_bytes(int64_t Ta, int64_t Tb) { return Ta * code_pitch(Tb); }

}  // namespace fdm
