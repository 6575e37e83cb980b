// fd_stoi.h -- host side of the intelligibility measures (include/fastdiff_hip_ext.h: "STOI and ESTOI"): the constants, the one-third
// octave band table computed from its rule, the frame and segment counts, and the tables the kernels read (window, twiddles).
// Plain C++ without the HIP runtime, so a stand-alone host program can include it.  tests/stoi_ref.py is the float64 oracle.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fd_dft.h"

namespace fds {

constexpr int RATE = 10000;                                   // the rate the measure is defined at
constexpr int RATE_MIN = 8000, RATE_MAX = 192000;             // what fd_stoi_measure resamples from
constexpr int FRAME = 256, HOP = 128, NFFT = 512;
constexpr int BANDS = 15, SEG = 30;                           // one-third octave bands; frames of a 384 ms segment
constexpr double F_LOW = 150.0;                               // centre of the lowest band
constexpr double DYN_RANGE = 1e-4;                            // 40 dB on the frame norm = 1e-4 on the frame energy
constexpr double EPS = 2.220446049250313e-16;                 // 2^-52
constexpr int SCAN_TILE = 1024;                               // FD_STOI_SCAN_TILE: frames per workgroup of the compaction
constexpr int SEG_TILE = 16;                                  // FD_STOI_SEG_TILE: segments per workgroup of the segment stage
constexpr int BIN_LO = 7, BIN_HI = 219;                       // the bins the bands cover: [BIN_LO, BIN_HI)
constexpr int TAB_FLOATS = FRAME + 2 * NFFT;                  // window [256], cos [512], sin [512]

// F0 = len(range(0, n - 256, 128)): the last full frame is left out when n - 256 is a multiple of 128
inline int64_t frames(int64_t n) { return n > FRAME ? (n - FRAME + HOP - 1) / HOP : 0; }
// J for K kept frames: the silence-free signal has 128 (K - 1) + 256 samples, so M = frames(that) = K - 1 and J = M - 29
inline int64_t segments(int64_t kept) { return kept - 1 >= SEG ? kept - 1 - (SEG - 1) : 0; }

// lo[j], hi[j]: the bins nearest to 150 * 2^((2j - 1)/6) and 150 * 2^((2j + 1)/6) Hz on the grid k * 10000 / 512; band j = [lo, hi)
inline void bands(int *lo, int *hi)
{
    for (int j = 0; j < BANDS; ++j) {
        const double fl = F_LOW * pow(2.0, (2 * j - 1) / 6.0), fr = F_LOW * pow(2.0, (2 * j + 1) / 6.0);
        lo[j] = (int)floor(fl * NFFT / RATE + 0.5);
        hi[j] = (int)floor(fr * NFFT / RATE + 0.5);
    }
}

// w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257) (hanning(258)[1:-1]), then cos and sin of 2 pi m / 512, all rounded once from double
inline void tables(float *tab)
{
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < FRAME; ++i) tab[i] = (float)(0.5 - 0.5 * cos(2.0 * pi * (i + 1) / (FRAME + 1)));
    fdt::twiddles(NFFT, tab + FRAME, tab + FRAME + NFFT);
}

}  // namespace fds
