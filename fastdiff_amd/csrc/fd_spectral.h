// fd_spectral.h -- host side of the multi-resolution STFT distances (include/fastdiff_hip_ext.h: "Multi-resolution STFT distances"): the
// constants that decide which workgroup and thread handles which frame and bin, the accepted configurations with their refusals, the
// frame counts, the tables the kernels read (window, twiddles) and the LDS sizing.  The transform itself is described by fd_dft.h.
// Plain C++ without the HIP runtime, so a stand-alone host program can include it.  tests/spectral_ref.py is the float64 oracle.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/fastdiff_hip_ext.h"
#include "fd_dft.h"

namespace fdx {

constexpr int MAX_RES = 4;                                    // FD_SPECTRAL_MAX_RES
constexpr int FRAME_TILE = 4;                                 // FD_SPECTRAL_FRAME_TILE: consecutive frames per workgroup of the transform stage
constexpr int SUM_CHUNK = 256;                                // FD_SPECTRAL_SUM_CHUNK: interleaved runs of frames in the finaliser
constexpr int THREADS = fdt::THREADS;                         // every workgroup
constexpr int NFFT_MIN = 512, NFFT_MAX = 2048;
constexpr int HOP_MIN = 16, WIN_MIN = 2;
constexpr int64_t MAX_SAMPLES = (int64_t)1 << 30;
constexpr int MSG = 160;                                      // room for a refusal's text

inline void defaults(fd_spectral_config *c)
{
    const int res[3][3] = {{512, 50, 240}, {1024, 120, 600}, {2048, 240, 1200}};      // Parallel WaveGAN's
    c->n_res = 3; c->reserved = 0;
    for (int r = 0; r < MAX_RES; ++r) {
        c->nfft[r] = r < 3 ? res[r][0] : 0;
        c->hop[r] = r < 3 ? res[r][1] : 0;
        c->win[r] = r < 3 ? res[r][2] : 0;
    }
    c->floor = 1e-7;
}

// neither infinite nor NaN, read from the bits (the library is built without NaN-honouring comparisons)
inline bool finite(double v)
{
    uint64_t u;
    memcpy(&u, &v, sizeof(u));
    return ((u >> 52) & 0x7FF) != 0x7FF;
}

// null = accepted, else what is wrong, with the value, in msg
inline const char *refusal(const fd_spectral_config &c, char (&msg)[MSG])
{
    if (c.reserved != 0) { snprintf(msg, MSG, "reserved = %d is not 0", (int)c.reserved); return msg; }
    if (c.n_res < 1 || c.n_res > MAX_RES) { snprintf(msg, MSG, "n_res = %d outside 1 .. %d", (int)c.n_res, MAX_RES); return msg; }
    if (!finite(c.floor) || !(c.floor > 0.0)) { snprintf(msg, MSG, "floor = %g is not a positive finite number", c.floor); return msg; }
    for (int r = 0; r < c.n_res; ++r) {
        if (!fdt::split_n1(c.nfft[r])) { snprintf(msg, MSG, "nfft[%d] = %d is not 512, 1024 or 2048", r, (int)c.nfft[r]); return msg; }
        if (c.win[r] < WIN_MIN || c.win[r] > c.nfft[r]) {
            snprintf(msg, MSG, "win[%d] = %d outside %d .. nfft = %d", r, (int)c.win[r], WIN_MIN, (int)c.nfft[r]);
            return msg;
        }
        if (c.hop[r] < HOP_MIN || c.hop[r] > c.nfft[r]) {
            snprintf(msg, MSG, "hop[%d] = %d outside %d .. nfft = %d", r, (int)c.hop[r], HOP_MIN, (int)c.nfft[r]);
            return msg;
        }
    }
    return nullptr;
}

inline int64_t frames(int64_t n, int hop) { return 1 + n / hop; }

// n <= short_len(c) is FD_SPECTRAL_SHORT: the largest nfft / 2 of an accepted configuration
inline int short_len(const fd_spectral_config &c)
{
    int m = 0;
    for (int r = 0; r < c.n_res; ++r) m = c.nfft[r] / 2 > m ? c.nfft[r] / 2 : m;
    return m;
}

inline int win_offset(int nfft, int win) { return (nfft - win) / 2; }

// the n1 of the first pass that can hold a sample under the window: [lo, hi)
inline void n1_range(int nfft, int win, int *lo, int *hi)
{
    const int n2 = fdt::split_n2(nfft), off = win_offset(nfft, win);
    *lo = off / n2;
    *hi = (off + win - 1) / n2 + 1;
}

// the table of one (nfft, win): the window placed in the frame [nfft], cos and sin of 2 pi m / nfft [nfft] each, rounded once from double
inline size_t table_floats(int nfft) { return 3 * (size_t)nfft; }
inline void tables(int nfft, int win, float *tab)
{
    const double pi = 3.14159265358979323846;
    const int off = win_offset(nfft, win);
    for (int i = 0; i < nfft; ++i) tab[i] = 0.0f;
    for (int i = 0; i < win; ++i) tab[off + i] = (float)(0.5 - 0.5 * cos(2.0 * pi * i / win));
    fdt::twiddles(nfft, tab + nfft, tab + 2 * nfft);
}

// static LDS of the transform workgroup: the transform's own floats and the reduction's four doubles per thread
constexpr size_t lds_bytes(int nfft) { return sizeof(float) * fdt::lds_floats(nfft) + sizeof(double) * 4 * THREADS; }
constexpr size_t LDS_WORKGROUP_MAX = 64 * 1024;               // what one workgroup takes without asking; two of the largest fit a CU's 160 KiB

}  // namespace fdx
