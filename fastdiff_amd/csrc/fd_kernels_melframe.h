// fd_kernels_melframe.h -- one frame of the mel front-end for a 256-thread workgroup: window, the split 1024-point DFT of
// fd_kernels_dft.h, the 513 magnitudes, the 80 triangular filters and the log.  k_mel_frontend (fd_kernels_mel.hip) writes the value out;
// k_cepstra (fd_kernels_mcd.hip) goes on to the cepstrum with it, so both see the same float for the same frame.
#pragma once
#include "fd_kernels_dft.h"

namespace fdk {

struct MelFrameLds { float ct[1024], st[1024], xw[1024], br[32 * fdt::row(1024)], bi[32 * fdt::row(1024)], mag[544]; };

// Frame t of the n_samples samples at w -> the log-mel of filter tid in the threads tid < 80 (the others return 0).  TACO: the signal is
// reflected about its end samples (n_samples > 512) and the log is ln(max(1e-5, .)); else zeros around it and log10(max(1e-6, .)).
// Nothing at or behind w + n_samples is read.  Contains three barriers; every thread of the workgroup calls it.
template <bool TACO>
__device__ __forceinline__ float mel_frame(MelFrameLds &s, const float *__restrict__ w, int64_t n_samples, int t, const float *__restrict__ tab,
                                           const int *__restrict__ fb_lo, const int *__restrict__ fb_n, const int *__restrict__ fb_off,
                                           const float *__restrict__ fb_w, int tid)
{
    constexpr int N = 1024;
    static_assert(fdt::split_n1(N) == 32 && fdt::split_n2(N) == 32, "the bins below are cut as 32 x 32");
    const int lo5 = tid & 31, g = tid >> 5;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = j * 256 + tid;
        int64_t p = (int64_t)t * 256 + n - 512;                       // center=True: n_fft/2 zeros in front (pad_mode="constant")
        if (TACO) p = p < 0 ? -p : (p >= n_samples ? 2 * (n_samples - 1) - p : p);      // ... or the signal mirrored about its end samples
        s.ct[n] = tab[n];
        s.st[n] = tab[1024 + n];
        s.xw[n] = (p >= 0 && p < n_samples) ? w[p] * tab[2048 + n] : 0.0f;      // periodic Hann window
    }
    __syncthreads();
    dft_pass1<N>(s.xw, s.ct, s.st, 0, 32, s.br, s.bi, tid);
    __syncthreads();
    // pass 2: thread = (k1 = lo5, k2 in {g, g + 8, 16 (g == 0)}); only k <= 512 is kept
    {
        float re[3], im[3];
        const int k2s[3] = {g, g + 8, 16};
        dft_pass2<N, 8>(s.br, s.bi, s.ct, s.st, lo5, k2s, re, im);
        // |X| = sqrt(re re + im im), rounded the way this kernel has always been compiled -- the two bins of every thread contracted to
        // fmaf(im, im, re re), bin 512 not contracted -- and written out, so that the compiler's choice no longer decides a mel value
        s.mag[lo5 + 32 * g] = sqrtf(fmaf(im[0], im[0], __fmul_rn(re[0], re[0])));
        s.mag[lo5 + 32 * (g + 8)] = sqrtf(fmaf(im[1], im[1], __fmul_rn(re[1], re[1])));
        if (g == 0 && lo5 == 0) s.mag[512] = sqrtf(__fadd_rn(__fmul_rn(re[2], re[2]), __fmul_rn(im[2], im[2])));
    }
    __syncthreads();
    if (tid >= 80) return 0.0f;
    const float *wv = fb_w + fb_off[tid];
    const float *mg = s.mag + fb_lo[tid];
    float acc = 0.0f;
    for (int j = 0; j < fb_n[tid]; ++j) acc = fmaf(wv[j], mg[j], acc);
    return TACO ? logf(fmaxf(1e-5f, acc)) : log10f(fmaxf(1e-6f, acc));
}

}  // namespace fdk
