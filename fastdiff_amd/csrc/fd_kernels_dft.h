// fd_kernels_dft.h -- the one N-point DFT of a real frame that the mel front-end (fd_kernels_mel.hip, N = 1024), STOI
// (fd_kernels_stoi.hip, N = 512) and the STFT distances (fd_kernels_spectral.hip, N = 512, 1024, 2048) run, for a 256-thread workgroup:
// one Cooley-Tukey split N = N1 N2 (fd_dft.h: 16 x 32, 32 x 32, 32 x 64) through LDS, n = N2 n1 + n2, k = k1 + N1 k2,
//     A[n2][k1] = sum_n1 x[N2 n1 + n2] W_N1^(n1 k1);   B = A W_N^(n2 k1);   X[k1 + N1 k2] = sum_n2 B[n2][k1] W_N2^(n2 k2)
// two passes of N1- and N2-term sums instead of N-term ones.  Everything is float32: each sum is one fmaf chain over n1 (pass 1) or n2
// (pass 2) in ascending order, the step between them is rounded as written below, and every table index is an exact integer product
// into the one cos / sin table of 2 pi m / N (W_N1^q = (ct, -sn)[N2 q], W_N2^q = (ct, -sn)[N1 q]); there are no recurrences.  So a bin
// is the same float whichever thread forms it and whichever terms that are exactly zero are left out.  The caller loads ct, sn
// (fdt::twiddles) and its windowed frame into LDS, then: barrier, dft_pass1, barrier, dft_pass2, and a barrier before the next frame
// overwrites anything.  Neither function contains a barrier.
#pragma once
#include "fd_dft.h"

namespace fdk {

// Pass 1 and the step to pass 2: xw = the frame, of which only the n1 in [n1_lo, n1_hi) are read (all others are zero) -> the twiddled
// ar, ai [N2][ROW].  All pointers into LDS.  Thread = (n2 = tid % N2, k1 = g + G q), g = tid / N2, q < Q.
template <int N>
__device__ __forceinline__ void dft_pass1(const float *xw, const float *ct, const float *sn, int n1_lo, int n1_hi, float *ar, float *ai, int tid)
{
    constexpr int N1 = fdt::split_n1(N), N2 = fdt::split_n2(N), ROW = fdt::row(N), G = fdt::THREADS / N2, Q = N1 / G;
    static_assert(N1 * N2 == N && fdt::THREADS % N2 == 0 && N1 % G == 0 && ROW >= N1, "the split");
    const int n2 = tid % N2, g = tid / N2;
    float re[Q], im[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) re[q] = im[q] = 0.0f;
    for (int n1 = n1_lo; n1 < n1_hi; ++n1) {
        const float xv = xw[N2 * n1 + n2];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int t = ((n1 * (g + G * q)) & (N1 - 1)) * N2;
            re[q] = fmaf(xv, ct[t], re[q]);
            im[q] = fmaf(-xv, sn[t], im[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {                          // times W_N^(n2 k1) = (c, -s); n2 k1 <= (N2 - 1)(N1 - 1) < N
        const int k1 = g + G * q, t = n2 * k1;
        const float c = ct[t], s = sn[t];
        ar[n2 * ROW + k1] = fmaf(re[q], c, __fmul_rn(im[q], s));
        ai[n2 * ROW + k1] = fmaf(im[q], c, -__fmul_rn(re[q], s));
    }
}

// Pass 2: the bins k1 + N1 k2[j], j < K, of one k1; every ar[n2][k1], ai[n2][k1] is read once for the whole list.  UNROLL: the n2 whose
// LDS reads are issued together (it changes no value).
template <int N, int UNROLL = 4, int K>
__device__ __forceinline__ void dft_pass2(const float *ar, const float *ai, const float *ct, const float *sn, int k1, const int (&k2)[K],
                                          float (&re)[K], float (&im)[K])
{
    constexpr int N1 = fdt::split_n1(N), N2 = fdt::split_n2(N), ROW = fdt::row(N);
#pragma unroll
    for (int j = 0; j < K; ++j) re[j] = im[j] = 0.0f;
#pragma unroll UNROLL
    for (int n2 = 0; n2 < N2; ++n2) {
        const float xr = ar[n2 * ROW + k1], xi = ai[n2 * ROW + k1];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int t = ((n2 * k2[j]) & (N2 - 1)) * N1;
            const float c = ct[t], s = sn[t];              // times (c - i s)
            re[j] = fmaf(xr, c, fmaf(xi, s, re[j]));
            im[j] = fmaf(xi, c, fmaf(-xr, s, im[j]));
        }
    }
}

}  // namespace fdk
