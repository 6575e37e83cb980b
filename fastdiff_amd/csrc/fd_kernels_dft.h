// fd_kernels_dft.h -- the one N-point DFT of a real frame that the mel front-end (fd_kernels_mel.hip, N = 1024), STOI
// (fd_kernels_stoi.hip, N = 512) and the STFT distances (fd_kernels_spectral.hip, N = 512, 1024, 2048) run, for a 256-thread workgroup:
// one Cooley-Tukey split N = N1 N2 (fd_dft.h: 16 x 32, 32 x 32, 32 x 64) through LDS, n = N2 n1 + n2, k = k1 + N1 k2,
//     A[n2][k1] = sum_n1 x[N2 n1 + n2] W_N1^(n1 k1);   B = A W_N^(n2 k1);   X[k1 + N1 k2] = sum_n2 B[n2][k1] W_N2^(n2 k2)
// two passes of N1- and N2-term sums instead of N-term ones.  Everything is float32: each sum is one fmaf chain over n1 (pass 1) or n2
// (pass 2) in ascending order, the step between them is rounded as written below, and every table index is an exact integer product
// into the one cos / sin table of 2 pi m / N (W_N1^q = (ct, -sn)[N2 q], W_N2^q = (ct, -sn)[N1 q]); there are no recurrences.  So a bin
// is the same float whichever thread forms it and whichever terms that are exactly zero are left out.  The caller loads ct, sn
// (fdt::twiddles) and its windowed frame into LDS, then: barrier, dft_pass1, barrier, dft_pass2, and a barrier before the next frame
// overwrites anything.  Neither function contains a barrier.  Behind them: the inverse of the 1024-point transform for Griffin-Lim
// (fd_kernels_gl.hip), idft_pass1 and idft_pass2, the same split read backwards over the same table.
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

// The inverse of the 1024-point transform (fd_kernels_gl.hip; include/fastdiff_hip_ext.h, "Griffin-Lim", states it): the Hermitian half
// spectrum cr, ci [N / 2 + 1] -> the N real samples, through the same split read backwards, k = k1 + N1 k2, n = N2 n1 + n2:
//     D[k1][n2] = sum_k2 C^[k1 + N1 k2] W_N2^(-k2 n2);   E = D W_N^(-k1 n2);   x[N2 n1 + n2] = (1 / N) sum_k1 Re(E[k1][n2] W_N1^(-k1 n1))
// C^[k] = conj C[N - k] behind N / 2 makes the row N1 - k1 of E W_N1^(-k1 n1) the conjugate of the row k1: only k1 <= N1 / 2 is formed,
// the rows between count twice.  r1c, r1s [N1]: cos and sin of 2 pi j / N1 = (ct, sn)[N2 j], the table's own values laid side by side
// (a stride of N2 floats would put every lane of pass 1 on one LDS bank).  Again each sum is one fmaf chain in ascending order and the
// step between the passes is rounded as written.  The caller stores ci[0] = ci[N / 2] = 0 (a C2R transform ignores them), then: barrier,
// idft_pass1, barrier, idft_pass2.  Neither function contains a barrier.

// Pass 1 and the step to pass 2: -> er, ei [N1 / 2 + 1][N2].  Thread = (n2 = tid % N2, k1 in {g, g + G, N1 / 2}), g = tid / N2; every
// thread forms the row N1 / 2, the threads of g = 0 store it.
template <int N>
__device__ __forceinline__ void idft_pass1(const float *cr, const float *ci, const float *ct, const float *sn, const float *r1c, const float *r1s,
                                           float *er, float *ei, int tid)
{
    constexpr int N1 = fdt::split_n1(N), N2 = fdt::split_n2(N), G = fdt::THREADS / N2, H = N1 / 2;
    static_assert(N1 == N2 && 2 * G == H, "written for the 32 x 32 split: k1 = g, g + G and N1 / 2 are the rows 0 .. N1 / 2");
    const int n2 = tid % N2, g = tid / N2;
    const int k1[3] = {g, g + G, H};
    float re[3], im[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) re[j] = im[j] = 0.0f;
#pragma unroll 4
    for (int k2 = 0; k2 < N2 / 2; ++k2) {                  // k <= N / 2: the bin itself
        const int t = (k2 * n2) & (N2 - 1);
        const float c = r1c[t], s = r1s[t];                // times (c + i s)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float vr = cr[k1[j] + N1 * k2], vi = ci[k1[j] + N1 * k2];
            re[j] = fmaf(vr, c, fmaf(-vi, s, re[j]));
            im[j] = fmaf(vr, s, fmaf(vi, c, im[j]));
        }
    }
#pragma unroll 4
    for (int k2 = N2 / 2; k2 < N2; ++k2) {                 // k >= N / 2: the conjugate of bin N - k (k1 = 0, k2 = N2 / 2: bin N / 2 itself, ci = 0)
        const int t = (k2 * n2) & (N2 - 1);
        const float c = r1c[t], s = r1s[t];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float vr = cr[N - k1[j] - N1 * k2], vi = -ci[N - k1[j] - N1 * k2];
            re[j] = fmaf(vr, c, fmaf(-vi, s, re[j]));
            im[j] = fmaf(vr, s, fmaf(vi, c, im[j]));
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {                          // times W_N^(-k1 n2) = (c, +s); k1 n2 <= (N1 / 2)(N2 - 1) < N
        if (j == 2 && g != 0) break;
        const int t = k1[j] * n2;
        const float c = ct[t], s = sn[t];
        er[k1[j] * N2 + n2] = fmaf(re[j], c, -__fmul_rn(im[j], s));
        ei[k1[j] * N2 + n2] = fmaf(im[j], c, __fmul_rn(re[j], s));
    }
}

// Pass 2: the samples N2 n1[q] + n2, q < Q, of one n2; every er[k1][n2], ei[k1][n2] is read once for the whole list.
template <int N, int Q>
__device__ __forceinline__ void idft_pass2(const float *er, const float *ei, const float *r1c, const float *r1s, int n2, const int (&n1)[Q],
                                           float (&x)[Q])
{
    constexpr int N1 = fdt::split_n1(N), N2 = fdt::split_n2(N), H = N1 / 2;
    float acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.0f;
#pragma unroll 5
    for (int k1 = 1; k1 < H; ++k1) {
        const float xr = er[k1 * N2 + n2], xi = ei[k1 * N2 + n2];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int t = (k1 * n1[q]) & (N1 - 1);
            acc[q] = fmaf(xr, r1c[t], fmaf(-xi, r1s[t], acc[q]));
        }
    }
    const float e0 = er[n2], eh = er[H * N2 + n2];
#pragma unroll
    for (int q = 0; q < Q; ++q)                            // (the factors 2 and 1 / N are exact)
        x[q] = __fmul_rn(__fadd_rn(__fadd_rn(e0, (n1[q] & 1) ? -eh : eh), __fmul_rn(2.0f, acc[q])), 1.0f / N);
}

}  // namespace fdk
