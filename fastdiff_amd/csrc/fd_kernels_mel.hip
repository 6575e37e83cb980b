// fd_kernels_mel.hip -- the mel front-end in front of the vocoder: wav -> log-mel [80, T].
//
// Reference: data_gen/tts/data_gen_utils.py:93-147 (process_utterance, vocoder='pwg'):
//   librosa.stft(n_fft=1024, hop=256, win=1024, window="hann", center, pad_mode="constant") -> |.| -> librosa.filters.mel(22050, 1024,
//   80, 80, 7600) @ . -> log10(max(1e-6, .)).   One workgroup = one frame.  The 1024-point DFT is the split transform of
// fd_kernels_dft.h (32 x 32): two passes of 32-term sums through LDS, ~700 FMAs per thread instead of the ~4000 LDS-bound ones of a
// direct DFT (0.16 ms for the B=8 x 864-frame benchmark batch).  The 513 magnitudes go back to LDS and 80 threads apply their
// triangular filter and the log.
//
// TACO = the Tacotron front-end (data_gen/tts/tacotron/layers.py:42-80 TacotronSTFT.mel_spectrogram over tacotron/stft.py:78-104
// STFT.transform, driven by vocoder_binarizer_tacotron.py:110-116): the same transform with the signal REFLECT-padded by 512
// (stft.py:84-88), filters.mel(22050, 1024, 80, 0, 8000) and ln(clamp(., 1e-5)) (audio_processing.py:78-84).
#include "fd_internal.h"
#include "fd_kernels.h"
#include "fd_kernels_dft.h"

namespace fdk {

template <bool TACO>
__global__ void __launch_bounds__(256) k_mel_frontend(const float *__restrict__ wav, float *__restrict__ mel, const float *__restrict__ tab,
                                                      const int *__restrict__ fb_lo, const int *__restrict__ fb_n,
                                                      const int *__restrict__ fb_off, const float *__restrict__ fb_w, int64_t n_samples,
                                                      int T)
{
    constexpr int N = 1024;
    static_assert(fdt::split_n1(N) == 32 && fdt::split_n2(N) == 32, "the bins below are cut as 32 x 32");
    __shared__ float ct[N], st[N], xw[N], br[32 * fdt::row(N)], bi[32 * fdt::row(N)], mag[544];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lo5 = tid & 31, g = tid >> 5;
    const float *w = wav + (int64_t)b * n_samples;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = j * 256 + tid;
        int64_t p = (int64_t)t * 256 + n - 512;                       // center=True: n_fft/2 zeros in front (pad_mode="constant")
        if (TACO) p = p < 0 ? -p : (p >= n_samples ? 2 * (n_samples - 1) - p : p);      // ... or the signal mirrored about its end samples
        ct[n] = tab[n];
        st[n] = tab[1024 + n];
        xw[n] = (p >= 0 && p < n_samples) ? w[p] * tab[2048 + n] : 0.0f;      // periodic Hann window
    }
    __syncthreads();
    dft_pass1<N>(xw, ct, st, 0, 32, br, bi, tid);
    __syncthreads();
    // pass 2: thread = (k1 = lo5, k2 in {g, g + 8, 16 (g == 0)}); only k <= 512 is kept
    {
        float re[3], im[3];
        const int k2s[3] = {g, g + 8, 16};
        dft_pass2<N, 8>(br, bi, ct, st, lo5, k2s, re, im);
        // |X| = sqrt(re re + im im), rounded the way this kernel has always been compiled -- the two bins of every thread contracted to
        // fmaf(im, im, re re), bin 512 not contracted -- and written out, so that the compiler's choice no longer decides a mel value
        mag[lo5 + 32 * g] = sqrtf(fmaf(im[0], im[0], __fmul_rn(re[0], re[0])));
        mag[lo5 + 32 * (g + 8)] = sqrtf(fmaf(im[1], im[1], __fmul_rn(re[1], re[1])));
        if (g == 0 && lo5 == 0) mag[512] = sqrtf(__fadd_rn(__fmul_rn(re[2], re[2]), __fmul_rn(im[2], im[2])));
    }
    __syncthreads();
    if (tid < 80) {
        const float *wv = fb_w + fb_off[tid];
        const float *mg = mag + fb_lo[tid];
        float acc = 0.0f;
        for (int j = 0; j < fb_n[tid]; ++j) acc = fmaf(wv[j], mg[j], acc);
        mel[((int64_t)b * 80 + tid) * T + t] = TACO ? logf(fmaxf(1e-5f, acc)) : log10f(fmaxf(1e-6f, acc));
    }
}

hipError_t mel_frontend(const Launch &L, const float *wav, int B, int64_t n_samples, float *mel, int T)
{
    const MelTables &m = L.ctx->mel[L.ctx->mel_variant];
    if (L.ctx->mel_variant == MEL_TACOTRON)
        FD_LAUNCH(L, "mel_frontend_tacotron", k_mel_frontend<true>, dim3(T, B), dim3(256), 0, wav, mel, m.tab, m.fb_lo, m.fb_n, m.fb_off, m.fb_w, n_samples, T);
    else
        FD_LAUNCH(L, "mel_frontend", k_mel_frontend<false>, dim3(T, B), dim3(256), 0, wav, mel, m.tab, m.fb_lo, m.fb_n, m.fb_off, m.fb_w, n_samples, T);
    return hipSuccess;
}

}  // namespace fdk
