// fd_kernels_mel.hip -- the mel front-end in front of the vocoder: wav -> log-mel [80, T].
//
// Reference: data_gen/tts/data_gen_utils.py:93-147 (process_utterance, vocoder='pwg'):
//   librosa.stft(n_fft=1024, hop=256, win=1024, window="hann", center, pad_mode="constant") -> |.| -> librosa.filters.mel(22050, 1024,
//   80, 80, 7600) @ . -> log10(max(1e-6, .)).   One workgroup = one frame.  The 1024-point DFT is the split transform of
// fd_kernels_dft.h (32 x 32): two passes of 32-term sums through LDS, ~700 FMAs per thread instead of the ~4000 LDS-bound ones of a
// direct DFT (0.16 ms for the B=8 x 864-frame benchmark batch).  The 513 magnitudes go back to LDS and 80 threads apply their
// triangular filter and the log.  The frame itself is mel_frame (fd_kernels_melframe.h), which the cepstrum kernel shares.
//
// TACO = the Tacotron front-end (data_gen/tts/tacotron/layers.py:42-80 TacotronSTFT.mel_spectrogram over tacotron/stft.py:78-104
// STFT.transform, driven by vocoder_binarizer_tacotron.py:110-116): the same transform with the signal REFLECT-padded by 512
// (stft.py:84-88), filters.mel(22050, 1024, 80, 0, 8000) and ln(clamp(., 1e-5)) (audio_processing.py:78-84).
#include "fd_internal.h"
#include "fd_kernels.h"
#include "fd_kernels_melframe.h"

namespace fdk {

template <bool TACO>
__global__ void __launch_bounds__(256) k_mel_frontend(const float *__restrict__ wav, float *__restrict__ mel, const float *__restrict__ tab,
                                                      const int *__restrict__ fb_lo, const int *__restrict__ fb_n,
                                                      const int *__restrict__ fb_off, const float *__restrict__ fb_w, int64_t n_samples,
                                                      int T)
{
    __shared__ MelFrameLds s;
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float v = mel_frame<TACO>(s, wav + (int64_t)b * n_samples, n_samples, t, tab, fb_lo, fb_n, fb_off, fb_w, tid);
    if (tid < 80) mel[((int64_t)b * 80 + tid) * T + t] = v;
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
