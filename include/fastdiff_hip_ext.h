/*
 * fastdiff_hip_ext.h -- libfastdiff_hip.so: the rows next to the inference path (the int16 waveform epilogue
 * behind fd_sample and the mel front-end in front of it) and the test / introspection hooks.  Conventions: fastdiff_hip.h.
 */
#ifndef FASTDIFF_HIP_EXT_H
#define FASTDIFF_HIP_EXT_H

#include "fastdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Waveform epilogue: wav/abs(wav).max() per utterance (FastDiff.py:110), *32767 -> int16
 * (utils/audio.py:11-16).  wav [B,1,L] device -> pcm [B,L] device int16. */
FD_API int fd_peak_normalize_int16(fd_handle h, const float *wav, int B, int64_t L, int16_t *pcm, void *stream);
/* The same for a zero-padded batch (fd_sample with lens): valid [B] host = samples of each utterance (lens[b]*256); the peak is
 * searched over the utterance's own samples only -- what FastDiff.py:110 sees for a batch of one -- and pcm behind them is 0.
 * valid NULL = the call above.  B <= 4096. */
FD_API int fd_peak_normalize_int16_ragged(fd_handle h, const float *wav, int B, int64_t L, const int64_t *valid, int16_t *pcm,
                                          void *stream);

/* Mel front-end in front of the vocoder: process_utterance(..., vocoder='pwg') of
 * data_gen/tts/data_gen_utils.py:93-147 = librosa.stft(n_fft 1024, hop 256, win 1024, "hann", center, pad_mode "constant") ->
 * magnitude -> librosa.filters.mel(22050, 1024, 80, fmin 80, fmax 7600) -> log10(max(1e-6, .)).
 *   wav [B][n_samples] device, float (int16 PCM / 32768, as librosa.core.load scales it)
 *   mel [B][80][T] device, T <= 1 + n_samples/256 frames (librosa's frame count; the test-time collater then drops the last one).
 * With option "mel" = "tacotron": TacotronSTFT.mel_spectrogram of data_gen/tts/tacotron/layers.py:42-80 (over tacotron/stft.py:78-104,
 * as vocoder_binarizer_tacotron.py:110-116 drives it for FastDiff_tacotron.yaml): the signal reflect-padded by 512 instead of
 * zero-padded (needs n_samples > 512), filters.mel(22050, 1024, 80, 0, 8000), ln(clamp(., 1e-5)). */
FD_API int fd_mel_spectrogram(fd_handle h, const float *wav, int B, int64_t n_samples, float *mel, int T, void *stream);

/* The mel filter bank of the front-end selected by option "mel" -- the matrix the reference gets from
 * librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) at data_gen/tts/data_gen_utils.py:122-134 ('pwg') and
 * data_gen/tts/tacotron/layers.py:42-60 (TacotronSTFT.mel_basis).
 *   fd_set_mel_filterbank: fb [80][513] HOST, row-major (librosa's own layout) -- the weights are then used exactly as given (per filter
 *     the span first..last non-zero bin, summed in ascending bin order); fb NULL restores the default.  A deployment that has librosa
 *     passes `librosa.filters.mel(sr=22050, n_fft=1024, n_mels=80, fmin=80, fmax=7600)` ('pwg') or `(..., fmin=0, fmax=8000)`
 *     (Tacotron) itself.  Takes effect for the calls enqueued after it; n_mels / n_bins must be 80 / 513.
 *   fd_get_mel_filterbank: copies the bank in use to fb_out [80][513] host; returns 1 if it was supplied by the caller, 0 if it is the
 *     default, < 0 on error.
 * The DEFAULT is a restatement of librosa's published algorithm (Slaney scale, area-normalised triangles) -- librosa is absent from the
 * build image; its values are pinned on an independent derivation and on a third-party implementation of librosa.filters.mel
 * (transformers.audio_utils.mel_filter_bank, slaney / slaney: equal to 2e-16; tests/test_mel_frontend.py), not on librosa itself. */
FD_API int fd_set_mel_filterbank(fd_handle h, const float *fb, int n_mels, int n_bins);
FD_API int fd_get_mel_filterbank(fd_handle h, float *fb_out, int n_mels, int n_bins);

/* Sample-rate conversion around the vocoder: recordings of any rate and channel count in, waveforms of any rate out -- what the
 * reference gets from librosa.core.load(wav_path, sr=sample_rate) at the first line of its front-end (data_gen/tts/data_gen_utils.py:111,
 * :40-49; vocoders/pwg.py:132): down-mix to mono, resample to the model's rate.
 *
 * The operator.  up / down = sr_out / sr_in reduced by their gcd, q = max(up, down), half = Z q.  The prototype low-pass in double,
 *     g[k] = sinc(rolloff (k - half) / q) * kaiser(k; 2 half + 1, beta),  k = 0 .. 2 half,  divided by its sum
 * (= scipy.signal.firwin(2 half + 1, rolloff / q, window=("kaiser", beta))), h = up g rounded once to float32, and
 *     y[i] = sum_j x[j] h[i down - j up + half],   x = 0 outside [0, n),   i = 0 .. n_out - 1,   n_out = ceil(n up / down)
 * (= scipy.signal.resample_poly(x, up, down, window=g), sample for sample).  Z = 64 zero crossings, rolloff = 0.9475937167399596,
 * beta = 14.769656459379492: the parameters resampy publishes for its "kaiser_best" filter, which the librosa of the reference's time
 * used by default.  They are restated here, not checked against resampy / librosa (absent from the build image), and resampy
 * interpolates a tabulated filter where this evaluates it at the exact tap positions: the same design, not the same bits.
 * Taps per output: K = ceil((2 half + 1) / up) (48k -> 22.05k: 279; 16k -> 22.05k: 129).
 *
 * Summation order (fixed: an item's output is bit-identical alone, anywhere in a ragged batch, at any pitch or alignment): output i
 * adds its products x[j] h[.] with j ASCENDING into one float32 accumulator that starts at +0, one fmaf per product; products whose x
 * lies outside [0, n) are left out (they are exact zeros).  No atomics, no scratch of the handle.
 *
 * The polyphase table ([up][K rounded up to 4], every row in the order its output walks x) is built on the host in double, cached on
 * the handle per reduced ratio and uploaded at the first use of that ratio -- never inside a stream capture, where a ratio that has
 * not been used before is refused with FD_ERR_STATE. */
#define FD_RESAMPLE_TILE 256      /* consecutive outputs of one item that one workgroup computes */
#define FD_RESAMPLE_MAX_RATIO 1024 /* max(up, down) after reduction */
enum { FD_PCM_F32 = 0, FD_PCM_S16 = 1, FD_PCM_S32 = 2, FD_PCM_U8 = 3 };

/* n_out = ceil(n up / down) for n >= 0 (pure host code, no handle).  FD_ERR_INVALID: n < 0 or a rate < 1; FD_ERR_UNSUPPORTED:
 * max(up, down) > 1024 after reduction.  Equal rates give n. */
FD_API int64_t fd_resample_out_len(int64_t n, int sr_in, int sr_out);
/* The float32 prototype h (2 half + 1 values; pure host code, no handle, like fd_pack_source).  Returns its length and writes the first
 * min(capacity, length) values (taps NULL: sizes only); up / down / half receive the reduced ratio and half (each may be NULL).  Equal
 * rates: up = down = 1, the filter a converter between two different rates would use (fd_resample itself then copies). */
FD_API int fd_resample_taps(int sr_in, int sr_out, float *taps, int64_t capacity, int *up, int *down, int *half);
/* src -> dst [B][out_len(n_in)] float mono at sr_out, asynchronous on `stream`, one launch per 64 items.
 *   src        device; item b's frame j, channel c at element (b * src_pitch + j * channels + c) of the source type `format`:
 *              FD_PCM_F32 as is, _S16 / 32768, _S32 float(v) / 2^31, _U8 (v - 128) / 128 (what librosa.core.load hands on); any alignment
 *              the type allows
 *   channels   1 .. 8 interleaved; summed in channel order in float32, then divided by `channels` (correctly rounded)
 *   n_in       frames per item; src_pitch >= n_in * channels ELEMENTS between items
 *   valid_in   HOST [B] or NULL: frames of each item that count, 1 .. n_in; its outputs behind out_len(valid_in[b]) up to out_len(n_in)
 *              are written as 0
 *   dst_pitch  floats between the rows of dst, >= out_len(n_in)
 * Equal rates: conversion, down-mix and copy, no filter.
 * FD_ERR_INVALID: a null pointer, channels outside 1..8, an unknown format, B < 1, n_in < 1, a pitch too short, valid_in[b] outside
 * [1, n_in]; FD_ERR_UNSUPPORTED: max(up, down) > 1024.  Every refusal with a handle leaves its message in fd_last_error. */
FD_API int fd_resample(fd_handle h, const void *src, int format, int channels, int B, int64_t n_in, int64_t src_pitch,
                       const int64_t *valid_in, int sr_in, int sr_out, float *dst, int64_t dst_pitch, void *stream);

/* BS.1770 loudness: measure a waveform's integrated loudness and normalise it to a target, on the device -- the level control behind the
 * vocoder next to the peak epilogue, and the reference's process_utterance(loud_norm=True) in front of the mel
 * (data_gen/tts/data_gen_utils.py:115-120: pyloudnorm.Meter(rate) with its defaults, one channel, -22 LUFS; :42-47: -20 LUFS).
 *
 * The measurement.  K-weighting = two biquads in series, RBJ forms divided by a0, w0 = 2 pi fc / rate, alpha = sin w0 / (2 Q):
 *   high shelf  G = 4 dB, Q = 1/sqrt 2, fc = 1500, A = 10^(G/40), c = cos w0, s = 2 sqrt(A) alpha:
 *     b = [A((A+1)+(A-1)c+s), -2A((A-1)+(A+1)c), A((A+1)+(A-1)c-s)],  a = [(A+1)-(A-1)c+s, 2((A-1)-(A+1)c), (A+1)-(A-1)c-s]
 *   high pass   Q = 0.5, fc = 38:  b = [(1+c)/2, -(1+c), (1+c)/2],  a = [1+alpha, -2c, 1-alpha]
 * from zero state.  These are pyloudnorm's filters, NOT the 48 kHz coefficient table of ITU-R BS.1770: a full-scale 997 Hz sine reads
 * -3.052 / -3.066 / -3.083 LUFS at 48000 / 22050 / 16000 Hz where the ITU table gives -3.01.  The reference depends on pyloudnorm, so
 * that is what is followed.  Blocks of T_g = 0.4 s every 0.1 s: nb = int(round((n / rate - 0.4) / 0.1) + 1) (round half to even),
 * block j = samples [int(0.4 (0.25 j) rate), int(0.4 (0.25 j + 1) rate)) cut to n, z_j = sum y^2 / (0.4 rate),
 * l_j = -0.691 + 10 log10 z_j.  Absolute gate J = {l_j >= -70}; relative threshold = -0.691 + 10 log10(mean_J z) - 10;
 * J' = {l_j > threshold and l_j > -70}; LUFS = -0.691 + 10 log10(mean_J' z).  gain = 10^((target - LUFS) / 20); where peak gain > 1
 * the reference divides by the new peak instead (:119-120), which is peak normalisation of that utterance.
 *
 * Status of an utterance: FD_LOUDNESS_SHORT  n < int(0.4 rate) (pyloudnorm raises), FD_LOUDNESS_SILENT  J or J' empty,
 * FD_LOUDNESS_CLIPPED  the gain was replaced by 1 / peak, else FD_LOUDNESS_OK.
 *
 * The filter is a linear recurrence and is computed exactly, not with a warm-up: an utterance is cut into tiles of FD_LOUDNESS_TILE
 * samples (one workgroup each: the grid is tiles x B, so one long waveform fills the device), a tile into 256 runs of 64 samples, one
 * per lane.  With the cascade written as s' = A s + B x (4 states), pass 1 runs every run from zero state and combines the end states
 * with A^64, A^128, ... A^8192 (computed on the host in double, passed by value) into the tile's zero-state end state; a carry step
 * propagates the true state across tiles with A^16384; pass 2 runs every run again from its true incoming state and sums y^2 per
 * 100 ms segment (block j is segments j .. j + 3: both borders are the same double expression).  The filtered signal never reaches
 * memory.  State, powers and sums are float64.  Summation order is fixed -- a lane adds its samples in ascending order, a run that
 * straddles a segment border gives two partials, a tile's partials are added over lanes in a fixed order, a segment's over tiles in tile
 * order, no floating-point atomics (the peak is an atomicMax on non-negative float bits, which has no order) -- so an utterance's record
 * and output are bit-identical alone, anywhere in a ragged batch and from call to call.  Samples behind valid[b] are never read as signal.
 * Coefficients and powers travel as kernel arguments: nothing is uploaded, the calls can be captured (with `valid`, its B lengths go
 * through the handle's staging ring as in fd_peak_normalize_int16_ragged).  Tile states and partial sums live in a buffer of the handle
 * that grows at the first call that needs more -- never inside a stream capture, where such a call is refused with FD_ERR_STATE.  A
 * graph that holds a captured call points into that buffer: capture after the largest shape has been seen, or capture again. */
#define FD_LOUDNESS_TILE 16384      /* samples of one utterance that one workgroup filters */
enum { FD_LOUDNESS_OK = 0, FD_LOUDNESS_SHORT = 1, FD_LOUDNESS_SILENT = 2, FD_LOUDNESS_CLIPPED = 3 };
typedef struct fd_loudness {
    double lufs;           /* integrated loudness; -inf for SHORT and SILENT */
    float gain;            /* what fd_loudness_normalize scales with: 10^((target - lufs) / 20), 1 / peak if CLIPPED, 1 if SHORT / SILENT
                              (and always 1 from fd_loudness_measure) */
    float peak;            /* max |wav| over the utterance's own samples */
    int32_t blocks;        /* nb (0 if SHORT) */
    int32_t gated;         /* |J'|: the blocks the result is the mean of */
    int32_t status;        /* FD_LOUDNESS_* */
    int32_t reserved;      /* 0 */
} fd_loudness;

/* The ten coefficients, divided by a0: shelf b0 b1 b2 a1 a2, high pass b0 b1 b2 a1 a2 (pure host code, no handle).
 * FD_ERR_INVALID: coef10 NULL or a rate outside 8000 .. 192000. */
FD_API int fd_loudness_design(int rate, double *coef10);
/* nb for n samples at `rate`, 0 if n < int(0.4 rate) (SHORT); pure host code.  FD_ERR_INVALID: n < 0 or a rate outside 8000 .. 192000. */
FD_API int64_t fd_loudness_blocks(int64_t n, int rate);
/* wav [B][L] device float -> rec_dev [B] device records, asynchronous on `stream`.  valid: HOST [B] or NULL = samples of each
 * utterance that count (1 .. L).  B <= 4096, rate 8000 .. 192000. */
FD_API int fd_loudness_measure(fd_handle h, const float *wav, int B, int64_t L, const int64_t *valid, int rate, fd_loudness *rec_dev,
                               void *stream);
/* Measure, then scale to target_lufs.  out_f32 [B][L] and / or out_pcm [B][L] (device; at least one), rec_dev [B] device or NULL.
 *   out_f32: wav gain; CLIPPED: wav / peak; SHORT and SILENT: wav unchanged
 *   out_pcm: v = wav gain in float32, (int16_t)(v * 32767.0f); SHORT, SILENT and CLIPPED: exactly what
 *            fd_peak_normalize_int16_ragged writes (wav / peak, then * 32767), bit for bit
 * Both are 0 behind valid[b].  Like the peak epilogue and fd_mel_spectrogram, neither call settles a pending lazily checked fd_sample
 * (fastdiff_hip.h: fd_sample_check): their result is provisional with it.
 * FD_ERR_INVALID: a null pointer, B outside 1 .. 4096, L < 1, a rate outside 8000 .. 192000, valid[b] outside [1, L], a target that
 * is not finite; FD_ERR_STATE: the scratch buffer would have to grow inside a stream capture. */
FD_API int fd_loudness_normalize(fd_handle h, const float *wav, int B, int64_t L, const int64_t *valid, int rate, double target_lufs,
                                 float *out_f32, int16_t *out_pcm, fd_loudness *rec_dev, void *stream);

/* STOI and ESTOI: how intelligible a degraded waveform is against the clean one (Taal, Hendriks, Heusdens, Jensen 2011; Jensen and Taal
 * 2016) -- the objective score next to MOS and PESQ in the FastDiff paper's table, which the reference has no code for: people run pystoi
 * over the *_gt.wav / *_pred.wav pairs that test_step writes (FastDiff.py:113-117).  pystoi is not in the build image, so THIS TEXT defines
 * the measurement; it follows pystoi's conventions AS RECALLED, NOT AS CHECKED against its source, and tests/stoi_ref.py restates it in
 * float64 numpy.  A deployment that has pystoi should expect agreement to about the third decimal, from the two deviations stated below.
 *
 * Inputs: a clean waveform x and a degraded one y of the same length n and rate.
 *  1. Resample.  If the rate is not 10000, both go through fd_resample to 10000 Hz: n' = fd_resample_out_len(n, rate, 10000) samples.
 *     DEVIATION: pystoi uses an Octave-compatible polyphase filter here; this is the library's own kaiser_best design.
 *  2. Frames.  w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257), i = 0 .. 255 (hanning(258)[1:-1]).  Frame i covers samples
 *     [128 i, 128 i + 256), i = 0 .. F0 - 1, F0 = ceil((n' - 256) / 128) for n' > 256, else 0 (pystoi's range(0, len - 256, 128): the
 *     last full frame is left out when n' - 256 is a multiple of 128).
 *  3. Silent frames.  E_i = sum (w x_i)^2 on the clean signal only; frame i is kept iff E_i > 1e-4 max_i E_i (40 dB on the frame norm;
 *     pystoi's "+ eps" inside its log matters only for an all-zero signal, which is SILENT here).  The kept frames in order,
 *     k = 0 .. K - 1 with source index src[k], windowed by w, are overlap-added at hop 128 into x_s and y_s of 128 (K - 1) + 256 samples
 *     each; the same mask serves y.  The hop is half a frame, so every sample of x_s is the sum of at most two windowed source
 *     samples: a gather.
 *  4. STFT.  M = K - 1 frames of x_s and y_s (rule 2 again: pystoi drops the last frame here too), each windowed by w again and
 *     zero-padded to 512; P[k] = |X[k]|^2, k = 0 .. 256.
 *  5. Bands.  A[j][m] = sqrt(sum_{k = lo[j]}^{hi[j] - 1} P[k]), j = 0 .. 14, with
 *       lo = 7 9 11 14 17 22 27 34 43 55 69 87 109 138 174,   hi = 9 11 14 17 22 27 34 43 55 69 87 109 138 174 219:
 *     the bins nearest to 150 * 2^((2j -+ 1) / 6) Hz on the grid k * 10000 / 512 (fd_stoi_bands computes them from that rule).
 *  6. Segments.  Segment s = 0 .. J - 1 holds frames [s, s + 30) (384 ms), J = M - 29.
 *  7. STOI.  Per segment and band over the 30 frames: c = ||X|| / (||Y|| + eps), eps = 2^-52; Y' = min(c Y, (1 + 10^(15/20)) X); the
 *     means of X and Y' removed, each divided by its norm plus eps; d = sum X Y' / (15 J).
 *  8. ESTOI.  Per segment on the 15 x 30 matrices of X and Y separately: each row (a band over time) mean removed and divided by its
 *     norm plus eps, then each column (a frame over bands) likewise; d_e = sum X Y / (30 J).
 *     DEVIATION: pystoi adds eps-scaled random noise before each normalisation; that is left out.
 *  9. Status.  FD_STOI_SHORT: F0 = 0, or K < 31 (M < 30: not one segment; pystoi returns 1e-5 with a warning);  FD_STOI_SILENT: F0 > 0 and
 *     max E_i == 0;  else FD_STOI_OK.  stoi and estoi are NaN unless OK.
 *
 * On the device: frame energies in float32 (one wavefront per frame; the maximum by atomicMax on non-negative float bits, which has no
 * order), the mask and an exclusive scan over tiles of FD_STOI_SCAN_TILE frames with a carry across tiles (any frame count) that writes
 * src[] and K, then one workgroup per STFT frame and signal (gather, window, a 16 x 32 split 512-point transform in LDS, 15 float32
 * band amplitudes), then the segment stage in float64, FD_STOI_SEG_TILE segments per workgroup, and per-segment partials added in
 * segment order.  Every sum has a fixed order and there are no floating-point atomics: an utterance's record is bit-identical alone,
 * anywhere in a ragged batch with anything behind it, and from call to call.  Samples behind valid[b] are never read as signal.
 * Scratch (energies, src, band amplitudes, partials, the two 10 kHz signals) lives in a buffer of the handle that grows at the first call
 * that needs more -- never inside a stream capture, where such a call is refused with FD_ERR_STATE; the window and twiddle table is
 * uploaded at the first call; the internal resample inherits fd_resample's rule about a ratio first seen inside a capture.  A graph that
 * holds a captured call points into that buffer: capture after the largest shape has been seen, or capture again. */
#define FD_STOI_SCAN_TILE 1024      /* frames of one utterance per workgroup of the compaction scan */
#define FD_STOI_SEG_TILE 16         /* segments of one utterance per workgroup of the segment stage */
enum { FD_STOI_OK = 0, FD_STOI_SHORT = 1, FD_STOI_SILENT = 2 };
typedef struct fd_stoi {
    double stoi, estoi;    /* NaN unless status is FD_STOI_OK */
    int32_t frames;        /* F0 */
    int32_t kept;          /* K */
    int32_t segments;      /* J (0 unless OK) */
    int32_t status;        /* FD_STOI_* */
} fd_stoi;                 /* 32 bytes */

/* The band table of step 5, computed from its rule: lo15[j], hi15[j] (pure host code, no handle).  FD_ERR_INVALID: a null pointer. */
FD_API int fd_stoi_bands(int *lo15, int *hi15);
/* F0 for n10k samples at 10 kHz (pure host code).  FD_ERR_INVALID: n10k < 0. */
FD_API int64_t fd_stoi_frames(int64_t n10k);
/* clean, degraded [B][L] device float at `rate` -> rec_dev [B] device records, asynchronous on `stream`.  valid: HOST [B] or NULL =
 * samples of each pair that count (1 .. L), as in fd_loudness_measure.  B 1 .. 4096, rate 8000 .. 192000, at most 2^30 samples at 10 kHz.
 * Like fd_loudness_measure it does not settle a pending lazily checked fd_sample: its result is provisional with it.
 * FD_ERR_INVALID: a null pointer, B, L, rate or valid[b] out of range; FD_ERR_STATE: the scratch buffer (or a resampling table) would
 * have to be built inside a stream capture. */
FD_API int fd_stoi_measure(fd_handle h, const float *clean, const float *degraded, int B, int64_t L, const int64_t *valid, int rate,
                           fd_stoi *rec_dev, void *stream);

/* F0 tracking (YIN: de Cheveigne and Kawahara 2002) and the pitch scores of a vocoded waveform against its recording: F0 RMSE in cents,
 * gross pitch error, voicing decision error.  The reference's data pipeline extracts one F0 per mel frame with Praat or WORLD
 * (data_gen/tts/data_gen_utils.py: get_pitch, 80 .. 750 Hz, one value per hop); neither is in the build image, so THIS TEXT defines the
 * measurement and tests/pitch_ref.py restates it in float64 numpy.  It is YIN, not Praat's autocorrelation method and not WORLD: the
 * values differ from the reference's binarised F0, the frame grid is the same.
 *
 * Parameters (fd_pitch_config; fd_pitch_default_config fills the values in brackets): rate [22050], hop [256], win [1024], f0_min [80],
 * f0_max [750], threshold [0.15].  Derived (fd_pitch_lags):
 *     tau_min = floor(rate / f0_max),  tau_max = ceil(rate / f0_min),  L = tau_max + 2 (the lags 0 .. tau_max + 1: one past tau_max for
 *     the interpolation),  span = win + tau_max + 1.
 * A configuration is refused (FD_ERR_INVALID) when tau_min < 2, tau_max <= tau_min, L > FD_PITCH_MAX_LAGS, win < 64, win > 2048, hop < 1,
 * or threshold is not inside (0, 1); also when rate < 1, f0_min or f0_max is not positive, or `reserved` is not 0.
 *
 * One utterance of n valid samples, at its own rate (nothing is resampled):
 *  1. Frames.  F = n / hop (integer division; the mel frame count for n = T * hop; fd_pitch_frames).  Frame i reads `span` samples from
 *     s_i = i * hop + hop / 2 - span / 2 (integer divisions); samples outside [0, n) read as zero.
 *  2. Difference function.  d(tau) = sum_{j = 0}^{win - 1} (x[s + j] - x[s + j + tau])^2, tau = 0 .. tau_max + 1: the direct form, not
 *     e(0) + e(tau) - 2 r(tau), whose cancellation at the minima is exactly where the answer is read.
 *  3. Cumulative mean normalised difference.  d'(0) = 1;  d'(tau) = d(tau) tau / sum_{j = 1}^{tau} d(j);  where that sum is 0,
 *     d'(tau) = 1 (silence is unvoiced).
 *  4. Decision.  k0 = the smallest tau in [tau_min, tau_max] with d'(tau) < threshold.  None: the frame is unvoiced, f0 = 0 and aper = the
 *     minimum of d' over [tau_min, tau_max].  Otherwise walk down from k0:  k = k0;  while k + 1 <= tau_max and d'(k + 1) < d'(k): ++k.
 *  5. Refinement.  a, b, c = d'(k - 1), d'(k), d'(k + 1);  den = a - 2 b + c;  off = 0.5 (a - c) / den if den > 0, else 0, clamped to
 *     [-1, 1];  f0 = rate / (k + off),  aper = d'(k).
 * Outputs: f0 (0 where unvoiced) and aper, float32 [B][out_pitch], F values per row.  Frames of a row behind its own F up to the F of
 * the longest row (L / hop) are written as f0 = 0, aper = 1.
 *
 * Comparison of two tracks of one utterance over F frames (fd_pitch_compare; a frame is voiced when its f0 > 0):
 *     rmse_cents = sqrt(mean over the both-voiced frames of (1200 log2(f_deg / f_ref))^2)
 *     gpe        = the share of the both-voiced frames with |f_deg / f_ref - 1| > 0.2
 *     vde        = the share of all F frames whose voicing differs
 * Status.  FD_PITCH_SHORT: F = 0, all three are NaN;  FD_PITCH_UNVOICED: F > 0 and no frame is voiced in both, vde is valid and the other
 * two are NaN;  FD_PITCH_OK otherwise.
 *
 * On the device.  fd_pitch_track: one workgroup per FD_PITCH_FRAME_TILE consecutive frames of one utterance stages their samples in LDS
 * once (they overlap by span - hop); where a large hop would not let the tile fit into FD_PITCH_STAGE_FLOATS samples, g frames at a
 * time, g = min(FD_PITCH_FRAME_TILE, 1 + (FD_PITCH_STAGE_FLOATS - span) / hop) (integer division; a span alone always fits).  A wavefront takes one (frame, chunk of FD_PITCH_LAG_CHUNK lags) after the other, a lane per lag:
 * x[s + j] is an LDS broadcast, x[s + j + tau] is conflict-free across the lanes.  d(tau) is summed in float32 into four accumulators
 * (j mod 4) that are added as (a0 + a1) + (a2 + a3): an order that depends on nothing but win.  Steps 3-5 run in float64 from the float32
 * sums, a wavefront per frame: the lanes own consecutive runs of lags, the running sum is a scan over the lanes, k0 and k are minimum
 * reductions over lag indices (the lowest index, no atomics).  fd_pitch_compare: one workgroup per utterance, float64 partials over 256
 * consecutive runs of frames added in run order.  Every sum has a fixed order that depends on the utterance alone: a row is bit-identical
 * alone, anywhere in a ragged batch with anything behind it, at any row pitch and from call to call.  Nothing at or behind valid[b] is
 * read.  The only scratch is the device copy of valid / frames, in a buffer of the handle that grows at the first call that needs more --
 * never inside a stream capture, where such a call is refused with FD_ERR_STATE. */
#define FD_PITCH_MAX_LAGS 1024      /* the largest L = tau_max + 2 */
#define FD_PITCH_FRAME_TILE 4       /* consecutive frames of one utterance per workgroup of the tracker */
#define FD_PITCH_LAG_CHUNK 64       /* lags of one frame per wavefront pass of the tracker */
#define FD_PITCH_STAGE_FLOATS 6144  /* samples of a tile's frames that are staged in LDS together */
enum { FD_PITCH_OK = 0, FD_PITCH_SHORT = 1, FD_PITCH_UNVOICED = 2 };
typedef struct fd_pitch_config {
    int32_t rate, hop, win, reserved;      /* reserved: 0 */
    double f0_min, f0_max, threshold;
} fd_pitch_config;                         /* 40 bytes */
typedef struct fd_pitch {
    double rmse_cents, gpe;    /* NaN unless status is FD_PITCH_OK */
    double vde;                /* NaN when status is FD_PITCH_SHORT */
    int32_t frames;            /* F */
    int32_t both_voiced, ref_voiced, deg_voiced;
    int32_t status;            /* FD_PITCH_* */
    int32_t reserved;          /* 0 */
} fd_pitch;                    /* 48 bytes */

/* The bracketed defaults (pure host code).  FD_ERR_INVALID: a null pointer. */
FD_API int fd_pitch_default_config(fd_pitch_config *cfg);
/* tau_min and tau_max of a configuration (pure host code; either pointer may be NULL).  FD_ERR_INVALID: a null or refused configuration. */
FD_API int fd_pitch_lags(const fd_pitch_config *cfg, int *tau_min, int *tau_max);
/* F for n samples (pure host code).  FD_ERR_INVALID (< 0): n < 0 or hop < 1. */
FD_API int64_t fd_pitch_frames(int64_t n, int hop);
/* wav [B][L] device float -> f0_dev, aper_dev [B][out_pitch] device float, asynchronous on `stream`.  valid: HOST [B] or NULL = samples of
 * each row that count (0 .. L).  B 1 .. 4096, L >= 1 with L / hop <= 2^30, out_pitch >= max(L / hop, 1).  Like fd_stoi_measure it does not
 * settle a pending lazily checked fd_sample.  FD_ERR_INVALID: a null pointer, a refused configuration, B, L, out_pitch or valid[b] out of
 * range; FD_ERR_STATE: the scratch buffer would have to grow inside a stream capture. */
FD_API int fd_pitch_track(fd_handle h, const float *wav, int B, int64_t L, const int64_t *valid, const fd_pitch_config *cfg, float *f0_dev,
                          float *aper_dev, int64_t out_pitch, void *stream);
/* f0_ref, f0_deg [B][pitch] device float (two tracks of fd_pitch_track) -> rec_dev [B] device records, asynchronous on `stream`.
 * frames: HOST [B] or NULL = frames of each row that count (0 .. pitch; NULL: pitch).  B 1 .. 4096, pitch 1 .. 2^30.
 * FD_ERR_INVALID: a null pointer, B, pitch or frames[b] out of range; FD_ERR_STATE: as above. */
FD_API int fd_pitch_compare(fd_handle h, const float *f0_ref, const float *f0_deg, int B, int64_t pitch, const int64_t *frames,
                            fd_pitch *rec_dev, void *stream);

/* Multi-resolution STFT distances: how close the spectrum of a vocoded waveform is to the recording's -- spectral convergence and
 * log-magnitude distance at several window sizes (the multi-resolution STFT error of Parallel WaveGAN, Yamamoto, Song, Kim 2020) and the
 * log-spectral distance.  The reference ships modules/parallel_wavegan without its STFT loss and utils/torch_stft.py without a caller;
 * people compute these offline with torch over the *_gt.wav / *_pred.wav pairs that test_step writes.  THIS TEXT defines the measurement;
 * tests/spectral_ref.py restates it in float64 numpy, and torch.stft on the CPU confirms that restatement.
 *
 * Inputs: a recording x and a vocoded waveform y of the same length n.  A configuration (fd_spectral_config; fd_spectral_default_config
 * fills the values in brackets) holds n_res resolutions, 1 .. FD_SPECTRAL_MAX_RES, each (nfft, hop, win) in samples whatever the rate
 * [3: (512, 50, 240), (1024, 120, 600), (2048, 240, 1200)], and a power floor [1e-7].  Accepted: nfft in {512, 1024, 2048},
 * 2 <= win <= nfft, 16 <= hop <= nfft, floor > 0 (and finite), reserved = 0.
 *
 * Per resolution, with the conventions of torch.stft(center=True, pad_mode="reflect", window=hann_window(win, periodic=True)):
 *  1. Padding.  The signal is reflected by nfft / 2 on both sides: position p < 0 reads s[-p], p >= n reads s[2 (n - 1) - p].  Only the
 *     signal's own n samples are read: nothing at or behind valid[b].
 *  2. Frames.  F = 1 + n / hop (integer division; fd_spectral_frames).  Frame f covers padded positions f hop - nfft / 2 + i,
 *     i = 0 .. nfft - 1.
 *  3. Window.  w[i] = 0.5 - 0.5 cos(2 pi i / win), i = 0 .. win - 1, at offset (nfft - win) / 2 (integer division) inside the nfft frame
 *     and zero elsewhere.
 *  4. Magnitudes.  For k = 0 .. nfft / 2:  X[f][k] = sqrt(max(re^2 + im^2, floor)) of the nfft-point transform of the windowed frame of
 *     x; Y[f][k] likewise of y.
 *  5. sc = sqrt(sum (X - Y)^2 / sum X^2) over all frames and bins: the spectral convergence.
 *  6. logmag = mean |ln X - ln Y| over all frames and bins, in nepers.
 *  7. lsd_db = mean_f sqrt(mean_k (20 log10 X - 20 log10 Y)^2): the log-spectral distance in dB.
 * The record holds the three values per resolution, their means over the n_res resolutions (mr_sc, mr_logmag, lsd_db), frames[r], n_res
 * and the status.  FD_SPECTRAL_SHORT: n <= max_r nfft / 2, where the reflection is undefined: every value is NaN (frames[r] is still
 * F).  FD_SPECTRAL_OK otherwise; the floor keeps sum X^2 > 0, so silence is measured like anything else.  The values of the unused
 * resolutions r >= n_res are NaN and their frames 0.
 *
 * On the device.  Transform stage, one launch per resolution: one workgroup takes FD_SPECTRAL_FRAME_TILE consecutive frames of one pair,
 * one after the other, and for each frame first x, then y THROUGH THE SAME CODE: the windowed frame (only the win samples under the
 * window are read) is staged in LDS and transformed in float32 as a split N1 x N2 transform (16 x 32, 32 x 32, 32 x 64 for 512, 1024,
 * 2048; n = N2 n1 + n2, k = k1 + N1 k2):
 *     A[n2][k1] = sum_n1 xw[N2 n1 + n2] W_N1^(n1 k1);   B = A W_nfft^(n2 k1);   X[k1 + N1 k2] = sum_n2 B[n2][k1] W_N2^(n2 k2)
 * with the twiddles read from one table of cos and sin of 2 pi m / nfft, rounded once from double, at exact integer indices (no
 * recurrences); only the bins 0 .. nfft / 2 are computed.  The powers of x stay in registers until the same thread has the power of y
 * at the same bin; then, in float64, the floor, the root and the logarithms, and the frame's four partial sums -- sum (X - Y)^2,
 * sum X^2, sum |d|, sum d^2 with d = ln X - ln Y -- each thread over its own bins in ascending order, the 256 threads by a fixed tree.
 * They are written to the handle's scratch, four doubles per frame: no spectrogram reaches memory.  Identical signals go through identical
 * arithmetic, so a copy scores exactly 0.  Finalise stage, one workgroup per pair: per resolution, thread t adds the partials of the
 * frames t, t + FD_SPECTRAL_SUM_CHUNK, ... in ascending order (sum d^2 after the root of its mean), thread 0 adds the
 * FD_SPECTRAL_SUM_CHUNK sums in thread order, takes the roots and means and writes the record.  No order depends on B or on where the
 * pair lies in the batch, and there are no floating-point atomics: a pair's record is bit-identical alone, anywhere in a ragged batch with
 * anything behind it, at any row pitch and from call to call.  The window and twiddle table of each distinct (nfft, win) is uploaded at
 * the first call that uses it and kept on the handle; the partials live in a buffer of the handle that grows at the first call that needs
 * more.  Neither can happen inside a stream capture, where such a call is refused with FD_ERR_STATE: call it once before.  A graph that
 * holds a captured call points into that buffer: capture after the largest shape has been seen, or capture again. */
#define FD_SPECTRAL_MAX_RES 4       /* resolutions of one configuration */
#define FD_SPECTRAL_FRAME_TILE 4    /* consecutive frames of one pair per workgroup of the transform stage */
#define FD_SPECTRAL_SUM_CHUNK 256   /* interleaved runs of frames the finaliser adds before it adds the runs */
enum { FD_SPECTRAL_OK = 0, FD_SPECTRAL_SHORT = 1 };
typedef struct fd_spectral_config {
    int32_t n_res, reserved;               /* reserved: 0 */
    int32_t nfft[FD_SPECTRAL_MAX_RES], hop[FD_SPECTRAL_MAX_RES], win[FD_SPECTRAL_MAX_RES];
    double floor;                          /* on the power re^2 + im^2 */
} fd_spectral_config;                      /* 64 bytes */
typedef struct fd_spectral {
    double sc[FD_SPECTRAL_MAX_RES], logmag[FD_SPECTRAL_MAX_RES], lsd[FD_SPECTRAL_MAX_RES];      /* per resolution; lsd in dB */
    double mr_sc, mr_logmag, lsd_db;       /* their means over the n_res resolutions */
    int32_t frames[FD_SPECTRAL_MAX_RES];   /* F per resolution (0 for r >= n_res) */
    int32_t n_res;
    int32_t status;                        /* FD_SPECTRAL_* */
} fd_spectral;                             /* 144 bytes */

/* The bracketed defaults (pure host code).  FD_ERR_INVALID: a null pointer. */
FD_API int fd_spectral_default_config(fd_spectral_config *cfg);
/* F for n samples at `hop` (pure host code).  FD_ERR_INVALID (< 0): n < 0 or hop < 1. */
FD_API int64_t fd_spectral_frames(int64_t n, int hop);
/* clean, degraded [B][L] device float -> rec_dev [B] device records, asynchronous on `stream`.  valid: HOST [B] or NULL = samples of each
 * pair that count (1 .. L).  cfg: NULL = the default.  B 1 .. 4096, L 1 .. 2^30.  Like fd_stoi_measure it does not settle a pending lazily
 * checked fd_sample.  The arguments are checked before the handle is looked at, so a refusal's text is left with fd_last_error(NULL)
 * when the handle is NULL.  FD_ERR_INVALID: a null handle or pointer, B, L, valid[b] or a configuration value out of range (the message
 * names the value); FD_ERR_STATE: a table or the scratch buffer would have to be made inside a stream capture. */
FD_API int fd_spectral_measure(fd_handle h, const float *clean, const float *degraded, int B, int64_t L, const int64_t *valid,
                               const fd_spectral_config *cfg, fd_spectral *rec_dev, void *stream);

/* Griffin-Lim: the baseline vocoder (the reference's GLLinear / GLMel, vocoders/gl_linear.py, vocoders/gl_mel.py over
 * utils/audio.py:35-63 griffin_lim and :123-158 griffin_lim_torch) -- a waveform from magnitudes alone, by alternating projections
 * (Griffin and Lim 1984).  With it come the two primitives it is made of: an inverse STFT and the magnitude-only reconstruction loop.
 * THIS TEXT defines the computation; tests/gl_ref.py restates it in float64 numpy, and torch.stft / torch.istft on the CPU confirm that
 * restatement.
 *
 * Constants: N = FD_GL_NFFT = 1024, hop = FD_GL_HOP = 256, bins k = 0 .. 512, w = the periodic Hann window of 1024 points, the mel
 * front-end's.  Inputs: amplitudes A[b][k][t] >= 0, float32 [B][513][T]; frame counts lens[b] (NULL: T).  Item b yields
 * L_b = fd_gl_samples(lens[b]) = 256 (lens[b] - 1) samples: the front-end's T = 1 + len / 256 read backwards, so the T + 1 frames of a
 * recording's mel give the T 256 samples that fd_sample produces from its first T frames.
 *
 * stft(y):   X[k][t] = sum_n w[n] ypad[256 t + n] e^(-2 pi i k n / N), k <= 512, ypad = y with 512 zeros on each side
 *            (librosa.stft(center=True, pad_mode="constant"), what fd_mel_spectrogram transforms; not torch.stft's reflect padding).
 * istft(C):  f_t[n] = w[n] (1 / N) sum_{k < N} C^[k][t] e^(+2 pi i k n / N), C^ the Hermitian extension of C, the imaginary parts of
 *            bins 0 and 512 ignored as a C2R transform ignores them;
 *            y~[m] = sum_t f_t[m - 256 t] / sum_t w^2[m - 256 t] over the frames t < lens[b] that cover m;  y[j] = y~[j + 512], j < L_b.
 *            The envelope sum_t w^2 is at least 1.25 on that range (1.5 where four frames overlap): no guard, no epsilon.
 *            (librosa.istft, torch.istft(center=True).)
 * The loop:  C_0 = A e^(i theta0), y_0 = istft(C_0); for i = 1 .. n_iters: X = stft(y_{i-1}), C = A X / |X| (X = 0: C = A, as
 *            np.angle(0) = 0), y_i = istft(C).  No angle is formed inside the loop.
 * theta0:    the caller's angles[b][k][t] (GLLinear.spec2wav's phase=; with a recording's own phase an upper bound), or, angles NULL,
 *            theta = 6.2831855f u with u the float32 uniform ((float)(r >> 8) + 0.5f) 2^-24 of one Philox4x32-10 word r:
 *            key = (seed lo, seed hi), counter = (pos lo, pos hi ^ id lo, FD_GL_PHILOX_STREAM, 0x5EED ^ id hi), pos = 129 t + k / 4,
 *            r = output word k % 4 -- the generator of fd_sample's noise on a stream word of its own (0xFFFFFFFF is x_T, small values the
 *            step indices, 0xFFFFFFF9 .. 0xFFFFFFFE the training draws).  id = stream_ids[b] (NULL: b), so with ids an item's start
 *            does not depend on the batch it sits in.
 * Results:   wav_out[b][0 .. L_b), zeros behind it up to fd_gl_samples(T); one record per item: the status and the final inconsistency
 *            sc = || |stft(y_n)| - A ||_F / || A ||_F from one more forward pass over the returned waveform, its sums in float64 in
 *            a fixed order as fd_spectral_measure's.  FD_GL_SHORT: lens[b] < 2; FD_GL_NONFINITE: an amplitude is negative, infinite
 *            or NaN; FD_GL_SILENT: every amplitude is 0.  In all three the row is zeros and sc NaN; the other items are not affected.
 *
 * On the device.  The transform is the mel front-end's split 32 x 32 transform in float32 (fd_spectral_measure's text above) and its
 * mirror image: with k = k1 + 32 k2, n = 32 n1 + n2,
 *     D[k1][n2] = sum_k2 C^[k1 + 32 k2] e^(+2 pi i k2 n2 / 32);   E = D e^(+2 pi i k1 n2 / N), k1 = 0 .. 16;
 *     x[32 n1 + n2] = (Re E[0][n2] + (-1)^n1 Re E[16][n2] + 2 sum_{k1 = 1 .. 15} Re(E[k1][n2] e^(+2 pi i k1 n1 / 32))) / N
 * (the rows k1 > 16 are the conjugates of the rows 32 - k1), every sum one fmaf chain in ascending order over the same table of cos and
 * sin of 2 pi m / N.  |X| = sqrt(fma(im, im, re re)) and C = (re s, im s) with s = A / |X|, each operation rounded once as written.
 * One launch per iteration and no grid-wide barrier: a workgroup takes FD_GL_FRAME_TILE consecutive frames of one item; it forms ypad
 * under them from the previous iteration's synthesis frames -- per sample the at most four covering frames added in ascending t, divided
 * by the envelope, which is summed from w^2 in the same order -- then per frame: window, forward transform, re-phase, inverse
 * transform, window, and writes the synthesis frame f_t to the other of two frame buffers [B][T][1024].  No spectrum reaches memory, no
 * sum depends on which workgroup forms it, there are no atomics: an item's waveform and record are bit-identical alone, anywhere in a
 * ragged batch and from call to call.  The waveform is written once, by a last gather launch.  The frame buffers, the amplitudes
 * transposed to [B][T][513] and the per-frame sums live in a buffer of the handle that grows at the first call that needs more; that
 * and the upload of the front-end's tables cannot happen inside a stream capture, where such a call is refused with FD_ERR_STATE: call
 * it once before.  Otherwise a call is capturable. */
#define FD_GL_NFFT 1024
#define FD_GL_HOP 256
#define FD_GL_BINS 513
#define FD_GL_FRAME_TILE 4          /* consecutive frames of one item per workgroup */
#define FD_GL_SUM_CHUNK 256         /* interleaved runs of frames the record's finaliser adds before it adds the runs */
#define FD_GL_MAX_ITERS 10000
#define FD_GL_MAX_FRAMES 1048576    /* T */
#define FD_GL_PHILOX_STREAM 0xFFFFFFF8u
enum { FD_GL_OK = 0, FD_GL_SHORT = 1, FD_GL_SILENT = 2, FD_GL_NONFINITE = 3 };
enum { FD_GL_PWG = 0, FD_GL_TACOTRON = 1 };      /* fd_mel_to_linear's variant: the mel is log10 / ln of the filter bank's output */
typedef struct fd_gl {
    double sc;                             /* the inconsistency of the returned waveform; NaN unless FD_GL_OK */
    double norm;                           /* || A ||_F over the item's own frames; NaN if SHORT or NONFINITE */
    int32_t frames, samples;               /* lens[b]; L_b (0 if SHORT) */
    int32_t iters;                         /* n_iters */
    int32_t status;                        /* FD_GL_* */
} fd_gl;                                   /* 32 bytes */

/* 256 (frames - 1), or -1 below 2 frames (pure host code). */
FD_API int64_t fd_gl_samples(int64_t frames);
/* 60: griffin_lim_iters of egs_bases/tts/base.yaml (pure host code). */
FD_API int fd_gl_default_iters(void);
/* Mel inversion (utils/audio.py:91-95 _mel_to_linear): amp_out[b][k][t] = max(1e-10, sum_j P[k][j] g(mel[b][j][t])), g = 10^x for
 * FD_GL_PWG, e^x for FD_GL_TACOTRON; one thread per (k, t), the 80 terms one fmaf chain in ascending j.  mel [B][80][T] and amp_out
 * [B][513][T] device float; pinv_513x80: HOST, P = pinv(filter bank) [513][80] float32, uploaded at the first call and whenever its
 * values differ from the last call's with that variant (not inside a stream capture: FD_ERR_STATE).  This is the pseudo-inverse, the
 * default inversion; GLMel's non-negative least squares is fd_mel_to_linear_nnls below.  Asynchronous on `stream`.  The arguments are checked before the handle is looked at.  FD_ERR_INVALID: a
 * null pointer or handle, B outside 1 .. 4096, T outside 1 .. FD_GL_MAX_FRAMES, an unknown variant, an element of P that is not finite. */
FD_API int fd_mel_to_linear(fd_handle h, const float *mel, int B, int T, const float *pinv_513x80, int variant, float *amp_out, void *stream);
/* amp [B][513][T], angles [B][513][T] or NULL (Philox), wav_out [B] rows wav_pitch floats apart, rec_dev [B]: device; lens (frames,
 * 0 .. T; below 2: FD_GL_SHORT) and stream_ids: HOST [B] or NULL.  Asynchronous on `stream`.  The arguments are checked before the
 * handle is looked at, so a refusal's text is left with fd_last_error(NULL) when the handle is NULL.  FD_ERR_INVALID: a null handle or
 * pointer, B outside 1 .. 4096, T outside 2 .. FD_GL_MAX_FRAMES, n_iters outside 0 .. FD_GL_MAX_ITERS, wav_pitch < fd_gl_samples(T),
 * lens[b] out of range; FD_ERR_STATE: the tables or the scratch buffer would have to be made inside a stream capture. */
FD_API int fd_griffin_lim(fd_handle h, const float *amp, const float *angles, int B, int T, const int64_t *lens, int n_iters, uint64_t seed,
                          const uint64_t *stream_ids, float *wav_out, int64_t wav_pitch, fd_gl *rec_dev, void *stream);

/* Non-negative mel inversion (the reference's GLMel, vocoders/gl_mel.py:15-19: librosa.util.nnls(mel_basis, spec), the pseudo-inverse
 * clipped at 0 and refined under x >= 0).  Per frame the convex problem min_x || A x - g ||^2, x >= 0, with A = the bank [80][513]
 * float32, P = its pseudo-inverse [513][80] float32 (what fd_mel_to_linear takes) and g = g(mel) as fd_mel_to_linear forms it, solved
 * by an accelerated projected gradient (FISTA) with a fixed step and a fixed iteration count:
 *     x_0 = max(0, P g)      (fd_mel_to_linear's 80-term fmaf chain in ascending j);   y_0 = x_0
 *     k = 0 .. n_iters - 1:  r = A y_k - g  [80];   x_{k+1} = max(0, fma(-s, A^T r, y_k))  [513];   y_{k+1} = fma(beta_k, x_{k+1} - x_k, x_{k+1})
 *     amp_out = max(1e-10, x_n)      (the pseudo-inverse path's floor; n_iters = 0 is fd_mel_to_linear bit for bit)
 * s = float32(1 / L), L an upper bound of the largest eigenvalue of A A^T: fd_nnls_step_bound, on the host in float64 when a bank is
 * first seen -- 200 power iterations on the 80 x 80 Gram matrix from the start vector v_j = 1 + j / 80, then 1.01 times the Rayleigh
 * quotient -- cached with the bank and P per variant.  beta_k = (t_k - 1) / t_{k+1}, t_0 = 1, t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2: a
 * host table in double, rounded to float32 once.  No adaptive restart and no data-dependent stopping: a frame's result is a function
 * of that frame alone.  A is dense and of any sign to the kernel.
 *
 * On the device.  One launch does the whole solve: a workgroup of 256 threads takes FD_NNLS_FRAME_TILE = 32 consecutive frames of one
 * item -- the column count of one v_mfma_f32_32x32x2_f32, the exact-fp32 matrix instruction both products run on (bit for bit an fmaf
 * chain; no fp16 split: r cancels to 1e-7 of its operands).  y [513][32] lives in LDS as the B operand of A y, x_k in the registers
 * of the lane that owns the element in the instruction's result layout; A streams from L2 twice per iteration, once as the zero-padded
 * transpose [520][96] (A y: the 260 bin pairs split over the four waves in fixed ranges, the four partial sums added in wave order)
 * and once as [80][544] (A^T r: 17 bin tiles of 32 dealt to the waves).  A tile of 32 frames needs 127 KB of the 160 KB of LDS, so
 * one workgroup per CU; 16 frames with half of A resident would halve the columns every streamed element of A feeds.  Only
 * amp_out and four doubles per frame reach memory.  A second pass in the same kernel forms, from the amplitudes written, in float64
 * sum_j (A amp - g)_j^2 (each an fma chain in ascending bin, the 80 squares added in ascending j), sum_j g_j^2 and the count of g that
 * are not finite; k_nnls_finish adds the frames as k_gl_finish does.  Frames at or behind lens[b] are never read and their amp_out is
 * 1e-10.  Every sum has a fixed order that does not depend on the batch; no atomics: an item is bit-identical alone, anywhere in a
 * ragged batch and from call to call.
 *
 * The record: resid = || A amp - g ||_F / || g ||_F over the item's own frames (0 if || g || = 0), NaN unless OK; norm = || g ||_F (NaN
 * unless OK).  FD_NNLS_EMPTY: lens[b] == 0.  FD_NNLS_NONFINITE: a mel value is NaN or infinite, or g overflows; that item's amplitudes
 * are all 1e-10, the other items are not affected. */
#define FD_NNLS_MAX_ITERS 4096
#define FD_NNLS_FRAME_TILE 32       /* consecutive frames of one item per workgroup */
enum { FD_NNLS_OK = 0, FD_NNLS_EMPTY = 1, FD_NNLS_NONFINITE = 2 };
typedef struct fd_nnls {
    double resid;                          /* || A amp - g || / || g || over the item's own frames; NaN unless FD_NNLS_OK */
    double norm;                           /* || g ||_F; NaN unless FD_NNLS_OK */
    int32_t frames;                        /* lens[b] */
    int32_t iters;                         /* n_iters */
    int32_t status;                        /* FD_NNLS_* */
    int32_t reserved;
} fd_nnls;                                 /* 32 bytes */

/* 128 (pure host code). */
FD_API int fd_nnls_default_iters(void);
/* L as defined above for a bank [80][513] (pure host code, no handle).  FD_ERR_INVALID: a null pointer, an element that is not finite. */
FD_API int fd_nnls_step_bound(const float *bank_80x513, double *L_out);
/* mel [B][80][T], amp_out [B][513][T], rec_dev [B] or NULL: device; lens (frames, 0 .. T), bank_80x513 and pinv_513x80: HOST (lens may be
 * NULL).  The bank, P, L and the beta table are uploaded at the first call and whenever the bank's or P's values differ from the last
 * call's with that variant; that and a growth of the scratch buffer (lens, the frame sums) cannot happen inside a stream capture:
 * FD_ERR_STATE, call it once before.  Asynchronous on `stream`.  The arguments are checked before the handle is looked at.
 * FD_ERR_INVALID: a null pointer or handle, B outside 1 .. 4096, T outside 1 .. FD_GL_MAX_FRAMES, n_iters outside 0 ..
 * FD_NNLS_MAX_ITERS, an unknown variant, an element of the bank or of P that is not finite, lens[b] outside 0 .. T. */
FD_API int fd_mel_to_linear_nnls(fd_handle h, const float *mel, int B, int T, const int64_t *lens, const float *bank_80x513,
                                 const float *pinv_513x80, int variant, int n_iters, float *amp_out, fd_nnls *rec_dev, void *stream);

/* K-means bins over feature rows (no counterpart in the reference): one pass of Lloyd's algorithm, the device half of the NDB / JSD
 * diversity scores of Richardson & Weiss 2018 (fastdiff_amd/diversity.py fits the bins on the training corpus' mel frames and counts a
 * sampler's frames in them).  Sample i is the D floats at x + i * ld (ld = D: a packed matrix; ld > D: the leading D of wider rows, whose
 * rest is never read); x may have any 4-byte alignment and the result does not depend on it.
 *
 * Standardisation, as the row is loaded (x is never written):  z_d = fl(fl(x_d - shift_d) * scale_d), two float32 roundings, no fused
 * multiply-add; shift = scale = NULL: z = x.
 * Assignment, all in float32:
 *     h_k   = fl(0.5 * a_D),  a_0 = 0,  a_{d+1} = fma(c_kd, c_kd, a_d)                 (once per pass)
 *     dot_k = b_D,            b_0 = 0,  b_{d+1} = fma(c_kd, z_d, b_d)                  (ascending d; on v_mfma_f32_32x32x2_f32, exact fp32)
 *     s_k   = fl(h_k - dot_k);   assign = the lowest k with s_k = min_j s_j             (|| z ||^2 is common to every k)
 * so an assigned bin is the nearest in Euclidean distance up to the rounding of s: with d64 the float64 squared distance over the
 * float32 z, d64(assigned) - min_k d64(k) <= 2 g (E_assigned + E_best), E_k = || c_k ||^2 / 2 + sum_d |z_d| |c_kd|, g = n u / (1 - n u),
 * n = D + 2, u = 2^-24.  A row with a z_d that is not finite (a NaN or infinite x_d, or an overflow of the two operations) is assigned
 * -1, counted in `nonfinite` and enters no sum or count; the other rows' results are those of a call without it.
 * The record:  counts[k] = rows assigned to k (0 for k >= K);  inertia = sum over the assigned rows of sum_d (z_d - c_kd)^2 in float64 for
 * the row's bin -- per row the two halves of d as fma chains in ascending d, rows added per position in the 128-row block over the
 * blocks of a chunk, the 256 positions in order, then the chunks in ascending order;  moved = rows whose assignment differs from
 * assign_io on entry (-1 when assign_io is NULL; the first pass of a fit starts from an array of -1);  nonfinite;  empty = bins k < K
 * with counts[k] = 0;  status.
 * Update (centroids_out not NULL):  centroids_out[k][d] = (float)(S_kd / counts[k]), S_kd = the sums over chunks of FD_BINS_CHUNK
 * consecutive rows added in ascending chunk order in float64; inside a chunk the sum is float32, s <- fl(s + z_d) over the bin's rows in
 * ascending row order (the product one-hot(assign)^T Z on the same matrix instruction).  A bin with counts[k] = 0 keeps centroids[k]
 * bit for bit.  centroids_out may not overlap centroids.
 *
 * On the device.  One workgroup of 256 threads per chunk keeps the centroids ([K][D], at most 64 KB) in LDS and reads its rows once, 128
 * at a time into LDS; each wave multiplies its 32 rows with every centroid, and the K x D tiles of the update are dealt to the four waves
 * and stay in registers for the whole chunk.  Only assign_io, and per chunk the sums [K][D], counts, inertia and two integers reach
 * memory (the handle's scratch grower; a growth cannot happen inside a stream capture: FD_ERR_STATE, call it once before).  k_bins_update
 * (one workgroup per bin) and k_bins_record add the chunks.  Every sum has a fixed order that does not depend on the grid; the only
 * atomics are integer adds in LDS: two calls give the same bits.  Nothing at or behind x + (N - 1) ld + D is read.  Asynchronous on
 * `stream`; does not settle a pending lazily checked fd_sample.
 *
 * x, shift [D], scale [D], centroids [K][D], assign_io [N] int32, centroids_out [K][D], rec_dev: DEVICE.  shift and scale: both or
 * neither; assign_io, centroids_out, rec_dev: each may be NULL, not all three.  The arguments are checked before the handle is looked at.
 * FD_ERR_INVALID: a null x, centroids or handle, N outside 1 .. 2^40, D not a multiple of 4 in 4 .. 128, K outside 1 .. 128, ld < D or
 * ld > 2^21, x not 4-byte aligned, one of shift / scale alone, no output, centroids_out overlapping centroids. */
#define FD_BINS_CHUNK 4096          /* consecutive rows whose sums are formed in float32; one workgroup */
#define FD_BINS_MAX_K 128
#define FD_BINS_MAX_D 128
enum { FD_BINS_OK = 0, FD_BINS_NONFINITE = 1, FD_BINS_EMPTY = 2 };      /* rows were left out as not finite; no row was assigned */
typedef struct fd_bins {
    int64_t counts[FD_BINS_MAX_K];
    double inertia;
    int64_t moved;
    int64_t nonfinite;
    int32_t empty;
    int32_t status;                        /* FD_BINS_* */
} fd_bins;                                 /* 1056 bytes */

/* FD_BINS_CHUNK (pure host code). */
FD_API int fd_bins_chunk(void);
/* sizeof(fd_bins) = 1056 (pure host code). */
FD_API int fd_bins_record_bytes(void);
FD_API int fd_bins_pass(fd_handle h, const float *x, int64_t N, int D, int64_t ld, const float *shift, const float *scale,
                        const float *centroids, int K, int32_t *assign_io, float *centroids_out, fd_bins *rec_dev, void *stream);

/* Mel-cepstral distortion with time alignment: the MCD column of the vocoder tables, and the one score here that does not compare frame i
 * with frame i.  Three layers, each an entry point of its own.  The reference has no MCD; its alignment (utils/pitch_distance.py:
 * time_warp, align_from_distances) is a numba-compiled double loop on the CPU.  THIS TEXT defines the computation; tests/mcd_ref.py
 * restates it in float64 numpy.
 *
 * 1. fd_cepstra: waveform -> mel-cepstral rows.  A row of n samples has T = 1 + n / 256 frames (fd_mcd_frames), those of
 *    fd_mel_spectrogram: frame t is the log-mel of the front-end that option "mel" selects -- pwg: zero padding, log10(max(1e-6, .));
 *    tacotron: reflection, ln(max(1e-5, .)), which needs n > 512 -- through the SAME device code as fd_mel_spectrogram, with the handle's
 *    filter bank (fd_set_mel_filterbank).  Nothing at or behind the row's own n is read.  The 80 values become natural logarithms in
 *    float32 (pwg: m_j = fl(log10 value * fl(ln 10)); tacotron: as they are) and then, by the orthonormal DCT-II over the 80 bands,
 *        c_d = sqrt(2 / 80) sum_j m_j cos(pi d (j + 1/2) / 80),   d = 1 .. n_coef
 *    one fmaf chain per d over ascending j from a table rounded once from double (csrc/fd_mcd.h: dct_table), kept in LDS.  c_0, the
 *    gain, is dropped.  n_coef 1 .. FD_MCD_MAX_COEF [13].  No mel reaches memory.  cep_out [B][T_pitch][n_coef]: the rows t < T of item b
 *    hold the cepstra, the rows T <= t < T_pitch zeros.  A tacotron row with n <= 512 holds NaN in its T rows, and so does a frame
 *    under whose window a sample is NaN or infinite (the front-end's floor alone would take it for silence).
 *    This is the cepstrum of the mel filter bank, NOT the SPTK / WORLD mcep of a spectral envelope: the values are comparable among runs
 *    of this tool (and with other mel-filter-bank MCDs of the same front-end), not with tables computed from mcep.
 *
 * 2. fd_dtw: dynamic time warping of two sequences of feature rows.  a: item b has frames_a[b] rows of D floats, row i at
 *    a + (b pitch_a + i) ld; b likewise with pitch_b and frames_b (NULL: pitch_a / pitch_b rows); D 1 .. FD_MCD_MAX_COEF, ld >= D, any
 *    4-byte alignment.  Nothing behind an item's own rows, and nothing of a row behind its D floats, is read.
 *        cost(i, j) = sqrtf(s_D),  s_0 = 0,  s_{d+1} = fmaf(a_id - b_jd, a_id - b_jd, s_d)      (float32, from the differences)
 *        D(0, 0) = cost(0, 0);   D(i, j) = cost(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1))   (float64; outside the matrix: absent)
 *    A tie goes to the first of (diagonal, i - 1, j - 1): a later candidate replaces an earlier one only when strictly smaller.  Each cell
 *    carries (D, cells on its path, diagonal steps on its path) forward from the predecessor it chose; with the fixed tie rule these are
 *    the values of the path a trace-back from (Ta - 1, Tb - 1) finds, so the record needs no trace-back and no matrix in memory:
 *        cost = D(Ta - 1, Tb - 1);  path_len = cells of the path (a copy: T);  n_diag = its diagonal steps (a copy: T - 1).
 *    FD_MCD_NONFINITE: a feature of the pair is NaN or infinite (read from its bits): cost is NaN, path_len = n_diag = 0 and align_out is
 *    -1.  align_out (may be NULL) [B][align_pitch] int32: for each i < frames_a[b] the smallest j with (i, j) on the path (the reference's
 *    align_from_distances), -1 for i >= frames_a[b].  Only then are the directions kept: two bits per cell, four cells of a row to a byte,
 *    frames_a ceil(frames_b / 4) bytes of the handle's scratch per pair, walked back by the pair's workgroup when the sweep is done.  A
 *    pair of more than FD_DTW_MAX_ALIGN_CELLS cells is then refused.  No float [Ta][Tb] matrix exists at any time.
 *    On the device: ONE WORKGROUP PER PAIR; workgroups never wait for each other (no flags, no grid barrier).  It takes FD_DTW_ROWS
 *    consecutive rows of a at a time; thread r keeps row i0 + r in registers and is at column s - r in step s.  b is staged in LDS in
 *    tiles of FD_DTW_COLS columns (a ring of FD_DTW_ROWS + FD_DTW_COLS).  The value above comes from thread r - 1: by a cross-lane move
 *    inside a wavefront, through LDS between wavefronts; the diagonal one is the value above of the step before; one workgroup barrier
 *    per step.  The bottom row of a row block goes through the scratch to the next block.  The order of every operation depends on the
 *    pair alone: a record is bit-identical alone, anywhere in a ragged batch, at any ld and alignment, and from call to call.
 *
 * 3. fd_mcd_measure: cepstra of both waveforms, then the alignment -- the same kernels, so the record is bit-identical to two fd_cepstra
 *    and one fd_dtw.  clean [B][Lc] and degraded [B][Ld] may differ in length.  With K = 10 sqrt(2) / ln 10:
 *        mcd_dtw    = K cost / path_len
 *        mcd_linear = K mean_{i < min(Tc, Td)} cost(i, i): no alignment; thread t adds the frames t, t + 256, ... in float64 in ascending
 *                     order, thread 0 the 256 sums in thread order.
 *    A copy scores exactly 0 with path_len = n_diag + 1 = T.  FD_MCD_SHORT: tacotron front-end and one of the two has n <= 512;
 *    FD_MCD_NONFINITE: a cepstral value is not finite; the values are then NaN and path_len = n_diag = 0.
 *
 * All three: asynchronous on `stream`; like fd_spectral_measure they do not settle a pending lazily checked fd_sample, and the arguments
 * are checked before the handle is looked at.  The tables (front-end, DCT) are uploaded at the first call and the scratch grows at the first
 * call that needs more; neither can happen inside a stream capture (FD_ERR_STATE: call it once before).  B 1 .. 4096; a row has at most
 * FD_MCD_MAX_FRAMES frames.  FD_ERR_INVALID: a null handle or pointer, a count or configuration value out of range (the message names
 * the value). */
#define FD_MCD_MAX_COEF 40
#define FD_MCD_MAX_FRAMES 4194304   /* 2^22 frames of one row */
#define FD_DTW_ROWS 256             /* rows of a one workgroup sweeps together; its threads */
#define FD_DTW_COLS 64              /* columns of b staged together */
#define FD_DTW_MAX_ALIGN_CELLS 67108864      /* 2^26: the largest Ta Tb with align_out */
enum { FD_MCD_OK = 0, FD_MCD_SHORT = 1, FD_MCD_NONFINITE = 2 };
typedef struct fd_mcd_config { int32_t n_coef, reserved; } fd_mcd_config;      /* 8 bytes; reserved: 0 */
typedef struct fd_dtw_rec {
    double cost;
    int32_t path_len, n_diag, frames_a, frames_b;
    int32_t status, reserved;              /* FD_MCD_OK / FD_MCD_NONFINITE */
} fd_dtw_rec;                              /* 32 bytes */
typedef struct fd_mcd {
    double mcd_dtw, mcd_linear, cost;      /* dB, dB, the accumulated distance */
    int32_t path_len, n_diag, frames_clean, frames_degraded;
    int32_t status, reserved;              /* FD_MCD_* */
} fd_mcd;                                  /* 48 bytes */

/* n_coef = 13 (pure host code).  FD_ERR_INVALID: a null pointer. */
FD_API int fd_mcd_default_config(fd_mcd_config *cfg);
/* T for n samples (pure host code): 1 + n / 256.  FD_ERR_INVALID (< 0): n < 0. */
FD_API int64_t fd_mcd_frames(int64_t n);
/* wav [B][L] device, valid HOST [B] or NULL (1 .. L) -> cep_out [B][T_pitch][n_coef] device, T_pitch >= fd_mcd_frames(L). */
FD_API int fd_cepstra(fd_handle h, const float *wav, int B, int64_t L, const int64_t *valid, int n_coef, float *cep_out, int64_t T_pitch,
                      void *stream);
/* a, b device; frames_a, frames_b HOST [B] or NULL (1 .. pitch_a / pitch_b) -> rec_dev [B] device, align_out NULL or [B][align_pitch]
 * device int32 with align_pitch >= pitch_a. */
FD_API int fd_dtw(fd_handle h, const float *a, const float *b, int B, int D, int64_t ld, int64_t pitch_a, int64_t pitch_b,
                  const int64_t *frames_a, const int64_t *frames_b, fd_dtw_rec *rec_dev, int32_t *align_out, int64_t align_pitch, void *stream);
/* clean [B][Lc], degraded [B][Ld] device; valid_clean, valid_degraded HOST [B] or NULL -> rec_dev [B] device.  cfg: NULL = the default. */
FD_API int fd_mcd_measure(fd_handle h, const float *clean, int64_t Lc, const float *degraded, int64_t Ld, int B, const int64_t *valid_clean,
                          const int64_t *valid_degraded, const fd_mcd_config *cfg, fd_mcd *rec_dev, void *stream);

/* Cutting long silences: the `trim_long_sil` switch of the reference's process_utterance (data_gen/tts/data_gen_utils.py:93-147 ->
 * trim_long_silences, :27-90): flag short windows as speech or not, smooth the flags with a moving average, dilate them so that a short
 * pause survives, and drop every sample that is not under the mask.  THIS TEXT defines the method; tests/trim_ref.py restates it in
 * float64 numpy.  Two things differ from the reference on purpose.  (1) The detector is an ENERGY detector, not WebRTC's sub-band GMM
 * (webrtcvad is not in the build image and nobody can run it here): the flags of step 3 are not WebRTC's, and nothing claims closeness
 * to them; steps 4-5 are the reference's exactly.  (2) The reference resamples to 16 kHz to get windows of 480 samples and maps the mask
 * back; here the windows lie on the NATIVE rate's grid (661 samples at 22050 Hz), so no sample is filtered and the output is a bit copy
 * of input samples.  The reference's loudness normalisation in front (to -20 LUFS, :42-47) is fd_loudness_normalize: the caller's step.
 *
 * Parameters (fd_trim_params): sample_rate; window_ms 10, 20 or 30 [30]; top_db [40, the dynamic range fd_stoi_measure uses for the same
 * question] finite and > 0; floor_db [-70] finite; average_width A [8] 1 .. 64; max_silence G [12] even, 0 .. 254; mode
 * FD_TRIM_LONG / FD_TRIM_EDGES; reserved 0.  One utterance of n valid samples:
 *  1. Windows.  W = window_ms sample_rate / 1000, M = max(1, n / W) (integer divisions; fd_trim_windows).  Window w < M - 1 covers
 *     [w W, (w + 1) W), the last one [(M - 1) W, n): it takes the tail, up to 2 W - 1 samples, or fewer than W when n < W.
 *  2. Level.  m_w = the window's mean, e_w = the mean of (x - m_w)^2, level_w = 10 log10(max(e_w, 1e-20)) dB re full scale; float64
 *     from the float32 samples.  A window that holds a sample that is not finite (on the bits) has no level: it is not speech, takes no
 *     part in the peak and is counted in `nonfinite`.
 *  3. Decision.  peak = max_w level_w (-inf if no window has a level); threshold = max(peak - top_db, floor_db);
 *     speech_w = level_w > threshold.
 *  4. Smoothing (:75-82).  c_w = the speech flags among windows w - (A - 1) / 2 .. w + A / 2 (integer divisions; outside 0 .. M - 1:
 *     0);  smooth_w = 2 c_w > A  (np.round takes halves to even: 4 of 8 is 0).
 *  5. Dilation (:85).  keep_w = any smooth_v with |v - w| <= G / 2: binary_dilation(smooth, ones(G + 1)).  FD_TRIM_EDGES instead keeps
 *     every window from the first kept one to the last: the edge-only trim of vocoder recipes.
 *  6. Compaction.  out = the samples of the kept windows in order, bit copies; n_out = their count; out[n_out .. L - 1] = 0.
 *  7. Status.  FD_TRIM_OK;  FD_TRIM_SILENT: no window kept, n_out = 0;  FD_TRIM_EMPTY: n = 0 (the record then counts 0 windows).
 *
 * On the device, three launches, none of which waits on another workgroup.  Levels: a wavefront per window; a lane adds every 64th
 * group of 4 consecutive samples of the window in ascending order, the lanes are added by a butterfly (xor 32 .. 1), once for the mean
 * and once for the squares (a window of up to 3075 samples -- every rate up to 48 kHz -- is loaded once and held in registers for
 * both; a longer one is read again from the cache, in the same order); 16-byte loads where a group's address allows,
 * 4-byte ones elsewhere -- the order of the sum does not depend on the address.  Mask: one workgroup per utterance, FD_TRIM_CHUNK windows
 * at a time with the running counts carried from chunk to chunk: the peak, then prefix counts of the speech flags, from them the
 * smoothed flags and their prefix counts, from those the kept flags and the exclusive prefix of kept samples per window; it writes
 * out_valid, the flags and the record.  Gather: a workgroup per tile of output samples finds the window of its first sample by
 * bisection in that prefix table and copies run by run; tiles behind n_out write zeros.  A window's level depends on its samples alone, and
 * nothing at or behind valid[b] is read: an utterance's outputs are bit-identical alone, anywhere in a ragged batch with anything behind
 * it, at any 4-byte alignment and from call to call.  Scratch (levels, prefix tables) lives in a buffer of the handle that grows at the
 * first call that needs more -- never inside a stream capture (FD_ERR_STATE). */
#define FD_TRIM_CHUNK 256           /* windows of one utterance per pass of the mask kernel's workgroup */
enum { FD_TRIM_OK = 0, FD_TRIM_SILENT = 1, FD_TRIM_EMPTY = 2 };
enum { FD_TRIM_LONG = 0, FD_TRIM_EDGES = 1 };
typedef struct fd_trim_params {
    int32_t sample_rate, window_ms, average_width, max_silence, mode, reserved;      /* reserved: 0 */
    double top_db, floor_db;
} fd_trim_params;                   /* 40 bytes */
typedef struct fd_trim {
    int32_t n_out, windows, speech, kept_windows, nonfinite, status;      /* status: FD_TRIM_* */
    double peak_db, threshold_db;
} fd_trim;                          /* 40 bytes */

/* 30 ms windows, top_db 40, floor_db -70, A = 8, G = 12, FD_TRIM_LONG at `sample_rate` (pure host code).  FD_ERR_INVALID: null. */
FD_API int fd_trim_default_params(int sample_rate, fd_trim_params *p);
/* W and M of n samples (pure host code; either pointer may be NULL).  FD_ERR_INVALID: n < 0, a rate outside 8000 .. 192000, a window_ms
 * other than 10, 20, 30. */
FD_API int fd_trim_windows(int64_t n, int sample_rate, int window_ms, int64_t *W, int64_t *M);
/* Steps 4-5 on the host (csrc/fd_trim.h), for tests and for callers with flags of their own: speech [M] (0 / 1) -> flags_out [M], bit 0
 * speech, bit 1 smooth, bit 2 keep.  FD_ERR_INVALID: a null pointer, M < 1, A, G or mode out of range. */
FD_API int fd_trim_mask(const uint8_t *speech, int64_t M, int average_width, int max_silence, int mode, uint8_t *flags_out);
/* Step 2 alone: wav [B][L] device -> levels_out [B][Mmax] device float64, Mmax = M of L; a window without a level holds a quiet NaN
 * (0x7FF8000000000000), columns behind an item's M hold 0.  Arguments as in fd_trim_silences. */
FD_API int fd_trim_levels(fd_handle h, const float *wav, int B, int64_t L, const int64_t *valid, int sample_rate, int window_ms,
                          double *levels_out, void *stream);
/* wav [B][L] device float -> out [B][L] device float (steps 1-6; must not overlap wav) and out_valid [B] device int32 = n_out.
 * valid: HOST [B] or NULL = samples of each row that count (0 .. L).  flags: NULL or device uint8 [B][Mmax], Mmax = M of L: bit 0
 * speech, bit 1 smooth, bit 2 keep, 0 behind an item's M.  rec_dev: NULL or device [B].  Asynchronous on `stream` and capturable: the
 * output has the input's capacity, so no host read decides a launch.  B 1 .. 4096, L 1 .. 2^31 - 1.  Like fd_loudness_measure it does
 * not settle a pending lazily checked fd_sample.
 * FD_ERR_INVALID: a null pointer, wav or out not 4-byte aligned, out overlapping wav, B, L or valid[b] out of range, parameters refused
 * (the message says which); FD_ERR_STATE: the scratch buffer would have to grow inside a stream capture. */
FD_API int fd_trim_silences(fd_handle h, const float *wav, int B, int64_t L, const int64_t *valid, const fd_trim_params *params, float *out,
                            int32_t *out_valid, uint8_t *flags, fd_trim *rec_dev, void *stream);

/* Parallel WaveGAN: the reference's neural baseline vocoder (vocoders/pwg.py over modules/parallel_wavegan: ParallelWaveGANGenerator,
 * Yamamoto et al. 2020), behind the interface of the other two vocoders.  THIS TEXT defines the computation; tests/pwg_ref.py restates
 * it in float64, and the executed reference confirms that restatement (tools/gen_pwg_reference.py).
 *
 * The network, weight norm removed.  w = aux_context_window, scales s_1 .. s_n, hop = their product, T frames -> L = hop T samples.
 *   c      [80][T + 2 w]: the conditioning, already padded.  fd_pwg_generate forms it from a mel [80][T] when padded = 0, as
 *          PWG.spec2wav does: the optional (mel - mean) / scale per channel, then w frames of edge replication on each side.
 *   u_0    = conv_in(c): 80 -> 80, 2 w + 1 taps, no bias, no padding: [80][T].
 *   u_i    [80][T s_1 .. s_i], i = 1 .. n: u_{i-1} stretched by s_i (each sample repeated s_i times), then 2 s_i + 1 taps per channel
 *          with zero padding s_i, no bias: u_i[m] = sum_k taps_i[k] stretched[m + k - s_i], zero outside the stretched signal.
 *   x_0    = first_conv(z): 1 -> 64, x_0[j][t] = w[j] z[t] + b[j].
 *   layer l = 0 .. layers - 1, dilation d = 2^(l mod (layers / stacks)):
 *          g = conv(x_l): 64 -> 128, taps at t - d, t, t + d, zero outside [0, L), with bias;  g += W_aux_l u_n  (128 x 80, no bias);
 *          h = tanh(g[0 .. 63]) * sigmoid(g[64 .. 127]);   skip += W_skip h + b_skip;   x_{l+1} = (W_out h + b_out + x_l) * sqrt(1/2).
 *   y      = W_2 relu(W_1 relu(skip * sqrt(1 / layers)) + b_1) + b_2: 64 -> 64 -> 1.
 * z is the caller's [B][L], or, z NULL, sample t of item b is component t & 3 of the float4 t >> 2 of fd_sample's generator
 * (Philox4x32-10 + Box-Muller) on the stream word FD_PWG_PHILOX_STREAM with id = stream_ids[b] (NULL: b): with ids an item's noise does
 * not depend on the batch it sits in.  fd_pwg_draw writes exactly those values.
 *
 * What is fixed: residual 64, gate 128, skip 64, aux 80 channels, kernel size 3, non-causal, bias, one input and one output channel,
 * ConvInUpsampleNetwork with nearest interpolation, no activation and frequency kernel 1.  Free: layers 1 .. 30, stacks dividing
 * layers with the largest dilation <= 512, w 0 .. 4, 1 .. 4 scales of 2 .. 16 with hop <= 512.  fd_pwg_create refuses everything else
 * with the field and its value in the message.
 *
 * On the device.  The up-sampling network is linear, has no activation and acts per channel along time, so it commutes with every
 * layer's 128 x 80 projection, the zero padding of every stage included.  fd_pwg_commit composes W_aux_l conv_in on the host in float64
 * into one convolution of 2 w + 1 taps with 128 layers outputs; the front kernel runs it at the frame rate: G[b][l][128][T], float32,
 * each output one fmaf chain over (channel, tap) ascending.  The [80][L] conditioning never exists.  The n stages composed act on G as
 * at most five neighbouring frames with coefficients that depend on the sample alone (its phase in every stage, and which of its
 * neighbours lie outside the item at that stage's rate: those contribute zero): one small kernel per call writes them, K[b][5][L], summed
 * in float64 over the stage paths in a fixed order.  Then one kernel per residual block: a workgroup of 256 threads owns FD_PWG_TILE = 512
 * samples of one item, each wave 64 of them at a time.  Both contractions (128 x 192 and 128 x 64, out and skip stacked) run on the exact-fp32
 * matrix instruction v_mfma_f32_32x32x2_f32 (bit for bit an fmaf chain): the x operand is read straight from x_l [B][64][L] -- 32
 * consecutive samples per half wave, zero outside [0, L_b) whatever lies there in memory -- the weights from an image packed at commit
 * in the instruction's operand order.  The conditioning and the biases are further steps of the same contractions (k = a frame of G under the wave times the
 * sample's coefficient on it; k = the bias times one), after the taps; the 128 rows go in two passes of 32 + 32; h crosses from the result
 * layout to the operand layout through LDS.  x_{l+1} goes to the other of two buffers, skip is float32 and read, added to and written
 * by its one owner (layer 0 writes it; the last layer writes no x).  Layer 0 forms x_0 from z itself, halo included.  The tail is a
 * kernel of its own on the same instruction; it writes zeros from L_b to hop T.  Every sum has a fixed order that does not depend on
 * the batch, there are no atomics and no workgroup waits for another: an item is bit-identical alone, anywhere in a ragged batch and
 * from call to call.  Tiles behind an item's L_b return at once.  G, K, the two x buffers and skip live in a buffer of the handle that
 * grows at the first call that needs more (not inside a stream capture: FD_ERR_STATE; call it once before); otherwise a call is
 * asynchronous on `stream` and capturable. */
#define FD_PWG_TILE 512                 /* samples of one item per workgroup of the layer kernel */
#define FD_PWG_PHILOX_STREAM 0xFFFFFFF7u
#define FD_PWG_MAX_LAYERS 30
#define FD_PWG_MAX_DILATION 512
#define FD_PWG_MAX_CONTEXT 4
#define FD_PWG_MAX_SCALES 4
#define FD_PWG_MAX_SCALE 16
#define FD_PWG_MAX_HOP 512
#define FD_PWG_MAX_FRAMES 32768         /* T: 64 channels of hop T float32 samples stay below 2^32 bytes */
enum { FD_PWG_CONV_IN_UPSAMPLE = 0, FD_PWG_UPSAMPLE = 1, FD_PWG_MELGAN = 2 };      /* fd_pwg_config::upsample_net */
typedef struct fd_pwg_config {          /* the reference constructor's arguments; fd_pwg_default_config sets its defaults */
    int32_t in_channels, out_channels, kernel_size, layers, stacks;
    int32_t residual_channels, gate_channels, skip_channels, aux_channels, aux_context_window;
    int32_t bias, use_causal_conv, upsample_conditional_features, use_pitch_embed, use_nsf;
    int32_t upsample_net;               /* FD_PWG_CONV_IN_UPSAMPLE */
    int32_t n_scales, upsample_scales[8];
    int32_t upsample_activation;        /* 0: none (nonlinear_activation = None) */
    int32_t interpolate_nearest;        /* 1: interpolate_mode = "nearest" */
    int32_t freq_axis_kernel_size;      /* 1 */
} fd_pwg_config;                        /* 112 bytes */
typedef struct fd_pwg *fd_pwg_handle;

FD_API void fd_pwg_default_config(fd_pwg_config *cfg);
/* hop * frames, or -1 for a configuration fd_pwg_create refuses or frames < 0 (pure host code). */
FD_API int64_t fd_pwg_samples(const fd_pwg_config *cfg, int64_t frames);
/* 2 * (the sum of the layers' dilations) + 1: 6139 for the default; -1 for a configuration fd_pwg_create refuses (pure host code). */
FD_API int64_t fd_pwg_receptive_field(const fd_pwg_config *cfg);
/* A generator on the device of `h`, whose error text and scratch buffer it uses (fd_last_error(h); of a refusal made before any handle
 * exists: fd_last_error(NULL)).  Destroy it before `h`.  The configuration is checked before the handle is looked at.
 * FD_ERR_INVALID: a null pointer; FD_ERR_UNSUPPORTED: a field outside the specialised path, named with its value. */
FD_API int fd_pwg_create(fd_handle h, const fd_pwg_config *cfg, fd_pwg_handle *out);
/* One tensor by the reference's state-dict name after weight-norm removal (first_conv.weight, upsample_net.conv_in.weight,
 * upsample_net.upsample.up_layers.{1,3,..}.weight, conv_layers.L.{conv,conv1x1_aux,conv1x1_out,conv1x1_skip}.{weight,bias},
 * last_conv_layers.{1,3}.{weight,bias}): HOST float32, n elements in the reference's layout.  FD_ERR_MISSING: no such tensor in this
 * configuration; FD_ERR_INVALID: n is not its size, or an element is not finite. */
FD_API int fd_pwg_set_weight(fd_pwg_handle p, const char *name, const float *data, int64_t n);
/* Packs the images and uploads them (synchronous; not inside a stream capture).  FD_ERR_MISSING: a tensor was never set (named). */
FD_API int fd_pwg_commit(fd_pwg_handle p);
/* mean, scale: HOST [80] (a StandardScaler's mean_ and scale_), or both NULL: no scaler.  Applies to calls with padded = 0.  Synchronous
 * upload: not inside a stream capture.  FD_ERR_INVALID: one NULL, a value not finite, a scale of 0. */
FD_API int fd_pwg_set_scaler(fd_pwg_handle p, const float *mean, const float *scale);
/* mel_or_c: device, [B][80][T] (padded = 0: a mel; the scaler and the edge replication happen inside, by index clamp against lens[b])
 * or [B][80][T + 2 w] (padded = 1: c as ParallelWaveGANGenerator.forward takes it; item b's frames are its first lens[b] + 2 w columns).
 * lens: HOST [B] frames, 0 .. T, or NULL (T); item b yields L_b = hop lens[b] samples.  z: device [B][hop T] or NULL (Philox: seed,
 * stream_ids HOST [B] or NULL).  wav_out: device, [B] rows wav_pitch >= hop T floats apart: y on [0, L_b), zeros from L_b to hop T.
 * Asynchronous on `stream`.  The arguments are checked before the handles are looked at.  FD_ERR_INVALID: a null pointer or handle, B
 * outside 1 .. 4096, T outside 1 .. FD_PWG_MAX_FRAMES, wav_pitch < hop T, lens[b] out of range; FD_ERR_STATE: not committed, or the
 * scratch buffer would have to grow inside a stream capture. */
FD_API int fd_pwg_generate(fd_pwg_handle p, const float *mel_or_c, int padded, int B, int T, const int64_t *lens, const float *z, uint64_t seed,
                           const uint64_t *stream_ids, float *wav_out, int64_t wav_pitch, void *stream);
/* z_out[b][t], t < L, rows z_pitch >= L floats apart: the z that fd_pwg_generate draws for item b with z NULL (device; stream_ids HOST
 * [B] or NULL).  Asynchronous on `stream`.  FD_ERR_INVALID: a null pointer or handle, B outside 1 .. 4096, L outside 1 .. 2^31 - 1. */
FD_API int fd_pwg_draw(fd_handle h, int B, int64_t L, uint64_t seed, const uint64_t *stream_ids, float *z_out, int64_t z_pitch, void *stream);
/* Frees the device images (waits for the device).  NULL is accepted. */
FD_API int fd_pwg_destroy(fd_pwg_handle p);

/* Long-form and streaming synthesis (no counterpart in the reference, which vocodes an utterance in one piece).  The denoiser's
 * receptive field is finite: one reverse step moves an output sample only through inputs within h = 16 frames of it, N steps within
 * H = N*h.  fd_sample_span therefore computes an utterance window by window -- each window a batch item of fd_sample
 * with `lens`, its own zero padding at its edges, its Philox noise keyed on the utterance's absolute sample index -- and keeps from each
 * window the centre that lies at least H frames from its inner edges.  The result is bit-identical to the whole-utterance fd_sample
 * (with fd_set_noise_streams({stream_id})) on every kept frame unless a window batch handed a stage over to the fp32 kernels (range
 * check, see fd_sample), and the device memory it needs depends on the window, not on the utterance: an utterance past fd_sample's
 * B*T*256*32 < 2^31 limit, or one whose mel is still arriving, can be vocoded.  A streaming caller needs H frames of mel beyond the last
 * frame it asks for: that is the lookahead (64 frames = 0.74 s at N = 4, 22.05 kHz). */

/* Frames of halo per side that fd_sample_span adds for an N-step schedule of the base.yaml architecture (pure host code, no handle, like
 * fd_kernel_index).  < 0 for N outside 1..1024. */
FD_API int fd_sample_halo_frames(int N);

/* x_0 on frames [t0, t1) of ONE utterance, computed window by window, with each window as a batch item of fd_sample.
 *   mel        [1,80,mel_frames] device: utterance frames [mel_first, mel_first + mel_frames)
 *   utt_frames the utterance's length, or -1 while it is not yet known (streaming); then t1 + H <= mel_first + mel_frames
 *   mel must cover [max(0, t0 - H), min(utt_frames, t1 + H)), with H = fd_sample_halo_frames(N)
 *   t0 a multiple of 32; t1 a multiple of 32 unless t1 == utt_frames
 *   x_T, z     NULL = Philox (seed, stream_id) keyed on the absolute sample index, i.e. the noise that fd_set_noise_streams({stream_id})
 *              + fd_sample on the whole utterance draws.  Or caller tensors over the same frames as mel ([1,1,mel_frames*256],
 *              [N,1,1,mel_frames*256]; z only for N <= 8)
 *   window_frames  centre frames per window (a multiple of 32), 0 = the library's default: windows of max(1024, 4H) frames rounded up
 *              to 32, centre = that - 2H (N = 4: 1024-frame windows, 896-frame centres)
 *   out        [1,1,(t1-t0)*256] device
 * Window starts are multiples of 32 frames (the kernels' frame phase); about 16k frames run as one fd_sample batch: up to 32 windows
 * with Philox noise (the call is then one span of fd_sample_spans, below), up to 8 with injected x_T / z.
 * Settles its own range check before it returns, whatever defer_check says.  Settles a pending deferred fd_sample first.
 * FD_ERR_UNSUPPORTED: a handle of another architecture than base.yaml's, or any stage on the naive kernels (they ignore lens).
 * FD_ERR_INVALID: t0 / t1 misaligned or t1 > utt_frames, mel not covering the halo, injected z with N > 8. */
FD_API int fd_sample_span(fd_handle h, const float *mel, int64_t mel_first, int64_t mel_frames, int64_t utt_frames, int64_t t0, int64_t t1,
                          const fd_step *table, int N, int ddim, const float *x_T, const float *z, uint64_t seed, uint64_t stream_id,
                          int window_frames, float *out, void *stream);

/* Frame ranges of MANY utterances in shared window batches: a directory of long recordings, or the chunks that became ready on a set
 * of live streams, vocoded with the sampler's batch filled instead of one call per utterance ("Many utterances per
 * window batch").  One fd_span is what one fd_sample_span call takes, Philox noise only, with the mel either in a plain buffer or in a
 * ring that fd_mel_ring_append feeds. */
typedef struct fd_span {          /* one frame range of one utterance */
    const float *mel;             /* device; channel c, utterance frame f at mel[c*mel_pitch + col(f)] */
    int64_t mel_pitch;            /* floats between channel rows */
    int64_t mel_cap;              /* 0: col(f) = f - mel_first (a plain buffer); > 0: col(f) = f % mel_cap (a ring) */
    int64_t mel_first, mel_frames;/* the utterance frames the buffer holds; mel_frames <= mel_cap for a ring */
    int64_t utt_frames;           /* or -1: not known yet */
    int64_t t0, t1;               /* same rules as fd_sample_span */
    uint64_t stream_id;
    float *out;                   /* device, [(t1 - t0) * 256] */
} fd_span;
/* One window of the plan: batch item of fd_sample call number `batch`, utterance frames [start, start + len) of span `span`, of which
 * the centre [c0, c0 + clen) is kept. */
typedef struct fd_span_window { int32_t span, batch, len, clen; int64_t start, c0; } fd_span_window;
/* `frames` frames of src ([80][frames] device, rows src_pitch floats apart) = utterance frames first_frame .. of a ring of `cap` columns
 * (rows `pitch` floats apart) */
typedef struct fd_ring_chunk { float *ring; int64_t pitch, cap, first_frame; const float *src; int64_t src_pitch, frames; } fd_ring_chunk;

/* The plan fd_sample_spans runs (pure host code, no handle; the pointers of the spans are not looked at).  Every span is cut into
 * windows by fd_sample_span's rules -- centres of C = window_frames (0 = the default above) frames, window start max(0, floor32(c0 - H)),
 * window end min(utt_frames, c0 + clen + H) -- and the windows of ALL spans fill the batches in span order: a batch holds at most 32
 * windows and at most 16384 padded frames, and a span may continue in the next batch.  *Wp = the padded frames of every batch item,
 * which follow the centre actually needed: min(C, the longest span rounded up to 32) plus the halos, so 32 one-chunk stream windows do
 * not reserve 32 default-size windows (the workspace costs about 298 KB per padded frame).
 * Returns the number of windows and writes the first max_windows of them (windows NULL: counts only); 0 for n_spans = 0.
 * FD_ERR_INVALID: a refusal of fd_sample_span in any span, a ring with mel_frames > mel_cap, mel_pitch shorter than a row. */
FD_API int fd_sample_spans_plan(const fd_span *spans, int n_spans, int N, int window_frames, fd_span_window *windows, int max_windows,
                                int *Wp);

/* x_0 of every span, written to its own `out`.  Per batch of the plan: one gather launch (k_spans_gather: plain or ring columns ->
 * [Bw,80,Wp]), one fd_sample with lens, each window's stream id and absolute sample offset, Philox noise (`seed` per call, stream_id per
 * span), its range check settled, one scatter launch (k_spans_scatter).  Preconditions and status codes of fd_sample_span; n_spans = 0
 * succeeds and does nothing.
 *   - The caller gives distinct utterances distinct stream_ids: two utterances with one id draw the same noise at the same samples.
 *   - The outputs of one call must not overlap (each span's [(t1-t0)*256] floats; any alignment -- a 16-byte aligned one is copied 16
 *     bytes per lane).  The mel buffers are only read and may be shared.
 *   - Every span's result is bit-identical to its own fd_sample_span call, whatever else shares the call, while no batch hands a stage
 *     over to the fp32 kernels: a batch that raised a range flag is redone as a whole, so a window that shares it with the offending
 *     one is then computed on the fp32 twins too.  That is already the rule among the windows of one utterance.
 *   - Counter "calls_redone" (fd_get_counter) tells when this happened. */
FD_API int fd_sample_spans(fd_handle h, const fd_span *spans, int n_spans, const fd_step *table, int N, int ddim, uint64_t seed,
                           int window_frames, void *stream);

/* Appends mel to rings on the device, n <= 4096 chunks in one launch (k_ring_append): frame first_frame + i of a chunk goes to column
 * (first_frame + i) % cap of each of the ring's 80 rows.  A ring keeps the last `cap` frames of its utterance; a span on it names the
 * frames it still holds (mel_first, mel_frames) and the gather decides validity on those utterance frames, never on columns, so a
 * reused ring need not be cleared.  The chunks of one call must not write the same column of the same ring.  Asynchronous on `stream`.
 * FD_ERR_INVALID: frames > cap, pitch < cap, src_pitch < frames, a null pointer. */
FD_API int fd_mel_ring_append(fd_handle h, const fd_ring_chunk *chunks, int n, void *stream);

/* Weights from live device tensors (no counterpart in the reference, whose modules read their own parameters).  fd_set_weight +
 * fd_commit_weights go through the host and rebuild everything a handle holds: a new weight arena, every captured graph dropped, the
 * device synchronised.  A training loop that evaluates its model every few hundred steps (FastDiff.py:52-119) changes only the VALUES:
 * fd_refresh_weights_device rebuilds every operand pack of the tuned kernel set IN PLACE, on the device, from the parameter tensors where
 * they lie -- weight norm folded as fd_commit_weights folds it (per row the double sum of squares in index order, one correctly rounded
 * float division), the packs gathered through the same index functions as the host packer's (csrc/fd_wpack.h) -- so the arena ends up
 * byte-equal to a host commit of the same tensors, no pointer of the handle changes, and the captured graphs stay valid.
 *   items      HOST array of n tensors; name / dims as fd_set_weight takes them (<parameter>.weight, or .weight_v + .weight_g, and
 *              .bias); data: DEVICE pointer on the handle's device, float32, contiguous.  They are read by kernels enqueued on `stream`:
 *              keep them alive and unwritten until those have run (stream order suffices).  fc_t1 / fc_t2 must come as .weight.
 *   Asynchronous on `stream`; allocates only at the first call (a work list of a few KB; never inside a capture); never synchronises
 *   the device.  Ordered like every other call of the handle (one stream at a time, fastdiff_hip.h); settles a pending deferred
 *   fd_sample first, which would otherwise be redone on the new weights.  The cached step-embedding rows are invalidated.
 *   Range flags: whether every weight of a kernel family fits the fp16 range decides which kernels that family launches, and a captured
 *   graph has the choice baked in.  The kernels OR the families that do not fit into one device word; the first inference call after a
 *   refresh waits for the refresh alone, reads that word, and only if a family changed sides -- a weight left or re-entered
 *   |w| < 32768 -- synchronises and drops the graphs.
 * FD_ERR_UNSUPPORTED: a handle of another architecture than base.yaml's (use fd_set_weight + fd_commit_weights), fc_t1 / fc_t2 given
 * weight-normed.  FD_ERR_INVALID: no committed weights yet (fd_commit_weights lays the arena out once), an unknown key, a wrong shape, a
 * missing tensor.  Nothing has been written when an error is returned.  A later fd_set_weight + fd_commit_weights works as before. */
typedef struct fd_weight_ref {
    const char *name;
    const float *data;
    const int64_t *dims;
    int32_t ndim, reserved;
} fd_weight_ref;
FD_API int fd_refresh_weights_device(fd_handle h, const fd_weight_ref *items, int n, void *stream);

/* Test / introspection hooks (not on the reference's API surface) -------------------------------------- */

/* The committed weight image (the arena of the tuned kernel set, or the generic path's weights) as bytes; host_buf NULL: *nbytes := its
 * size.  Synchronises the device.  Two handles hold equal images exactly when they hold the same weights in the same packs. */
FD_API int fd_get_weight_image(fd_handle h, void *host_buf, size_t *nbytes);
/* The six range flags of the tuned kernel set's weights as bits (1 = every weight of the family fits fp16): 1 predictor GEMM, 2 its
 * Winograd form, 4 LVC convs, 8 DBlocks, 16 ConvTranspose, 32 predictor front.  Settles a pending refresh's flags (waits for it). */
FD_API int fd_get_weight_flags(fd_handle h, unsigned *ok_mask);
/* The layout functions both weight packers share (csrc/fd_wpack.h), for tests (pure host code, no handle): the index into the folded
 * source tensor that destination position `pos` of a pack holds.  pack: "pack_a" / "a_h2" (p0 = cin, p1 = ks: fp32 / fp16-piece
 * A operands of a conv weight [cout][cin][ks]; a_h2: pos = mt * inner + i over one piece), "up" / "up_h2" (p0 = ratio r: ConvTranspose
 * weight [32][32][2r]; up_h2: pos = ph * 2048 + i), "h16" (pos = (rt*3 + tap) * 512 + idx into [32][32][3]), "final_fuse" (into [32][7];
 * 224 = the pad), "gemm_row" (pos = packed record position: kernel_conv row, or 24576 + bias_conv row), "gemm" / "gemm_h2" (pos inside a
 * 32-column tile: column * 192 + weight).  < 0: unknown pack. */
FD_API int fd_pack_source(const char *pack, int p0, int p1, int pos);

/* Copies an intermediate of the LAST fd_forward to host (synchronises).  Names: "noise" [B,3,80], "a0".."a3",
 * "kp_h<n>" [B,64,T], "kpack<n>" [B,T,24832] (packed predicted kernels+bias of block n), "x<n>" [B,32,L_n],
 * "range_flags" (32 int32 bit patterns: [0] predictor GEMM, [1 + 4*block + layer] LVC layer, [13 + d] DBlock d,
 * [16 + n] ConvTranspose of block n -- set when an operand of the last fd_forward did not fit fp16 and the fp32 kernel redid
 * that launch; fd_sample clears them every step), "range_flags_call" (the same 32 words OR-ed over all steps of the last fd_sample).
 * Returns the number of floats (also when host_dst is NULL), or a negative status. */
FD_API int64_t fd_read_tap(fd_handle h, const char *name, float *host_dst, int64_t capacity);

/* Position of predicted-kernel element (layer, in, out, tap), and of predicted bias (layer, out), inside one frame's
 * 24832-float packed record.  Lets tests unpack "kpack<n>" into the reference's [B,4,32,64,3,T] / [B,4,64,T] views
 * (modules.py:333-342). */
FD_API int fd_kernel_index(int layer, int in_ch, int out_ch, int tap);
FD_API int fd_bias_index(int layer, int out_ch);

/* Per-kernel timing gathered with hipEvents on the launch stream while option "profile"="1" (graph off).
 * Fills up to `capacity` entries; returns the number of distinct kernels. */
typedef struct fd_kernel_stat {
    char name[48];
    int64_t launches;
    double total_ms;
} fd_kernel_stat;
FD_API int fd_get_profile(fd_handle h, fd_kernel_stat *stats, int capacity);
FD_API int fd_reset_profile(fd_handle h);

/* Bookkeeping of the host-checked range fallback (option "fallback" = "host") and of the graph cache.  Names:
 *   "pieces"         8-step pieces the last fd_sample of more than 8 steps was enqueued as (0 for a shorter call);
 *   "pieces_redone"  of those, the pieces that raised a range flag and were run again from the saved x (settles a pending last piece);
 *   "pieces_fp32"    of those, the pieces enqueued with stages already on their fp32 kernels (after an earlier piece had flagged them);
 *   "fp32_mask"      the flag words (bit i = word i of "range_flags") those later pieces ran on fp32 -- sticky over the call;
 *   "calls_redone"   fd_sample calls of up to 8 steps run again as a whole since fd_create;
 *   "graph_captures" / "graph_hits" / "graph_evictions"   fd_sample's graph look-ups since fd_create that captured a new graph / found
 *                    one / pushed the least recently used one out; "graphs_resident" / "graphs_retired" = kept now / evicted but not
 *                    yet destroyed (their last replay has not completed).
 *   "weight_refreshes" fd_refresh_weights_device calls since fd_create; "refresh_graph_drops" = of those, the ones after which a range
 *                    flag had changed and the graphs were dropped.
 *   "span_batches" / "span_windows"   fd_sample calls made by fd_sample_span and fd_sample_spans since fd_create / the windows in them.
 *   "workspace_bytes" device memory of the handle's sampler workspace and of fd_sample_span's window batch (bounded by the window, not
 *                    by the utterance).
 * Returns the value (>= 0) or a negative status. */
FD_API int64_t fd_get_counter(fd_handle h, const char *name);

#ifdef __cplusplus
}
#endif
#endif /* FASTDIFF_HIP_EXT_H */
