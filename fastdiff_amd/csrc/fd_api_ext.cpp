// fd_api_ext.cpp -- host side of the entry points of include/fastdiff_hip_ext.h.  In front of the vocoder: the mel front-end, sample-rate
// conversion (fd_resample), the cutting of long silences (fd_trim_*).  Behind it: the int16 epilogue, BS.1770 loudness (fd_loudness_*).
// Scores against a recording: STOI / ESTOI (fd_stoi_*), F0 and the pitch scores (fd_pitch_*), the STFT distances (fd_spectral_*), MCD with
// its alignment (fd_cepstra, fd_dtw, fd_mcd_measure); against a corpus: the k-means bin pass under NDB / JSD (fd_bins_pass).  The baseline
// vocoder: fd_griffin_lim, fd_mel_to_linear, fd_mel_to_linear_nnls; the neural baseline: fd_pwg_*.  Then taps, layout introspection, counters, profiling.  
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "fd_kernels.h"
#include "fd_host.h"
#include "fd_resample.h"
#include "fd_pwg.h"

// The host path the tools below share ("One host path under these tools"): check_counts, enter, the tables (upload_table
// under first_use and refresh), stage_counts, and reserve and run (fd_host.h), in the order arguments, counts, handle, tables, scratch,
// launch.  Every table refuses to be made inside a stream capture but the mel tables under fd_mel_spectrogram / fd_get_mel_filterbank ----
static_assert(sizeof(long long) == sizeof(int64_t), "the kernels read the callers' int64_t counts as long long");

// the caller's counts [B] (null: every row whole) lie in [lo, hi]; checked before the call touches the device or the handle
static int check_counts(fd_handle h, const char *who, const char *name, const int64_t *counts, int B, int64_t lo, int64_t hi)
{
    for (int b = 0; counts && b < B; ++b)
        if (counts[b] < lo || counts[b] > hi)
            FD_FAIL(h, FD_ERR_INVALID, "%s: %s[%d] = %lld outside [%lld, %lld]", who, name, b, (long long)counts[b], (long long)lo, (long long)hi);
    return FD_OK;
}

// the handle's device, and a pending sampler call settled unless it is lazily checked: these tools touch no sampler state, and their
// result is provisional with such a call
static int enter(fd_handle h)
{
    FD_HIP(h, hipSetDevice(h->device));
    return (h->pending.active && h->pending.lazy) ? FD_OK : fd_settle(h);
}

// a constant table -> device memory the handle owns until fd_destroy (a replaced table stays valid for launches still in flight); a
// synchronous copy from pageable memory: complete on return.  Whether this may happen inside a capture is the caller's decision.
static int upload_table(fd_handle h, const char *who, const void *src, size_t bytes, const void **dst)
{
    void *d = nullptr;
    FD_HIP(h, hipMalloc(&d, bytes));
    const hipError_t e = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hipFree(d);
        FD_FAIL(h, FD_ERR_HIP, "%s: table upload failed: %s", who, hipGetErrorString(e));
    }
    h->tables.push_back(d);
    *dst = d;
    return FD_OK;
}

// what is made at a first use is never made inside a stream capture, whose replays would not make it again; what: as the refusal names it
static int refuse_in_capture(fd_handle h, const char *who, hipStream_t stream, const char *what)
{
    if (capturing(stream))
        FD_FAIL(h, FD_ERR_STATE, "%s: %s is made at the first call that uses it, which cannot happen inside a stream capture: call it once before", who, what);
    return FD_OK;
}

// A constant table of the handle made at its first use: `slot` once it is set; else, outside a capture, build() -> std::vector<float>
// on the host and upload_table
template <class Build>
static int first_use(fd_handle h, const char *who, hipStream_t stream, const char *what, const float *&slot, Build &&build)
{
    if (slot) return FD_OK;
    const int rc = refuse_in_capture(h, who, stream, what);
    if (rc != FD_OK) return rc;
    const std::vector<float> tab = build();
    return upload_table(h, who, tab.data(), tab.size() * sizeof(float), reinterpret_cast<const void **>(&slot));
}

// ... and a table keyed on the caller's host values src[n] (fd_context::KeyedTable): kept while they compare equal to the last call's,
// else made again as at a first use from build() (the replaced one stays in `tables`: launches in flight may still read it)
template <class Build>
static int refresh(fd_handle h, const char *who, hipStream_t stream, const char *what, fd_context::KeyedTable &t, const float *src, size_t n, Build &&build)
{
    if (t.dev && memcmp(t.host.data(), src, sizeof(float) * n) == 0) return FD_OK;
    const float *dev = nullptr;
    const int rc = first_use(h, who, stream, what, dev, build);
    if (rc == FD_OK) { t.dev = dev; t.host.assign(src, src + n); }
    return rc;
}

// host counts [B] -> `slot` on the device through the pinned staging ring; *dev: the slot, or null with null counts (every row whole)
static int stage_counts(fd_handle h, const int64_t *counts, int B, long long *slot, hipStream_t stream, const long long **dev)
{
    *dev = counts ? slot : nullptr;
    return counts ? fd_stage_upload(h, counts, sizeof(long long) * B, slot, stream) : FD_OK;
}

// A Parallel WaveGAN generator (fd_pwg_create): the host copies of its tensors by name, and their device image once committed
struct fd_pwg {
    fd_handle owner = nullptr;
    fd_pwg_config cfg{};
    std::vector<fdpwg::Tensor> tensors;
    std::map<std::string, std::vector<float>> w;
    std::vector<float> scaler;          // mean [80], scale [80]
    float *img = nullptr;
    bool committed = false, has_scaler = false;
};

extern "C" {

// The DEFAULT filter bank of a front-end, dense [80][513]: librosa.filters.mel(22050, 1024, 80, fmin, fmax) restated in double
// precision (Slaney mel scale, triangular weights on the FFT bin centres, each filter scaled by 2 / (f[m+2] - f[m])) for 'pwg' (fmin
// 80, fmax 7600; base.yaml:8-9) and Tacotron (0, 8000; FastDiff_tacotron.yaml:20-21).  librosa is not in this image, so these values
// are a restatement pinned only against an independent derivation (tests/test_mel_frontend.py); a deployment that has librosa hands
// its own matrix to fd_set_mel_filterbank and this function is then not used.
static const int MEL_NM = 80, MEL_NB = 513;
static std::vector<float> default_mel_bank(int variant)
{
    const double sr = 22050.0;
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
    auto hz_to_mel = [&](double f) { return f >= min_log_hz ? min_log_mel + log(f / min_log_hz) / logstep : f / f_sp; };
    auto mel_to_hz = [&](double m) { return m >= min_log_mel ? min_log_hz * exp(logstep * (m - min_log_mel)) : f_sp * m; };
    const double band[MEL_VARIANTS][2] = {{80.0, 7600.0}, {0.0, 8000.0}};
    std::vector<double> mf(MEL_NM + 2);
    const double m0 = hz_to_mel(band[variant][0]), m1 = hz_to_mel(band[variant][1]);
    for (int i = 0; i < MEL_NM + 2; ++i) mf[i] = mel_to_hz(m0 + (m1 - m0) * i / (MEL_NM + 1));
    std::vector<float> fb((size_t)MEL_NM * MEL_NB, 0.0f);
    for (int m = 0; m < MEL_NM; ++m) {
        const double enorm = 2.0 / (mf[m + 2] - mf[m]);
        for (int k = 0; k < MEL_NB; ++k) {
            const double fk = (sr / 2.0) * k / (MEL_NB - 1);
            const double lower = (fk - mf[m]) / (mf[m + 1] - mf[m]), upper = (mf[m + 2] - fk) / (mf[m + 2] - mf[m + 1]);
            const double wv = std::max(0.0, std::min(lower, upper));
            if (wv > 0.0) fb[(size_t)m * MEL_NB + k] = (float)(wv * enorm);
        }
    }
    return fb;
}

static int mel_upload(fd_handle h, const void *src, size_t bytes, const void **dst) { return upload_table(h, "mel tables", src, bytes, dst); }

// A dense bank [80][513] as the kernel reads it: per filter the first non-zero bin, the span up to the last non-zero one, and the
// weights of that span exactly as given (k_mel_frontend adds w[k] * |X_k| over the span in ascending k; a zero inside it adds zero).
static int upload_mel_bank(fd_handle h, int variant, const float *fb)
{
    std::vector<int> lo(MEL_NM, 0), cnt(MEL_NM, 0), off(MEL_NM, 0);
    std::vector<float> wts;
    for (int m = 0; m < MEL_NM; ++m) {
        int first = -1, last = -1;
        for (int k = 0; k < MEL_NB; ++k)
            if (fb[(size_t)m * MEL_NB + k] != 0.0f) { if (first < 0) first = k; last = k; }
        off[m] = (int)wts.size();
        if (first >= 0) {
            lo[m] = first; cnt[m] = last - first + 1;
            wts.insert(wts.end(), fb + (size_t)m * MEL_NB + first, fb + (size_t)m * MEL_NB + last + 1);
        }
    }
    if (wts.empty()) wts.push_back(0.0f);
    MelTables t = h->mel[variant];
    int rc;
    if ((rc = mel_upload(h, lo.data(), lo.size() * sizeof(int), reinterpret_cast<const void **>(&t.fb_lo))) != FD_OK) return rc;
    if ((rc = mel_upload(h, cnt.data(), cnt.size() * sizeof(int), reinterpret_cast<const void **>(&t.fb_n))) != FD_OK) return rc;
    if ((rc = mel_upload(h, off.data(), off.size() * sizeof(int), reinterpret_cast<const void **>(&t.fb_off))) != FD_OK) return rc;
    if ((rc = mel_upload(h, wts.data(), wts.size() * sizeof(float), reinterpret_cast<const void **>(&t.fb_w))) != FD_OK) return rc;
    h->mel[variant] = t;
    h->mel_bank[variant].assign(fb, fb + (size_t)MEL_NM * MEL_NB);
    return FD_OK;
}

// Tables of the mel front-end: twiddles and the periodic Hann window in double precision (shared), and each front-end's filter bank
// (the caller's, if fd_set_mel_filterbank supplied one before the first use, else the default above).
static int ensure_mel_tables(fd_handle h)
{
    if (h->mel[MEL_VARIANTS - 1].tab) return FD_OK;
    const int NF = 1024;
    const double pi = 3.14159265358979323846;
    std::vector<float> tab(3 * NF);
    fdt::twiddles(NF, tab.data(), tab.data() + NF);
    for (int i = 0; i < NF; ++i) tab[2 * NF + i] = (float)(0.5 - 0.5 * cos(2.0 * pi * i / NF));
    const float *tab_dev = nullptr;
    int rc;
    if ((rc = mel_upload(h, tab.data(), tab.size() * sizeof(float), reinterpret_cast<const void **>(&tab_dev))) != FD_OK) return rc;
    for (int v = 0; v < MEL_VARIANTS; ++v) {
        if (!h->mel[v].fb_w) {
            const std::vector<float> fb = default_mel_bank(v);
            if ((rc = upload_mel_bank(h, v, fb.data())) != FD_OK) return rc;
        }
        h->mel[v].tab = tab_dev;                           // last: marks this variant ready
    }
    return FD_OK;
}

// ... for the tools behind the front-end (fd_griffin_lim, fd_cepstra, fd_mcd_measure): made at their first call, never inside a capture
static int mel_tables_first_use(fd_handle h, const char *who, hipStream_t stream)
{
    if (h->mel[MEL_VARIANTS - 1].tab) return FD_OK;
    const int rc = refuse_in_capture(h, who, stream, "the set of the mel front-end's tables");
    return rc != FD_OK ? rc : ensure_mel_tables(h);
}

int fd_set_mel_filterbank(fd_handle h, const float *fb, int n_mels, int n_bins)
{
    if (!h) return FD_ERR_INVALID;
    if (n_mels != MEL_NM || n_bins != MEL_NB)
        FD_FAIL(h, FD_ERR_INVALID, "fd_set_mel_filterbank: the front-end is 80 filters over the 513 bins of a 1024-point FFT, got [%d][%d]", n_mels, n_bins);
    FD_HIP(h, hipSetDevice(h->device));
    const int v = h->mel_variant;
    if (!fb) {                                             // back to the restated default
        const std::vector<float> def = default_mel_bank(v);
        h->mel_bank_user[v] = false;
        return upload_mel_bank(h, v, def.data());
    }
    const long bad = fdn::first_nonfinite(fb, (size_t)MEL_NM * MEL_NB);
    if (bad >= 0) FD_FAIL(h, FD_ERR_INVALID, "fd_set_mel_filterbank: element %zu is not finite", (size_t)bad);
    const int rc = upload_mel_bank(h, v, fb);
    if (rc == FD_OK) h->mel_bank_user[v] = true;
    return rc;
}

int fd_get_mel_filterbank(fd_handle h, float *fb_out, int n_mels, int n_bins)
{
    if (!h || !fb_out) return FD_ERR_INVALID;
    if (n_mels != MEL_NM || n_bins != MEL_NB) FD_FAIL(h, FD_ERR_INVALID, "fd_get_mel_filterbank: expects [80][513], got [%d][%d]", n_mels, n_bins);
    FD_HIP(h, hipSetDevice(h->device));
    const int rc = ensure_mel_tables(h);
    if (rc != FD_OK) return rc;
    const int v = h->mel_variant;
    memcpy(fb_out, h->mel_bank[v].data(), sizeof(float) * MEL_NM * MEL_NB);
    return h->mel_bank_user[v] ? 1 : 0;
}

int fd_mel_spectrogram(fd_handle h, const float *wav, int B, int64_t n_samples, float *mel, int T, void *stream)
{
    if (!h || !wav || !mel || B <= 0 || n_samples <= 0 || B > 65535) return FD_ERR_INVALID;
    if (T < 1 || T > 1 + n_samples / 256) FD_FAIL(h, FD_ERR_INVALID, "fd_mel_spectrogram: T=%d outside 1..1+n_samples/256=%lld", T, (long long)(1 + n_samples / 256));
    if (h->mel_variant == MEL_TACOTRON && n_samples <= 512)      // F.pad(mode='reflect') needs pad < length (tacotron/stft.py:84-88)
        FD_FAIL(h, FD_ERR_INVALID, "fd_mel_spectrogram: reflect padding of 512 needs more than 512 samples, got %lld", (long long)n_samples);
    int rc = enter(h);
    if (rc != FD_OK) return rc;
    rc = ensure_mel_tables(h);
    if (rc != FD_OK) return rc;
    return run(h, stream, "fd_mel_spectrogram", [&](const fdk::Launch &L) { return fdk::mel_frontend(L, wav, B, n_samples, mel, T); });
}

int fd_peak_normalize_int16_ragged(fd_handle h, const float *wav, int B, int64_t len, const int64_t *valid, int16_t *pcm, void *stream)
{
    if (!h || !wav || !pcm || B <= 0 || len <= 0 || B > 4096) return FD_ERR_INVALID;
    int rc = enter(h);      // (this entry point has always settled before it looks at the counts)
    if (rc != FD_OK) return rc;
    if ((rc = check_counts(h, "fd_peak_normalize_int16_ragged", "valid", valid, B, 1, len)) != FD_OK) return rc;
    const long long *valid_dev = nullptr;      // behind the abs-max words
    if ((rc = stage_counts(h, valid, B, reinterpret_cast<long long *>(reinterpret_cast<char *>(h->scratch) + 32768), (hipStream_t)stream, &valid_dev)) != FD_OK) return rc;
    return run(h, stream, "fd_peak_normalize_int16", [&](const fdk::Launch &L) { return fdk::peak_normalize_int16(L, wav, B, len, pcm, valid_dev); });
}

int fd_peak_normalize_int16(fd_handle h, const float *wav, int B, int64_t len, int16_t *pcm, void *stream)
{
    return fd_peak_normalize_int16_ragged(h, wav, B, len, nullptr, pcm, stream);
}

// Sample-rate conversion (fastdiff_hip_ext.h; the filter design: fd_resample.h, the kernels: fd_kernels_resample.hip) -----------------
int64_t fd_resample_out_len(int64_t n, int sr_in, int sr_out)
{
    fdr::Ratio r;
    if (n < 0 || !fdr::reduce(sr_in, sr_out, r)) return FD_ERR_INVALID;
    if (std::max(r.up, r.down) > fdr::MAX_RATIO) return FD_ERR_UNSUPPORTED;
    return fdr::out_len(n, r);
}

int fd_resample_taps(int sr_in, int sr_out, float *taps, int64_t capacity, int *up, int *down, int *half)
{
    fdr::Ratio r;
    if (!fdr::reduce(sr_in, sr_out, r) || (taps && capacity < 0)) return FD_ERR_INVALID;
    if (std::max(r.up, r.down) > fdr::MAX_RATIO) return FD_ERR_UNSUPPORTED;
    if (up) *up = r.up;
    if (down) *down = r.down;
    if (half) *half = r.half;
    const int n = 2 * r.half + 1;
    if (taps) {
        const std::vector<float> hp = fdr::taps(r);
        memcpy(taps, hp.data(), sizeof(float) * (size_t)std::min<int64_t>(capacity, n));
    }
    return n;
}

// the device table of a ratio (fd_resample, and fd_stoi_measure's way to 10 kHz)
static int resample_table(fd_handle h, const char *who, const fdr::Ratio &r, hipStream_t stream, const float **dev)
{
    const float *&slot = h->resample_tabs[{r.up, r.down}];      // (a null slot counts as none)
    char what[64] = "";
    if (!slot) snprintf(what, sizeof(what), "the table of ratio %d/%d", r.up, r.down);
    const int rc = first_use(h, who, stream, what, slot, [&] { return fdr::table(r); });
    *dev = slot;
    return rc;
}

int fd_resample(fd_handle h, const void *src, int format, int channels, int B, int64_t n_in, int64_t src_pitch, const int64_t *valid_in,
                int sr_in, int sr_out, float *dst, int64_t dst_pitch, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!src || !dst) FD_FAIL(h, FD_ERR_INVALID, "fd_resample: null %s", !src ? "src" : "dst");
    if (format != FD_PCM_F32 && format != FD_PCM_S16 && format != FD_PCM_S32 && format != FD_PCM_U8)
        FD_FAIL(h, FD_ERR_INVALID, "fd_resample: unknown sample format %d (FD_PCM_F32 / _S16 / _S32 / _U8)", format);
    if (channels < 1 || channels > 8) FD_FAIL(h, FD_ERR_INVALID, "fd_resample: %d channels, 1..8 are supported", channels);
    if (B < 1 || n_in < 1) FD_FAIL(h, FD_ERR_INVALID, "fd_resample: B = %d items of n_in = %lld frames", B, (long long)n_in);
    if (n_in > (INT64_MAX >> 12) / channels) FD_FAIL(h, FD_ERR_INVALID, "fd_resample: n_in = %lld is too long", (long long)n_in);
    fdr::Ratio r;
    if (!fdr::reduce(sr_in, sr_out, r)) FD_FAIL(h, FD_ERR_INVALID, "fd_resample: sample rates %d -> %d", sr_in, sr_out);
    if (std::max(r.up, r.down) > fdr::MAX_RATIO)
        FD_FAIL(h, FD_ERR_UNSUPPORTED, "fd_resample: %d -> %d Hz reduces to %d/%d; ratios up to %d are supported", sr_in, sr_out, r.up, r.down, fdr::MAX_RATIO);
    const int64_t n_out = fdr::out_len(n_in, r);
    if (src_pitch < n_in * channels)
        FD_FAIL(h, FD_ERR_INVALID, "fd_resample: src_pitch = %lld < n_in * channels = %lld", (long long)src_pitch, (long long)(n_in * channels));
    if (dst_pitch < n_out) FD_FAIL(h, FD_ERR_INVALID, "fd_resample: dst_pitch = %lld < out_len(n_in) = %lld", (long long)dst_pitch, (long long)n_out);
    int rc = check_counts(h, "fd_resample", "valid_in", valid_in, B, 1, n_in);
    if (rc != FD_OK || (rc = enter(h)) != FD_OK) return rc;
    const float *table = nullptr;
    if (r.up != r.down && (rc = resample_table(h, "fd_resample", r, (hipStream_t)stream, &table)) != FD_OK) return rc;
    return run(h, stream, "fd_resample", [&](const fdk::Launch &La) {
        return fdk::resample(La, src, format, channels, B, n_in, src_pitch, valid_in, r.up, r.down, r.half, r.K, r.Kp, n_out, table, dst, dst_pitch);
    });
}

// BS.1770 loudness (fastdiff_hip_ext.h; the filter design: fd_loudness.h, the kernels: fd_kernels_loudness.hip) ------------------------
int fd_loudness_design(int rate, double *coef10)
{
    if (!coef10 || !fdl::rate_ok(rate)) return FD_ERR_INVALID;
    fdl::design(rate, coef10);
    return FD_OK;
}

int64_t fd_loudness_blocks(int64_t n, int rate)
{
    if (n < 0 || !fdl::rate_ok(rate)) return FD_ERR_INVALID;
    return fdl::blocks(n, rate);
}

static int loudness_call(fd_handle h, const char *who, const float *wav, int B, int64_t L, const int64_t *valid, int rate, bool normalize,
                         double target, float *out_f32, int16_t *out_pcm, fd_loudness *rec_dev, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!wav) FD_FAIL(h, FD_ERR_INVALID, "%s: null wav", who);
    if (B < 1 || B > 4096 || L < 1 || L > ((int64_t)1 << 40)) FD_FAIL(h, FD_ERR_INVALID, "%s: B = %d utterances (1 .. 4096) of L = %lld samples", who, B, (long long)L);
    if (!fdl::rate_ok(rate)) FD_FAIL(h, FD_ERR_INVALID, "%s: sample rate %d outside %d .. %d", who, rate, fdl::RATE_MIN, fdl::RATE_MAX);
    if (normalize && !out_f32 && !out_pcm) FD_FAIL(h, FD_ERR_INVALID, "%s: neither out_f32 nor out_pcm", who);
    if (normalize && !isfinite(target)) FD_FAIL(h, FD_ERR_INVALID, "%s: the target is not finite", who);
    if (!normalize && !rec_dev) FD_FAIL(h, FD_ERR_INVALID, "%s: null rec_dev", who);
    int rc = check_counts(h, who, "valid", valid, B, 1, L);
    if (rc != FD_OK || (rc = enter(h)) != FD_OK) return rc;
    Scratch &s = h->loud_scratch;
    if ((rc = reserve(h, who, s, fdk::loudness_scratch_bytes(B, L, rate), (hipStream_t)stream)) != FD_OK) return rc;
    const long long *valid_dev = nullptr;
    if ((rc = stage_counts(h, valid, B, fdk::loudness_valid_slot(s.p, B, L, rate), (hipStream_t)stream, &valid_dev)) != FD_OK) return rc;
    fdk::LoudnessFilter F;
    fdl::make_filter(rate, F);
    return run(h, stream, who, [&](const fdk::Launch &La) {
        return fdk::loudness(La, wav, B, L, valid_dev, rate, F, normalize, target, rec_dev, out_f32, out_pcm, s.p);
    });
}

int fd_loudness_measure(fd_handle h, const float *wav, int B, int64_t L, const int64_t *valid, int rate, fd_loudness *rec_dev, void *stream)
{
    return loudness_call(h, "fd_loudness_measure", wav, B, L, valid, rate, false, 0.0, nullptr, nullptr, rec_dev, stream);
}

int fd_loudness_normalize(fd_handle h, const float *wav, int B, int64_t L, const int64_t *valid, int rate, double target_lufs, float *out_f32,
                          int16_t *out_pcm, fd_loudness *rec_dev, void *stream)
{
    return loudness_call(h, "fd_loudness_normalize", wav, B, L, valid, rate, true, target_lufs, out_f32, out_pcm, rec_dev, stream);
}

// STOI / ESTOI (fastdiff_hip_ext.h; constants, band table and counts: fd_stoi.h, the kernels: fd_kernels_stoi.hip) --------------------
int fd_stoi_bands(int *lo15, int *hi15)
{
    if (!lo15 || !hi15) return FD_ERR_INVALID;
    fds::bands(lo15, hi15);
    return FD_OK;
}

int64_t fd_stoi_frames(int64_t n10k)
{
    if (n10k < 0) return FD_ERR_INVALID;
    return fds::frames(n10k);
}

int fd_stoi_measure(fd_handle h, const float *clean, const float *degraded, int B, int64_t L, const int64_t *valid, int rate, fd_stoi *rec_dev,
                    void *stream)
{
    const char *who = "fd_stoi_measure";
    if (!h) return FD_ERR_INVALID;
    if (!clean || !degraded || !rec_dev) FD_FAIL(h, FD_ERR_INVALID, "%s: null %s", who, !clean ? "clean" : (!degraded ? "degraded" : "rec_dev"));
    if (B < 1 || B > 4096 || L < 1) FD_FAIL(h, FD_ERR_INVALID, "%s: B = %d pairs (1 .. 4096) of L = %lld samples", who, B, (long long)L);
    if (rate < fds::RATE_MIN || rate > fds::RATE_MAX) FD_FAIL(h, FD_ERR_INVALID, "%s: sample rate %d outside %d .. %d", who, rate, fds::RATE_MIN, fds::RATE_MAX);
    const bool resampled = rate != fds::RATE;
    fdr::Ratio r;
    if (resampled) {
        if (!fdr::reduce(rate, fds::RATE, r)) FD_FAIL(h, FD_ERR_INVALID, "%s: sample rates %d -> %d", who, rate, fds::RATE);
        if (std::max(r.up, r.down) > fdr::MAX_RATIO)
            FD_FAIL(h, FD_ERR_UNSUPPORTED, "%s: %d -> %d Hz reduces to %d/%d; ratios up to %d are supported", who, rate, fds::RATE, r.up, r.down, fdr::MAX_RATIO);
        if (L > (INT64_MAX >> 12)) FD_FAIL(h, FD_ERR_INVALID, "%s: L = %lld is too long", who, (long long)L);
    }
    const int64_t n10 = resampled ? fdr::out_len(L, r) : L;
    if (n10 > ((int64_t)1 << 30)) FD_FAIL(h, FD_ERR_INVALID, "%s: L = %lld is %lld samples at 10 kHz, at most 2^30 are supported", who, (long long)L, (long long)n10);
    int rc = check_counts(h, who, "valid", valid, B, 1, L);
    if (rc != FD_OK || (rc = enter(h)) != FD_OK) return rc;
    rc = first_use(h, who, (hipStream_t)stream, "the window and twiddle table", h->stoi_tab,
                   [] { std::vector<float> t(fds::TAB_FLOATS); fds::tables(t.data()); return t; });
    if (rc != FD_OK) return rc;
    Scratch &s = h->stoi_scratch;
    if ((rc = reserve(h, who, s, fdk::stoi_scratch_bytes(B, n10, resampled), (hipStream_t)stream)) != FD_OK) return rc;
    const float *table = nullptr;
    if (resampled && (rc = resample_table(h, who, r, (hipStream_t)stream, &table)) != FD_OK) return rc;
    const fdk::StoiSlots sl10 = fdk::stoi_slots(s.p, B, n10, resampled);
    std::vector<int64_t> lens10;      // each pair's own length at 10 kHz
    if (valid && resampled) {
        lens10.resize(B);
        for (int b = 0; b < B; ++b) lens10[b] = fdr::out_len(valid[b], r);
    }
    const long long *lens_dev = nullptr;
    if ((rc = stage_counts(h, lens10.empty() ? valid : lens10.data(), B, sl10.lens, (hipStream_t)stream, &lens_dev)) != FD_OK) return rc;
    fdk::StoiBands bd;
    fds::bands(bd.lo, bd.hi);
    return run(h, stream, who, [&](const fdk::Launch &La) {
        const float *x = clean, *y = degraded;
        long long pitch = L;
        if (resampled) {
            for (int k = 0; k < 2; ++k) {
                const hipError_t e = fdk::resample(La, k ? degraded : clean, FD_PCM_F32, 1, B, L, L, valid, r.up, r.down, r.half, r.K, r.Kp, n10, table,
                                                   k ? sl10.y10 : sl10.x10, sl10.pitch10);
                if (e != hipSuccess) return e;
            }
            x = sl10.x10; y = sl10.y10; pitch = sl10.pitch10;
        }
        return fdk::stoi(La, x, y, pitch, B, n10, lens_dev, h->stoi_tab, bd, rec_dev, s.p, resampled);
    });
}

// F0 tracking and the pitch scores (fastdiff_hip_ext.h; constants, lags and counts: fd_pitch.h, the kernels: fd_kernels_pitch.hip) ------
int fd_pitch_default_config(fd_pitch_config *cfg)
{
    if (!cfg) return FD_ERR_INVALID;
    fdp::defaults(cfg);
    return FD_OK;
}

int fd_pitch_lags(const fd_pitch_config *cfg, int *tau_min, int *tau_max)
{
    fdp::Lags lg;
    if (!cfg || fdp::lags(*cfg, lg)) return FD_ERR_INVALID;
    if (tau_min) *tau_min = lg.tau_min;
    if (tau_max) *tau_max = lg.tau_max;
    return FD_OK;
}

int64_t fd_pitch_frames(int64_t n, int hop)
{
    if (n < 0 || hop < 1) return FD_ERR_INVALID;
    return fdp::frames(n, hop);
}

// the host counts [B] of a pitch call -> slot `which` (0: fd_pitch_track's valid, 1: fd_pitch_compare's frames) of the handle's pitch
// scratch, allocated at the first call that passes counts; *dev = null when counts is null
static int pitch_counts(fd_handle h, const char *who, const int64_t *counts, int B, int which, hipStream_t stream, const long long **dev)
{
    *dev = nullptr;
    if (!counts) return FD_OK;
    const size_t slot = fdk::align256(sizeof(long long) * 4096);      // B <= 4096
    const int rc = reserve(h, who, h->pitch_scratch, 2 * slot, stream);
    if (rc != FD_OK) return rc;
    return stage_counts(h, counts, B, reinterpret_cast<long long *>(reinterpret_cast<char *>(h->pitch_scratch.p) + which * slot), stream, dev);
}

int fd_pitch_track(fd_handle h, const float *wav, int B, int64_t L, const int64_t *valid, const fd_pitch_config *cfg, float *f0_dev,
                   float *aper_dev, int64_t out_pitch, void *stream)
{
    const char *who = "fd_pitch_track";
    if (!h) return FD_ERR_INVALID;
    if (!wav || !cfg || !f0_dev || !aper_dev)
        FD_FAIL(h, FD_ERR_INVALID, "%s: null %s", who, !wav ? "wav" : (!cfg ? "cfg" : (!f0_dev ? "f0_dev" : "aper_dev")));
    fdp::Lags lg;
    if (const char *why = fdp::lags(*cfg, lg)) FD_FAIL(h, FD_ERR_INVALID, "%s: configuration refused: %s", who, why);
    if (B < 1 || B > 4096 || L < 1) FD_FAIL(h, FD_ERR_INVALID, "%s: B = %d utterances (1 .. 4096) of L = %lld samples", who, B, (long long)L);
    const int64_t F = fdp::frames(L, cfg->hop);
    if (F > fdp::MAX_FRAMES) FD_FAIL(h, FD_ERR_INVALID, "%s: L = %lld is %lld frames, at most 2^30 are supported", who, (long long)L, (long long)F);
    if (out_pitch < std::max<int64_t>(F, 1))
        FD_FAIL(h, FD_ERR_INVALID, "%s: out_pitch = %lld is less than the %lld frames of L = %lld", who, (long long)out_pitch, (long long)F, (long long)L);
    int rc = check_counts(h, who, "valid", valid, B, 0, L);
    if (rc != FD_OK || (rc = enter(h)) != FD_OK) return rc;
    const long long *lens_dev = nullptr;
    if ((rc = pitch_counts(h, who, valid, B, 0, (hipStream_t)stream, &lens_dev)) != FD_OK) return rc;
    return run(h, stream, who, [&](const fdk::Launch &La) { return fdk::pitch_track(La, wav, L, B, L, lens_dev, *cfg, lg, f0_dev, aper_dev, out_pitch); });
}

int fd_pitch_compare(fd_handle h, const float *f0_ref, const float *f0_deg, int B, int64_t pitch, const int64_t *frames, fd_pitch *rec_dev,
                     void *stream)
{
    const char *who = "fd_pitch_compare";
    if (!h) return FD_ERR_INVALID;
    if (!f0_ref || !f0_deg || !rec_dev) FD_FAIL(h, FD_ERR_INVALID, "%s: null %s", who, !f0_ref ? "f0_ref" : (!f0_deg ? "f0_deg" : "rec_dev"));
    if (B < 1 || B > 4096 || pitch < 1 || pitch > fdp::MAX_FRAMES)
        FD_FAIL(h, FD_ERR_INVALID, "%s: B = %d tracks (1 .. 4096) of pitch = %lld frames (1 .. 2^30)", who, B, (long long)pitch);
    int rc = check_counts(h, who, "frames", frames, B, 0, pitch);
    if (rc != FD_OK) return rc;
    FD_HIP(h, hipSetDevice(h->device));      // no settle: the tracks are the caller's, and the scores touch no sampler state
    const long long *frames_dev = nullptr;
    if ((rc = pitch_counts(h, who, frames, B, 1, (hipStream_t)stream, &frames_dev)) != FD_OK) return rc;
    return run(h, stream, who, [&](const fdk::Launch &La) { return fdk::pitch_compare(La, f0_ref, f0_deg, pitch, B, frames_dev, rec_dev); });
}

// Multi-resolution STFT distances (fastdiff_hip_ext.h; constants, refusals, counts and tables: fd_spectral.h, the kernels:
// fd_kernels_spectral.hip) ---------------------------------------------------------------------------------------------------------
int fd_spectral_default_config(fd_spectral_config *cfg)
{
    if (!cfg) return FD_ERR_INVALID;
    fdx::defaults(cfg);
    return FD_OK;
}

int64_t fd_spectral_frames(int64_t n, int hop)
{
    if (n < 0 || hop < 1) return FD_ERR_INVALID;
    return fdx::frames(n, hop);
}

int fd_spectral_measure(fd_handle h, const float *clean, const float *degraded, int B, int64_t L, const int64_t *valid,
                        const fd_spectral_config *cfg, fd_spectral *rec_dev, void *stream)
{
    // (the arguments first: their refusals need no handle, and without one the text is left where fd_last_error(NULL) reads it)
    const char *who = "fd_spectral_measure";
    if (!clean || !degraded || !rec_dev) FD_FAIL(h, FD_ERR_INVALID, "%s: null %s", who, !clean ? "clean" : (!degraded ? "degraded" : "rec_dev"));
    if (B < 1 || B > 4096 || L < 1 || L > fdx::MAX_SAMPLES)
        FD_FAIL(h, FD_ERR_INVALID, "%s: B = %d pairs (1 .. 4096) of L = %lld samples (1 .. 2^30)", who, B, (long long)L);
    fd_spectral_config c;
    if (cfg) c = *cfg; else fdx::defaults(&c);
    char why[fdx::MSG];
    if (fdx::refusal(c, why)) FD_FAIL(h, FD_ERR_INVALID, "%s: configuration refused: %s", who, why);
    int rc = check_counts(h, who, "valid", valid, B, 1, L);
    if (rc != FD_OK) return rc;
    if (!h) FD_FAIL(h, FD_ERR_INVALID, "%s: null handle", who);
    if ((rc = enter(h)) != FD_OK) return rc;
    const float *tabs[fdx::MAX_RES] = {nullptr, nullptr, nullptr, nullptr};
    for (int r = 0; r < c.n_res; ++r) {
        const float *&slot = h->spectral_tabs[{c.nfft[r], c.win[r]}];      // (a null slot counts as none)
        char what[96] = "";
        if (!slot) snprintf(what, sizeof(what), "the window and twiddle table of nfft = %d, win = %d", c.nfft[r], c.win[r]);
        rc = first_use(h, who, (hipStream_t)stream, what, slot,
                       [&] { std::vector<float> t(fdx::table_floats(c.nfft[r])); fdx::tables(c.nfft[r], c.win[r], t.data()); return t; });
        if (rc != FD_OK) return rc;
        tabs[r] = slot;
    }
    Scratch &s = h->spectral_scratch;
    if ((rc = reserve(h, who, s, fdk::spectral_scratch_bytes(B, L, c), (hipStream_t)stream)) != FD_OK) return rc;
    const long long *lens_dev = nullptr;
    if ((rc = stage_counts(h, valid, B, fdk::spectral_lens_slot(s.p), (hipStream_t)stream, &lens_dev)) != FD_OK) return rc;
    return run(h, stream, who, [&](const fdk::Launch &La) { return fdk::spectral(La, clean, degraded, L, B, L, lens_dev, c, tabs, rec_dev, s.p); });
}

// Griffin-Lim and the mel inversion in front of it (fastdiff_hip_ext.h; lengths, refusals, scratch and counter layout: fd_gl.h, the
// kernels: fd_kernels_gl.hip) ----------------------------------------------------------------------------------------------------------
int64_t fd_gl_samples(int64_t frames) { return fdgl::samples(frames); }

int fd_gl_default_iters(void) { return fdgl::DEFAULT_ITERS; }

int fd_mel_to_linear(fd_handle h, const float *mel, int B, int T, const float *pinv_513x80, int variant, float *amp_out, void *stream)
{
    // (the arguments first, as fd_spectral_measure checks them: their refusals need no handle)
    const char *who = "fd_mel_to_linear";
    if (!mel || !pinv_513x80 || !amp_out) FD_FAIL(h, FD_ERR_INVALID, "%s: null %s", who, !mel ? "mel" : (!pinv_513x80 ? "pinv_513x80" : "amp_out"));
    if (B < 1 || B > fdgl::MAX_B || T < 1 || T > fdgl::MAX_T)
        FD_FAIL(h, FD_ERR_INVALID, "%s: B = %d items (1 .. %d) of T = %d frames (1 .. %d)", who, B, fdgl::MAX_B, T, fdgl::MAX_T);
    if (variant != FD_GL_PWG && variant != FD_GL_TACOTRON) FD_FAIL(h, FD_ERR_INVALID, "%s: unknown variant %d (FD_GL_PWG / FD_GL_TACOTRON)", who, variant);
    const size_t np = (size_t)fdgl::BINS * fdgl::MELS;
    const long bad = fdn::first_nonfinite(pinv_513x80, np);
    if (bad >= 0) FD_FAIL(h, FD_ERR_INVALID, "%s: element %zu of pinv_513x80 is not finite", who, (size_t)bad);
    if (!h) FD_FAIL(h, FD_ERR_INVALID, "%s: null handle", who);
    int rc = enter(h);
    if (rc != FD_OK) return rc;
    rc = refresh(h, who, (hipStream_t)stream, "the device copy of this pseudo-inverse", h->gl_pinv[variant], pinv_513x80, np,
                 [&] { return std::vector<float>(pinv_513x80, pinv_513x80 + np); });
    if (rc != FD_OK) return rc;
    const float *P = h->gl_pinv[variant].dev;
    return run(h, stream, who, [&](const fdk::Launch &La) { return fdk::mel_to_linear(La, mel, B, T, P, variant, amp_out); });
}

int fd_griffin_lim(fd_handle h, const float *amp, const float *angles, int B, int T, const int64_t *lens, int n_iters, uint64_t seed,
                   const uint64_t *stream_ids, float *wav_out, int64_t wav_pitch, fd_gl *rec_dev, void *stream)
{
    const char *who = "fd_griffin_lim";
    if (!amp || !wav_out || !rec_dev) FD_FAIL(h, FD_ERR_INVALID, "%s: null %s", who, !amp ? "amp" : (!wav_out ? "wav_out" : "rec_dev"));
    char why[fdgl::MSG];
    if (fdgl::refusal(B, T, n_iters, wav_pitch, why)) FD_FAIL(h, FD_ERR_INVALID, "%s: %s", who, why);
    int rc = check_counts(h, who, "lens", lens, B, 0, T);
    if (rc != FD_OK) return rc;
    if (!h) FD_FAIL(h, FD_ERR_INVALID, "%s: null handle", who);
    if ((rc = enter(h)) != FD_OK || (rc = mel_tables_first_use(h, who, (hipStream_t)stream)) != FD_OK) return rc;
    const float *tab = h->mel[0].tab;
    Scratch &s = h->gl_scratch;
    if ((rc = reserve(h, who, s, fdk::gl_scratch_bytes(B, T), (hipStream_t)stream)) != FD_OK) return rc;
    const fdk::GlSlots sl = fdk::gl_slots(s.p, B, T);
    const long long *lens_dev = nullptr, *ids_dev = nullptr;
    if ((rc = stage_counts(h, lens, B, sl.lens, (hipStream_t)stream, &lens_dev)) != FD_OK) return rc;
    static_assert(sizeof(uint64_t) == sizeof(int64_t), "the ids travel as the counts do");
    if ((rc = stage_counts(h, reinterpret_cast<const int64_t *>(stream_ids), B, reinterpret_cast<long long *>(sl.ids), (hipStream_t)stream, &ids_dev)) != FD_OK) return rc;
    return run(h, stream, who, [&](const fdk::Launch &La) {
        return fdk::griffin_lim(La, amp, angles, B, T, lens_dev, reinterpret_cast<const unsigned long long *>(ids_dev), n_iters, (unsigned long long)seed, tab,
                                wav_out, wav_pitch, rec_dev, s.p);
    });
}

// The non-negative mel inversion (fastdiff_hip_ext.h; refusals, L, the momentum table, the bank's images and the scratch layout:
// fd_nnls.h, the kernels: fd_kernels_nnls.hip)
int fd_nnls_default_iters(void) { return fdn::DEFAULT_ITERS; }

int fd_nnls_step_bound(const float *bank_80x513, double *L_out)
{
    const fd_handle h = nullptr;
    const char *who = "fd_nnls_step_bound";
    if (!bank_80x513 || !L_out) FD_FAIL(h, FD_ERR_INVALID, "%s: null %s", who, !bank_80x513 ? "bank_80x513" : "L_out");
    const long bad = fdn::first_nonfinite(bank_80x513, (size_t)fdn::MELS * fdn::BINS);
    if (bad >= 0) FD_FAIL(h, FD_ERR_INVALID, "%s: element %ld of bank_80x513 is not finite", who, bad);
    *L_out = fdn::step_bound(bank_80x513);
    return FD_OK;
}

int fd_mel_to_linear_nnls(fd_handle h, const float *mel, int B, int T, const int64_t *lens, const float *bank_80x513, const float *pinv_513x80,
                          int variant, int n_iters, float *amp_out, fd_nnls *rec_dev, void *stream)
{
    const char *who = "fd_mel_to_linear_nnls";
    if (!mel || !bank_80x513 || !pinv_513x80 || !amp_out)
        FD_FAIL(h, FD_ERR_INVALID, "%s: null %s", who, !mel ? "mel" : (!bank_80x513 ? "bank_80x513" : (!pinv_513x80 ? "pinv_513x80" : "amp_out")));
    char why[fdn::MSG];
    if (fdn::refusal(B, T, n_iters, variant, why)) FD_FAIL(h, FD_ERR_INVALID, "%s: %s", who, why);
    const size_t np = (size_t)fdn::BINS * fdn::MELS;
    long bad = fdn::first_nonfinite(bank_80x513, np);
    if (bad >= 0) FD_FAIL(h, FD_ERR_INVALID, "%s: element %ld of bank_80x513 is not finite", who, bad);
    if ((bad = fdn::first_nonfinite(pinv_513x80, np)) >= 0) FD_FAIL(h, FD_ERR_INVALID, "%s: element %ld of pinv_513x80 is not finite", who, bad);
    int rc = check_counts(h, who, "lens", lens, B, 0, T);
    if (rc != FD_OK) return rc;
    if (!h) FD_FAIL(h, FD_ERR_INVALID, "%s: null handle", who);
    if ((rc = enter(h)) != FD_OK) return rc;
    fd_context::NnlsBank &nb = h->nnls_bank[variant];
    const float *const tab_before = nb.bank.dev;      // (inside a capture the first table that is new refuses: neither is uploaded there)
    rc = refresh(h, who, (hipStream_t)stream, "the device table of this bank", nb.bank, bank_80x513, np,
                 [&] { std::vector<float> t(fdn::table().total); fdn::fill_table(bank_80x513, t.data()); return t; });
    if (rc != FD_OK) return rc;
    if (nb.bank.dev != tab_before) nb.L = fdn::step_bound(bank_80x513);
    rc = refresh(h, who, (hipStream_t)stream, "the device copy of this pseudo-inverse", nb.pinv, pinv_513x80, np,
                 [&] { return std::vector<float>(pinv_513x80, pinv_513x80 + np); });
    if (rc != FD_OK) return rc;
    Scratch &s = h->nnls_scratch;
    if ((rc = reserve(h, who, s, fdk::nnls_scratch_bytes(B, T), (hipStream_t)stream)) != FD_OK) return rc;
    const long long *lens_dev = nullptr;
    if ((rc = stage_counts(h, lens, B, fdk::nnls_lens_slot(s.p), (hipStream_t)stream, &lens_dev)) != FD_OK) return rc;
    const float step = fdn::step(nb.L);
    const float *tab = nb.bank.dev, *P = nb.pinv.dev;
    return run(h, stream, who, [&](const fdk::Launch &La) {
        return fdk::mel_to_linear_nnls(La, mel, B, T, lens_dev, P, tab, step, variant, n_iters, amp_out, rec_dev, s.p);
    });
}

// The k-means bin pass (fastdiff_hip_ext.h; refusals, LDS and scratch layout: fd_bins.h, the kernels: fd_kernels_bins.hip)
int fd_bins_chunk(void) { return fdb::CHUNK; }

int fd_bins_record_bytes(void) { return (int)sizeof(fd_bins); }

int fd_bins_pass(fd_handle h, const float *x, int64_t N, int D, int64_t ld, const float *shift, const float *scale, const float *centroids, int K,
                 int32_t *assign_io, float *centroids_out, fd_bins *rec_dev, void *stream)
{
    const char *who = "fd_bins_pass";
    if (!x || !centroids) FD_FAIL(h, FD_ERR_INVALID, "%s: null %s", who, !x ? "x" : "centroids");
    if (!assign_io && !centroids_out && !rec_dev) FD_FAIL(h, FD_ERR_INVALID, "%s: assign_io, centroids_out and rec_dev are all null: nothing to write", who);
    char why[fdb::MSG];
    if (fdb::refusal(x, N, D, ld, shift != nullptr, scale != nullptr, K, centroids, centroids_out, why)) FD_FAIL(h, FD_ERR_INVALID, "%s: %s", who, why);
    if (!h) FD_FAIL(h, FD_ERR_INVALID, "%s: null handle", who);
    int rc;
    if ((rc = enter(h)) != FD_OK) return rc;
    Scratch &s = h->bins_scratch;
    if ((rc = reserve(h, who, s, fdk::bins_scratch_bytes(N, K, D, centroids_out != nullptr), (hipStream_t)stream)) != FD_OK) return rc;
    return run(h, stream, who, [&](const fdk::Launch &La) {
        return fdk::bins_pass(La, x, N, D, ld, shift, scale, centroids, K, assign_io, centroids_out, rec_dev, s.p);
    });
}

// Mel-cepstral distortion with time alignment (fastdiff_hip_ext.h; constants, refusals, the DCT table and the sweep's index ranges:
// fd_mcd.h, the kernels: fd_kernels_mcd.hip) -----------------------------------------------------------------------------------------
int fd_mcd_default_config(fd_mcd_config *cfg)
{
    if (!cfg) return FD_ERR_INVALID;
    fdm::defaults(cfg);
    return FD_OK;
}

int64_t fd_mcd_frames(int64_t n)
{
    if (n < 0) return FD_ERR_INVALID;
    return fdm::frames(n);
}

// the front-end's tables and the DCT table
static int mcd_tables(fd_handle h, const char *who, hipStream_t stream)
{
    const int rc = mel_tables_first_use(h, who, stream);
    return rc != FD_OK ? rc : first_use(h, who, stream, "the DCT table", h->mcd_dct,
                                        [] { std::vector<float> t((size_t)fdm::MAX_COEF * fdm::MELS); fdm::dct_table(t.data()); return t; });
}

int fd_cepstra(fd_handle h, const float *wav, int B, int64_t L, const int64_t *valid, int n_coef, float *cep_out, int64_t T_pitch, void *stream)
{
    const char *who = "fd_cepstra";
    if (!wav || !cep_out) FD_FAIL(h, FD_ERR_INVALID, "%s: null %s", who, !wav ? "wav" : "cep_out");
    char why[fdm::MSG];
    if (fdm::coef_refusal(n_coef, why) || fdm::wave_refusal(B, L, "L", why)) FD_FAIL(h, FD_ERR_INVALID, "%s: %s", who, why);
    if (T_pitch < fdm::frames(L) || T_pitch > fdm::MAX_FRAMES)
        FD_FAIL(h, FD_ERR_INVALID, "%s: T_pitch = %lld outside the %lld frames of L = %lld .. %lld", who, (long long)T_pitch, (long long)fdm::frames(L), (long long)L,
                (long long)fdm::MAX_FRAMES);
    int rc = check_counts(h, who, "valid", valid, B, 1, L);
    if (rc != FD_OK) return rc;
    if (!h) FD_FAIL(h, FD_ERR_INVALID, "%s: null handle", who);
    if ((rc = enter(h)) != FD_OK || (rc = mcd_tables(h, who, (hipStream_t)stream)) != FD_OK) return rc;
    Scratch &s = h->mcd_scratch;
    if ((rc = reserve(h, who, s, fdk::mcd_scratch_bytes(1, 0, 0, 0, 0), (hipStream_t)stream)) != FD_OK) return rc;
    const long long *lens_dev = nullptr;
    if ((rc = stage_counts(h, valid, B, fdk::mcd_count_slot(s.p, 0), (hipStream_t)stream, &lens_dev)) != FD_OK) return rc;
    return run(h, stream, who, [&](const fdk::Launch &La) { return fdk::cepstra(La, wav, B, L, lens_dev, n_coef, h->mcd_dct, cep_out, T_pitch); });
}

int fd_dtw(fd_handle h, const float *a, const float *b, int B, int D, int64_t ld, int64_t pitch_a, int64_t pitch_b, const int64_t *frames_a,
           const int64_t *frames_b, fd_dtw_rec *rec_dev, int32_t *align_out, int64_t align_pitch, void *stream)
{
    const char *who = "fd_dtw";
    if (!a || !b || !rec_dev) FD_FAIL(h, FD_ERR_INVALID, "%s: null %s", who, !a ? "a" : (!b ? "b" : "rec_dev"));
    char why[fdm::MSG];
    if (fdm::dtw_refusal(B, D, ld, pitch_a, pitch_b, align_out != nullptr, align_pitch, why)) FD_FAIL(h, FD_ERR_INVALID, "%s: %s", who, why);
    if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 3) FD_FAIL(h, FD_ERR_INVALID, "%s: a and b must be 4-byte aligned", who);
    int rc = check_counts(h, who, "frames_a", frames_a, B, 1, pitch_a);
    if (rc != FD_OK || (rc = check_counts(h, who, "frames_b", frames_b, B, 1, pitch_b)) != FD_OK) return rc;
    int64_t code_stride = 0;
    if (align_out)
        for (int i = 0; i < B; ++i) {
            const int64_t Ta = frames_a ? frames_a[i] : pitch_a, Tb = frames_b ? frames_b[i] : pitch_b;
            if (fdm::align_refusal(i, Ta, Tb, why)) FD_FAIL(h, FD_ERR_INVALID, "%s: %s", who, why);
            code_stride = std::max(code_stride, fdm::code_bytes(Ta, Tb));
        }
    if (!h) FD_FAIL(h, FD_ERR_INVALID, "%s: null handle", who);
    FD_HIP(h, hipSetDevice(h->device));      // no settle: the features are the caller's, and the alignment touches no sampler state
    Scratch &s = h->mcd_scratch;
    if ((rc = reserve(h, who, s, fdk::mcd_scratch_bytes(B, pitch_b, code_stride, 0, 0), (hipStream_t)stream)) != FD_OK) return rc;
    const long long *fa_dev = nullptr, *fb_dev = nullptr;
    if ((rc = stage_counts(h, frames_a, B, fdk::mcd_count_slot(s.p, 2), (hipStream_t)stream, &fa_dev)) != FD_OK) return rc;
    if ((rc = stage_counts(h, frames_b, B, fdk::mcd_count_slot(s.p, 3), (hipStream_t)stream, &fb_dev)) != FD_OK) return rc;
    return run(h, stream, who, [&](const fdk::Launch &La) {
        return fdk::dtw(La, a, b, B, D, ld, pitch_a, pitch_b, fa_dev, fb_dev, rec_dev, align_out, align_pitch, code_stride, s.p);
    });
}

int fd_mcd_measure(fd_handle h, const float *clean, int64_t Lc, const float *degraded, int64_t Ld, int B, const int64_t *valid_clean,
                   const int64_t *valid_degraded, const fd_mcd_config *cfg, fd_mcd *rec_dev, void *stream)
{
    const char *who = "fd_mcd_measure";
    if (!clean || !degraded || !rec_dev) FD_FAIL(h, FD_ERR_INVALID, "%s: null %s", who, !clean ? "clean" : (!degraded ? "degraded" : "rec_dev"));
    fd_mcd_config c;
    if (cfg) c = *cfg; else fdm::defaults(&c);
    char why[fdm::MSG];
    if (fdm::refusal(c, why)) FD_FAIL(h, FD_ERR_INVALID, "%s: configuration refused: %s", who, why);
    if (fdm::wave_refusal(B, Lc, "Lc", why) || fdm::wave_refusal(B, Ld, "Ld", why)) FD_FAIL(h, FD_ERR_INVALID, "%s: %s", who, why);
    int rc = check_counts(h, who, "valid_clean", valid_clean, B, 1, Lc);
    if (rc != FD_OK || (rc = check_counts(h, who, "valid_degraded", valid_degraded, B, 1, Ld)) != FD_OK) return rc;
    if (!h) FD_FAIL(h, FD_ERR_INVALID, "%s: null handle", who);
    if ((rc = enter(h)) != FD_OK || (rc = mcd_tables(h, who, (hipStream_t)stream)) != FD_OK) return rc;
    const int D = c.n_coef;
    const int64_t Tc = fdm::frames(Lc), Td = fdm::frames(Ld), fl_a = (int64_t)B * Tc * D, fl_b = (int64_t)B * Td * D;
    Scratch &s = h->mcd_scratch;
    if ((rc = reserve(h, who, s, fdk::mcd_scratch_bytes(B, Td, 0, fl_a, fl_b), (hipStream_t)stream)) != FD_OK) return rc;
    std::vector<int64_t> fa, fb;      // each pair's own frames
    if (valid_clean) { fa.resize(B); for (int b = 0; b < B; ++b) fa[b] = fdm::frames(valid_clean[b]); }
    if (valid_degraded) { fb.resize(B); for (int b = 0; b < B; ++b) fb[b] = fdm::frames(valid_degraded[b]); }
    const int64_t *const counts[4] = {valid_clean, valid_degraded, valid_clean ? fa.data() : nullptr, valid_degraded ? fb.data() : nullptr};
    const long long *dev[4];
    for (int q = 0; q < 4; ++q)
        if ((rc = stage_counts(h, counts[q], B, fdk::mcd_count_slot(s.p, q), (hipStream_t)stream, &dev[q])) != FD_OK) return rc;
    const long long *na = dev[0], *nb = dev[1], *fa_dev = dev[2], *fb_dev = dev[3];
    float *ca = fdk::mcd_cep_slot(s.p, B, Td, 0, fl_a, fl_b, 0), *cb = fdk::mcd_cep_slot(s.p, B, Td, 0, fl_a, fl_b, 1);
    fd_dtw_rec *wrec = fdk::mcd_rec_slot(s.p, B, Td, 0);
    return run(h, stream, who, [&](const fdk::Launch &La) {
        hipError_t e = fdk::cepstra(La, clean, B, Lc, na, D, h->mcd_dct, ca, Tc);
        if (e != hipSuccess || (e = fdk::cepstra(La, degraded, B, Ld, nb, D, h->mcd_dct, cb, Td)) != hipSuccess) return e;
        if ((e = fdk::dtw(La, ca, cb, B, D, D, Tc, Td, fa_dev, fb_dev, wrec, nullptr, 0, 0, s.p)) != hipSuccess) return e;
        return fdk::mcd_finish(La, ca, cb, B, D, Tc, Td, fa_dev, fb_dev, na, Lc, nb, Ld, wrec, rec_dev);
    });
}

// Cutting long silences (fastdiff_hip_ext.h; limits, refusals, the window grid and the host statement of the mask: fd_trim.h, the
// kernels: fd_kernels_trim.hip) ----------------------------------------------------------------------------------------------------------
int fd_trim_default_params(int sample_rate, fd_trim_params *p)
{
    if (!p) return FD_ERR_INVALID;
    p->sample_rate = sample_rate; p->window_ms = 30; p->average_width = 8; p->max_silence = 12; p->mode = FD_TRIM_LONG; p->reserved = 0;
    p->top_db = 40.0; p->floor_db = -70.0;
    return FD_OK;
}

int fd_trim_windows(int64_t n, int sample_rate, int window_ms, int64_t *W, int64_t *M)
{
    return fdtr::windows(n, sample_rate, window_ms, W, M) ? FD_OK : FD_ERR_INVALID;
}

int fd_trim_mask(const uint8_t *speech, int64_t M, int average_width, int max_silence, int mode, uint8_t *flags_out)
{
    char why[fdtr::MSG];
    if (!speech || !flags_out || M < 1 || fdtr::refusal(fdl::RATE_MIN, 30, 1.0, 0.0, average_width, max_silence, mode, 0, why)) return FD_ERR_INVALID;
    fdtr::mask(speech, M, average_width, max_silence, mode, flags_out);
    return FD_OK;
}

// what the two device entry points check and prepare alike: the batch, the window grid, the counts on the device
static int trim_enter(fd_handle h, const char *who, const float *wav, int B, int64_t L, const int64_t *valid, int rate, int window_ms, void *stream,
                      int64_t *W, int64_t *Mp, int64_t *M_grid, const long long **valid_dev)
{
    if (!h) return FD_ERR_INVALID;
    if (!wav) FD_FAIL(h, FD_ERR_INVALID, "%s: null wav", who);
    if (reinterpret_cast<uintptr_t>(wav) & 3) FD_FAIL(h, FD_ERR_INVALID, "%s: wav must be 4-byte aligned", who);
    if (B < 1 || B > 4096 || L < 1 || L > fdtr::MAX_SAMPLES)
        FD_FAIL(h, FD_ERR_INVALID, "%s: B = %d utterances (1 .. 4096) of L = %lld samples (1 .. 2^31 - 1)", who, B, (long long)L);
    if (!fdtr::windows(L, rate, window_ms, W, Mp))
        FD_FAIL(h, FD_ERR_INVALID, "%s: sample rate %d outside %d .. %d, or window_ms = %d not 10, 20 or 30", who, rate, fdl::RATE_MIN, fdl::RATE_MAX, window_ms);
    int rc = check_counts(h, who, "valid", valid, B, 0, L);
    if (rc != FD_OK || (rc = enter(h)) != FD_OK) return rc;
    int64_t longest = valid ? 0 : L;
    for (int b = 0; valid && b < B; ++b) longest = std::max(longest, valid[b]);
    fdtr::windows(longest, rate, window_ms, nullptr, M_grid);
    Scratch &s = h->trim_scratch;
    if ((rc = reserve(h, who, s, fdk::trim_scratch_bytes(B, *Mp), (hipStream_t)stream)) != FD_OK) return rc;
    return stage_counts(h, valid, B, fdk::trim_valid_slot(s.p), (hipStream_t)stream, valid_dev);
}

int fd_trim_levels(fd_handle h, const float *wav, int B, int64_t L, const int64_t *valid, int sample_rate, int window_ms, double *levels_out,
                   void *stream)
{
    const char *who = "fd_trim_levels";
    if (h && !levels_out) FD_FAIL(h, FD_ERR_INVALID, "%s: null levels_out", who);
    int64_t W = 0, Mp = 0, M_grid = 0;
    const long long *valid_dev = nullptr;
    const int rc = trim_enter(h, who, wav, B, L, valid, sample_rate, window_ms, stream, &W, &Mp, &M_grid, &valid_dev);
    if (rc != FD_OK) return rc;
    return run(h, stream, who, [&](const fdk::Launch &La) { return fdk::trim_levels(La, wav, B, L, valid_dev, W, Mp, levels_out, Mp, true); });
}

int fd_trim_silences(fd_handle h, const float *wav, int B, int64_t L, const int64_t *valid, const fd_trim_params *params, float *out,
                     int32_t *out_valid, uint8_t *flags, fd_trim *rec_dev, void *stream)
{
    const char *who = "fd_trim_silences";
    if (!h) return FD_ERR_INVALID;
    if (!params || !out || !out_valid) FD_FAIL(h, FD_ERR_INVALID, "%s: null %s", who, !params ? "params" : (!out ? "out" : "out_valid"));
    const fd_trim_params p = *params;
    char why[fdtr::MSG];
    if (fdtr::refusal(p.sample_rate, p.window_ms, p.top_db, p.floor_db, p.average_width, p.max_silence, p.mode, p.reserved, why))
        FD_FAIL(h, FD_ERR_INVALID, "%s: parameters refused: %s", who, why);
    if (reinterpret_cast<uintptr_t>(out) & 3) FD_FAIL(h, FD_ERR_INVALID, "%s: out must be 4-byte aligned", who);
    if (wav && B >= 1 && L >= 1) {
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(wav), b0 = reinterpret_cast<uintptr_t>(out), bytes = sizeof(float) * (uintptr_t)B * (uintptr_t)L;
        if (a0 < b0 + bytes && b0 < a0 + bytes) FD_FAIL(h, FD_ERR_INVALID, "%s: out overlaps wav (the compaction is not done in place)", who);
    }
    int64_t W = 0, Mp = 0, M_grid = 0;
    const long long *valid_dev = nullptr;
    const int rc = trim_enter(h, who, wav, B, L, valid, p.sample_rate, p.window_ms, stream, &W, &Mp, &M_grid, &valid_dev);
    if (rc != FD_OK) return rc;
    return run(h, stream, who, [&](const fdk::Launch &La) {
        return fdk::trim(La, wav, B, L, valid_dev, p, W, Mp, M_grid, out, out_valid, flags, rec_dev, h->trim_scratch.p);
    });
}

// Parallel WaveGAN (fastdiff_hip_ext.h; the configuration's refusals, the tensors, the images and the scratch layout: fd_pwg.h, the
// kernels: fd_kernels_pwg.hip)
void fd_pwg_default_config(fd_pwg_config *cfg)
{
    if (cfg) fdpwg::default_config(cfg);
}

int64_t fd_pwg_samples(const fd_pwg_config *cfg, int64_t frames) { return cfg ? fdpwg::samples(*cfg, frames) : -1; }

int64_t fd_pwg_receptive_field(const fd_pwg_config *cfg) { return cfg ? fdpwg::receptive_field(*cfg) : -1; }

int fd_pwg_create(fd_handle h, const fd_pwg_config *cfg, fd_pwg_handle *out)
{
    const char *who = "fd_pwg_create";
    if (!cfg || !out) FD_FAIL(h, FD_ERR_INVALID, "%s: null %s", who, !cfg ? "cfg" : "out");
    char why[fdpwg::MSG];
    if (fdpwg::refusal(*cfg, why)) FD_FAIL(h, FD_ERR_UNSUPPORTED, "%s: %s", who, why);
    if (!h) FD_FAIL(h, FD_ERR_INVALID, "%s: null handle", who);
    fd_pwg *p = new fd_pwg();
    p->owner = h;
    p->cfg = *cfg;
    p->tensors = fdpwg::tensors(*cfg);
    p->scaler.assign(2 * fdpwg::AUX, 0.0f);
    std::fill(p->scaler.begin() + fdpwg::AUX, p->scaler.end(), 1.0f);
    *out = p;
    return FD_OK;
}

int fd_pwg_set_weight(fd_pwg_handle p, const char *name, const float *data, int64_t n)
{
    const char *who = "fd_pwg_set_weight";
    const fd_handle h = p ? p->owner : nullptr;
    if (!p || !name || !data) FD_FAIL(h, FD_ERR_INVALID, "%s: null %s", who, !p ? "generator" : (!name ? "name" : "data"));
    for (const fdpwg::Tensor &t : p->tensors) {
        if (t.name != name) continue;
        if (n != (int64_t)t.n) FD_FAIL(h, FD_ERR_INVALID, "%s: %s has %zu elements, got %lld", who, name, t.n, (long long)n);
        for (int64_t i = 0; i < n; ++i)
            if (!std::isfinite(data[i])) FD_FAIL(h, FD_ERR_INVALID, "%s: element %lld of %s is not finite", who, (long long)i, name);
        p->w[t.name].assign(data, data + n);
        p->committed = false;
        return FD_OK;
    }
    FD_FAIL(h, FD_ERR_MISSING, "%s: no tensor %s in this configuration", who, name);
}

int fd_pwg_commit(fd_pwg_handle p)
{
    const char *who = "fd_pwg_commit";
    const fd_handle h = p ? p->owner : nullptr;
    if (!p) FD_FAIL(h, FD_ERR_INVALID, "%s: null generator", who);
    for (const fdpwg::Tensor &t : p->tensors)
        if (!p->w.count(t.name)) FD_FAIL(h, FD_ERR_MISSING, "%s: %s was never set", who, t.name.c_str());
    const fd_pwg_config &c = p->cfg;
    const fdpwg::Image im = fdpwg::image(c);
    std::vector<float> img(im.total, 0.0f);
    auto W = [&](const std::string &n) -> const float * { return p->w[n].data(); };
    const int K = 2 * c.aux_context_window + 1, A = fdpwg::AUX, G = fdpwg::GATE, R = fdpwg::RES;
    const float *cin = W("upsample_net.conv_in.weight");            // [80 j][80 m][K]
    for (int l = 0; l < c.layers; ++l) {
        const std::string pre = "conv_layers." + std::to_string(l) + ".";
        const float *aux = W(pre + "conv1x1_aux.weight");           // [128][80]
        float *front = img.data() + im.front + (size_t)l * G * A * K;
        for (int g = 0; g < G; ++g)
            for (int mk = 0; mk < A * K; ++mk) {
                double sum = 0.0;
                for (int j = 0; j < A; ++j) sum += (double)aux[g * A + j] * (double)cin[(size_t)j * A * K + mk];
                front[(size_t)g * A * K + mk] = (float)sum;
            }
        float *Ll = img.data() + im.layer + fdpwg::LAYER_FLOATS * l;
        fdpwg::pack_a(Ll + fdpwg::L_CONV, W(pre + "conv.weight"), G, 3 * R, 3 * R, [&](int k) { return (k % R) * 3 + k / R; });      // k = tap 64 + channel
        std::copy_n(W(pre + "conv.bias"), G, Ll + fdpwg::L_BIAS);
        std::vector<float> mix((size_t)G * fdpwg::HALF);
        std::copy_n(W(pre + "conv1x1_out.weight"), (size_t)R * fdpwg::HALF, mix.begin());
        std::copy_n(W(pre + "conv1x1_skip.weight"), (size_t)fdpwg::SKIP * fdpwg::HALF, mix.begin() + (size_t)R * fdpwg::HALF);
        fdpwg::pack_a(Ll + fdpwg::L_MIX, mix.data(), G, fdpwg::HALF, fdpwg::HALF, [](int k) { return k; });
        std::copy_n(W(pre + "conv1x1_out.bias"), R, Ll + fdpwg::L_MIXB);
        std::copy_n(W(pre + "conv1x1_skip.bias"), fdpwg::SKIP, Ll + fdpwg::L_MIXB + R);
    }
    std::copy_n(W("first_conv.weight"), R, img.data() + im.first_w);
    std::copy_n(W("first_conv.bias"), R, img.data() + im.first_b);
    fdpwg::pack_a(img.data() + im.tail_w1, W("last_conv_layers.1.weight"), fdpwg::SKIP, fdpwg::SKIP, fdpwg::SKIP, [](int k) { return k; });
    std::copy_n(W("last_conv_layers.1.bias"), fdpwg::SKIP, img.data() + im.tail_b1);
    std::copy_n(W("last_conv_layers.3.weight"), fdpwg::SKIP, img.data() + im.tail_w2);
    img[im.tail_b2] = W("last_conv_layers.3.bias")[0];
    for (int i = 0; i < c.n_scales; ++i)
        fdpwg::phase_sums(W("upsample_net.upsample.up_layers." + std::to_string(2 * i + 1) + ".weight"), c.upsample_scales[i],
                          img.data() + im.phase + (size_t)i * fdpwg::MAX_SCALE * 3);
    std::copy(p->scaler.begin(), p->scaler.end(), img.begin() + im.scaler);
    FD_HIP(h, hipSetDevice(h->device));
    if (!p->img) {
        void *d = nullptr;
        FD_HIP(h, hipMalloc(&d, sizeof(float) * im.total));
        p->img = static_cast<float *>(d);
    } else {
        FD_HIP(h, hipDeviceSynchronize());      // launches in flight may still read the old values
    }
    FD_HIP(h, hipMemcpy(p->img, img.data(), sizeof(float) * im.total, hipMemcpyHostToDevice));
    p->committed = true;
    return FD_OK;
}

int fd_pwg_set_scaler(fd_pwg_handle p, const float *mean, const float *scale)
{
    const char *who = "fd_pwg_set_scaler";
    const fd_handle h = p ? p->owner : nullptr;
    if (!p) FD_FAIL(h, FD_ERR_INVALID, "%s: null generator", who);
    if (!mean != !scale) FD_FAIL(h, FD_ERR_INVALID, "%s: null %s (both or neither)", who, !mean ? "mean" : "scale");
    for (int m = 0; mean && m < fdpwg::AUX; ++m)
        if (!std::isfinite(mean[m]) || !std::isfinite(scale[m]) || scale[m] == 0.0f)
            FD_FAIL(h, FD_ERR_INVALID, "%s: channel %d: mean %g, scale %g", who, m, (double)mean[m], (double)scale[m]);
    for (int m = 0; m < fdpwg::AUX; ++m) {
        p->scaler[m] = mean ? mean[m] : 0.0f;
        p->scaler[fdpwg::AUX + m] = mean ? scale[m] : 1.0f;
    }
    p->has_scaler = mean != nullptr;
    if (p->img) {
        FD_HIP(h, hipSetDevice(h->device));
        FD_HIP(h, hipDeviceSynchronize());
        FD_HIP(h, hipMemcpy(p->img + fdpwg::image(p->cfg).scaler, p->scaler.data(), sizeof(float) * p->scaler.size(), hipMemcpyHostToDevice));
    }
    return FD_OK;
}

int fd_pwg_generate(fd_pwg_handle p, const float *mel_or_c, int padded, int B, int T, const int64_t *lens, const float *z, uint64_t seed,
                    const uint64_t *stream_ids, float *wav_out, int64_t wav_pitch, void *stream)
{
    const char *who = "fd_pwg_generate";
    const fd_handle h = p ? p->owner : nullptr;
    if (!mel_or_c || !wav_out) FD_FAIL(h, FD_ERR_INVALID, "%s: null %s", who, !mel_or_c ? "mel_or_c" : "wav_out");
    if (padded != 0 && padded != 1) FD_FAIL(h, FD_ERR_INVALID, "%s: padded = %d is neither 0 nor 1", who, padded);
    char why[fdpwg::MSG];
    if (fdpwg::call_refusal(p ? fdpwg::hop(p->cfg) : 1, B, T, p ? wav_pitch : INT64_MAX, why)) FD_FAIL(h, FD_ERR_INVALID, "%s: %s", who, why);
    int rc = check_counts(h, who, "lens", lens, B, 0, T);
    if (rc != FD_OK) return rc;
    if (!p) FD_FAIL(h, FD_ERR_INVALID, "%s: null generator", who);
    if (!p->committed) FD_FAIL(h, FD_ERR_STATE, "%s: fd_pwg_commit has not run since the last fd_pwg_set_weight", who);
    if ((rc = enter(h)) != FD_OK) return rc;
    const fdpwg::Layout o = fdpwg::layout(p->cfg.layers, fdpwg::hop(p->cfg), B, T);
    Scratch &s = h->pwg_scratch;
    if ((rc = reserve(h, who, s, o.total, (hipStream_t)stream)) != FD_OK) return rc;
    char *base = reinterpret_cast<char *>(s.p);
    const long long *lens_dev = nullptr, *ids_dev = nullptr;
    if ((rc = stage_counts(h, lens, B, reinterpret_cast<long long *>(base + o.lens), (hipStream_t)stream, &lens_dev)) != FD_OK) return rc;
    if ((rc = stage_counts(h, reinterpret_cast<const int64_t *>(stream_ids), B, reinterpret_cast<long long *>(base + o.ids), (hipStream_t)stream, &ids_dev)) != FD_OK)
        return rc;
    const fdk::PwgNet net{p->img, p->cfg, p->has_scaler};
    return run(h, stream, who, [&](const fdk::Launch &La) {
        return fdk::pwg_generate(La, net, mel_or_c, padded, B, T, lens_dev, reinterpret_cast<const unsigned long long *>(ids_dev), z, (unsigned long long)seed,
                                 wav_out, wav_pitch, s.p);
    });
}

int fd_pwg_draw(fd_handle h, int B, int64_t L, uint64_t seed, const uint64_t *stream_ids, float *z_out, int64_t z_pitch, void *stream)
{
    const char *who = "fd_pwg_draw";
    if (!z_out) FD_FAIL(h, FD_ERR_INVALID, "%s: null z_out", who);
    if (B < 1 || B > fdpwg::MAX_B || L < 1 || L > INT32_MAX || z_pitch < L)
        FD_FAIL(h, FD_ERR_INVALID, "%s: B = %d items (1 .. %d) of L = %lld samples (1 .. 2^31 - 1) at a pitch of %lld", who, B, fdpwg::MAX_B, (long long)L, (long long)z_pitch);
    if (!h) FD_FAIL(h, FD_ERR_INVALID, "%s: null handle", who);
    int rc = enter(h);
    if (rc != FD_OK) return rc;
    const fdpwg::Layout o = fdpwg::layout(1, 1, B, 1);      // (the slots of the counts depend on B alone)
    Scratch &s = h->pwg_scratch;
    if ((rc = reserve(h, who, s, o.G, (hipStream_t)stream)) != FD_OK) return rc;
    const long long *ids_dev = nullptr;
    if ((rc = stage_counts(h, reinterpret_cast<const int64_t *>(stream_ids), B, reinterpret_cast<long long *>(reinterpret_cast<char *>(s.p) + o.ids), (hipStream_t)stream, &ids_dev)) != FD_OK)
        return rc;
    return run(h, stream, who, [&](const fdk::Launch &La) {
        return fdk::pwg_draw(La, B, L, (unsigned long long)seed, reinterpret_cast<const unsigned long long *>(ids_dev), z_out, z_pitch);
    });
}

int fd_pwg_destroy(fd_pwg_handle p)
{
    if (!p) return FD_OK;
    if (p->img) {
        (void)hipSetDevice(p->owner->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(p->img);
    }
    delete p;
    return FD_OK;
}

int64_t fd_read_tap(fd_handle h, const char *name, float *host_dst, int64_t capacity)
{
    if (!h || !name) return FD_ERR_INVALID;
    {
        const int rcs = fd_settle(h);
        if (rcs != FD_OK) return rcs;
    }
    if (h->gen) FD_FAIL(h, FD_ERR_UNSUPPORTED, "fd_read_tap: intermediates are kept by the tuned kernel set only (base.yaml's architecture)");
    const int B = h->last_B, T = h->last_T;
    if (B == 0) FD_FAIL(h, FD_ERR_STATE, "fd_read_tap: no forward has run yet");
    const Workspace &w = h->ws;
    const int64_t L = (int64_t)T * fd::HOPT;
    const std::string k(name);
    const float *src = nullptr;
    int64_t n = 0;
    if (k == "noise") { src = w.noise; n = (int64_t)B * fd::NBLK * fd::COND; }
    else if (k == "a0") { src = w.a[0]; n = B * fd::C * L; }
    else if (k == "a1") { src = w.a[1]; n = B * fd::C * L / 4; }
    else if (k == "a2") { src = w.a[2]; n = B * fd::C * L / 32; }
    else if (k == "a3") { src = w.a[3]; n = (int64_t)B * fd::C * T; }
    else if (k.size() == 6 && k.compare(0, 5, "kpack") == 0 && k[5] >= '0' && k[5] <= '2') {
        n = (int64_t)B * T * fd::KREC; src = w.kpack + (k[5] - '0') * n;
    } else if (k.size() == 5 && k.compare(0, 4, "kp_h") == 0 && k[4] >= '0' && k[4] <= '2') {
        n = (int64_t)B * fd::HID * T; src = w.kp_hB + (k[4] - '0') * n;
    } else if (k.size() == 2 && k[0] == 'x' && k[1] >= '0' && k[1] <= '2') {
        if (!h->mode.keep_taps) FD_FAIL(h, FD_ERR_STATE, "fd_read_tap: set option taps=1 before the forward to keep block outputs");
        const int blk = k[1] - '0';
        src = w.xtap[blk]; n = (int64_t)B * fd::C * T * fd::hop(blk);
    } else if (k == "range_flags") {       // 32 int32 (bit patterns): fp16-range flags of the last step, see Workspace::range_flag
        src = reinterpret_cast<const float *>(w.range_flag); n = fd::flags::WORDS;
    } else if (k == "range_flags_call") {  // the same, OR-ed over every step since the start of the last call (the sticky words)
        src = reinterpret_cast<const float *>(w.range_flag + fd::flags::STICKY); n = fd::flags::WORDS;
    } else FD_FAIL(h, FD_ERR_INVALID, "fd_read_tap: unknown tap '%s'", name);
    if (!host_dst) return n;
    if (capacity < n) FD_FAIL(h, FD_ERR_INVALID, "fd_read_tap: capacity %lld < %lld", (long long)capacity, (long long)n);
    FD_HIP(h, hipSetDevice(h->device));
    FD_HIP(h, hipDeviceSynchronize());
    FD_HIP(h, hipMemcpy(host_dst, src, sizeof(float) * n, hipMemcpyDeviceToHost));
    return n;
}

int fd_kernel_index(int layer, int in_ch, int out_ch, int tap)
{
    if (layer < 0 || layer >= fd::LAYERS || in_ch < 0 || in_ch >= fd::C || out_ch < 0 || out_ch >= 2 * fd::C || tap < 0 || tap >= 3)
        return FD_ERR_INVALID;
    return fd::kernel_index(layer, in_ch, out_ch, tap);
}

int fd_bias_index(int layer, int out_ch)
{
    if (layer < 0 || layer >= fd::LAYERS || out_ch < 0 || out_ch >= 2 * fd::C) return FD_ERR_INVALID;
    return fd::bias_index(layer, out_ch);
}

int64_t fd_get_counter(fd_handle h, const char *name)
{
    if (!h || !name) return FD_ERR_INVALID;
    const std::string k(name);
    if (k == "pieces_redone" || k == "fp32_mask") {      // the last piece of a long call may still be waiting for its check
        const int rcs = fd_settle(h);
        if (rcs != FD_OK) return rcs;
    }
    if (k == "pieces") return h->n_pieces;
    if (k == "pieces_redone") return h->n_pieces_redone;
    if (k == "pieces_fp32") return h->n_pieces_fp32;
    if (k == "fp32_mask") return (int64_t)h->call_fp32_mask;
    if (k == "calls_redone") return h->n_calls_redone;
    if (k == "graph_captures") return h->n_graph_captures;
    if (k == "graph_hits") return h->n_graph_hits;
    if (k == "graph_evictions") return h->n_graph_evictions;
    if (k == "weight_refreshes") return h->n_refreshes;
    if (k == "refresh_graph_drops") return h->n_refresh_graph_drops;
    if (k == "graphs_resident") return (int64_t)h->graphs.size();
    if (k == "graphs_retired") return (int64_t)h->retired.size();
    if (k == "span_batches") return h->n_span_batches;
    if (k == "span_windows") return h->n_span_windows;
    if (k == "workspace_bytes") return (int64_t)(h->ws.bytes + h->span_scratch.bytes);
    FD_FAIL(h, FD_ERR_INVALID, "fd_get_counter: unknown counter '%s'", name);
}

int fd_get_profile(fd_handle h, fd_kernel_stat *stats, int capacity)
{
    if (!h) return FD_ERR_INVALID;
    hipSetDevice(h->device);
    fd_prof_drain(h);
    int i = 0;
    for (const auto &kv : h->prof_acc) {
        if (stats && i < capacity) {
            memset(&stats[i], 0, sizeof(fd_kernel_stat));
            strncpy(stats[i].name, kv.first.c_str(), sizeof(stats[i].name) - 1);
            stats[i].launches = kv.second.first;
            stats[i].total_ms = kv.second.second;
        }
        ++i;
    }
    return i;
}

int fd_reset_profile(fd_handle h)
{
    if (!h) return FD_ERR_INVALID;
    fd_prof_drain(h);
    h->prof_acc.clear();
    return FD_OK;
}

}  // extern "C"
