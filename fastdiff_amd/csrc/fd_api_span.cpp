// fd_api_span.cpp -- host side of fd_sample_span / fd_sample_halo_frames (include/fastdiff_hip_ext.h): x_0 of a frame range of ONE
// utterance of any length, computed window by window.  Each window is a batch item of fd_sample -- the tuned kernels, graphs, hoisted
// predictor and range check unchanged -- computed as if it were an utterance of its own (zero padding at its edges, `lens` for a short
// last window), with its noise drawn at the whole utterance's sample positions (StepParams::offs4).  The network's receptive field is
// finite, so each window's output equals the whole-utterance result, bit for bit, on every frame at least H = N * 16 frames away from a
// window edge that is not an edge of the utterance; those centres are what the scatter keeps.
#include <stdlib.h>

#include <algorithm>

#include "fd_kernels.h"
#include "fd_host.h"

namespace {
// Frames of one reverse step's reach: perturbing one input sample moves outputs within [-3574, +4071] samples, one mel frame within
// +-3889 (tests/test_long_form.py measures it again on the float64 port).  16 * 256 = 4096 covers both.
constexpr int HALO_PER_STEP = 16;
// Window starts are multiples of this many frames counted from the utterance's start: the Winograd GEMM pairs frames (2p, 2p+1) and
// the kernels tile the frame axis from the utterance's start, so a window must keep their phase to compute what the whole call does.
constexpr int ALIGN = 32;
constexpr int64_t BATCH_FRAMES = 16384;      // frames of one window batch (Bw * Wp), so the workspace does not grow with the utterance
constexpr int64_t I32 = (int64_t)1 << 31;

int64_t floor_to(int64_t v, int64_t a) { return v >= 0 ? v / a * a : -((-v + a - 1) / a) * a; }
int64_t ceil_to(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
}  // namespace

extern "C" {

int fd_sample_halo_frames(int N) { return (N < 1 || N > 1024) ? FD_ERR_INVALID : N * HALO_PER_STEP; }

int fd_sample_span(fd_handle h, const float *mel, int64_t mel_first, int64_t mel_frames, int64_t utt_frames, int64_t t0, int64_t t1,
                   const fd_step *table, int N, int ddim, const float *x_T, const float *z, uint64_t seed, uint64_t stream_id,
                   int window_frames, float *out, void *stream_)
{
    if (!h) return FD_ERR_INVALID;
    if (h->gen)
        FD_FAIL(h, FD_ERR_UNSUPPORTED, "fd_sample_span: windowed synthesis needs base.yaml's architecture (its halo is the receptive field "
                                       "of that network); this handle runs another configuration");
    int rc = fd_settle(h);
    if (rc != FD_OK) return rc;
    if (!h->committed) FD_FAIL(h, FD_ERR_STATE, "fd_sample_span: weights not committed (call fd_commit_weights after fd_set_weight)");
    FD_HIP(h, hipSetDevice(h->device));
    if ((rc = fd_settle_refresh(h)) != FD_OK) return rc;
    for (int i = 0; i < ST_COUNT; ++i)
        if (!h->mode.fast[i])
            FD_FAIL(h, FD_ERR_UNSUPPORTED, "fd_sample_span: needs the fast kernel set; the naive kernels (option kernels.<stage> = naive) "
                                           "ignore `lens`, which the last window of an utterance goes through");
    if (!mel || !table || !out) FD_FAIL(h, FD_ERR_INVALID, "fd_sample_span: null pointer");
    const int H = fd_sample_halo_frames(N);
    if (H < 0) FD_FAIL(h, FD_ERR_INVALID, "fd_sample_span: N=%d outside 1..1024", N);
    if (utt_frames < -1 || utt_frames == 0) FD_FAIL(h, FD_ERR_INVALID, "fd_sample_span: utt_frames=%lld (frames, or -1 = not known yet)", (long long)utt_frames);
    if (t0 < 0 || t0 % 32 != 0 || t1 <= t0)
        FD_FAIL(h, FD_ERR_INVALID, "fd_sample_span: [t0=%lld, t1=%lld) must be non-empty with t0 a multiple of 32", (long long)t0, (long long)t1);
    if (utt_frames >= 0 && t1 > utt_frames)
        FD_FAIL(h, FD_ERR_INVALID, "fd_sample_span: t1=%lld past the utterance's %lld frames", (long long)t1, (long long)utt_frames);
    if (t1 % 32 != 0 && t1 != utt_frames)
        FD_FAIL(h, FD_ERR_INVALID, "fd_sample_span: t1=%lld must be a multiple of 32 or the utterance's end", (long long)t1);
    if (mel_first < 0 || mel_frames < 1 || (utt_frames >= 0 && mel_first + mel_frames > utt_frames))
        FD_FAIL(h, FD_ERR_INVALID, "fd_sample_span: mel frames [%lld, %lld) outside the utterance", (long long)mel_first,
                (long long)(mel_first + mel_frames));
    const int64_t need_lo = std::max<int64_t>(0, t0 - H), need_hi = utt_frames >= 0 ? std::min(utt_frames, t1 + H) : t1 + H;
    if (mel_first > need_lo || mel_first + mel_frames < need_hi)
        FD_FAIL(h, FD_ERR_INVALID, "fd_sample_span: frames [%lld, %lld) need mel over [%lld, %lld) (halo %d frames per side for N=%d), got [%lld, %lld)",
                (long long)t0, (long long)t1, (long long)need_lo, (long long)need_hi, H, N, (long long)mel_first, (long long)(mel_first + mel_frames));
    if (z && N > 8) FD_FAIL(h, FD_ERR_INVALID, "fd_sample_span: injected z needs N <= 8 (N=%d); leave z NULL for Philox noise", N);
    if (window_frames < 0 || window_frames % 32 != 0)
        FD_FAIL(h, FD_ERR_INVALID, "fd_sample_span: window_frames=%d must be a non-negative multiple of 32", window_frames);

    // the window: `lead` frames in front of its centre (the halo rounded up to the alignment), the centre, the halo behind it
    const int64_t C = window_frames ? window_frames : ceil_to(std::max(1024, 4 * H), 32) - 2 * H;
    const int64_t lead = ceil_to(H, ALIGN), Wp64 = ceil_to(lead + C + H, 32);
    if (Wp64 * fd::HOPT * fd::C >= I32)
        FD_FAIL(h, FD_ERR_INVALID, "fd_sample_span: a window of %lld frames is too large for one batch item", (long long)Wp64);
    const int Wp = (int)Wp64;
    const int64_t n_windows = (t1 - t0 + C - 1) / C;
    int64_t Bw = std::min<int64_t>(fdk::SPAN_MAX_WINDOWS, std::max<int64_t>(1, BATCH_FRAMES / Wp));
    Bw = std::min(Bw, std::max<int64_t>(1, (I32 - 1) / (Wp64 * fd::HOPT * fd::C)));
    Bw = std::min(Bw, n_windows);

    // the window batch's buffers, sized by the batch alone (not by the utterance)
    const int64_t L = Wp64 * fd::HOPT;
    auto al = [](int64_t f) { return (f + 63) / 64 * 64; };
    const int64_t f_mel = al(Bw * fd::COND * Wp64), f_x = x_T ? al(Bw * L) : 0, f_z = z ? al((int64_t)N * Bw * L) : 0, f_out = al(Bw * L);
    const size_t need = sizeof(float) * (size_t)(f_mel + f_x + f_z + f_out);
    Scratch &s = h->span_scratch;
    if (s.bytes < need) {
        FD_HIP(h, hipDeviceSynchronize());      // the previous span call's copies may still read the old buffer
        if (s.p) hipFree(s.p);
        s = Scratch{};
        FD_HIP(h, hipMalloc(reinterpret_cast<void **>(&s.p), need));
        s.bytes = need;
    }
    float *mel_w = s.p, *x_w = x_T ? mel_w + f_mel : nullptr, *z_w = z ? mel_w + f_mel + f_x : nullptr, *out_w = mel_w + f_mel + f_x + f_z;

    hipStream_t stream = (hipStream_t)stream_;
    if ((rc = fd_follow_stream(h, stream)) != FD_OK) return rc;
    const fdk::Launch Lc = {h, stream, false, nullptr};
    for (int64_t c_next = t0; c_next < t1;) {
        fdk::SpanWindows w = {};
        std::vector<int> lens;
        std::vector<long long> offs;
        for (; c_next < t1 && w.n < Bw; c_next += C) {
            const int64_t ce = std::min(c_next + C, t1), ws = std::max<int64_t>(0, floor_to(c_next - H, ALIGN));
            const int64_t we = utt_frames >= 0 ? std::min(utt_frames, ce + H) : ce + H;
            w.start[w.n] = ws; w.len[w.n] = (int)(we - ws); w.c0[w.n] = c_next; w.clen[w.n] = (int)(ce - c_next);
            lens.push_back(w.len[w.n]);
            offs.push_back((long long)ws * (fd::HOPT / 4));
            ++w.n;
        }
        hipError_t e = fdk::span_gather(Lc, w, Wp, mel, x_T, z, N, mel_first, mel_frames, mel_w, x_w, z_w);
        if (e != hipSuccess) FD_FAIL(h, FD_ERR_HIP, "fd_sample_span: window gather failed: %s", hipGetErrorString(e));
        h->noise_ids.assign(w.n, (unsigned long long)stream_id);
        h->noise_offs = offs;
        if ((rc = fd_sample(h, mel_w, w.n, Wp, lens.data(), table, N, ddim, x_w, z_w, seed, out_w, nullptr, stream_)) != FD_OK) return rc;
        // final before its centres are kept: a batch that raised a range flag is redone here, on the fp32 kernels
        if ((rc = fd_settle(h)) != FD_OK) return rc;
        if ((e = fdk::span_scatter(Lc, w, Wp, out_w, t0, out)) != hipSuccess)
            FD_FAIL(h, FD_ERR_HIP, "fd_sample_span: window scatter failed: %s", hipGetErrorString(e));
    }
    return fd_mark_tail(h, stream);
}

}  // extern "C"
