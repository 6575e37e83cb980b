// fd_api_span.cpp -- host side of fd_sample_span / fd_sample_halo_frames (include/fastdiff_hip_ext.h): x_0 of a frame range of ONE
// utterance of any length, computed window by window.  Each window is a batch item of fd_sample -- the tuned kernels, graphs, hoisted
// predictor and range check unchanged -- computed as if it were an utterance of its own (zero padding at its edges, `lens` for a short
// last window), with its noise drawn at the whole utterance's sample positions (StepParams::offs4).  The network's receptive field is
// finite, so each window's output equals the whole-utterance result, bit for bit, on every frame at least H = N * 16 frames away from a
// window edge that is not an edge of the utterance; those centres are what the scatter keeps.
// fd_sample_spans does the same for frame ranges of MANY utterances at once: fd_sample_spans_plan cuts every span into windows and packs
// the windows of all of them into shared batches, so a directory of recordings or a set of live streams fills the sampler's batch.
#include <limits.h>
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

// The refusals of one span (`who`: the entry point, `at`: " of span 3" or ""), the pointers left to the caller.  "" = fine.
std::string span_refusal(const char *who, const char *at, int H, int N, int64_t mel_first, int64_t mel_frames, int64_t mel_cap, int64_t mel_pitch,
                         int64_t utt_frames, int64_t t0, int64_t t1)
{
    char b[512];
    b[0] = 0;
    const int64_t need_lo = std::max<int64_t>(0, t0 - H), need_hi = utt_frames >= 0 ? std::min(utt_frames, t1 + H) : t1 + H;
    if (utt_frames < -1 || utt_frames == 0)
        snprintf(b, sizeof(b), "%s: utt_frames=%lld%s (frames, or -1 = not known yet)", who, (long long)utt_frames, at);
    else if (t0 < 0 || t0 % 32 != 0 || t1 <= t0)
        snprintf(b, sizeof(b), "%s: [t0=%lld, t1=%lld)%s must be non-empty with t0 a multiple of 32", who, (long long)t0, (long long)t1, at);
    else if (utt_frames >= 0 && t1 > utt_frames)
        snprintf(b, sizeof(b), "%s: t1=%lld%s past the utterance's %lld frames", who, (long long)t1, at, (long long)utt_frames);
    else if (t1 % 32 != 0 && t1 != utt_frames)
        snprintf(b, sizeof(b), "%s: t1=%lld%s must be a multiple of 32 or the utterance's end", who, (long long)t1, at);
    else if (mel_first < 0 || mel_frames < 1 || (utt_frames >= 0 && mel_first + mel_frames > utt_frames))
        snprintf(b, sizeof(b), "%s: mel frames [%lld, %lld)%s outside the utterance", who, (long long)mel_first, (long long)(mel_first + mel_frames), at);
    else if (mel_cap < 0 || (mel_cap > 0 && mel_frames > mel_cap))
        snprintf(b, sizeof(b), "%s: a ring of mel_cap=%lld columns%s cannot hold mel_frames=%lld", who, (long long)mel_cap, at, (long long)mel_frames);
    else if (mel_pitch < (mel_cap > 0 ? mel_cap : mel_frames))
        snprintf(b, sizeof(b), "%s: mel_pitch=%lld%s shorter than a row of %lld columns", who, (long long)mel_pitch, at,
                 (long long)(mel_cap > 0 ? mel_cap : mel_frames));
    else if (mel_first > need_lo || mel_first + mel_frames < need_hi)
        snprintf(b, sizeof(b), "%s: frames [%lld, %lld)%s need mel over [%lld, %lld) (halo %d frames per side for N=%d), got [%lld, %lld)", who,
                 (long long)t0, (long long)t1, at, (long long)need_lo, (long long)need_hi, H, N, (long long)mel_first,
                 (long long)(mel_first + mel_frames));
    return b;
}

// fd_sample_spans_plan with the reason of a refusal.  C: centre frames per window; Wp: padded frames of every batch item; Bw: windows
// per batch.  Window i goes to batch i / Bw: the windows of all spans fill the batches in span order.
int plan_spans(const char *who, const fd_span *spans, int n_spans, int N, int window_frames, std::vector<fd_span_window> &out, int *Wp_out,
               std::string &why)
{
    char b[256];
    out.clear();
    *Wp_out = 0;
    const int H = fd_sample_halo_frames(N);
    if (H < 0) { snprintf(b, sizeof(b), "%s: N=%d outside 1..1024", who, N); why = b; return FD_ERR_INVALID; }
    if (n_spans < 0 || (n_spans > 0 && !spans)) { snprintf(b, sizeof(b), "%s: n_spans=%d / null spans", who, n_spans); why = b; return FD_ERR_INVALID; }
    if (window_frames < 0 || window_frames % 32 != 0) {
        snprintf(b, sizeof(b), "%s: window_frames=%d must be a non-negative multiple of 32", who, window_frames);
        why = b;
        return FD_ERR_INVALID;
    }
    if (n_spans == 0) return 0;
    int64_t longest = 0, total = 0;
    const int64_t C = window_frames ? window_frames : ceil_to(std::max(1024, 4 * H), 32) - 2 * H;
    for (int i = 0; i < n_spans; ++i) {
        const fd_span &s = spans[i];
        char at[32];
        snprintf(at, sizeof(at), n_spans > 1 ? " of span %d" : "", i);
        why = span_refusal(who, at, H, N, s.mel_first, s.mel_frames, s.mel_cap, s.mel_pitch, s.utt_frames, s.t0, s.t1);
        if (!why.empty()) return FD_ERR_INVALID;
        longest = std::max(longest, s.t1 - s.t0);
        total += (s.t1 - s.t0 + C - 1) / C;
    }
    // the padded length follows the centre actually needed: a batch of short stream windows does not reserve default-size windows
    const int64_t lead = ceil_to(H, ALIGN), Wp64 = ceil_to(lead + std::min(C, ceil_to(longest, 32)) + H, 32);
    if (Wp64 * fd::HOPT * fd::C >= I32) {
        snprintf(b, sizeof(b), "%s: a window of %lld frames is too large for one batch item", who, (long long)Wp64);
        why = b;
        return FD_ERR_INVALID;
    }
    if (total > INT_MAX / 2) { snprintf(b, sizeof(b), "%s: %lld windows are too many for one call", who, (long long)total); why = b; return FD_ERR_INVALID; }
    int64_t Bw = std::min<int64_t>(fdk::SPANS_MAX_WINDOWS, std::max<int64_t>(1, BATCH_FRAMES / Wp64));
    Bw = std::min(Bw, std::max<int64_t>(1, (I32 - 1) / (Wp64 * fd::HOPT * fd::C)));
    out.reserve((size_t)total);
    for (int i = 0; i < n_spans; ++i) {
        const fd_span &s = spans[i];
        for (int64_t c0 = s.t0; c0 < s.t1; c0 += C) {
            const int64_t ce = std::min(c0 + C, s.t1), ws = std::max<int64_t>(0, floor_to(c0 - H, ALIGN));
            const int64_t we = s.utt_frames >= 0 ? std::min(s.utt_frames, ce + H) : ce + H;
            out.push_back({i, (int32_t)((int64_t)out.size() / Bw), (int32_t)(we - ws), (int32_t)(ce - c0), ws, c0});
        }
    }
    *Wp_out = (int)Wp64;
    return (int)out.size();
}

int span_preconditions(fd_handle h, const char *who)
{
    if (h->gen)
        FD_FAIL(h, FD_ERR_UNSUPPORTED, "%s: windowed synthesis needs base.yaml's architecture (its halo is the receptive field "
                                       "of that network); this handle runs another configuration", who);
    int rc = fd_settle(h);
    if (rc != FD_OK) return rc;
    if (!h->committed) FD_FAIL(h, FD_ERR_STATE, "%s: weights not committed (call fd_commit_weights after fd_set_weight)", who);
    FD_HIP(h, hipSetDevice(h->device));
    if ((rc = fd_settle_refresh(h)) != FD_OK) return rc;
    for (int i = 0; i < ST_COUNT; ++i)
        if (!h->mode.fast[i])
            FD_FAIL(h, FD_ERR_UNSUPPORTED, "%s: needs the fast kernel set; the naive kernels (option kernels.<stage> = naive) "
                                           "ignore `lens`, which the last window of an utterance goes through", who);
    return FD_OK;
}

// the window batch's buffer holds at least `need` bytes
int span_reserve(fd_handle h, size_t need)
{
    Scratch &s = h->span_scratch;
    if (s.bytes >= need) return FD_OK;
    FD_HIP(h, hipDeviceSynchronize());      // the previous span call's copies may still read the old buffer
    if (s.p) hipFree(s.p);
    s = Scratch{};
    FD_HIP(h, hipMalloc(reinterpret_cast<void **>(&s.p), need));
    s.bytes = need;
    return FD_OK;
}

int sample_spans(fd_handle h, const char *who, const fd_span *spans, int n_spans, const fd_step *table, int N, int ddim, uint64_t seed,
                 int window_frames, void *stream_)
{
    int rc = span_preconditions(h, who);
    if (rc != FD_OK) return rc;
    if (n_spans < 0 || (n_spans > 0 && !spans) || !table) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    for (int i = 0; i < n_spans; ++i)
        if (!spans[i].mel || !spans[i].out) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer in span %d", who, i);
    std::vector<fd_span_window> win;
    std::string why;
    int Wp = 0;
    const int n_win = plan_spans(who, spans, n_spans, N, window_frames, win, &Wp, why);
    if (n_win < 0) FD_FAIL(h, n_win, "%s", why.c_str());
    if (n_win == 0) return FD_OK;
    int Bmax = 0;       // windows of the fullest batch (the first: every batch but the last is full)
    for (const fd_span_window &w : win) Bmax += w.batch == 0;

    // the window batch's buffers, sized by the batch alone (not by the utterances): records, mel, x_0
    const int64_t L = (int64_t)Wp * fd::HOPT;
    auto al = [](int64_t f) { return (f + 63) / 64 * 64; };
    const int64_t f_rec = al((int64_t)(fdk::SPANS_MAX_WINDOWS * sizeof(fdk::SpanRec) / sizeof(float))), f_mel = al((int64_t)Bmax * fd::COND * Wp);
    if ((rc = span_reserve(h, sizeof(float) * (size_t)(f_rec + f_mel + al(Bmax * L)))) != FD_OK) return rc;
    fdk::SpanRec *rec_dev = reinterpret_cast<fdk::SpanRec *>(h->span_scratch.p);
    float *mel_w = h->span_scratch.p + f_rec, *out_w = mel_w + f_mel;

    hipStream_t stream = (hipStream_t)stream_;
    if ((rc = fd_follow_stream(h, stream)) != FD_OK) return rc;
    const fdk::Launch Lc = {h, stream, false, nullptr};
    for (int first = 0; first < n_win;) {
        fdk::SpanRec recs[fdk::SPANS_MAX_WINDOWS] = {};
        std::vector<int> lens;
        std::vector<long long> offs;
        std::vector<unsigned long long> ids;
        int n = 0, max_clen = 0;
        for (; first + n < n_win && win[first + n].batch == win[first].batch; ++n) {
            const fd_span_window &w = win[first + n];
            const fd_span &s = spans[w.span];
            recs[n] = {s.mel, s.out + (w.c0 - s.t0) * fd::HOPT, (long long)s.mel_pitch, (long long)s.mel_cap, (long long)s.mel_first,
                       (long long)s.mel_frames, (long long)w.start, (long long)w.c0, w.len, w.clen, 0};
            lens.push_back(w.len);
            offs.push_back((long long)w.start * (fd::HOPT / 4));
            ids.push_back((unsigned long long)s.stream_id);
            max_clen = std::max(max_clen, (int)w.clen);
        }
        if ((rc = fd_stage_upload(h, recs, sizeof(fdk::SpanRec) * n, rec_dev, stream)) != FD_OK) return rc;
        hipError_t e = fdk::spans_gather(Lc, rec_dev, n, Wp, mel_w);
        if (e != hipSuccess) FD_FAIL(h, FD_ERR_HIP, "%s: window gather failed: %s", who, hipGetErrorString(e));
        h->noise_ids = ids;
        h->noise_offs = offs;
        ++h->n_span_batches;
        h->n_span_windows += n;
        if ((rc = fd_sample(h, mel_w, n, Wp, lens.data(), table, N, ddim, nullptr, nullptr, seed, out_w, nullptr, stream_)) != FD_OK) return rc;
        // final before its centres are kept: a batch that raised a range flag is redone here, on the fp32 kernels
        if ((rc = fd_settle(h)) != FD_OK) return rc;
        if ((e = fdk::spans_scatter(Lc, rec_dev, n, Wp, max_clen, out_w)) != hipSuccess)
            FD_FAIL(h, FD_ERR_HIP, "%s: window scatter failed: %s", who, hipGetErrorString(e));
        first += n;
    }
    return fd_mark_tail(h, stream);
}
}  // namespace

extern "C" {

int fd_sample_halo_frames(int N) { return (N < 1 || N > 1024) ? FD_ERR_INVALID : N * HALO_PER_STEP; }

int fd_sample_span(fd_handle h, const float *mel, int64_t mel_first, int64_t mel_frames, int64_t utt_frames, int64_t t0, int64_t t1,
                   const fd_step *table, int N, int ddim, const float *x_T, const float *z, uint64_t seed, uint64_t stream_id,
                   int window_frames, float *out, void *stream_)
{
    if (!h) return FD_ERR_INVALID;
    if (!x_T && !z) {      // Philox noise: one span of fd_sample_spans (a plain buffer of mel_frames columns)
        const fd_span one = {mel, mel_frames, 0, mel_first, mel_frames, utt_frames, t0, t1, stream_id, out};
        return sample_spans(h, "fd_sample_span", &one, 1, table, N, ddim, seed, window_frames, stream_);
    }
    // injected x_T / z: windows of this one utterance, passed to the copy kernels by value
    int rc = span_preconditions(h, "fd_sample_span");
    if (rc != FD_OK) return rc;
    if (!mel || !table || !out) FD_FAIL(h, FD_ERR_INVALID, "fd_sample_span: null pointer");
    const int H = fd_sample_halo_frames(N);
    if (H < 0) FD_FAIL(h, FD_ERR_INVALID, "fd_sample_span: N=%d outside 1..1024", N);
    const std::string why = span_refusal("fd_sample_span", "", H, N, mel_first, mel_frames, 0, mel_frames, utt_frames, t0, t1);
    if (!why.empty()) FD_FAIL(h, FD_ERR_INVALID, "%s", why.c_str());
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
    if ((rc = span_reserve(h, sizeof(float) * (size_t)(f_mel + f_x + f_z + f_out))) != FD_OK) return rc;
    float *mel_w = h->span_scratch.p, *x_w = x_T ? mel_w + f_mel : nullptr, *z_w = z ? mel_w + f_mel + f_x : nullptr, *out_w = mel_w + f_mel + f_x + f_z;

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
        ++h->n_span_batches;
        h->n_span_windows += w.n;
        if ((rc = fd_sample(h, mel_w, w.n, Wp, lens.data(), table, N, ddim, x_w, z_w, seed, out_w, nullptr, stream_)) != FD_OK) return rc;
        // final before its centres are kept: a batch that raised a range flag is redone here, on the fp32 kernels
        if ((rc = fd_settle(h)) != FD_OK) return rc;
        if ((e = fdk::span_scatter(Lc, w, Wp, out_w, t0, out)) != hipSuccess)
            FD_FAIL(h, FD_ERR_HIP, "fd_sample_span: window scatter failed: %s", hipGetErrorString(e));
    }
    return fd_mark_tail(h, stream);
}

int fd_sample_spans_plan(const fd_span *spans, int n_spans, int N, int window_frames, fd_span_window *windows, int max_windows, int *Wp)
{
    std::vector<fd_span_window> win;
    std::string why;
    int wp = 0;
    const int n = plan_spans("fd_sample_spans_plan", spans, n_spans, N, window_frames, win, &wp, why);
    if (n < 0) return n;
    if (Wp) *Wp = wp;
    for (int i = 0; windows && i < n && i < max_windows; ++i) windows[i] = win[i];
    return n;
}

int fd_sample_spans(fd_handle h, const fd_span *spans, int n_spans, const fd_step *table, int N, int ddim, uint64_t seed, int window_frames,
                    void *stream)
{
    if (!h) return FD_ERR_INVALID;
    return sample_spans(h, "fd_sample_spans", spans, n_spans, table, N, ddim, seed, window_frames, stream);
}

int fd_mel_ring_append(fd_handle h, const fd_ring_chunk *chunks, int n, void *stream_)
{
    if (!h) return FD_ERR_INVALID;
    if (n < 0 || n > 4096 || (n > 0 && !chunks)) FD_FAIL(h, FD_ERR_INVALID, "fd_mel_ring_append: n=%d chunks (0..4096)", n);
    int64_t longest = 0;
    for (int i = 0; i < n; ++i) {
        const fd_ring_chunk &c = chunks[i];
        if (!c.ring || !c.src) FD_FAIL(h, FD_ERR_INVALID, "fd_mel_ring_append: null pointer in chunk %d", i);
        if (c.cap < 1 || c.pitch < c.cap || c.first_frame < 0 || c.frames < 0 || c.src_pitch < c.frames)
            FD_FAIL(h, FD_ERR_INVALID, "fd_mel_ring_append: chunk %d: cap=%lld pitch=%lld first_frame=%lld frames=%lld src_pitch=%lld", i,
                    (long long)c.cap, (long long)c.pitch, (long long)c.first_frame, (long long)c.frames, (long long)c.src_pitch);
        if (c.frames > c.cap)
            FD_FAIL(h, FD_ERR_INVALID, "fd_mel_ring_append: chunk %d has %lld frames, the ring holds %lld", i, (long long)c.frames, (long long)c.cap);
        longest = std::max<int64_t>(longest, c.frames);
    }
    if (longest == 0) return FD_OK;
    FD_HIP(h, hipSetDevice(h->device));
    hipStream_t stream = (hipStream_t)stream_;
    int rc = fd_follow_stream(h, stream);
    if (rc != FD_OK) return rc;
    const size_t bytes = sizeof(fd_ring_chunk) * (size_t)n;
    Scratch &s = h->ring_scratch;
    if (s.bytes < bytes) {
        FD_HIP(h, hipDeviceSynchronize());      // an earlier append may still read the old records
        if (s.p) hipFree(s.p);
        s = Scratch{};
        const size_t cap = std::max<size_t>(4096, 2 * bytes);
        FD_HIP(h, hipMalloc(reinterpret_cast<void **>(&s.p), cap));
        s.bytes = cap;
    }
    if ((rc = fd_stage_upload(h, chunks, bytes, s.p, stream)) != FD_OK) return rc;
    const fdk::Launch Lc = {h, stream, false, nullptr};
    const hipError_t e = fdk::ring_append(Lc, reinterpret_cast<const fd_ring_chunk *>(s.p), n, longest);
    if (e != hipSuccess) FD_FAIL(h, FD_ERR_HIP, "fd_mel_ring_append: launch failed: %s", hipGetErrorString(e));
    return fd_mark_tail(h, stream);
}

}  // extern "C"
