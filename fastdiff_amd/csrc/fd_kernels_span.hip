// fd_kernels_span.hip -- the two copies around a window batch of fd_sample_span / fd_sample_spans (fd_api_span.cpp): the caller's long
// tensors into the padded [n][..][Wp] batch that fd_sample takes, and each window's exact centre of x_0 back into the caller's output.
// The denoiser itself runs on the tuned kernels, unchanged.  k_span_* serve one utterance with injected noise (windows by value);
// k_spans_* serve windows of many utterances, plain buffers and rings, from records in device memory; k_ring_append feeds the rings.
#include <algorithm>

#include "fd_kernels.h"

namespace fdk {

// blockIdx.y = one destination row: [0, 80n) mel rows (window b = row / 80, channel row % 80; unit 1 value per frame), then n rows of
// x_T, then nz * n rows of z (unit 256 samples per frame).  Element i of a row is frame-position start[b] * unit + i of the utterance:
// copied when it lies inside the window's own length and inside the caller's frames [mel_first, mel_first + mel_frames), zero
// otherwise (a window's padding behind its length, or the frames in front of mel_first that a 32-aligned window start may reach:
// they are further than the halo from every sample the window keeps).
__global__ void k_span_gather(SpanWindows w, int Wp, const float *__restrict__ mel, const float *__restrict__ x_T,
                              const float *__restrict__ z, long long mel_first, long long mel_frames, float *__restrict__ mel_w,
                              float *__restrict__ x_w, float *__restrict__ z_w)
{
    const int r = blockIdx.y, n = w.n, mel_rows = n * fd::COND, x_rows = x_T ? n : 0;
    int b, unit;
    const float *src;
    float *dst;
    if (r < mel_rows) {
        b = r / fd::COND;
        unit = 1;
        src = mel + (int64_t)(r % fd::COND) * mel_frames;
        dst = mel_w + (int64_t)r * Wp;
    } else if (r < mel_rows + x_rows) {
        b = r - mel_rows;
        unit = fd::HOPT;
        src = x_T;
        dst = x_w + (int64_t)b * Wp * fd::HOPT;
    } else {
        const int q = r - mel_rows - x_rows, k = q / n;
        b = q % n;
        unit = fd::HOPT;
        src = z + (int64_t)k * mel_frames * fd::HOPT;
        dst = z_w + (int64_t)q * Wp * fd::HOPT;
    }
    const int64_t width = (int64_t)Wp * unit, valid = (int64_t)w.len[b] * unit;
    const int64_t base = (w.start[b] - mel_first) * unit, avail = mel_frames * unit;      // position of element 0 in the caller's row
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < width; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = base + i;
        dst[i] = (i < valid && s >= 0 && s < avail) ? src[s] : 0.0f;
    }
}

// blockIdx.y = window b: samples [(c0 - start) * 256, + clen * 256) of its x_0 row -> out[(c0 - t0) * 256 ...]
__global__ void k_span_scatter(SpanWindows w, int Wp, const float *__restrict__ x_w, long long t0, float *__restrict__ out)
{
    const int b = blockIdx.y;
    const int64_t n_el = (int64_t)w.clen[b] * fd::HOPT;
    const float *src = x_w + (int64_t)b * Wp * fd::HOPT + (w.c0[b] - w.start[b]) * fd::HOPT;
    float *dst = out + (w.c0[b] - t0) * fd::HOPT;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_el; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

static unsigned span_blocks(int64_t width) { return (unsigned)std::min<int64_t>((width + 255) / 256, 1024); }

hipError_t span_gather(const Launch &L, const SpanWindows &w, int Wp, const float *mel, const float *x_T, const float *z, int nz,
                       long long mel_first, long long mel_frames, float *mel_w, float *x_w, float *z_w)
{
    const int rows = w.n * fd::COND + (x_T ? w.n : 0) + (z ? nz * w.n : 0);
    const int64_t width = (int64_t)Wp * (x_T || z ? fd::HOPT : 1);
    FD_LAUNCH(L, "span_gather", k_span_gather, dim3(span_blocks(width), rows), dim3(256), 0, w, Wp, mel, x_T, z, mel_first, mel_frames, mel_w,
              x_w, z_w);
    return hipSuccess;
}

hipError_t span_scatter(const Launch &L, const SpanWindows &w, int Wp, const float *x_w, long long t0, float *out)
{
    FD_LAUNCH(L, "span_scatter", k_span_scatter, dim3(span_blocks((int64_t)Wp * fd::HOPT), w.n), dim3(256), 0, w, Wp, x_w, t0, out);
    return hipSuccess;
}

// blockIdx.y = destination row r of mel_w [n][80][Wp]: window r / 80, channel r % 80.  Element i is utterance frame start + i, read at
// its plain or ring column when it lies inside the window's own length and inside the frames the source holds, else 0.  Validity is
// decided on UTTERANCE frames, never on ring columns: a ring slot still holds the frames of whoever used it before, and a 32-aligned
// window start may reach in front of mel_first (further than the halo from every sample the window keeps).  Consecutive lanes read
// consecutive columns; a ring window is at most two such runs per row.
__global__ void k_spans_gather(const SpanRec *__restrict__ recs, int Wp, float *__restrict__ mel_w)
{
    const int r = blockIdx.y;
    const SpanRec w = recs[r / fd::COND];
    const float *src = w.src + (int64_t)(r % fd::COND) * w.pitch;
    float *dst = mel_w + (int64_t)r * Wp;
    const int64_t held_end = w.mel_first + w.mel_frames;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < Wp; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = w.start + i;
        float v = 0.0f;
        if (i < w.len && f >= w.mel_first && f < held_end) v = src[w.cap > 0 ? f % w.cap : f - w.mel_first];
        dst[i] = v;
    }
}

// blockIdx.y = window b: samples [(c0 - start) * 256, + clen * 256) of its x_0 row -> its record's dst.  The source is 16-byte aligned
// (rows of Wp * 256 floats in a 256-byte aligned buffer); a destination that is too moves 16 bytes per lane, any other goes float by
// float -- chosen per window.
__global__ void k_spans_scatter(const SpanRec *__restrict__ recs, int Wp, const float *__restrict__ x_w)
{
    const int b = blockIdx.y;
    const SpanRec w = recs[b];
    const int64_t n_el = (int64_t)w.clen * fd::HOPT;
    const float *src = x_w + (int64_t)b * Wp * fd::HOPT + (w.c0 - w.start) * fd::HOPT;
    float *dst = w.dst;
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        const float4 *s4 = reinterpret_cast<const float4 *>(src);
        float4 *d4 = reinterpret_cast<float4 *>(dst);
        for (int64_t i = first; i < n_el / 4; i += stride) d4[i] = s4[i];
    } else {
        for (int64_t i = first; i < n_el; i += stride) dst[i] = src[i];
    }
}

// blockIdx.z = chunk, blockIdx.y = channel: src[c][i] -> ring[c][(first_frame + i) % cap], i < frames (<= cap: the host checked)
__global__ void k_ring_append(const fd_ring_chunk *__restrict__ chunks)
{
    const fd_ring_chunk c = chunks[blockIdx.z];
    const float *src = c.src + (int64_t)blockIdx.y * c.src_pitch;
    float *dst = c.ring + (int64_t)blockIdx.y * c.pitch;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < c.frames; i += (int64_t)gridDim.x * blockDim.x)
        dst[(c.first_frame + i) % c.cap] = src[i];
}

hipError_t spans_gather(const Launch &L, const SpanRec *recs, int n, int Wp, float *mel_w)
{
    FD_LAUNCH(L, "spans_gather", k_spans_gather, dim3(span_blocks(Wp), n * fd::COND), dim3(256), 0, recs, Wp, mel_w);
    return hipSuccess;
}

hipError_t spans_scatter(const Launch &L, const SpanRec *recs, int n, int Wp, int max_clen, const float *x_w)
{
    FD_LAUNCH(L, "spans_scatter", k_spans_scatter, dim3(span_blocks((int64_t)max_clen * (fd::HOPT / 4)), n), dim3(256), 0, recs, Wp, x_w);
    return hipSuccess;
}

hipError_t ring_append(const Launch &L, const fd_ring_chunk *chunks, int n, long long max_frames)
{
    FD_LAUNCH(L, "ring_append", k_ring_append, dim3(span_blocks(max_frames), fd::COND, n), dim3(256), 0, chunks);
    return hipSuccess;
}

}  // namespace fdk
