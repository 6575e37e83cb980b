// fd_kernels_trim.hip -- cutting long silences on the device (include/fastdiff_hip_ext.h: fd_trim_silences / fd_trim_levels, which define
// the method): what the reference gets from trim_long_silences in process_utterance(trim_long_sil=True) (data_gen/tts/
// data_gen_utils.py:27-90), with an energy detector on the native rate's window grid in place of WebRTC's at 16 kHz.
//
//   k_trim_levels   grid (windows / 4, B), a wavefront per window.  Lane l adds groups l, l + 64, ... of 4 consecutive samples of the
//                   window in ascending order (16-byte loads where the group's address allows; the order does not depend on it), the lanes
//                   are added by the butterfly of fd_kernels_sums.h; once for the mean, once for the squares.  A window of up to
//                   256 TR_HELD + 3 samples (every window up to 48 kHz) is loaded once and held in registers for both passes; a longer
//                   one is read twice, the second time from the cache, with the same order of additions.  -> level bits per window,
//                   TR_NOLEVEL for a window with a sample that is not finite.
//   k_trim_mask     one workgroup per utterance, TR_CHUNK windows at a time, running counts carried across chunks: (1) peak and
//                   nonfinite count, (2) speech flags as inclusive prefix counts ps[], (3) smoothed flags from differences of ps[], as
//                   prefix counts pm[], with the first and last smoothed window, (4) kept flags from differences of pm[] (or the span
//                   between the edges), the exclusive prefix kp[] of kept samples, flags, out_valid and the record.  A pass reads what
//                   the pass before wrote for OTHER windows only behind a __syncthreads.
//   k_trim_gather   grid (tiles of TR_TILE output samples over L, B): the window of the tile's first sample by bisection in kp[], then
//                   run by run -- the workgroup copies what the tile takes of a kept window, coalesced, and steps to the next kept
//                   window (the neighbour, or by bisection across a cut stretch); zeros at and behind n_out.
//
// No workgroup waits on another.  Nothing at or behind an utterance's own length is read.
#include "fd_internal.h"
#include "fd_kernels.h"
#include "fd_kernels_common.h"
#include "fd_kernels_sums.h"
#include "fd_trim.h"

namespace fdk {

constexpr int TR_WAVES = 4, TR_CHUNK = fdtr::CHUNK, TR_TILE = 2048;
constexpr int TR_HELD = 12;                                    // groups of 4 samples a lane holds in registers for both passes of a window
constexpr unsigned long long TR_NOLEVEL = 0x7FF8000000000000ull;
static_assert(TR_CHUNK == FD_TRIM_CHUNK && TR_CHUNK == 256, "a chunk is one window per thread of the mask kernel's workgroup");

__device__ __forceinline__ long long tr_windows(long long n, long long W) { const long long m = n / W; return m > 1 ? m : 1; }

// 4 consecutive samples: one 16-byte load or four 4-byte ones
__device__ __forceinline__ float4 tr_load4(const float *__restrict__ p, bool aligned)
{
    if (aligned) return *reinterpret_cast<const float4 *>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

__global__ void __launch_bounds__(256) k_trim_levels(const float *__restrict__ wav, long long L, const long long *__restrict__ valid, long long W,
                                                     unsigned long long *__restrict__ levels, long long pitch, int fill_tail)
{
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * TR_WAVES + (threadIdx.x >> 6);
    const long long n = own_len(valid, b, L);
    const long long M = tr_windows(n, W);
    unsigned long long *__restrict__ lv = levels + (long long)b * pitch;
    if (n == 0 || w >= M) {                                // (the whole wavefront) no such window
        if (fill_tail && w < pitch && lane == 0) lv[w] = 0ull;
        return;
    }
    const long long s0 = w * W;
    const long long cnt = w < M - 1 ? W : n - s0;          // the last window takes the tail
    const float *__restrict__ x = wav + (long long)b * L + s0;
    const bool aligned = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const long long groups = cnt >> 2;
    const bool tail = lane == (int)(groups & 63);          // the incomplete last group, in its turn
    double s = 0.0, q = 0.0, m;
    bool bad = false;
    if (groups <= 64 * TR_HELD) {
        // the window in registers: loaded once, for both passes (a window of up to 256 TR_HELD + 3 samples: every rate up to 48 kHz)
        float4 r[TR_HELD];
        float t[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < TR_HELD; ++k) r[k] = lane + 64 * k < groups ? tr_load4(x + 4 * (lane + 64 * k), aligned) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (tail)
            for (int i = 0; i < 3; ++i) t[i] = 4 * groups + i < cnt ? x[4 * groups + i] : 0.0f;
#pragma unroll
        for (int k = 0; k < TR_HELD; ++k)
            if (lane + 64 * k < groups) {
                const float4 v = r[k];
                bad = bad || not_finite(v.x) || not_finite(v.y) || not_finite(v.z) || not_finite(v.w);
                s += (double)v.x; s += (double)v.y; s += (double)v.z; s += (double)v.w;
            }
        if (tail)
            for (int i = 0; i < 3; ++i)
                if (4 * groups + i < cnt) {
                    bad = bad || not_finite(t[i]);
                    s += (double)t[i];
                }
        m = wave_sum(s) / (double)cnt;
#pragma unroll
        for (int k = 0; k < TR_HELD; ++k)
            if (lane + 64 * k < groups) {
                const float4 v = r[k];
                const double d0 = (double)v.x - m, d1 = (double)v.y - m, d2 = (double)v.z - m, d3 = (double)v.w - m;
                q += d0 * d0; q += d1 * d1; q += d2 * d2; q += d3 * d3;
            }
        if (tail)
            for (int i = 0; i < 3; ++i)
                if (4 * groups + i < cnt) {
                    const double d = (double)t[i] - m;
                    q += d * d;
                }
    } else {
        // a longer window: the second pass reads what the first left in the cache; the same order of additions
        for (long long g = lane; g < groups; g += 64) {
            const float4 v = tr_load4(x + 4 * g, aligned);
            bad = bad || not_finite(v.x) || not_finite(v.y) || not_finite(v.z) || not_finite(v.w);
            s += (double)v.x; s += (double)v.y; s += (double)v.z; s += (double)v.w;
        }
        if (tail)
            for (long long i = 4 * groups; i < cnt; ++i) {
                const float v = x[i];
                bad = bad || not_finite(v);
                s += (double)v;
            }
        m = wave_sum(s) / (double)cnt;
        for (long long g = lane; g < groups; g += 64) {
            const float4 v = tr_load4(x + 4 * g, aligned);
            const double d0 = (double)v.x - m, d1 = (double)v.y - m, d2 = (double)v.z - m, d3 = (double)v.w - m;
            q += d0 * d0; q += d1 * d1; q += d2 * d2; q += d3 * d3;
        }
        if (tail)
            for (long long i = 4 * groups; i < cnt; ++i) {
                const double d = (double)x[i] - m;
                q += d * d;
            }
    }
    const double e = wave_sum(q) / (double)cnt;
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane == 0) lv[w] = any_bad ? TR_NOLEVEL : (unsigned long long)__double_as_longlong(10.0 * log10(fmax(e, fdtr::E_FLOOR)));
}

struct TrimParams { double top_db, floor_db; int A, G, mode; };

// inclusive scan of v over the workgroup's 256 threads (lane order, then wave order); total: the sum of all
template <class T>
__device__ __forceinline__ T tr_scan(T v, T *ws, T &total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T u = __shfl_up(v, off, 64);
        if (lane >= off) v += u;
    }
    __syncthreads();                                       // (ws is free)
    if (lane == 63) ws[wv] = v;
    __syncthreads();
    T base = 0;
    for (int k = 0; k < wv; ++k) base += ws[k];
    total = (ws[0] + ws[1]) + (ws[2] + ws[3]);
    return v + base;
}

__global__ void __launch_bounds__(256) k_trim_mask(long long L, const long long *__restrict__ valid, long long W, TrimParams p,
                                                   const unsigned long long *__restrict__ levels, int *ps_all, int *pm_all, long long *kp_all,
                                                   long long pitch, int *__restrict__ out_valid, unsigned char *__restrict__ flags,
                                                   fd_trim *__restrict__ rec)
{
    __shared__ int wsi[4];
    __shared__ long long wsl[4];
    __shared__ double wsd[4];
    __shared__ long long wmin[4], wmax[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long n = own_len(valid, b, L);
    const double ninf = -__builtin_huge_val();
    unsigned char *fl = flags ? flags + (long long)b * pitch : nullptr;
    if (n == 0) {
        for (long long w = tid; fl && w < pitch; w += 256) fl[w] = 0;
        if (tid == 0) {
            out_valid[b] = 0;
            if (rec) {
                fd_trim r;
                r.n_out = 0; r.windows = 0; r.speech = 0; r.kept_windows = 0; r.nonfinite = 0; r.status = FD_TRIM_EMPTY;
                r.peak_db = ninf; r.threshold_db = p.floor_db;
                rec[b] = r;
            }
        }
        return;
    }
    const long long M = tr_windows(n, W);
    const unsigned long long *__restrict__ lv = levels + (long long)b * pitch;
    int *ps = ps_all + (long long)b * pitch, *pm = pm_all + (long long)b * pitch;
    long long *kp = kp_all + (long long)b * (pitch + 1);

    // (1) the peak over the windows that have a level, and the count of those that have none
    double peak = ninf;
    int nf = 0;
    for (long long w = tid; w < M; w += 256) {
        const unsigned long long bits = lv[w];
        if (bits == TR_NOLEVEL) ++nf;
        else peak = fmax(peak, __longlong_as_double((long long)bits));
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { peak = fmax(peak, __shfl_xor(peak, m, 64)); nf += __shfl_xor(nf, m, 64); }
    if (lane == 0) { wsd[wv] = peak; wsi[wv] = nf; }
    __syncthreads();
    peak = fmax(fmax(wsd[0], wsd[1]), fmax(wsd[2], wsd[3]));
    nf = (wsi[0] + wsi[1]) + (wsi[2] + wsi[3]);
    const double thr = fmax(peak - p.top_db, p.floor_db);

    // (2) speech flags as inclusive prefix counts
    int carry = 0;
    for (long long c0 = 0; c0 < M; c0 += TR_CHUNK) {
        const long long w = c0 + tid;
        int s = 0;
        if (w < M) {
            const unsigned long long bits = lv[w];
            s = (bits != TR_NOLEVEL && __longlong_as_double((long long)bits) > thr) ? 1 : 0;
        }
        int total;
        const int inc = tr_scan(s, wsi, total);
        if (w < M) ps[w] = carry + inc;
        carry += total;
    }
    const int n_speech = carry;
    __syncthreads();

    // (3) smoothed flags: 2 c_w > A over w - (A - 1) / 2 .. w + A / 2, as prefix counts; the first and last smoothed window
    long long first = M, last = -1;
    carry = 0;
    for (long long c0 = 0; c0 < M; c0 += TR_CHUNK) {
        const long long w = c0 + tid;
        int s = 0;
        if (w < M) {
            const long long lo = w - (p.A - 1) / 2, hi = w + p.A / 2;
            const int c = ps[hi < M - 1 ? hi : M - 1] - (lo > 0 ? ps[lo - 1] : 0);
            s = 2 * c > p.A ? 1 : 0;
            if (s) { first = first < w ? first : w; last = w; }
        }
        int total;
        const int inc = tr_scan(s, wsi, total);
        if (w < M) pm[w] = carry + inc;
        carry += total;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const long long f = __shfl_xor(first, m, 64), l = __shfl_xor(last, m, 64);
        first = f < first ? f : first;
        last = l > last ? l : last;
    }
    __syncthreads();
    if (lane == 0) { wmin[wv] = first; wmax[wv] = last; }
    __syncthreads();                                       // (also: pm[] of every window is written)
    for (int k = 0; k < 4; ++k) { first = wmin[k] < first ? wmin[k] : first; last = wmax[k] > last ? wmax[k] : last; }
    // MODE_EDGES: from the first kept window to the last one = the dilated edges of the smoothed span
    const long long e_lo = first - p.G / 2, e_hi = last + p.G / 2;

    // (4) kept flags, the exclusive prefix of kept samples per window, the flags
    long long kcarry = 0;
    int n_kept = 0;
    for (long long c0 = 0; c0 < M; c0 += TR_CHUNK) {
        const long long w = c0 + tid;
        long long take = 0;
        int keep = 0;
        if (w < M) {
            if (p.mode == fdtr::MODE_EDGES) {
                keep = (last >= 0 && w >= e_lo && w <= e_hi) ? 1 : 0;
            } else {
                const long long lo = w - p.G / 2, hi = w + p.G / 2;
                keep = pm[hi < M - 1 ? hi : M - 1] - (lo > 0 ? pm[lo - 1] : 0) > 0 ? 1 : 0;
            }
            take = keep ? (w < M - 1 ? W : n - w * W) : 0;
            n_kept += keep;
        }
        long long total;
        const long long inc = tr_scan(take, wsl, total);
        if (w < M) {
            kp[w] = kcarry + inc - take;
            if (fl) {
                const int sp = ps[w] - (w > 0 ? ps[w - 1] : 0), sm = pm[w] - (w > 0 ? pm[w - 1] : 0);
                fl[w] = (unsigned char)(sp | (sm << 1) | (keep << 2));
            }
        }
        kcarry += total;
    }
    for (long long w = M + tid; fl && w < pitch; w += 256) fl[w] = 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) n_kept += __shfl_xor(n_kept, m, 64);
    __syncthreads();
    if (lane == 0) wsi[wv] = n_kept;
    __syncthreads();
    if (tid != 0) return;
    n_kept = (wsi[0] + wsi[1]) + (wsi[2] + wsi[3]);
    kp[M] = kcarry;
    out_valid[b] = (int)kcarry;
    if (rec) {
        fd_trim r;
        r.n_out = (int)kcarry; r.windows = (int)M; r.speech = n_speech; r.kept_windows = n_kept; r.nonfinite = nf;
        r.status = n_kept > 0 ? FD_TRIM_OK : FD_TRIM_SILENT;
        r.peak_db = peak; r.threshold_db = thr;
        rec[b] = r;
    }
}

// the largest w in [lo, hi) with kp[w] <= j, given kp[lo] <= j < kp[hi]
__device__ __forceinline__ long long tr_find(const long long *__restrict__ kp, long long lo, long long hi, long long j)
{
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (kp[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}

// (samples as words: bit copies whatever they hold)
__global__ void __launch_bounds__(256) k_trim_gather(const unsigned int *__restrict__ wav, long long L, const long long *__restrict__ valid, long long W,
                                                     const long long *__restrict__ kp_all, long long pitch, const int *__restrict__ out_valid,
                                                     unsigned int *__restrict__ out)
{
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * TR_TILE;
    const long long n_out = out_valid[b];
    unsigned int *__restrict__ orow = out + (long long)b * L;
    if (t0 >= n_out) {                                     // (the whole workgroup) a tile of zeros
        for (int q = 0; q < TR_TILE / 256; ++q) {
            const long long j = t0 + q * 256 + tid;
            if (j < L) orow[j] = 0u;
        }
        return;
    }
    const long long n = own_len(valid, b, L);
    const long long M = tr_windows(n, W);
    const long long *__restrict__ kp = kp_all + (long long)b * (pitch + 1);      // kp[0] = 0, kp[M] = n_out
    const unsigned int *__restrict__ row = wav + (long long)b * L;
    const long long t_end = t0 + TR_TILE < n_out ? t0 + TR_TILE : n_out;
    // run by run: the kept window w that holds output `pos`, its samples up to the tile's end, then the next kept window.  Everything
    // here but j is the same in every thread.
    long long pos = t0, w = tr_find(kp, 0, M, t0);
    while (pos < t_end) {
        const long long k0 = kp[w], k1 = kp[w + 1];
        const long long end = k1 < t_end ? k1 : t_end;
        const unsigned int *__restrict__ src = row + (w * W - k0);      // output j of this window is sample w W + (j - k0)
        for (long long j = pos + tid; j < end; j += 256) orow[j] = src[j];
        pos = end;
        if (pos < t_end)                                   // (so kp[w + 1] = pos < kp[M]: window w + 1 exists)
            w = kp[w + 2] > pos ? w + 1 : tr_find(kp, w + 1, M, pos);      // the neighbour if it is kept, else the next kept one
    }
    for (long long j = t_end + tid; j < t0 + TR_TILE && j < L; j += 256) orow[j] = 0u;
}

// the scratch buffer: valid [B], levels [B][Mp], ps [B][Mp], pm [B][Mp], kp [B][Mp + 1]; Mp = the windows of L samples
struct TrLayout { size_t valid, levels, ps, pm, kp, total; };
static TrLayout tr_layout(int B, int64_t Mp)
{
    TrLayout o;
    Carve c;
    o.valid = c.take(sizeof(long long) * B);
    o.levels = c.take(sizeof(unsigned long long) * (size_t)B * (size_t)Mp);
    o.ps = c.take(sizeof(int) * (size_t)B * (size_t)Mp);
    o.pm = c.take(sizeof(int) * (size_t)B * (size_t)Mp);
    o.kp = c.take(sizeof(long long) * (size_t)B * (size_t)(Mp + 1));
    o.total = c.at;
    return o;
}

size_t trim_scratch_bytes(int B, int64_t Mp) { return tr_layout(B, Mp).total; }
long long *trim_valid_slot(void *scratch) { return reinterpret_cast<long long *>(static_cast<char *>(scratch) + tr_layout(1, 1).valid); }

hipError_t trim_levels(const Launch &La, const float *wav, int B, int64_t L, const long long *valid_dev, int64_t W, int64_t M_grid, double *levels,
                       int64_t pitch, bool fill_tail)
{
    const dim3 grid((unsigned)((M_grid + TR_WAVES - 1) / TR_WAVES), B);
    FD_LAUNCH(La, "trim_levels", k_trim_levels, grid, dim3(256), 0, wav, (long long)L, valid_dev, (long long)W,
              reinterpret_cast<unsigned long long *>(levels), (long long)pitch, fill_tail ? 1 : 0);
    return hipSuccess;
}

hipError_t trim(const Launch &La, const float *wav, int B, int64_t L, const long long *valid_dev, const fd_trim_params &p, int64_t W, int64_t Mp,
                int64_t M_grid, float *out, int *out_valid, unsigned char *flags, fd_trim *rec, void *scratch)
{
    const TrLayout o = tr_layout(B, Mp);
    char *base = static_cast<char *>(scratch);
    double *levels = reinterpret_cast<double *>(base + o.levels);
    int *ps = reinterpret_cast<int *>(base + o.ps), *pm = reinterpret_cast<int *>(base + o.pm);
    long long *kp = reinterpret_cast<long long *>(base + o.kp);
    const hipError_t e = trim_levels(La, wav, B, L, valid_dev, W, M_grid, levels, Mp, false);
    if (e != hipSuccess) return e;
    const TrimParams tp = {p.top_db, p.floor_db, p.average_width, p.max_silence, p.mode};
    FD_LAUNCH(La, "trim_mask", k_trim_mask, dim3(B), dim3(256), 0, (long long)L, valid_dev, (long long)W, tp,
              reinterpret_cast<const unsigned long long *>(levels), ps, pm, kp, (long long)Mp, out_valid, flags, rec);
    const dim3 grid((unsigned)((L + TR_TILE - 1) / TR_TILE), B);
    FD_LAUNCH(La, "trim_gather", k_trim_gather, grid, dim3(256), 0, reinterpret_cast<const unsigned int *>(wav), (long long)L, valid_dev,
              (long long)W, (const long long *)kp, (long long)Mp, (const int *)out_valid, reinterpret_cast<unsigned int *>(out));
    return hipSuccess;
}

}  // namespace fdk
