// fd_kernels_stoi.hip -- STOI (Taal et al. 2011) and ESTOI (Jensen and Taal 2016) on the device (include/fastdiff_hip_ext.h:
// fd_stoi_measure, which defines the measurement): what people get from pystoi over the *_gt.wav / *_pred.wav pairs that the reference's
// test_step writes (modules/FastDiff/task/FastDiff.py:113-117); the reference itself has no code for it.  Both signals are at 10 kHz here
// (the host side resamples them with fd_resample first).
//
//   k_stoi_energy     one wavefront per frame of the clean signal: E_i = sum (w x_i)^2 in float32, four products per lane in ascending
//                     order, then a fixed shuffle tree; the utterance's maximum by atomicMax on non-negative float bits (no order).
//   k_stoi_count      grid (scan tiles, B): the kept frames (E_i > 1e-4 max E, compared in double) of ST_SCAN frames per workgroup.
//   k_stoi_offsets    one workgroup per utterance: exclusive scan of the tile counts, 256 tiles at a time with a carry, so any frame
//                     count works; writes K.
//   k_stoi_compact    the tile's flags again, an exclusive scan over its 256 threads (4 consecutive frames each), src[k] = i.
//   k_stoi_bands      grid (M, B, 2 signals), one workgroup per STFT frame: sample j of frame m of the silence-free signal is the sum of
//                     at most two windowed source samples (kept frames m - 1 | m for j < 128, m | m + 1 above: a gather); windowed
//                     again, 512-point DFT of the 256 samples by the split transform of fd_kernels_dft.h (16 x 32, n1 < 8 non-zero),
//                     only k2 < 14 (bins 0 .. 223; the bands cover 7 .. 218); 15 threads add their band's |X|^2 in ascending k and
//                     write the root.
//   k_stoi_segments   grid (segment tiles, B), float64: ST_SEGS segments per workgroup, their 45 frames staged in LDS.  STOI: one
//                     thread per (segment, band), the 15 bands then added in band order.  ESTOI: one wavefront per segment (four
//                     segments one after the other): rows, then columns, then 30 column sums added in frame order.
//   k_stoi_finish     one workgroup per utterance: the per-segment partials added in segment order (256 consecutive runs, then the runs
//                     in order) -> the 32-byte record.
//
// Every sum has a fixed order that depends on the utterance alone and there are no floating-point atomics, so a record is bit-identical
// alone, anywhere in a ragged batch and from call to call.  Nothing at or behind an utterance's own length is read.
#include "fd_internal.h"
#include "fd_kernels.h"
#include "fd_kernels_common.h"
#include "fd_kernels_dft.h"

namespace fdk {

constexpr int ST_FRAME = fds::FRAME, ST_HOP = fds::HOP, ST_NFFT = fds::NFFT, ST_BANDS = fds::BANDS, ST_SEG = fds::SEG;
constexpr int ST_SCAN = fds::SCAN_TILE, ST_SEGS = fds::SEG_TILE;
static_assert(ST_SCAN == FD_STOI_SCAN_TILE && ST_SEGS == FD_STOI_SEG_TILE, "the exported tile sizes are the kernels'");
static_assert(ST_FRAME == 256 && ST_HOP == 128 && ST_NFFT == 512 && ST_SCAN == 1024 && ST_SEGS == 16, "256-thread workgroups throughout");
constexpr int ST_SPAN = ST_SEGS + ST_SEG - 1;              // frames a tile of segments touches: 45
constexpr int ST_ROW = ST_SEG + 1;                         // ESTOI matrix rows padded against bank conflicts

__device__ __forceinline__ int st_frames(long long n) { return n > ST_FRAME ? (int)((n - ST_FRAME + ST_HOP - 1) / ST_HOP) : 0; }
__device__ __forceinline__ int st_kept_flag(float e, float emax) { return (double)e > fds::DYN_RANGE * (double)emax ? 1 : 0; }

__global__ void __launch_bounds__(256) k_stoi_energy(const float *__restrict__ x, long long pitch, const long long *__restrict__ lens,
                                                     long long n_all, const float *__restrict__ tab, float *__restrict__ E, int Fp,
                                                     unsigned int *__restrict__ maxbits)
{
    __shared__ float wm[4];
    const int b = blockIdx.y, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int F0 = st_frames(own_len(lens, b, n_all));
    const int i = blockIdx.x * 4 + wv;
    float e = 0.0f;
    if (i < F0) {                                          // (the whole wavefront)
        const float *__restrict__ fr = x + (long long)b * pitch + (long long)i * ST_HOP;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = lane + 64 * k;
            const float v = __fmul_rn(tab[j], fr[j]);
            e = fmaf(v, v, e);
        }
    }
    for (int off = 32; off > 0; off >>= 1) e += __shfl_down(e, off, 64);
    if (lane == 0) {
        if (i < F0) E[(long long)b * Fp + i] = e;
        wm[wv] = e;
    }
    __syncthreads();
    if (tid == 0) atomicMax(maxbits + b, __float_as_uint(fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]))));
}

// flags of this thread's four consecutive frames of scan tile blockIdx.x (bit q = frame i0 + q kept); returns their count
__device__ __forceinline__ int st_flags(const float *__restrict__ E, int F0, float emax, int i0, int &bits)
{
    bits = 0;
    int c = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (i0 + q < F0 && st_kept_flag(E[i0 + q], emax)) { bits |= 1 << q; ++c; }
    return c;
}

// inclusive scan of one int per thread over the 256 threads of the workgroup
__device__ __forceinline__ int st_scan256(int *sc, int tid, int v)
{
    for (int off = 1; off < 256; off <<= 1) {
        __syncthreads();
        sc[tid] = v;
        __syncthreads();
        if (tid >= off) v += sc[tid - off];
    }
    return v;
}

__global__ void __launch_bounds__(256) k_stoi_count(const float *__restrict__ E, int Fp, const long long *__restrict__ lens, long long n_all,
                                                    const unsigned int *__restrict__ maxbits, int *__restrict__ blk, int nblk)
{
    __shared__ int sc[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int F0 = st_frames(own_len(lens, b, n_all));
    int bits;
    const int c = st_flags(E + (long long)b * Fp, F0, __uint_as_float(maxbits[b]), blockIdx.x * ST_SCAN + tid * 4, bits);
    const int incl = st_scan256(sc, tid, c);
    if (tid == 255) blk[(long long)b * nblk + blockIdx.x] = incl;
}

__global__ void __launch_bounds__(256) k_stoi_offsets(const long long *__restrict__ lens, long long n_all, int *__restrict__ blk, int nblk,
                                                      int *__restrict__ kept)
{
    __shared__ int sc[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int F0 = st_frames(own_len(lens, b, n_all));
    const int nb = (F0 + ST_SCAN - 1) / ST_SCAN;           // <= nblk
    int *__restrict__ row = blk + (long long)b * nblk;
    int carry = 0;
    for (int c0 = 0; c0 < nb; c0 += 256) {
        const int v = c0 + tid < nb ? row[c0 + tid] : 0;
        const int incl = st_scan256(sc, tid, v);
        if (c0 + tid < nb) row[c0 + tid] = carry + incl - v;
        __syncthreads();
        sc[tid] = incl;
        __syncthreads();
        carry += sc[255];
    }
    if (tid == 0) kept[b] = carry;
}

__global__ void __launch_bounds__(256) k_stoi_compact(const float *__restrict__ E, int Fp, const long long *__restrict__ lens, long long n_all,
                                                      const unsigned int *__restrict__ maxbits, const int *__restrict__ blk, int nblk,
                                                      int *__restrict__ src)
{
    __shared__ int sc[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int F0 = st_frames(own_len(lens, b, n_all));
    const int i0 = blockIdx.x * ST_SCAN + tid * 4;
    int bits;
    const int c = st_flags(E + (long long)b * Fp, F0, __uint_as_float(maxbits[b]), i0, bits);
    const int incl = st_scan256(sc, tid, c);
    if (blockIdx.x * ST_SCAN >= F0) return;                // (the whole workgroup) behind the utterance: its offset was not written
    int k = blk[(long long)b * nblk + blockIdx.x] + incl - c;      // < K <= F0 <= Fp wherever a flag is set
    int *__restrict__ out = src + (long long)b * Fp;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (bits & (1 << q)) out[k++] = i0 + q;
}

__global__ void __launch_bounds__(256) k_stoi_bands(const float *__restrict__ x, const float *__restrict__ y, long long pitch,
                                                    const float *__restrict__ tab, const int *__restrict__ src, int Fp,
                                                    const int *__restrict__ kept, StoiBands bd, float *__restrict__ bands, int B, int Mp)
{
    static_assert(fdt::split_n1(ST_NFFT) == 16 && fdt::split_n2(ST_NFFT) == 32, "the bins below are cut as 16 x 32");
    __shared__ float ct[ST_NFFT], sn[ST_NFFT], xw[ST_FRAME], ar[32 * fdt::row(ST_NFFT)], ai[32 * fdt::row(ST_NFFT)], pw[224];
    const int m = blockIdx.x, b = blockIdx.y, sig = blockIdx.z, tid = threadIdx.x;
    if (m >= kept[b] - 1) return;                          // (the whole workgroup) M = K - 1 frames
    const float *__restrict__ w = tab;
    ct[tid] = tab[ST_FRAME + tid]; ct[256 + tid] = tab[ST_FRAME + 256 + tid];
    sn[tid] = tab[ST_FRAME + ST_NFFT + tid]; sn[256 + tid] = tab[ST_FRAME + ST_NFFT + 256 + tid];
    {   // sample 128 m + tid of the silence-free signal: kept frames (m - 1, m) below 128, (m, m + 1) above; m + 1 <= K - 1
        const float *__restrict__ s = (sig ? y : x) + (long long)b * pitch;
        const int *__restrict__ sr = src + (long long)b * Fp;
        const int j = tid;
        const float own = __fmul_rn(w[j], s[(long long)sr[m] * ST_HOP + j]);
        float v = own;
        if (j >= ST_HOP) v = __fadd_rn(own, __fmul_rn(w[j - ST_HOP], s[(long long)sr[m + 1] * ST_HOP + j - ST_HOP]));
        else if (m >= 1) v = __fadd_rn(__fmul_rn(w[j + ST_HOP], s[(long long)sr[m - 1] * ST_HOP + j + ST_HOP]), own);
        xw[j] = __fmul_rn(v, w[j]);
    }
    __syncthreads();
    dft_pass1<ST_NFFT>(xw, ct, sn, 0, ST_FRAME / 32, ar, ai, tid);      // the frame's 256 samples: n1 < 8
    __syncthreads();
    {   // pass 2: thread = (k1, k2 < 14)
        const int k1 = tid & 15, k2[1] = {tid >> 4};
        if (k2[0] < 14) {
            float re[1], im[1];
            dft_pass2<ST_NFFT, 8>(ar, ai, ct, sn, k1, k2, re, im);
            pw[k1 + 16 * k2[0]] = fmaf(re[0], re[0], im[0] * im[0]);
        }
    }
    __syncthreads();
    if (tid < ST_BANDS) {
        float acc = 0.0f;
        for (int k = bd.lo[tid]; k < bd.hi[tid]; ++k) acc += pw[k];      // hi <= 219 < 224
        bands[(((long long)sig * B + b) * Mp + m) * 16 + tid] = sqrtf(acc);
    }
}

__global__ void __launch_bounds__(256) k_stoi_segments(const float *__restrict__ bands, int B, int Mp, const int *__restrict__ kept,
                                                       double *__restrict__ part, int Jp)
{
    __shared__ double X[ST_SPAN * 16], Y[ST_SPAN * 16];
    __shared__ double WX[4][ST_BANDS * ST_ROW], WY[4][ST_BANDS * ST_ROW];
    __shared__ double ds[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int M = kept[b] - 1, J = M - (ST_SEG - 1);
    const int s0 = blockIdx.x * ST_SEGS;
    if (s0 >= J) return;                                   // (the whole workgroup)
    const double eps = fds::EPS;
    for (int idx = tid; idx < ST_SPAN * 16; idx += 256) {
        const int f = s0 + (idx >> 4), j = idx & 15;
        const bool in = f < M && j < ST_BANDS;
        X[idx] = in ? (double)bands[((long long)b * Mp + f) * 16 + j] : 0.0;
        Y[idx] = in ? (double)bands[(((long long)B + b) * Mp + f) * 16 + j] : 0.0;
    }
    __syncthreads();
    {   // STOI: thread = (segment sl, band j)
        const int sl = tid >> 4, j = tid & 15;
        double d = 0.0;
        if (j < ST_BANDS && s0 + sl < J) {
            double xs[ST_SEG], ys[ST_SEG];
            double sxx = 0.0, syy = 0.0;
#pragma unroll
            for (int t = 0; t < ST_SEG; ++t) {
                xs[t] = X[(sl + t) * 16 + j]; ys[t] = Y[(sl + t) * 16 + j];
                sxx += xs[t] * xs[t]; syy += ys[t] * ys[t];
            }
            const double c = sqrt(sxx) / (sqrt(syy) + eps);
            const double beta = 1.0 + 5.623413251903491;   // 1 + 10^(15 / 20)
            double mx = 0.0, my = 0.0;
#pragma unroll
            for (int t = 0; t < ST_SEG; ++t) {
                const double yn = ys[t] * c, cl = xs[t] * beta;
                ys[t] = yn < cl ? yn : cl;
                mx += xs[t]; my += ys[t];
            }
            mx /= ST_SEG; my /= ST_SEG;
            double nx = 0.0, ny = 0.0;
#pragma unroll
            for (int t = 0; t < ST_SEG; ++t) {
                xs[t] -= mx; ys[t] -= my;
                nx += xs[t] * xs[t]; ny += ys[t] * ys[t];
            }
            nx = sqrt(nx) + eps; ny = sqrt(ny) + eps;
#pragma unroll
            for (int t = 0; t < ST_SEG; ++t) d += (ys[t] / ny) * (xs[t] / nx);
        }
        ds[tid] = d;
        __syncthreads();
        if (j == 0 && s0 + sl < J) {
            double sum = 0.0;
            for (int k = 0; k < ST_BANDS; ++k) sum += ds[tid + k];
            part[((long long)b * Jp + s0 + sl) * 2] = sum;
        }
    }
    // ESTOI: wavefront wv takes segments 4 wv .. 4 wv + 3 one after the other; lanes 0 .. 31 work on X, 32 .. 63 on Y
    const int wv = tid >> 6, lane = tid & 63, l5 = lane & 31;
    double *__restrict__ Wm = lane < 32 ? WX[wv] : WY[wv];
    const double *__restrict__ Sm = lane < 32 ? X : Y;
    for (int q = 0; q < 4; ++q) {                          // (every wavefront passes every barrier)
        const int sl = wv * 4 + q;
        const bool on = s0 + sl < J;
        __syncthreads();
        if (on)
            for (int idx = l5; idx < ST_BANDS * ST_SEG; idx += 32) {
                const int j = idx / ST_SEG, t = idx - j * ST_SEG;
                Wm[j * ST_ROW + t] = Sm[(sl + t) * 16 + j];
            }
        __syncthreads();
        if (on && l5 < ST_BANDS) {                         // a row: one band over the 30 frames
            double *__restrict__ r = Wm + l5 * ST_ROW;
            double mean = 0.0, nn = 0.0;
            for (int t = 0; t < ST_SEG; ++t) mean += r[t];
            mean /= ST_SEG;
            for (int t = 0; t < ST_SEG; ++t) { const double v = r[t] - mean; nn += v * v; }
            nn = sqrt(nn) + eps;
            for (int t = 0; t < ST_SEG; ++t) r[t] = (r[t] - mean) / nn;
        }
        __syncthreads();
        if (on && l5 < ST_SEG) {                           // a column: one frame over the 15 bands
            double *__restrict__ c = Wm + l5;
            double mean = 0.0, nn = 0.0;
            for (int j = 0; j < ST_BANDS; ++j) mean += c[j * ST_ROW];
            mean /= ST_BANDS;
            for (int j = 0; j < ST_BANDS; ++j) { const double v = c[j * ST_ROW] - mean; nn += v * v; }
            nn = sqrt(nn) + eps;
            for (int j = 0; j < ST_BANDS; ++j) c[j * ST_ROW] = (c[j * ST_ROW] - mean) / nn;
        }
        __syncthreads();
        if (on && lane < ST_SEG) {
            double sum = 0.0;
            for (int j = 0; j < ST_BANDS; ++j) sum += WX[wv][j * ST_ROW + lane] * WY[wv][j * ST_ROW + lane];
            ds[wv * 64 + lane] = sum;
        }
        __syncthreads();
        if (on && lane == 0) {
            double sum = 0.0;
            for (int t = 0; t < ST_SEG; ++t) sum += ds[wv * 64 + t];
            part[((long long)b * Jp + s0 + sl) * 2 + 1] = sum;
        }
    }
}

__global__ void __launch_bounds__(256) k_stoi_finish(const long long *__restrict__ lens, long long n_all, const unsigned int *__restrict__ maxbits,
                                                     const int *__restrict__ kept, const double *__restrict__ part, int Jp,
                                                     fd_stoi *__restrict__ rec)
{
    __shared__ double sa[256], sb[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int F0 = st_frames(own_len(lens, b, n_all));
    const int K = kept[b], J = K - ST_SEG;
    fd_stoi r;
    r.stoi = r.estoi = quiet_nan();
    r.frames = F0; r.kept = K; r.segments = 0;
    r.status = F0 == 0 ? FD_STOI_SHORT : (maxbits[b] == 0u ? FD_STOI_SILENT : (J < 1 ? FD_STOI_SHORT : FD_STOI_OK));
    if (r.status != FD_STOI_OK) {
        if (tid == 0) rec[b] = r;
        return;
    }
    const double *__restrict__ p = part + (long long)b * Jp * 2;
    const int run = (J + 255) / 256;
    double a = 0.0, e = 0.0;
    for (int s = tid * run; s < J && s < (tid + 1) * run; ++s) { a += p[2 * s]; e += p[2 * s + 1]; }
    sa[tid] = a; sb[tid] = e;
    __syncthreads();
    if (tid != 0) return;
    a = 0.0; e = 0.0;
    for (int t = 0; t < 256; ++t) { a += sa[t]; e += sb[t]; }
    r.stoi = a / ((double)ST_BANDS * J);
    r.estoi = e / ((double)ST_SEG * J);
    r.segments = J;
    rec[b] = r;
}

// the scratch buffer: lengths [B], max words [B] + K [B], the two 10 kHz signals [B][pitch10] (only when resampled), energies [B][Fp],
// tile counts / offsets [B][nblk], src [B][Fp], band amplitudes [2][B][Mp][16], per-segment partials [B][Jp][2]
struct StLayout { size_t lens, words, x10, y10, E, blk, src, bands, part, total; long long pitch10; int F0, Fp, nblk, M, Mp, J, Jp; };
static StLayout st_layout(int B, int64_t n10, bool resampled)
{
    StLayout o;
    o.F0 = (int)fds::frames(n10);
    o.Fp = o.F0 > 0 ? o.F0 : 1;
    o.nblk = (o.Fp + ST_SCAN - 1) / ST_SCAN;
    o.M = o.F0 > 0 ? o.F0 - 1 : 0;
    o.Mp = o.M > 0 ? o.M : 1;
    o.J = (int)fds::segments(o.F0);
    o.Jp = o.J > 0 ? o.J : 1;
    o.pitch10 = resampled ? (long long)((n10 + 3) & ~(int64_t)3) : 0;
    Carve c;
    o.lens = c.take(sizeof(long long) * B);
    o.words = c.take(sizeof(int) * 2 * (size_t)B);
    o.x10 = c.take(sizeof(float) * (size_t)B * (size_t)o.pitch10);
    o.y10 = c.take(sizeof(float) * (size_t)B * (size_t)o.pitch10);
    o.E = c.take(sizeof(float) * (size_t)B * o.Fp);
    o.blk = c.take(sizeof(int) * (size_t)B * o.nblk);
    o.src = c.take(sizeof(int) * (size_t)B * o.Fp);
    o.bands = c.take(sizeof(float) * 32 * (size_t)B * o.Mp);
    o.part = c.take(sizeof(double) * 2 * (size_t)B * o.Jp);
    o.total = c.at;
    return o;
}

size_t stoi_scratch_bytes(int B, int64_t n10, bool resampled) { return st_layout(B, n10, resampled).total; }

StoiSlots stoi_slots(void *scratch, int B, int64_t n10, bool resampled)
{
    const StLayout o = st_layout(B, n10, resampled);
    char *base = static_cast<char *>(scratch);
    StoiSlots s;
    s.lens = reinterpret_cast<long long *>(base + o.lens);
    s.x10 = reinterpret_cast<float *>(base + o.x10);
    s.y10 = reinterpret_cast<float *>(base + o.y10);
    s.pitch10 = o.pitch10;
    return s;
}

hipError_t stoi(const Launch &La, const float *x, const float *y, long long pitch, int B, int64_t n10, const long long *lens_dev,
                const float *tab, const StoiBands &bd, fd_stoi *rec, void *scratch, bool resampled)
{
    const StLayout o = st_layout(B, n10, resampled);
    char *base = static_cast<char *>(scratch);
    unsigned int *maxbits = reinterpret_cast<unsigned int *>(base + o.words);
    int *kept = reinterpret_cast<int *>(base + o.words) + B;
    float *E = reinterpret_cast<float *>(base + o.E), *bands = reinterpret_cast<float *>(base + o.bands);
    int *blk = reinterpret_cast<int *>(base + o.blk), *src = reinterpret_cast<int *>(base + o.src);
    double *part = reinterpret_cast<double *>(base + o.part);
    hipError_t e = hipMemsetAsync(maxbits, 0, sizeof(int) * 2 * (size_t)B, La.stream);      // the max words and K
    if (e != hipSuccess) return e;
    const long long n_all = (long long)n10;
    if (o.F0 > 0) {
        FD_LAUNCH(La, "stoi_energy", k_stoi_energy, dim3((o.F0 + 3) / 4, B), dim3(256), 0, x, pitch, lens_dev, n_all, tab, E, o.Fp, maxbits);
        FD_LAUNCH(La, "stoi_count", k_stoi_count, dim3(o.nblk, B), dim3(256), 0, (const float *)E, o.Fp, lens_dev, n_all,
                  (const unsigned int *)maxbits, blk, o.nblk);
        FD_LAUNCH(La, "stoi_offsets", k_stoi_offsets, dim3(B), dim3(256), 0, lens_dev, n_all, blk, o.nblk, kept);
        FD_LAUNCH(La, "stoi_compact", k_stoi_compact, dim3(o.nblk, B), dim3(256), 0, (const float *)E, o.Fp, lens_dev, n_all,
                  (const unsigned int *)maxbits, (const int *)blk, o.nblk, src);
    }
    if (o.M > 0)
        FD_LAUNCH(La, "stoi_bands", k_stoi_bands, dim3(o.M, B, 2), dim3(256), 0, x, y, pitch, tab, (const int *)src, o.Fp, (const int *)kept, bd,
                  bands, B, o.Mp);
    if (o.J > 0)
        FD_LAUNCH(La, "stoi_segments", k_stoi_segments, dim3((o.J + ST_SEGS - 1) / ST_SEGS, B), dim3(256), 0, (const float *)bands, B, o.Mp,
                  (const int *)kept, part, o.Jp);
    FD_LAUNCH(La, "stoi_finish", k_stoi_finish, dim3(B), dim3(256), 0, lens_dev, n_all, (const unsigned int *)maxbits, (const int *)kept,
              (const double *)part, o.Jp, rec);
    return hipSuccess;
}

}  // namespace fdk
