// fd_kernels_spectral.hip -- the multi-resolution STFT distances on the device (include/fastdiff_hip_ext.h: fd_spectral_measure, which
// defines the measurement): spectral convergence, log-magnitude distance and log-spectral distance of a vocoded waveform against its
// recording at up to four (nfft, hop, win), with torch.stft's conventions (center, reflect padding, periodic Hann window).  The reference
// has no code for it (modules/parallel_wavegan comes without its STFT loss, utils/torch_stft.py without a caller).
//
//   k_spectral_frames<nfft>     grid (frame tiles, B), one launch per resolution: SP_TILE consecutive frames of one pair per workgroup, one
//                     after the other; per frame x, then y, through the same code: the win samples under the window (reflected at the
//                     pair's own ends) times the window into LDS, then the nfft-point transform of fd_kernels_dft.h: pass 1 over the
//                     n1 that can lie under the window only; pass 2: thread = bins tid, tid + 256, ... < nfft / 2 (the same k1, so one
//                     call), thread 0 also the bin nfft / 2.  The power of x at a bin waits in a register for the power of y; then in
//                     float64 the floor, X - Y and d = (ln Px - ln Py) / 2, the thread's bins in ascending order, and a fixed tree over
//                     the 256 threads -> four doubles per frame in the scratch: sum (X - Y)^2, sum X^2, sum |d|, sum d^2.
//   k_spectral_finish one workgroup per pair: per resolution thread t adds the frames t, t + 256, ... in ascending order (sum d^2 after
//                     the root of its mean over the bins), thread 0 the 256 sums in thread order -> the 144-byte record.
//
// Every sum has a fixed order that depends on the pair's own length and the configuration alone and there are no floating-point atomics,
// so a record is bit-identical alone, anywhere in a ragged batch, at any row pitch and from call to call; x and y take the same path, so
// a copy scores exactly 0.  Nothing at or behind a pair's own length is read.
#include "fd_internal.h"
#include "fd_kernels.h"
#include "fd_kernels_common.h"
#include "fd_kernels_dft.h"

namespace fdk {

constexpr int SP_TILE = fdx::FRAME_TILE, SP_CHUNK = fdx::SUM_CHUNK, SP_RES = fdx::MAX_RES;
static_assert(SP_TILE == FD_SPECTRAL_FRAME_TILE && SP_CHUNK == FD_SPECTRAL_SUM_CHUNK && SP_RES == FD_SPECTRAL_MAX_RES, "the exported constants are the kernels'");
static_assert(fdx::THREADS == 256 && SP_CHUNK == 256, "256-thread workgroups throughout");
static_assert(sizeof(fd_spectral) == 144 && sizeof(fd_spectral_config) == 64, "the sizes the header states");
static_assert(fdx::lds_bytes(2048) <= fdx::LDS_WORKGROUP_MAX && fdx::lds_bytes(1024) <= fdx::LDS_WORKGROUP_MAX && fdx::lds_bytes(512) <= fdx::LDS_WORKGROUP_MAX,
              "a transform workgroup's LDS");

// sums the four doubles of every thread in a fixed tree; the result is in red[q][0]
__device__ __forceinline__ void sp_reduce(double (*red)[256], int tid, const double *a)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) red[q][tid] = a[q];
    for (int s = 128; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) {
#pragma unroll
            for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + s];
        }
    }
    __syncthreads();
}

// one bin: the powers of x and y -> the four sums
__device__ __forceinline__ void sp_bin(double *acc, float px, float py, double floor_)
{
    const double a = (double)px, c = (double)py;
    const double pa = a > floor_ ? a : floor_, pc = c > floor_ ? c : floor_;
    const double dm = sqrt(pa) - sqrt(pc), d = 0.5 * (log(pa) - log(pc));
    acc[0] += dm * dm;
    acc[1] += pa;
    acc[2] += fabs(d);
    acc[3] += d * d;
}

template <int N>
__global__ void __launch_bounds__(256) k_spectral_frames(const float *__restrict__ x, const float *__restrict__ y, long long pitch,
                                                         const long long *__restrict__ lens, long long n_all, const float *__restrict__ tab,
                                                         int hop, int win, int short_n, double floor_, double *__restrict__ part, int Fp)
{
    constexpr int N1 = fdt::split_n1(N), N2 = fdt::split_n2(N), ROW = fdt::row(N);
    constexpr int J = N / 512, K2S = 256 / N1;             // pass 2: thread = bins tid + 256 j, j < J
    static_assert(256 % N1 == 0 && J >= 1, "whole bins per thread");
    __shared__ float ct[N], sn[N], xw[N], ar[N2 * ROW], ai[N2 * ROW];
    __shared__ double red[4][256];
    static_assert(sizeof(float) * (3 * N + 2 * N2 * ROW) + sizeof(double) * 4 * 256 == fdx::lds_bytes(N), "fd_spectral.h states this workgroup's LDS");
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long n = own_len(lens, b, n_all);
    if (n <= short_n) return;                              // (the whole workgroup) SHORT: the reflection is undefined
    const long long F = 1 + n / hop;
    const long long f0 = (long long)blockIdx.x * SP_TILE;
    if (f0 >= F) return;                                   // (the whole workgroup) behind the pair's own frames
    for (int i = tid; i < N; i += 256) { ct[i] = tab[N + i]; sn[i] = tab[2 * N + i]; }
    const int off = (N - win) / 2;
    const int n1_lo = off / N2, n1_hi = (off + win - 1) / N2 + 1;
    const float *__restrict__ xb = x + (long long)b * pitch, *__restrict__ yb = y + (long long)b * pitch;
    for (int fi = 0; fi < SP_TILE && f0 + fi < F; ++fi) {
        const long long f = f0 + fi, start = f * hop - N / 2;      // f hop <= n
        float px[J], pn = 0.0f;                            // the powers of x at this thread's bins (pn: bin N / 2, thread 0)
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int sig = 0; sig < 2; ++sig) {
            const float *__restrict__ s = sig ? yb : xb;
            __syncthreads();                               // the tables are in; the last transform has read xw, ar, ai
            for (int i = tid; i < N; i += 256) {
                float v = 0.0f;
                if (i >= off && i < off + win) {           // n > N / 2: -p <= N / 2 <= n - 1, and 2 (n - 1) - p >= n - 1 - N / 2 >= 0
                    long long p = start + i;
                    p = p < 0 ? -p : (p >= n ? 2 * (n - 1) - p : p);
                    v = __fmul_rn(tab[i], s[p]);
                }
                xw[i] = v;
            }
            __syncthreads();
            dft_pass1<N>(xw, ct, sn, n1_lo, n1_hi, ar, ai, tid);
            __syncthreads();
            float pw[J], pwn = 0.0f;
            {   // this thread's bins tid + 256 j: k1 = tid % N1, k2 = tid / N1 + K2S j
                int k2[J];
                float re[J], im[J];
#pragma unroll
                for (int j = 0; j < J; ++j) k2[j] = tid / N1 + K2S * j;
                dft_pass2<N>(ar, ai, ct, sn, tid % N1, k2, re, im);
#pragma unroll
                for (int j = 0; j < J; ++j) pw[j] = fmaf(re[j], re[j], im[j] * im[j]);
                if (tid == 0) {                            // bin N / 2: k1 = 0, k2 = N2 / 2
                    const int kn[1] = {N2 / 2};
                    float rn[1], in[1];
                    // (one wavefront while three wait; unrolled by 32 at N2 = 64 the 2048-point kernel is 2 % slower, LABBOOK R25.1)
                    dft_pass2<N, (N2 == 32 ? 32 : 8)>(ar, ai, ct, sn, 0, kn, rn, in);
                    pwn = fmaf(rn[0], rn[0], in[0] * in[0]);
                }
            }
            if (sig == 0) {
#pragma unroll
                for (int j = 0; j < J; ++j) px[j] = pw[j];
                pn = pwn;
                continue;
            }
#pragma unroll
            for (int j = 0; j < J; ++j) sp_bin(acc, px[j], pw[j], floor_);
            if (tid == 0) sp_bin(acc, pn, pwn, floor_);
        }
        sp_reduce(red, tid, acc);
        if (tid < 4) part[((long long)b * Fp + f) * 4 + tid] = red[tid][0];
    }
}

struct SpectralPlan { int n_res, short_n; int nfft[SP_RES], hop[SP_RES], Fp[SP_RES]; long long at[SP_RES]; };      // at: the resolution's partials, in doubles

__global__ void __launch_bounds__(256) k_spectral_finish(const long long *__restrict__ lens, long long n_all, SpectralPlan pl,
                                                         const double *__restrict__ part, fd_spectral *__restrict__ rec)
{
    __shared__ double red[4][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long n = own_len(lens, b, n_all);
    const bool ok = n > pl.short_n;
    fd_spectral r;
    r.mr_sc = r.mr_logmag = r.lsd_db = quiet_nan();
    r.n_res = pl.n_res;
    r.status = ok ? FD_SPECTRAL_OK : FD_SPECTRAL_SHORT;
    double m_sc = 0.0, m_lm = 0.0, m_lsd = 0.0;
    for (int q = 0; q < SP_RES; ++q) {                     // (every thread passes every barrier)
        r.sc[q] = r.logmag[q] = r.lsd[q] = quiet_nan();
        r.frames[q] = 0;
        if (q >= pl.n_res) continue;
        const long long F = 1 + n / pl.hop[q];
        r.frames[q] = (int)F;
        if (!ok) continue;
        const double bins = (double)(pl.nfft[q] / 2 + 1);
        const double *__restrict__ p = part + pl.at[q] + (long long)b * pl.Fp[q] * 4;
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        for (long long f = tid; f < F; f += SP_CHUNK) {
            a[0] += p[4 * f]; a[1] += p[4 * f + 1]; a[2] += p[4 * f + 2];
            a[3] += sqrt(p[4 * f + 3] / bins);
        }
        __syncthreads();                                   // the last resolution's sums have been read
#pragma unroll
        for (int k = 0; k < 4; ++k) red[k][tid] = a[k];
        __syncthreads();
        if (tid != 0) continue;
        a[0] = a[1] = a[2] = a[3] = 0.0;
        for (int t = 0; t < SP_CHUNK; ++t) { a[0] += red[0][t]; a[1] += red[1][t]; a[2] += red[2][t]; a[3] += red[3][t]; }
        r.sc[q] = sqrt(a[0] / a[1]);
        r.logmag[q] = a[2] / ((double)F * bins);
        r.lsd[q] = 8.685889638065037 * a[3] / (double)F;      // 20 / ln 10
        m_sc += r.sc[q]; m_lm += r.logmag[q]; m_lsd += r.lsd[q];
    }
    if (tid != 0) return;
    if (ok) { r.mr_sc = m_sc / pl.n_res; r.mr_logmag = m_lm / pl.n_res; r.lsd_db = m_lsd / pl.n_res; }
    rec[b] = r;
}

// the scratch buffer: lengths [B], then per resolution the frame partials [B][Fp][4] doubles
struct SpLayout { size_t lens, part[SP_RES], total; int Fp[SP_RES]; };
static SpLayout sp_layout(int B, int64_t L, const fd_spectral_config &c)
{
    SpLayout o{};
    Carve cv;
    o.lens = cv.take(sizeof(long long) * (size_t)B);
    for (int r = 0; r < c.n_res; ++r) {
        o.Fp[r] = (int)fdx::frames(L, c.hop[r]);
        o.part[r] = cv.take(sizeof(double) * 4 * (size_t)B * (size_t)o.Fp[r]);
    }
    o.total = cv.at;
    return o;
}

size_t spectral_scratch_bytes(int B, int64_t L, const fd_spectral_config &c) { return sp_layout(B, L, c).total; }

long long *spectral_lens_slot(void *scratch) { return static_cast<long long *>(scratch); }

hipError_t spectral(const Launch &La, const float *x, const float *y, long long pitch, int B, int64_t L, const long long *lens_dev,
                    const fd_spectral_config &c, const float *const *tabs, fd_spectral *rec, void *scratch)
{
    const SpLayout o = sp_layout(B, L, c);
    double *base = reinterpret_cast<double *>(scratch);
    SpectralPlan pl{};
    pl.n_res = c.n_res;
    pl.short_n = fdx::short_len(c);
    const long long n_all = (long long)L;
    for (int r = 0; r < c.n_res; ++r) {
        pl.nfft[r] = c.nfft[r]; pl.hop[r] = c.hop[r]; pl.Fp[r] = o.Fp[r];
        pl.at[r] = (long long)(o.part[r] / sizeof(double));
        if (L <= pl.short_n) continue;                     // every pair is SHORT: nothing to transform
        const dim3 grid((unsigned)((o.Fp[r] + SP_TILE - 1) / SP_TILE), (unsigned)B);
        double *part = base + pl.at[r];
        switch (c.nfft[r]) {
        case 512:
            FD_LAUNCH(La, "spectral_frames_512", k_spectral_frames<512>, grid, dim3(256), 0, x, y, pitch, lens_dev, n_all, tabs[r], c.hop[r], c.win[r],
                      pl.short_n, c.floor, part, o.Fp[r]);
            break;
        case 1024:
            FD_LAUNCH(La, "spectral_frames_1024", k_spectral_frames<1024>, grid, dim3(256), 0, x, y, pitch, lens_dev, n_all, tabs[r], c.hop[r], c.win[r],
                      pl.short_n, c.floor, part, o.Fp[r]);
            break;
        default:
            FD_LAUNCH(La, "spectral_frames_2048", k_spectral_frames<2048>, grid, dim3(256), 0, x, y, pitch, lens_dev, n_all, tabs[r], c.hop[r], c.win[r],
                      pl.short_n, c.floor, part, o.Fp[r]);
            break;
        }
    }
    FD_LAUNCH(La, "spectral_finish", k_spectral_finish, dim3(B), dim3(256), 0, lens_dev, n_all, pl, (const double *)base, rec);
    return hipSuccess;
}

}  // namespace fdk
