// fd_kernels_gl.hip -- Griffin-Lim on the device (include/fastdiff_hip_ext.h: fd_griffin_lim and fd_mel_to_linear, which define the
// computation; the reference: vocoders/gl_linear.py, vocoders/gl_mel.py over utils/audio.py:35-63 griffin_lim, :91-95 _mel_to_linear).
//
//   k_gl_transpose    grid (frame tiles of 32, B): the amplitudes [B][513][T] -> [B][T][AMP_PITCH] through an LDS tile, so that the
//                     iterations read a frame's 513 amplitudes in one piece.
//   k_gl_frames<MODE> grid (frame tiles of FD_GL_FRAME_TILE, B), one launch per iteration.  START: per frame C = A e^(i theta0) (the
//                     caller's angles or Philox) -> inverse transform -> window -> the synthesis frame f_t [1024] of frame buffer 0.
//                     ITER: the workgroup first forms ypad under its frames from the other frame buffer (the overlap-add of the last
//                     iteration: per sample the covering frames in ascending t, divided by the envelope) into LDS; then per frame:
//                     window, forward transform (fd_kernels_dft.h), C = A X / |X| into LDS, inverse transform, window -> f_t.
//                     MEASURE: the same load and forward transform, then in float64 (|X| - A)^2, A^2 and the count of amplitudes
//                     that are negative or not finite, each thread's bins in ascending order and a fixed tree over the 256 threads
//                     -> four doubles per frame.
//   k_gl_finish       one workgroup per item: thread t adds the frames t, t + 256, ... in ascending order, thread 0 the 256 sums in
//                     thread order -> the record.
//   k_gl_gather       the waveform, once: wav[b][j] = ypad[j + 512] from the last frame buffer, zeros behind L_b and for an item
//                     whose status is not OK.
//   k_mel_to_linear   grid (frame tiles of 64, B): g(mel) of the tile into LDS, then thread = (frame, bins kq, kq + 4, ...): the 80-term
//                     fmaf chain over the pseudo-inverse's row, and the floor.
//
// No spectrum and no angle reaches memory; every sum has a fixed order that depends on the item's own length alone and there are no
// atomics, so a waveform is bit-identical alone, anywhere in a ragged batch and from call to call.  Nothing of an item behind its own
// frames is read.
#include "fd_internal.h"
#include "fd_kernels.h"
#include "fd_kernels_common.h"
#include "fd_kernels_dft.h"
#include "fd_gl.h"

namespace fdk {

namespace {
constexpr int GN = fdgl::N, GHOP = fdgl::HOP, GBINS = fdgl::BINS, GPAD = fdgl::PAD, GTILE = fdgl::FRAME_TILE, GSEG = fdgl::SEG, GAP = fdgl::AMP_PITCH;
enum GlMode { GL_START = 0, GL_ITER = 1, GL_MEASURE = 2 };
}
static_assert(sizeof(fd_gl) == 32, "the size the header states");
static_assert(fdgl::THREADS == 256 && GN == 4 * 256 && GHOP == 256 && GSEG == 256 * (GTILE + 3), "256-thread workgroups; one quarter frame per pass over the threads");

__global__ void __launch_bounds__(256) k_gl_transpose(const float *__restrict__ amp, float *__restrict__ at, int T)
{
    __shared__ float tile[32][33];
    const int b = blockIdx.y, t0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float *__restrict__ a = amp + (long long)b * GBINS * T;
    float *__restrict__ o = at + (long long)b * T * GAP;
    for (int k0 = 0; k0 < GBINS; k0 += 32) {
        __syncthreads();                                   // the last tile has been read
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + ty + 8 * j, t = t0 + tx;
            if (k < GBINS && t < T) tile[ty + 8 * j][tx] = a[(long long)k * T + t];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = t0 + ty + 8 * j, k = k0 + tx;
            if (k < GBINS && t < T) o[(long long)t * GAP + k] = tile[tx][ty + 8 * j];
        }
    }
}

// negative (and not -0), infinite or NaN, read from the bits (the library is built without NaN-honouring comparisons)
__device__ __forceinline__ bool gl_bad(float a)
{
    const uint32_t u = __float_as_uint(a);
    return ((u & 0x7F800000u) == 0x7F800000u) || ((u >> 31) && (u << 1) != 0u);
}

// sums the three doubles of every thread in a fixed tree; the result is in red[q][0]
__device__ __forceinline__ void gl_reduce(double (*red)[256], int tid, const double *a)
{
#pragma unroll
    for (int q = 0; q < 3; ++q) red[q][tid] = a[q];
    for (int s = 128; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) {
#pragma unroll
            for (int q = 0; q < 3; ++q) red[q][tid] += red[q][tid + s];
        }
    }
    __syncthreads();
}

// ypad[m] of an item of nfr frames from its synthesis frames F [nfr][1024]: the covering frames in ascending t, over the envelope summed
// from the window's squares in the same order; zero outside [512, 512 + 256 (nfr - 1)).  win: the window (LDS or global).
__device__ __forceinline__ float gl_ypad(const float *__restrict__ F, const float *win, long long m, long long nfr)
{
    if (m < GPAD || m >= GPAD + GHOP * (nfr - 1)) return 0.0f;
    const long long q = m >> 8;                            // m = 256 q + r: the frames q - 3 .. q hold it at n = 256 (q - t) + r
    const int r = (int)(m & 255);
    float s = 0.0f, e = 0.0f;
#pragma unroll
    for (int d = GN / GHOP - 1; d >= 0; --d) {             // ascending t = q - d
        const long long t = q - d;
        if (t < 0 || t >= nfr) continue;
        const float w = win[256 * d + r];
        s = __fadd_rn(s, F[t * GN + 256 * d + r]);
        e = fmaf(w, w, e);
    }
    return __fdiv_rn(s, e);
}

template <int MODE>
__global__ void __launch_bounds__(256) k_gl_frames(const float *__restrict__ at, const float *__restrict__ angles, const float *__restrict__ Fin,
                                                   float *__restrict__ Fout, double *__restrict__ part, const long long *__restrict__ lens,
                                                   const unsigned long long *__restrict__ ids, const float *__restrict__ tab,
                                                   unsigned long long seed, int T)
{
    constexpr int N = GN, ROW = fdt::row(N);
    constexpr bool FWD = MODE != GL_START, INV = MODE != GL_MEASURE;
    __shared__ float ct[N], sn[N], wn[N], r1c[32], r1s[32];
    __shared__ float seg[FWD ? GSEG : 1], xw[FWD ? N : 1], ar[FWD ? 32 * ROW : 1], ai[FWD ? 32 * ROW : 1];
    __shared__ float cr[INV ? GBINS + 3 : 1], ci[INV ? GBINS + 3 : 1], er[INV ? 17 * 32 : 1], ei[INV ? 17 * 32 : 1];
    __shared__ double red[MODE == GL_MEASURE ? 3 : 1][256];
    const int b = blockIdx.y, tid = threadIdx.x, lo5 = tid & 31, g = tid >> 5;
    const long long nfr = own_len(lens, b, T);
    const long long t0 = (long long)blockIdx.x * GTILE;
    if (nfr < 2 || t0 >= nfr) return;                      // (the whole workgroup) SHORT, or behind the item's own frames
    const int nf = (int)(nfr - t0 < GTILE ? nfr - t0 : GTILE);
    for (int i = tid; i < N; i += 256) { ct[i] = tab[i]; sn[i] = tab[N + i]; wn[i] = tab[2 * N + i]; }
    if (tid < 32) { r1c[tid] = tab[32 * tid]; r1s[tid] = tab[N + 32 * tid]; }
    const long long item = (long long)b * T;
    if (FWD) {
        __syncthreads();                                   // the window is in
        const float *__restrict__ Fb = Fin + item * N;
        for (int q = 0; q < nf + 3; ++q) seg[256 * q + tid] = gl_ypad(Fb, wn, 256 * (t0 + q) + tid, nfr);
    }
    for (int fi = 0; fi < nf; ++fi) {
        const long long t = t0 + fi;
        const float *__restrict__ A = at + (item + t) * GAP;
        const int k2s[3] = {g, g + 8, 16};                 // this thread's bins lo5 + 32 k2: two below 512, and bin 512 (kept by thread 0)
        float re[3], im[3];
        __syncthreads();                                   // the tables and seg are in; the last frame's transforms have read xw, cr, ci, er, ei
        if (FWD) {
#pragma unroll
            for (int j = 0; j < 4; ++j) xw[256 * j + tid] = __fmul_rn(wn[256 * j + tid], seg[256 * (fi + j) + tid]);
            __syncthreads();
            dft_pass1<N>(xw, ct, sn, 0, 32, ar, ai, tid);
            __syncthreads();
            dft_pass2<N, 8>(ar, ai, ct, sn, lo5, k2s, re, im);
        }
        if (MODE == GL_MEASURE) {
            double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (j == 2 && tid != 0) break;
                const float a = A[lo5 + 32 * k2s[j]];
                const float mag = __fsqrt_rn(fmaf(im[j], im[j], __fmul_rn(re[j], re[j])));
                const double d = (double)mag - (double)a;
                acc[0] += d * d;
                acc[1] += (double)a * (double)a;
                acc[2] += gl_bad(a) ? 1.0 : 0.0;
            }
            gl_reduce(red, tid, acc);
            if (tid < 3) part[(item + t) * 4 + tid] = red[tid][0];
            continue;
        }
        if (INV) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (j == 2 && tid != 0) break;
                const int k = lo5 + 32 * k2s[j];
                const float a = A[k];
                float vr, vi;
                if (MODE == GL_START) {
                    float th;
                    if (angles) th = angles[((long long)b * GBINS + k) * T + t];
                    else {
                        uint32_t r[4];
                        const uint64_t pos = (uint64_t)t * fdgl::CALLS_PER_FRAME + (uint64_t)(k >> 2);      // fdgl::philox_counter
                        const unsigned long long id = ids ? ids[b] : (unsigned long long)b;
                        philox4x32_10((uint32_t)pos, (uint32_t)(pos >> 32) ^ (uint32_t)id, FD_GL_PHILOX_STREAM, 0x5EEDu ^ (uint32_t)(id >> 32), (uint32_t)seed,
                                      (uint32_t)(seed >> 32), r);
                        const int c = k & 3;
                        const uint32_t word = c == 0 ? r[0] : (c == 1 ? r[1] : (c == 2 ? r[2] : r[3]));
                        th = __fmul_rn(6.283185307179586f, __fmul_rn(__fadd_rn((float)(word >> 8), 0.5f), 1.0f / 16777216.0f));
                    }
                    float s_, c_;
                    sincosf(th, &s_, &c_);
                    vr = __fmul_rn(a, c_);
                    vi = __fmul_rn(a, s_);
                } else {
                    const float mag = __fsqrt_rn(fmaf(im[j], im[j], __fmul_rn(re[j], re[j])));
                    if (mag == 0.0f) { vr = a; vi = 0.0f; }      // np.angle(0) = 0
                    else {
                        const float s_ = __fdiv_rn(a, mag);
                        vr = __fmul_rn(re[j], s_);
                        vi = __fmul_rn(im[j], s_);
                    }
                }
                cr[k] = vr;
                ci[k] = (k == 0 || k == N / 2) ? 0.0f : vi;      // a C2R transform ignores them
            }
            __syncthreads();
            idft_pass1<N>(cr, ci, ct, sn, r1c, r1s, er, ei, tid);
            __syncthreads();
            const int n1s[4] = {g, g + 8, g + 16, g + 24};
            float x[4];
            idft_pass2<N>(er, ei, r1c, r1s, lo5, n1s, x);
            float *__restrict__ fo = Fout + (item + t) * N;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = 32 * n1s[q] + lo5;
                fo[n] = __fmul_rn(wn[n], x[q]);
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_gl_finish(const long long *__restrict__ lens, int T, int n_iters, const double *__restrict__ part,
                                                   fd_gl *__restrict__ rec)
{
    __shared__ double red[3][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long nfr = own_len(lens, b, T);
    const double *__restrict__ p = part + (long long)b * T * 4;
    double a[3] = {0.0, 0.0, 0.0};
    if (nfr >= 2)
        for (long long f = tid; f < nfr; f += fdgl::SUM_CHUNK) { a[0] += p[4 * f]; a[1] += p[4 * f + 1]; a[2] += p[4 * f + 2]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) red[k][tid] = a[k];
    __syncthreads();
    if (tid != 0) return;
    a[0] = a[1] = a[2] = 0.0;
    for (int t = 0; t < fdgl::SUM_CHUNK; ++t) { a[0] += red[0][t]; a[1] += red[1][t]; a[2] += red[2][t]; }
    fd_gl r;
    r.sc = r.norm = quiet_nan();
    r.frames = (int)nfr;
    r.samples = nfr < 2 ? 0 : (int)(GHOP * (nfr - 1));
    r.iters = n_iters;
    if (nfr < 2) r.status = FD_GL_SHORT;
    else if (a[2] != 0.0) r.status = FD_GL_NONFINITE;
    else {
        r.norm = sqrt(a[1]);
        if (a[1] == 0.0) r.status = FD_GL_SILENT;
        else { r.status = FD_GL_OK; r.sc = sqrt(a[0] / a[1]); }
    }
    rec[b] = r;
}

__global__ void __launch_bounds__(256) k_gl_gather(const float *__restrict__ F, const float *__restrict__ tab, const long long *__restrict__ lens,
                                                   const fd_gl *__restrict__ rec, int T, float *__restrict__ wav, long long pitch)
{
    const int b = blockIdx.y;
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x, L = (long long)GHOP * (T - 1);
    if (j >= L) return;
    const long long nfr = own_len(lens, b, T);
    float v = 0.0f;
    if (rec[b].status == FD_GL_OK) v = gl_ypad(F + (long long)b * T * GN, tab + 2 * GN, j + GPAD, nfr);
    wav[(long long)b * pitch + j] = v;
}

template <bool TACO>
__global__ void __launch_bounds__(256) k_mel_to_linear(const float *__restrict__ mel, const float *__restrict__ P, float *__restrict__ amp, int T)
{
    __shared__ float gm[fdgl::MELS][64];
    const int b = blockIdx.y, t0 = blockIdx.x * 64, tt = threadIdx.x & 63, kq = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < fdgl::MELS * 64; i += 256) {
        const int j = i >> 6, t = t0 + (i & 63);
        float v = 0.0f;
        if (t < T) {
            const float x = mel[((long long)b * fdgl::MELS + j) * T + t];
            v = TACO ? expf(x) : exp10f(x);
        }
        gm[j][i & 63] = v;
    }
    __syncthreads();
    if (t0 + tt >= T) return;
    for (int k = kq; k < GBINS; k += 4) {
        const float *__restrict__ row = P + k * fdgl::MELS;
        float acc = 0.0f;
#pragma unroll 8
        for (int j = 0; j < fdgl::MELS; ++j) acc = fmaf(row[j], gm[j][tt], acc);
        amp[((long long)b * GBINS + k) * T + t0 + tt] = fmaxf(1e-10f, acc);
    }
}

size_t gl_scratch_bytes(int B, int T) { return fdgl::layout(B, T).total; }

GlSlots gl_slots(void *scratch, int B, int T)
{
    const fdgl::Layout o = fdgl::layout(B, T);
    char *p = static_cast<char *>(scratch);
    return GlSlots{reinterpret_cast<long long *>(p + o.lens), reinterpret_cast<unsigned long long *>(p + o.ids)};
}

hipError_t griffin_lim(const Launch &La, const float *amp, const float *angles, int B, int T, const long long *lens_dev,
                       const unsigned long long *ids_dev, int n_iters, unsigned long long seed, const float *tab, float *wav, long long pitch,
                       fd_gl *rec, void *scratch)
{
    const fdgl::Layout o = fdgl::layout(B, T);
    char *p = static_cast<char *>(scratch);
    float *at = reinterpret_cast<float *>(p + o.amp);
    float *F[2] = {reinterpret_cast<float *>(p + o.frames[0]), reinterpret_cast<float *>(p + o.frames[1])};
    double *part = reinterpret_cast<double *>(p + o.part);
    const dim3 grid((unsigned)((T + GTILE - 1) / GTILE), (unsigned)B);
    FD_LAUNCH(La, "gl_transpose", k_gl_transpose, dim3((unsigned)((T + 31) / 32), (unsigned)B), dim3(256), 0, amp, at, T);
    FD_LAUNCH(La, "gl_start", k_gl_frames<GL_START>, grid, dim3(256), 0, (const float *)at, angles, (const float *)nullptr, F[0], part, lens_dev, ids_dev, tab,
              seed, T);
    int cur = 0;
    for (int i = 0; i < n_iters; ++i, cur ^= 1)
        FD_LAUNCH(La, "gl_iter", k_gl_frames<GL_ITER>, grid, dim3(256), 0, (const float *)at, (const float *)nullptr, (const float *)F[cur], F[cur ^ 1], part,
                  lens_dev, ids_dev, tab, seed, T);
    FD_LAUNCH(La, "gl_measure", k_gl_frames<GL_MEASURE>, grid, dim3(256), 0, (const float *)at, (const float *)nullptr, (const float *)F[cur], (float *)nullptr,
              part, lens_dev, ids_dev, tab, seed, T);
    FD_LAUNCH(La, "gl_finish", k_gl_finish, dim3(B), dim3(256), 0, lens_dev, T, n_iters, (const double *)part, rec);
    FD_LAUNCH(La, "gl_gather", k_gl_gather, dim3((unsigned)(((long long)GHOP * (T - 1) + 255) / 256), (unsigned)B), dim3(256), 0, (const float *)F[cur], tab,
              lens_dev, (const fd_gl *)rec, T, wav, pitch);
    return hipSuccess;
}

hipError_t mel_to_linear(const Launch &La, const float *mel, int B, int T, const float *pinv_dev, int variant, float *amp)
{
    const dim3 grid((unsigned)((T + 63) / 64), (unsigned)B);
    if (variant == FD_GL_TACOTRON) FD_LAUNCH(La, "mel_to_linear_tacotron", k_mel_to_linear<true>, grid, dim3(256), 0, mel, pinv_dev, amp, T);
    else FD_LAUNCH(La, "mel_to_linear", k_mel_to_linear<false>, grid, dim3(256), 0, mel, pinv_dev, amp, T);
    return hipSuccess;
}

}  // namespace fdk
