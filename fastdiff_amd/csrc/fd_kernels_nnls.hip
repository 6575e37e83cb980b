// fd_kernels_nnls.hip -- the non-negative mel inversion on the device (include/fastdiff_hip_ext.h: fd_mel_to_linear_nnls, which defines
// the computation; the reference: vocoders/gl_mel.py:15-19 over librosa.util.nnls).  Host side: fd_nnls.h.
//
//   k_nnls<TACO>    grid (frame tiles of FD_NNLS_FRAME_TILE = 32, B), 256 threads = 4 waves, one launch for the whole solve.  A frame is
//                   a column of both matrix products, which run on v_mfma_f32_32x32x2_f32 (exact fp32, bit for bit an fmaf chain):
//                     g(mel) of the tile -> LDS; x_0 = max(0, P g) as k_mel_to_linear forms it -> y in LDS [520][32] (rows 513 .. 519
//                     stay zero) and into the registers of the lane that owns the element in the instruction's result layout;
//                     per iteration: wave w multiplies its fixed range of bin pairs of A (as the padded transpose AT [520][96]) with y
//                     -> four partial sums [80][32] in LDS, added in wave order, minus g -> r in LDS; wave w multiplies its bin tiles
//                     w, w + 4, ... of A (as AP [80][544]) with r and updates its own x and y.  The A operands of the next four
//                     pairs are fetched while the matrix pipe works on the current four, each product's first four during the
//                     phase before it.
//                   Then amp = max(1e-10, x) -> memory and LDS, and from those values in float64 per frame sum_j (A amp - g)_j^2,
//                   sum_j g_j^2 and the count of g that are not finite -> four doubles per frame.
//   k_nnls_finish   one workgroup per item: adds the frames as k_gl_finish does -> the record; an item with a g that is not finite
//                   has its amplitudes overwritten with the floor.
//
// Nothing of an item at or behind its own frames is read; a g that is not finite enters the solve as 0, so no NaN meets another frame's
// column.  No x, y, r or gradient reaches memory, every sum has a fixed order and there are no atomics.
#include "fd_internal.h"
#include "fd_kernels.h"
#include "fd_kernels_common.h"
#include "fd_nnls.h"

namespace fdk {

namespace {
constexpr int NM = fdn::MELS, NB = fdn::BINS, NT = fdn::TILE, NMP = fdn::MPAD, NBP = fdn::BPAD, NCH = fdn::CHUNK, NBT = fdn::MAX_BT;
constexpr float NNLS_FLOOR = 1e-10f;
using fdk_fast::mfma32;
using fdk_fast::drow;

__device__ __forceinline__ bool nn_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
template <bool TACO>
__device__ __forceinline__ float nn_g(float x) { return TACO ? expf(x) : exp10f(x); }
}
static_assert(sizeof(fd_nnls) == 32, "the size the header states");
static_assert(fdn::THREADS == 256 && NT == 32 && NBT == 5, "four waves, 32 frames per workgroup, at most five bin tiles per wave");

template <bool TACO>
__global__ void __launch_bounds__(256) k_nnls(const float *__restrict__ mel, const float *__restrict__ P, const float *__restrict__ tab, float step,
                                              const long long *__restrict__ lens, int T, int n_iters, float *__restrict__ amp,
                                              double *__restrict__ part)
{
    extern __shared__ double nn_lds_d[];                   // (double: the record pass keeps doubles in the partial sums' slot)
    float *const lds = reinterpret_cast<float *>(nn_lds_d);
    constexpr fdn::Lds O = fdn::lds();
    float *const ys = lds + O.y, *const ps = lds + O.part, *const rs = lds + O.r, *const gs = lds + O.g;
    const int b = blockIdx.y, t0 = blockIdx.x * NT, tid = threadIdx.x, lane = tid & 63, col = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6) & 3;
    const long long nfr = own_len(lens, b, T);
    float *__restrict__ ab = amp + (long long)b * NB * T;
    const int nt = T - t0 < NT ? T - t0 : NT;              // the tile's frames inside the batch's T ...
    const int nf = nfr - t0 < nt ? (int)(nfr - t0 < 0 ? 0 : nfr - t0) : nt;      // ... and of them the item's own
    if (nf <= 0) {                                         // (the whole workgroup) behind the item's own frames
        for (int i = tid; i < NB * NT; i += 256) {
            const int k = i >> 5, t = i & 31;
            if (t < nt) ab[(long long)k * T + t0 + t] = NNLS_FLOOR;
        }
        return;
    }
    const float *__restrict__ mb = mel + (long long)b * NM * T + t0;
    for (int i = tid; i < NM * NT; i += 256) {
        const int j = i >> 5, t = i & 31;
        float v = 0.0f;
        if (t < nf) {
            const float x = mb[(long long)j * T + t];
            v = nn_g<TACO>(x);
            if (!nn_finite(x) || !nn_finite(v)) v = 0.0f;  // counted by the record pass; the item is then NONFINITE
        }
        gs[i] = v;
    }
    for (int i = NB * NT + tid; i < fdn::YROWS * NT; i += 256) ys[i] = 0.0f;
    __syncthreads();
    {   // x_0, as k_mel_to_linear forms it
        const int tt = tid & 31, kq = tid >> 5;
        for (int k = kq; k < NB; k += 8) {
            const float *__restrict__ row = P + k * NM;
            float acc = 0.0f;
#pragma unroll 8
            for (int j = 0; j < NM; ++j) acc = fmaf(row[j], gs[j * NT + tt], acc);
            ys[k * NT + tt] = fmaxf(0.0f, acc);
        }
    }
    __syncthreads();
    constexpr fdn::Table TB = fdn::table();
    const float *__restrict__ AT = tab + TB.at, *__restrict__ AP = tab + TB.ap, *__restrict__ beta = tab + TB.beta;
    const bool five = wave == 0;                           // this wave's bin tiles are wave + 4 i, i < 4, and tile 16 for wave 0
#define NN_OWN(i) ((i) < NBT - 1 || five)
    float x[NBT][16];
#pragma unroll
    for (int i = 0; i < NBT; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int bin = 32 * (wave + 4 * i) + drow(v, hi);
            x[i][v] = (NN_OWN(i) && bin < NB) ? ys[bin * NT + col] : 0.0f;
        }
    const int kb = fdn::pair_begin(wave), ke = fdn::pair_begin(wave + 1);
    const float *__restrict__ at_l = AT + hi * NMP + col;          // pair kk, mel tile mt: at_l[2 kk NMP + 32 mt]
    const float *__restrict__ ap_l = AP + hi * NBP + 32 * wave + col;      // pair kk, own tile i: ap_l[2 kk NBP + 128 i]
    const float *ys_l = ys + hi * NT + col, *rs_l = rs + hi * NT + col;    // pair kk: [2 kk NT]
    float an1[NCH][fdn::MTILES], an2[NCH][NBT];            // the A operands of each product's first chunk, fetched a phase ahead
#pragma unroll
    for (int q = 0; q < NCH; ++q)
#pragma unroll
        for (int mt = 0; mt < fdn::MTILES; ++mt) an1[q][mt] = at_l[2 * (kb + q) * NMP + 32 * mt];
#pragma unroll 1
    for (int it = 0; it < n_iters; ++it) {
        {   // this wave's part of A y
            f32x16 c[fdn::MTILES];
#pragma unroll
            for (int mt = 0; mt < fdn::MTILES; ++mt)
#pragma unroll
                for (int v = 0; v < 16; ++v) c[mt][v] = 0.0f;
            float an[NCH][fdn::MTILES];
#pragma unroll
            for (int q = 0; q < NCH; ++q)
#pragma unroll
                for (int mt = 0; mt < fdn::MTILES; ++mt) an[q][mt] = an1[q][mt];
#pragma unroll 1
            for (int kk = kb; kk < ke; kk += NCH) {
                float a[NCH][fdn::MTILES], bv[NCH];
#pragma unroll
                for (int q = 0; q < NCH; ++q) {
                    bv[q] = ys_l[2 * (kk + q) * NT];
#pragma unroll
                    for (int mt = 0; mt < fdn::MTILES; ++mt) a[q][mt] = an[q][mt];
                }
                if (kk + NCH < ke) {
#pragma unroll
                    for (int q = 0; q < NCH; ++q)
#pragma unroll
                        for (int mt = 0; mt < fdn::MTILES; ++mt) an[q][mt] = at_l[2 * (kk + NCH + q) * NMP + 32 * mt];
                }
#pragma unroll
                for (int q = 0; q < NCH; ++q)
#pragma unroll
                    for (int mt = 0; mt < fdn::MTILES; ++mt) c[mt] = mfma32(a[q][mt], bv[q], c[mt]);
            }
#pragma unroll
            for (int q = 0; q < NCH; ++q)                  // the first chunk of A^T r: on its way during the exchange of the partial sums
#pragma unroll
                for (int i = 0; i < NBT; ++i) an2[q][i] = NN_OWN(i) ? ap_l[2 * q * NBP + 128 * i] : 0.0f;
#pragma unroll
            for (int mt = 0; mt < fdn::MTILES; ++mt)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int m = 32 * mt + drow(v, hi);
                    if (m < NM) ps[(wave * NM + m) * NT + col] = c[mt][v];
                }
        }
        __syncthreads();
        for (int i = tid; i < NM * NT; i += 256) {
            float s = __fadd_rn(ps[i], ps[NM * NT + i]);
            s = __fadd_rn(s, ps[2 * NM * NT + i]);
            s = __fadd_rn(s, ps[3 * NM * NT + i]);
            rs[i] = __fsub_rn(s, gs[i]);
        }
        __syncthreads();
        {   // A^T r on this wave's bin tiles, and the step
            f32x16 c[NBT];
#pragma unroll
            for (int i = 0; i < NBT; ++i)
#pragma unroll
                for (int v = 0; v < 16; ++v) c[i][v] = 0.0f;
            float an[NCH][NBT];
#pragma unroll
            for (int q = 0; q < NCH; ++q)
#pragma unroll
                for (int i = 0; i < NBT; ++i) an[q][i] = an2[q][i];
#pragma unroll 1
            for (int kk = 0; kk < NM / 2; kk += NCH) {
                float a[NCH][NBT], bv[NCH];
#pragma unroll
                for (int q = 0; q < NCH; ++q) {
                    bv[q] = rs_l[2 * (kk + q) * NT];
#pragma unroll
                    for (int i = 0; i < NBT; ++i) a[q][i] = an[q][i];
                }
                if (kk + NCH < NM / 2) {
#pragma unroll
                    for (int q = 0; q < NCH; ++q)
#pragma unroll
                        for (int i = 0; i < NBT; ++i)
                            if (NN_OWN(i)) an[q][i] = ap_l[2 * (kk + NCH + q) * NBP + 128 * i];
                }
#pragma unroll
                for (int q = 0; q < NCH; ++q)
#pragma unroll
                    for (int i = 0; i < NBT; ++i)
                        if (NN_OWN(i)) c[i] = mfma32(a[q][i], bv[q], c[i]);
            }
#pragma unroll
            for (int q = 0; q < NCH; ++q)                  // the first chunk of the next A y: on its way during the step
#pragma unroll
                for (int mt = 0; mt < fdn::MTILES; ++mt) an1[q][mt] = at_l[2 * (kb + q) * NMP + 32 * mt];
            const float be = beta[it];
#pragma unroll
            for (int i = 0; i < NBT; ++i)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int bin = 32 * (wave + 4 * i) + drow(v, hi);
                    if (NN_OWN(i) && bin < NB) {
                        const float xn = fmaxf(0.0f, fmaf(-step, c[i][v], ys[bin * NT + col]));
                        ys[bin * NT + col] = fmaf(be, __fsub_rn(xn, x[i][v]), xn);
                        x[i][v] = xn;
                    }
                }
        }
        __syncthreads();
    }
    // the amplitudes: to memory, and to LDS for the record pass
#pragma unroll
    for (int i = 0; i < NBT; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int bin = 32 * (wave + 4 * i) + drow(v, hi);
            if (NN_OWN(i) && bin < NB) {
                const float a = col < nf ? fmaxf(NNLS_FLOOR, x[i][v]) : NNLS_FLOOR;
                ys[bin * NT + col] = a;
                if (col < nt) ab[(long long)bin * T + t0 + col] = a;
            }
        }
    __syncthreads();
    double *const dd = reinterpret_cast<double *>(ps);     // [NM][NT]
    {
        const int mq = tid >> 5;
        for (int m = mq; m < NM; m += 8) {
            const float *__restrict__ arow = AP + m * NBP;
            double d = 0.0;
#pragma unroll 4
            for (int k = 0; k < NB; ++k) d = fma((double)arow[k], (double)ys[k * NT + col], d);
            d -= (double)gs[m * NT + col];
            dd[m * NT + col] = d * d;
        }
    }
    __syncthreads();
    if (tid < nf) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int m = 0; m < NM; ++m) {
            const double gv = (double)gs[m * NT + tid];
            s0 += dd[m * NT + tid];
            s1 += gv * gv;
            const float xm = mb[(long long)m * T + tid];
            s2 += (!nn_finite(xm) || !nn_finite(nn_g<TACO>(xm))) ? 1.0 : 0.0;
        }
        double *__restrict__ o = part + ((long long)b * T + t0 + tid) * 4;
        o[0] = s0; o[1] = s1; o[2] = s2; o[3] = 0.0;
    }
#undef NN_OWN
}

__global__ void __launch_bounds__(256) k_nnls_finish(const long long *__restrict__ lens, int T, int n_iters, const double *__restrict__ part,
                                                     float *__restrict__ amp, fd_nnls *__restrict__ rec)
{
    __shared__ double red[3][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long nfr = own_len(lens, b, T);
    const double *__restrict__ p = part + (long long)b * T * 4;
    double a[3] = {0.0, 0.0, 0.0};
    for (long long f = tid; f < nfr; f += 256) { a[0] += p[4 * f]; a[1] += p[4 * f + 1]; a[2] += p[4 * f + 2]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) red[k][tid] = a[k];
    __syncthreads();
    a[0] = a[1] = a[2] = 0.0;
    for (int t = 0; t < 256; ++t) { a[0] += red[0][t]; a[1] += red[1][t]; a[2] += red[2][t]; }      // (every thread: all need the status)
    const bool bad = nfr > 0 && a[2] != 0.0;
    if (bad) {
        float *__restrict__ ab = amp + (long long)b * NB * T;
        for (long long i = tid; i < (long long)NB * T; i += 256) ab[i] = NNLS_FLOOR;
    }
    if (tid != 0 || !rec) return;
    fd_nnls r;
    r.resid = r.norm = quiet_nan();
    r.frames = (int)nfr;
    r.iters = n_iters;
    r.reserved = 0;
    if (nfr <= 0) r.status = FD_NNLS_EMPTY;
    else if (bad) r.status = FD_NNLS_NONFINITE;
    else {
        r.status = FD_NNLS_OK;
        r.norm = sqrt(a[1]);
        r.resid = a[1] == 0.0 ? 0.0 : sqrt(a[0] / a[1]);
    }
    rec[b] = r;
}

size_t nnls_scratch_bytes(int B, int T) { return fdn::layout(B, T).total; }

long long *nnls_lens_slot(void *scratch) { return reinterpret_cast<long long *>(static_cast<char *>(scratch) + fdn::layout(1, 1).lens); }

hipError_t mel_to_linear_nnls(const Launch &La, const float *mel, int B, int T, const long long *lens_dev, const float *pinv_dev,
                              const float *tab_dev, float step, int variant, int n_iters, float *amp, fd_nnls *rec, void *scratch)
{
    double *part = reinterpret_cast<double *>(static_cast<char *>(scratch) + fdn::layout(B, T).part);
    const dim3 grid((unsigned)((T + NT - 1) / NT), (unsigned)B);
    const size_t shmem = sizeof(float) * fdn::lds().total;
    if (variant == FD_GL_TACOTRON) {
        const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void *>(k_nnls<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        if (ea != hipSuccess) return ea;
        FD_LAUNCH(La, "nnls_tacotron", k_nnls<true>, grid, dim3(256), shmem, mel, pinv_dev, tab_dev, step, lens_dev, T, n_iters, amp, part);
    } else {
        const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void *>(k_nnls<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        if (ea != hipSuccess) return ea;
        FD_LAUNCH(La, "nnls", k_nnls<false>, grid, dim3(256), shmem, mel, pinv_dev, tab_dev, step, lens_dev, T, n_iters, amp, part);
    }
    FD_LAUNCH(La, "nnls_finish", k_nnls_finish, dim3(B), dim3(256), 0, lens_dev, T, n_iters, (const double *)part, amp, rec);
    return hipSuccess;
}

}  // namespace fdk
