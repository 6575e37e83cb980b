// fd_kernels_bins.hip -- one pass of Lloyd's algorithm over a flat [N][D] feature matrix (include/fastdiff_hip_ext.h: fd_bins_pass, which
// defines the computation; NDB / JSD of Richardson & Weiss 2018 are built on it in fastdiff_amd/diversity.py).  Host side: fd_bins.h.
//
//   k_bins_pass<KT, NT>   grid = chunks of FD_BINS_CHUNK = 4096 consecutive rows, 256 threads = 4 waves.  The centroids [K][D], their
//                         halved squared norms h, shift and scale stay in LDS for the whole chunk.  Per block of 128 rows:
//                           the rows -> LDS, standardised as they are loaded (plain 4-byte loads: any alignment, any ld); a row with a z
//                           that is not finite is zeroed there and marked;
//                           wave w forms dot[k][row] for its 32 rows against all centroids on v_mfma_f32_32x32x2_f32 (exact fp32, bit
//                           for bit an fmaf chain in ascending d), s = h - dot, the argmin over k in ascending k per lane and between
//                           the two lanes that share a row -> assign (LDS and assign_io), the bin counts (LDS integer adds), moved;
//                           UPDATE: one-hot(assign)^T Z on the same instruction, the K x D tiles dealt to the waves, accumulated in
//                           registers over the whole chunk in ascending row order;
//                           two threads per row add (z_d - c_kd)^2 in float64 over the two halves of d.
//                         Then the chunk's sums [K][D], counts, inertia, moved and nonfinite -> scratch.
//   k_bins_update         one workgroup per bin: the chunks' sums added in ascending chunk order in float64, divided by the count.
//   k_bins_record         one workgroup: the record.
//
// Nothing at or behind x + (N - 1) ld + D is read, no row's padding (d >= D) either.  Every sum has a fixed order that depends on the row's
// position alone; the only atomics are integer adds in LDS.
#include "fd_internal.h"
#include "fd_kernels.h"
#include "fd_kernels_common.h"
#include "fd_bins.h"

namespace fdk {

namespace {
constexpr int BC = fdb::CHUNK, BB = fdb::BLOCK;
using fdk_fast::mfma32;
using fdk_fast::drow;

__device__ __forceinline__ bool bn_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
}
static_assert(sizeof(fd_bins) == 1056, "the size the header states");
static_assert(fdb::THREADS == 256 && BB == 128, "four waves of 32 rows");

// KT: matrix tiles of 32 bins; NT: tiles of the update per wave, ceil(KT * tiles(D) / 4), 0 = no update.  Two workgroups per CU where the
// LDS allows (K = 50, D = 80: 68 KB): one loads its next rows while the other multiplies.
template <int KT, int NT>
__global__ void __launch_bounds__(256, 2) k_bins_pass(const float *__restrict__ x, long long N, int D, long long ld, const float *__restrict__ shift,
                                                   const float *__restrict__ scale, const float *__restrict__ cent, int K, int *__restrict__ assign_io,
                                                   float *__restrict__ sums, int *__restrict__ counts, double *__restrict__ inertia,
                                                   int *__restrict__ moved, int *__restrict__ nonfinite)
{
    extern __shared__ double bn_lds_d[];
    double *const red = bn_lds_d;                          // [256]
    float *const hs = reinterpret_cast<float *>(red + 256), *const sh = hs + 128, *const sc = sh + 128;
    int *const asg = reinterpret_cast<int *>(sc + 128), *const bad = asg + BB, *const cnt = bad + BB, *const misc = cnt + 128;
    constexpr bool UPDATE = NT > 0;
    constexpr int NU = UPDATE ? NT : 1;
    const int DT = (D + 31) >> 5, DS = fdb::zstride(D);
    float *const cs = reinterpret_cast<float *>(misc + 4), *const zs = cs + 32 * KT * DS;
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6) & 3;
    const long long chunk = blockIdx.x, c0 = chunk * BC;
    const int nrows = N - c0 < BC ? (int)(N - c0) : BC;

    for (int i = tid; i < 32 * KT * DS; i += 256) {
        const int k = i / DS, d = i - k * DS;
        cs[i] = (k < K && d < D) ? cent[k * D + d] : 0.0f;
    }
    if (tid < 128) {
        sh[tid] = (shift && tid < D) ? shift[tid] : 0.0f;
        sc[tid] = (scale && tid < D) ? scale[tid] : 1.0f;
        asg[tid] = -2;
        bad[tid] = 0;
        cnt[tid] = 0;
    }
    if (tid < 4) misc[tid] = 0;                            // [0] a row of the block is marked, [1] rows that are not finite, [2] moved
    __syncthreads();
    if (tid < 128) {
        float a = 0.0f;
        if (tid < K)
            for (int d = 0; d < D; ++d) a = fmaf(cs[tid * DS + d], cs[tid * DS + d], a);
        hs[tid] = __fmul_rn(0.5f, a);
    }
    // element tid + 256 j of a block, j < D / 2, is (row, d): the same walk in every block
    const int row0 = tid / D, d0 = tid - row0 * D, qr = 256 / D, qd = 256 - qr * D;
    const long long step = qr * ld + qd;
    // the tiles of the update this wave owns: t = wave + 4 i < KT * DT, bins 32 (t / DT) .., features 32 (t % DT) ..; a wave with fewer
    // than NT multiplies a one-hot operand that never matches (the busiest wave sets the time)
    int tk[NU], td[NU];
#pragma unroll
    for (int i = 0; i < NU; ++i) {
        const int t = wave + 4 * i;
        tk[i] = t < KT * DT ? 32 * (t / DT) : -4096;
        td[i] = t < KT * DT ? 32 * (t % DT) : 0;
    }
    f32x16 U[NU];
#pragma unroll
    for (int i = 0; i < NU; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) U[i][v] = 0.0f;
    double my_inertia = 0.0;
    int my_moved = 0;
    __syncthreads();

#pragma unroll 1
    for (int r0 = 0; r0 < nrows; r0 += BB) {
        const int nr = nrows - r0 < BB ? nrows - r0 : BB;
        const float *__restrict__ xb = x + (c0 + r0) * ld;
        if (nr == BB) {                                    // a whole block: eight loads in flight per thread, then their eight results
            const int J = D >> 1;
            int row = row0, d = d0;
            long long off = (long long)row0 * ld + d0;
#pragma unroll 1
            for (int j0 = 0; j0 < J; j0 += 8) {
                float xv[8];
                int at[8], dc[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    xv[u] = xb[off];
                    at[u] = row * DS + d;
                    dc[u] = d;
                    if (j0 + u + 1 < J) {                  // (behind the last element: stay on it)
                        d += qd; row += qr; off += step;
                        if (d >= D) { d -= D; ++row; off += ld - D; }
                    }
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (j0 + u < J) {
                        const float z = __fmul_rn(__fsub_rn(xv[u], sh[dc[u]]), sc[dc[u]]);
                        if (!bn_finite(xv[u]) || !bn_finite(z)) { bad[at[u] / DS] = 1; misc[0] = 1; }
                        zs[at[u]] = z;
                    }
            }
        } else {
            int row = row0, d = d0;
#pragma unroll 4
            for (int j = 0; j < D / 2; ++j) {
                float z = 0.0f;
                if (row < nr) {
                    const float xv = xb[(long long)row * ld + d];
                    z = __fmul_rn(__fsub_rn(xv, sh[d]), sc[d]);
                    // (on the loaded value as well: the library is built with -fno-honor-nans, under which a test of the computed z sees an overflow but no NaN)
                    if (!bn_finite(xv) || !bn_finite(z)) { bad[row] = 1; misc[0] = 1; }
                }
                zs[row * DS + d] = z;
                d += qd; row += qr;
                if (d >= D) { d -= D; ++row; }
            }
        }
        __syncthreads();
        if (misc[0]) {                                     // (the whole workgroup) a marked row is zeroed: 0 * NaN would reach the other rows' sums
            int row = row0, d = d0;
            for (int j = 0; j < D / 2; ++j) {
                if (bad[row]) zs[row * DS + d] = 0.0f;
                d += qd; row += qr;
                if (d >= D) { d -= D; ++row; }
            }
            __syncthreads();
        }
        {   // this wave's 32 rows against every centroid
            f32x16 acc[KT];
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[kt][v] = 0.0f;
            const float *zb = zs + (32 * wave + col) * DS + hi, *cb = cs + col * DS + hi;
            // four features (two instructions per tile) per turn, the operands of the next turn on their way (D is a multiple of 4)
            float b0 = zb[0], b1 = zb[2], a0[KT], a1[KT];
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) { a0[kt] = cb[32 * kt * DS]; a1[kt] = cb[32 * kt * DS + 2]; }
#pragma unroll 1
            for (int dd = 0; dd < D; dd += 4) {
                const int nd = dd + 4 < D ? dd + 4 : dd;
                const float nb0 = zb[nd], nb1 = zb[nd + 2];
                float na0[KT], na1[KT];
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) { na0[kt] = cb[32 * kt * DS + nd]; na1[kt] = cb[32 * kt * DS + nd + 2]; }
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) acc[kt] = mfma32(a0[kt], b0, acc[kt]);
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) acc[kt] = mfma32(a1[kt], b1, acc[kt]);
                b0 = nb0; b1 = nb1;
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) { a0[kt] = na0[kt]; a1[kt] = na1[kt]; }
            }
            float best = __int_as_float(0x7F800000);
            int bk = 0;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int k = 32 * kt + drow(v, hi);
                    const float s = __fsub_rn(hs[k], acc[kt][v]);
                    if (k < K && s < best) { best = s; bk = k; }
                }
            const float ob = __shfl_xor(best, 32);
            const int ok = __shfl_xor(bk, 32);
            if (ob < best || (ob == best && ok < bk)) bk = ok;
            const int r = 32 * wave + col;
            if (hi == 0) {
                int a = -2;
                if (r < nr) {
                    if (bad[r]) { a = -1; bad[r] = 0; atomicAdd(&misc[1], 1); }
                    else { a = bk; atomicAdd(&cnt[bk], 1); }
                    if (assign_io) {
                        my_moved += assign_io[c0 + r0 + r] != a;
                        assign_io[c0 + r0 + r] = a;
                    }
                }
                asg[r] = a;
            }
        }
        __syncthreads();
        if (tid == 0) misc[0] = 0;
        if (UPDATE) {
            // four rows (two instructions per tile) per turn, the operands of the next turn on their way; rows at and behind nr are
            // zero and match no bin
            const int n4 = (nr + 3) & ~3;
            const int *ar = asg + hi;
            const float *zr = zs + hi * DS + col;
            int a0 = ar[0], a1 = ar[2];
            float b0[NU], b1[NU];
#pragma unroll
            for (int i = 0; i < NU; ++i) { b0[i] = zr[td[i]]; b1[i] = zr[2 * DS + td[i]]; }
#pragma unroll 1
            for (int r = 0; r < n4; r += 4) {
                const int nx = r + 4 < n4 ? r + 4 : r;
                const int na0 = ar[nx], na1 = ar[nx + 2];
                float nb0[NU], nb1[NU];
#pragma unroll
                for (int i = 0; i < NU; ++i) { nb0[i] = zr[nx * DS + td[i]]; nb1[i] = zr[(nx + 2) * DS + td[i]]; }
#pragma unroll
                for (int i = 0; i < NU; ++i) U[i] = mfma32(a0 == tk[i] + col ? 1.0f : 0.0f, b0[i], U[i]);
#pragma unroll
                for (int i = 0; i < NU; ++i) U[i] = mfma32(a1 == tk[i] + col ? 1.0f : 0.0f, b1[i], U[i]);
                a0 = na0; a1 = na1;
#pragma unroll
                for (int i = 0; i < NU; ++i) { b0[i] = nb0[i]; b1[i] = nb1[i]; }
            }
        }
        {
            const int row = tid >> 1, k = asg[row], half = D >> 1;
            if (k >= 0) {
                const float *zr = zs + row * DS + (tid & 1) * half, *cr = cs + k * DS + (tid & 1) * half;
                double s = 0.0;
#pragma unroll 4
                for (int d = 0; d < half; ++d) {
                    const double t = (double)zr[d] - (double)cr[d];
                    s = fma(t, t, s);
                }
                my_inertia += s;
            }
        }
        __syncthreads();
    }
    if (UPDATE) {
        float *__restrict__ so = sums + (size_t)chunk * K * D;
#pragma unroll
        for (int i = 0; i < NU; ++i)
            if (tk[i] >= 0) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int k = tk[i] + drow(v, hi), d = td[i] + col;
                    if (k < K && d < D) so[k * D + d] = U[i][v];
                }
            }
    }
    red[tid] = my_inertia;
    if (my_moved) atomicAdd(&misc[2], my_moved);
    __syncthreads();
    if (tid < 128) counts[chunk * 128 + tid] = cnt[tid];
    if (tid == 0) {
        double s = 0.0;
        for (int t = 0; t < 256; ++t) s += red[t];
        inertia[chunk] = s;
        moved[chunk] = misc[2];
        nonfinite[chunk] = misc[1];
    }
}

// sum_c p[c * stride], c ascending, in A; sixteen loads in flight (the adds stay one chain in that order)
template <class A, class T>
__device__ __forceinline__ A bn_chain(const T *__restrict__ p, size_t stride, long long n)
{
    A s = 0;
    long long c = 0;
    for (; c + 16 <= n; c += 16) {
        T v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = p[(size_t)(c + u) * stride];
#pragma unroll
        for (int u = 0; u < 16; ++u) s += (A)v[u];
    }
    for (; c < n; ++c) s += (A)p[(size_t)c * stride];
    return s;
}

// bin b = blockIdx.x: centroids_out[b][d] = (float)(S_bd / counts[b]), S the chunks' sums in ascending chunk order; an empty bin keeps its centroid
__global__ void __launch_bounds__(128) k_bins_update(const float *__restrict__ sums, const int *__restrict__ counts, long long nc, int K, int D,
                                                     const float *__restrict__ cent, float *__restrict__ cent_out)
{
    __shared__ long long red[128];
    const int b = blockIdx.x, tid = threadIdx.x;
    long long n = 0;
    for (long long c = tid; c < nc; c += 128) n += counts[c * 128 + b];
    red[tid] = n;
    __syncthreads();
    n = 0;
    for (int t = 0; t < 128; ++t) n += red[t];
    if (tid >= D) return;
    if (n == 0) { cent_out[b * D + tid] = cent[b * D + tid]; return; }
    const float *__restrict__ p = sums + (size_t)b * D + tid;
    cent_out[b * D + tid] = (float)(bn_chain<double>(p, (size_t)K * D, nc) / (double)n);
}

__global__ void __launch_bounds__(192) k_bins_record(const int *__restrict__ counts, const double *__restrict__ inertia, const int *__restrict__ moved,
                                                     const int *__restrict__ nonfinite, long long nc, int K, int has_assign, fd_bins *__restrict__ rec)
{
    __shared__ long long n_k[128], tot[2];
    __shared__ double in_all;
    const int tid = threadIdx.x;
    if (tid < 128) {                                       // a thread per bin; the third wave has the three scalars
        const long long n = tid < K ? bn_chain<long long>(counts + tid, 128, nc) : 0;
        n_k[tid] = n;
        rec->counts[tid] = n;
    } else if (tid == 128) {
        in_all = bn_chain<double>(inertia, 1, nc);
    } else if (tid == 129 || tid == 130) {
        tot[tid - 129] = bn_chain<long long>(tid == 129 ? moved : nonfinite, 1, nc);
    }
    __syncthreads();
    if (tid != 0) return;
    const double s = in_all;
    int empty = 0;
    long long all = 0;
    for (int k = 0; k < K; ++k) { empty += n_k[k] == 0; all += n_k[k]; }
    rec->inertia = s;
    rec->moved = has_assign ? tot[0] : -1;
    rec->nonfinite = tot[1];
    rec->empty = empty;
    rec->status = all == 0 ? FD_BINS_EMPTY : (tot[1] ? FD_BINS_NONFINITE : FD_BINS_OK);
}

size_t bins_scratch_bytes(long long N, int K, int D, bool update) { return fdb::layout(N, K, D, update).total; }

hipError_t bins_pass(const Launch &La, const float *x, long long N, int D, long long ld, const float *shift, const float *scale, const float *cent,
                     int K, int *assign_io, float *cent_out, fd_bins *rec, void *scratch)
{
    const fdb::Layout o = fdb::layout(N, K, D, cent_out != nullptr);
    char *const s = static_cast<char *>(scratch);
    int *counts = reinterpret_cast<int *>(s + o.counts), *moved = reinterpret_cast<int *>(s + o.moved), *nonf = reinterpret_cast<int *>(s + o.nonfinite);
    double *inertia = reinterpret_cast<double *>(s + o.inertia);
    float *sums = reinterpret_cast<float *>(s + o.sums);
    const long long nc = fdb::chunks(N);
    const size_t shmem = fdb::lds_bytes(K, D);
    const int KT = fdb::tiles(K), NT = cent_out ? (KT * fdb::tiles(D) + 3) / 4 : 0;
#define BN_PASS(kt, nt)                                                                                                                              \
    if (KT == kt && NT == nt) {                                                                                                                      \
        const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void *>(k_bins_pass<kt, nt>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem); \
        if (ea != hipSuccess) return ea;                                                                                                             \
        FD_LAUNCH(La, nt ? "bins_pass_update" : "bins_pass_assign", (k_bins_pass<kt, nt>), dim3((unsigned)nc), dim3(256), shmem, x, N, D, ld, shift, scale, cent, \
                  K, assign_io, sums, counts, inertia, moved, nonf);                                                                                 \
    }
    BN_PASS(1, 0) BN_PASS(2, 0) BN_PASS(3, 0) BN_PASS(4, 0)
    BN_PASS(1, 1) BN_PASS(2, 1) BN_PASS(2, 2) BN_PASS(3, 1) BN_PASS(3, 2) BN_PASS(3, 3) BN_PASS(4, 1) BN_PASS(4, 2) BN_PASS(4, 3) BN_PASS(4, 4)
#undef BN_PASS
    if (cent_out) FD_LAUNCH(La, "bins_update", k_bins_update, dim3(K), dim3(128), 0, (const float *)sums, (const int *)counts, nc, K, D, cent, cent_out);
    if (rec)
        FD_LAUNCH(La, "bins_record", k_bins_record, dim3(1), dim3(192), 0, (const int *)counts, (const double *)inertia, (const int *)moved, (const int *)nonf,
                  nc, K, assign_io != nullptr, rec);
    return hipSuccess;
}

}  // namespace fdk
