// fd_kernels_wpack.hip -- the weight packs of the tuned kernel set rebuilt on the device from live parameter tensors
// (fd_refresh_weights_device): weight norm folded into the reference-layout slots of the weight arena, then every operand pack gathered
// from those slots in destination order.  The layouts are fd_wpack.h's, the same functions the host packer (fd_weights.cpp) runs, and
// the arithmetic is the host's operation for operation, so the arena ends up byte-equal to a host commit of the same parameters.
// All of it is memory-bound: reads are staged through LDS where a gather would break them up (the fold's rows, the GEMM's columns),
// every pack is written 16 bytes per lane.
#include "fd_kernels.h"
#include "fd_wpack.h"

namespace fdk {

// blocks [first_block of job j, first_block of job j + 1) belong to job j: the last job that starts at or before block b
template <class Job> __device__ inline int find_job(const Job *jobs, int n_jobs, int b)
{
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].first_block <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---- weight norm ------------------------------------------------------------------------------------------------------------------------
// w[o][:] = v[o][:] * (g[o] / (float)sqrt(ss)), ss the double sum of squares of row o added in index order: the host's fold
// (fd_weights.cpp: fold_param), whose result depends on that order.  A block stages its rows in LDS with coalesced reads (row stride
// per + 1: lane o then walks row o without a bank conflict), ONE lane per row adds the row serially, and all lanes scale and store.
__global__ __launch_bounds__(256) void k_wpack_fold(const FoldJob *__restrict__ jobs, int n_jobs)
{
    __shared__ float rows[WPACK_FOLD_LDS];
    __shared__ float scale[64];
    const FoldJob job = jobs[find_job(jobs, n_jobs, blockIdx.x)];
    const int t = threadIdx.x, per = job.per, stride = per + 1;
    const int row0 = (blockIdx.x - job.first_block) * job.rows_per_block;
    const int nrows = min(job.rows_per_block, job.rows - row0), n = nrows * per;
    const float *v = job.v + (size_t)row0 * per;
    float *dst = job.dst + (size_t)row0 * per;
    const bool vec = (per & 3) == 0 && (reinterpret_cast<uintptr_t>(v) & 15) == 0;      // (dst: a 256-byte aligned arena slot)
    if (vec) {
        for (int i = 4 * t; i < n; i += 1024) {
            const float4 x = *reinterpret_cast<const float4 *>(v + i);
            const int r = i / per, a = r * stride + (i - r * per);
            rows[a] = x.x; rows[a + 1] = x.y; rows[a + 2] = x.z; rows[a + 3] = x.w;
        }
    } else {
        for (int i = t; i < n; i += 256) {
            const int r = i / per;
            rows[r * stride + (i - r * per)] = v[i];
        }
    }
    __syncthreads();
    if (t < nrows) {
        double ss = 0.0;
        for (int j = 0; j < per; ++j) {
            const double x = (double)rows[t * stride + j];
            ss += x * x;      // (the product of two floats is exact in double: fused or not, the sum is the host's)
        }
        scale[t] = __fdiv_rn(job.g[row0 + t], (float)__dsqrt_rn(ss));
    }
    __syncthreads();
    if ((per & 3) == 0) {
        for (int i = 4 * t; i < n; i += 1024) {
            const int r = i / per, a = r * stride + (i - r * per);
            const float s = scale[r];
            *reinterpret_cast<float4 *>(dst + i) = make_float4(rows[a] * s, rows[a + 1] * s, rows[a + 2] * s, rows[a + 3] * s);
        }
    } else {
        for (int i = t; i < n; i += 256) {
            const int r = i / per;
            dst[i] = rows[r * stride + (i - r * per)] * scale[r];
        }
    }
}

// ---- packs ------------------------------------------------------------------------------------------------------------------------------
struct alignas(16) Half8 { uint16_t h[8]; };

// 8 values -> their fp16 pieces, 16 bytes each; true when one of them does not fit
__device__ inline bool split8(const float (&v)[8], Half8 &hi, Half8 &lo)
{
    bool bad = false;
#pragma unroll
    for (int e = 0; e < 8; ++e) bad |= !fdp::split_f16(v[e], hi.h[e], lo.h[e]);
    return bad;
}

// One thread per 16 destination bytes: 4 floats of an fp32 pack, or 8 values of an fp16 pack (16 bytes to each of the two pieces).
// The sources are the small convs (at most 100 KB each, read many times over: they stay in L2); the destination is written in order.
__global__ __launch_bounds__(256) void k_wpack_gather(const PackJob *__restrict__ jobs, int n_jobs, unsigned *__restrict__ bad_word)
{
    const PackJob job = jobs[find_job(jobs, n_jobs, blockIdx.x)];
    const int u = (blockIdx.x - job.first_block) * 256 + threadIdx.x;
    const float *__restrict__ src = job.src;
    if (job.kind >= WP_A_H2) {
        const int d = 8 * u;
        if (d >= job.n) return;
        const int o = d / job.inner, i = d - o * job.inner;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
            v[e] = src[job.kind == WP_A_H2 ? fdp::pack_A_h2_src(o, i + e, job.p0, job.p1)
                                           : (job.kind == WP_UP_H2 ? fdp::up_h2_src(o, i + e, job.p0) : fdp::lvc_h16_src(o, i + e))];
        Half8 hi, lo;
        const bool bad = split8(v, hi, lo);
        uint16_t *dst = static_cast<uint16_t *>(job.dst) + (size_t)o * 2 * job.inner + i;
        *reinterpret_cast<Half8 *>(dst) = hi;
        *reinterpret_cast<Half8 *>(dst + job.inner) = lo;
        if (bad) atomicOr(bad_word, (unsigned)job.flag);
        return;
    }
    const int d = 4 * u;
    if (d >= job.n) return;
    float *dst = static_cast<float *>(job.dst) + d;
    float v[4];
    if (job.kind == WP_COPY) {
        if (d + 4 > job.n) {      // the last floats of a tensor whose size is no multiple of 4: the bytes behind it are not the pack's
            for (int e = 0; d + e < job.n; ++e) dst[e] = src[d + e];
            return;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = src[d + e];
    } else if (job.kind == WP_TRANSPOSE) {      // dst [cols][rows] <- src [rows][cols]; rows is a multiple of 4
        const int c = d / job.p0, r = d - c * job.p0;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = src[(size_t)(r + e) * job.p1 + c];
    } else if (job.kind == WP_PACK_A) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = src[fdp::pack_A_src(d + e, job.p0, job.p1)];
    } else if (job.kind == WP_UP_PACK) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = src[fdp::up_pack_src(d + e, job.p0)];
    } else {      // WP_FINAL_FUSE
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int s = fdp::final_fuse_src(d + e);
            v[e] = s < 0 ? 0.0f : src[s];
        }
    }
    *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
}

// The predictor GEMM's B operands: blockIdx.x = one tile of 32 packed columns, blockIdx.y = the LVC block.  A column is one row of
// kernel_conv / bias_conv -- 768 contiguous bytes, but the 32 rows of a tile lie scattered (fd_wpack.h: gemm_column_row) -- so the
// tile's rows are read once, whole, into LDS (row stride 192 + 1: the 32 columns a wave reads at one k fall on 32 banks) and the
// three forms of the tile (fp32, fp16 pieces, Winograd fp16 pieces) and its biases are written from there.
__global__ __launch_bounds__(256) void k_wpack_gemm(GemmJobs jobs, unsigned *__restrict__ bad_word)
{
    constexpr int ROW = fd::HID * 3, STRIDE = ROW + 1;
    __shared__ float rows[32 * STRIDE];
    __shared__ const float *rptr[32];
    __shared__ alignas(16) float rbias[32];
    const GemmJob &job = jobs.blk[blockIdx.y];
    const int t = threadIdx.x, pt = blockIdx.x;
    if (t < 32) {
        bool bias_conv;
        const int row = fdp::gemm_column_row(pt * 32 + t, &bias_conv);
        rptr[t] = (bias_conv ? job.bc_w : job.kc_w) + (size_t)row * ROW;
        rbias[t] = (bias_conv ? job.bc_b : job.kc_b)[row];
    }
    __syncthreads();
    for (int q = t; q < 32 * (ROW / 4); q += 256) {      // 48 float4 per row (the rows start 768-byte steps into a 256-byte aligned slot)
        const int c = q / (ROW / 4), j = 4 * (q - c * (ROW / 4));
        const float4 x = *reinterpret_cast<const float4 *>(rptr[c] + j);
        float *r = rows + c * STRIDE + j;
        r[0] = x.x; r[1] = x.y; r[2] = x.z; r[3] = x.w;
    }
    __syncthreads();
    if (t < 8) *reinterpret_cast<float4 *>(job.bias + pt * 32 + 4 * t) = *reinterpret_cast<const float4 *>(rbias + 4 * t);
    // fp32: [24 s4][lane][4]
    float *gp = job.pack + (size_t)pt * 24 * 256;
    for (int d = 4 * t; d < 24 * 256; d += 1024) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const fdp::TilePos q = fdp::gemm_pack_pos(d + e);
            v[e] = rows[q.col * STRIDE + q.widx];
        }
        *reinterpret_cast<float4 *>(gp + d) = make_float4(v[0], v[1], v[2], v[3]);
    }
    // fp16 pieces: [piece][12 kg][lane][8]
    unsigned bad = 0;
    uint16_t *h2 = job.h2 + (size_t)pt * 2 * 12 * 512;
    for (int i = 8 * t; i < 12 * 512; i += 2048) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const fdp::TilePos q = fdp::gemm_h2_pos(i + e);
            v[e] = rows[q.col * STRIDE + q.widx];
        }
        Half8 hi, lo;
        if (split8(v, hi, lo)) bad |= fdp::OK_GEMM;
        *reinterpret_cast<Half8 *>(h2 + i) = hi;
        *reinterpret_cast<Half8 *>(h2 + 12 * 512 + i) = lo;
    }
    // Winograd F(2,3) pieces: [piece][16 kg][lane][8]
    uint16_t *wn = job.wino + (size_t)pt * 2 * 16 * 512;
#pragma unroll
    for (int j = 0; j < 4; ++j) {      // 4 kg = 2048 positions per V_j: one pass of the block each, j a constant of the pass
        const int i = 2048 * j + 8 * t;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const fdp::Op16 q = fdp::op16(i + e);      // q.k >> 6 == j
            const float *w = rows + q.row * STRIDE + (q.k & 63) * 3;
            v[e] = fdp::wino_value(j, w[0], w[1], w[2]);
        }
        Half8 hi, lo;
        if (split8(v, hi, lo)) bad |= fdp::OK_GEMM_W;
        *reinterpret_cast<Half8 *>(wn + i) = hi;
        *reinterpret_cast<Half8 *>(wn + 16 * 512 + i) = lo;
    }
    if (bad) atomicOr(bad_word, bad);
}

hipError_t wpack_fold(const Launch &L, const FoldJob *jobs_dev, int n_jobs, int n_blocks)
{
    if (n_blocks == 0) return hipSuccess;
    FD_LAUNCH(L, "wpack_fold", k_wpack_fold, dim3(n_blocks), dim3(256), 0, jobs_dev, n_jobs);
    return hipSuccess;
}

hipError_t wpack_gather(const Launch &L, const PackJob *jobs_dev, int n_jobs, int n_blocks, unsigned *bad)
{
    if (n_blocks == 0) return hipSuccess;
    FD_LAUNCH(L, "wpack_gather", k_wpack_gather, dim3(n_blocks), dim3(256), 0, jobs_dev, n_jobs, bad);
    return hipSuccess;
}

hipError_t wpack_gemm(const Launch &L, const GemmJobs &jobs, unsigned *bad)
{
    FD_LAUNCH(L, "wpack_gemm", k_wpack_gemm, dim3(fd::KREC / 32, fd::NBLK), dim3(256), 0, jobs, bad);
    return hipSuccess;
}

}  // namespace fdk
