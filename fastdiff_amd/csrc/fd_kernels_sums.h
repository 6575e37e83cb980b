// fd_kernels_sums.h -- what the kernels around the training step share (fd_kernels_step.hip, fd_kernels_phi.hip; fd_kernels_cconv.hip
// takes wave_sum and find_item): the fixed-order sums, the search of a chunked launch, and the per-item draw of a step.  Header-only.
//
// Sums (loss, squared gradient norm, per-item distances, the residual of phi_loss): a thread adds RUN = FD_STEP_RUN elements serially, the
// 256 threads of a workgroup are added by a butterfly inside each wave (xor 32 ... 1) and a fixed tree over the four waves,
// (w0 + w1) + (w2 + w3); the per-workgroup results go to the handle's step scratch, and one final workgroup adds those by the same tree,
// 256 at a time and then the up to 256 results of that (65536 partial sums, 2^28 elements).  An element therefore passes through
// RUN + ceil(log2(n / RUN)) additions at most up to that size: the bound of tests/test_train_step.py.  No workgroup touches two items, no
// atomics: the order, and with it the result, is the same every run -- two runs agree bit for bit.
#pragma once
#include "fd_kernels.h"
#include "fd_device.h"

namespace fdk {

constexpr int RUN = FD_STEP_RUN;
constexpr int WG = 256;
constexpr int TILE = RUN * WG;             // elements per workgroup
inline int64_t tiles(int64_t n) { return (n + TILE - 1) / TILE; }

// inf or NaN, on the bits.  The build (-fno-honor-nans) lets the compiler assume that no float it computes with is a NaN -- it turns a
// plain exponent test on a value that also feeds an fma into "is infinite" -- so the bits pass through an empty asm first.
__device__ __forceinline__ bool not_finite(float v)
{
    unsigned u = __float_as_uint(v);
    asm volatile("" : "+v"(u));
    return (u & 0x7F800000u) == 0x7F800000u;
}

// the sum of v over the wave's 64 lanes, in every lane
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// ... and of a float64 (fd_kernels_trim.hip), by the same butterfly
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the sum of v over the workgroup's 256 threads, in every thread: wave_sum, then (w0 + w1) + (w2 + w3)
__device__ __forceinline__ float block_sum(float v)
{
    __shared__ float ws[WG / 64];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = (ws[0] + ws[1]) + (ws[2] + ws[3]);
    __syncthreads();      // (ws is free again: the final workgroup calls this in a loop)
    return r;
}

// the final workgroup's sum of P per-workgroup results, a tree as well: groups of 256 through block_sum into LDS, then those (P <= 65536,
// i.e. 2^28 elements; beyond that a thread first adds every 65536th serially).  Adding the zeros of an incomplete group is exact.
__device__ __forceinline__ float final_sum(const float *partial, int64_t P)
{
    __shared__ float level[WG];
    constexpr int64_t SPAN = (int64_t)WG * WG;
    if (P <= WG) return block_sum(threadIdx.x < P ? partial[threadIdx.x] : 0.0f);
    for (int c = 0; c < WG; ++c) {
        float acc = 0.0f;
        for (int64_t i = (int64_t)c * WG + threadIdx.x; i < P; i += SPAN) acc += partial[i];
        acc = (int64_t)c * WG < P ? block_sum(acc) : 0.0f;      // (uniform over the workgroup)
        if (threadIdx.x == 0) level[c] = acc;
    }
    __syncthreads();
    return block_sum(level[threadIdx.x]);
}

// ---- chunked launches ------------------------------------------------------------------------------------------------------------------
// Records of many tensors travel as kernel arguments, a chunk per launch: it[n], and first_block[0 .. n], the first workgroup of each
// tensor (no workgroup straddles two).  The tensor of workgroup blk < first_block[n], by bisection.
template <class Chunk>
__device__ __forceinline__ int find_item(const Chunk &c, int blk)
{
    int lo = 0, hi = c.n;      // first_block[lo] <= blk < first_block[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (c.first_block[mid] <= blk) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- the draws of a step -------------------------------------------------------------------------------------------------------------
// the step the draws are keyed on: the device counter of a captured step, else the caller's
__device__ __forceinline__ unsigned long long step_iter(const fd_train_state *state, unsigned long long iter_host)
{
    return state ? state->iter : iter_host;
}

__device__ __forceinline__ void philox_keyed(unsigned long long seed, uint32_t stream, uint64_t pos, unsigned long long uid, uint32_t r[4])
{
    philox4x32_10((uint32_t)pos, (uint32_t)(pos >> 32) ^ (uint32_t)uid, stream, 0x5EEDu ^ (uint32_t)(uid >> 32), (uint32_t)seed,
                  (uint32_t)(seed >> 32), r);
}

// the one uniform word of item (slot) b at step `it` on `stream`: four neighbours share a generator call (position b >> 2, word b & 3)
__device__ __forceinline__ uint32_t item_word(unsigned long long seed, uint32_t stream, int64_t b, unsigned long long it)
{
    uint32_t r[4];
    philox_keyed(seed, stream, (uint64_t)(b >> 2), it, r);
    const int c = (int)(b & 3);
    return c == 0 ? r[0] : (c == 1 ? r[1] : (c == 2 ? r[2] : r[3]));
}

// x_t = a x + d q on four samples, operation by operation as torch evaluates it: two rounded products and their rounded sum, whatever
// the including file lets the compiler contract
__device__ __forceinline__ float4 noised4(float a, float d, float4 x, float4 q)
{
#pragma clang fp contract(off)
    return make_float4(a * x.x + d * q.x, a * x.y + d * q.y, a * x.z + d * q.z, a * x.w + d * q.w);
}

}  // namespace fdk
