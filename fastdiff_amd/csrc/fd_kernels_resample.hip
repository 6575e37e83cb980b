// fd_kernels_resample.hip -- sample-rate conversion around the vocoder (include/fastdiff_hip_ext.h: fd_resample): what the reference gets
// from librosa.core.load(wav_path, sr=sample_rate) (data_gen/tts/data_gen_utils.py:111): a recording of any rate, sample type and
// channel count -> float mono at the model's rate, in one launch; and the vocoder's waveform -> any output rate.
//
//   y[i] = sum_j x[j] h[i down - j up + half]      (polyphase: a = i down + half, phase p = a % up, last input jmax = a / up)
//
// The table [up][Kp] (csrc/fd_resample.h: table()) holds row p in the order of ascending input, so output i is the dot product of
// its row with x[jmax - K + 1 .. jmax].  A table (160 - 320 KB for the usual ratios) is larger than a workgroup's LDS share and far
// smaller than an XCD's 4 MiB L2: rows are read from there, 16 bytes per lane.
//
// One workgroup = FD_RESAMPLE_TILE consecutive outputs of one item, one output per lane.  The inputs the tile needs
// (TILE down / up + K samples: 837 for 48k -> 22.05k) are staged in LDS in pieces of RS_CHUNK samples -- one piece for the usual ratios; a
// ratio near 1024 : 1 needs 390k samples per tile and walks them piece by piece -- with the source's sample type converted and its
// channels mixed down on the way (frames outside [0, valid) are never read: their products are exact zeros and are left out).
// Summation order: ascending input index into ONE float32 accumulator per output, one fmaf per product, whatever the piece borders,
// the item's place in the batch, its pitch or its alignment -- the staging path (16-byte reads for aligned float mono rows, element
// reads otherwise) only decides how the same values reach LDS.
#include "fd_internal.h"
#include "fd_kernels.h"

namespace fdk {

constexpr int RS_TILE = FD_RESAMPLE_TILE, RS_CHUNK = 4096;      // 16 KB of LDS
static_assert(RS_TILE == 256, "one output per lane of a 256-lane workgroup");

// frame j of a row as float mono: every sample divided by its type's full scale (infer.pcm_to_float), the channels added in channel
// order in float32 and the sum divided by their count, correctly rounded
template <int FMT>
__device__ __forceinline__ float rs_load(const void *__restrict__ row, long long j, int C)
{
    float s = 0.0f;
    for (int c = 0; c < C; ++c) {
        const long long e = j * C + c;
        float v;
        if (FMT == FD_PCM_S16) v = (float)static_cast<const short *>(row)[e] * (1.0f / 32768.0f);
        else if (FMT == FD_PCM_S32) v = (float)static_cast<const int *>(row)[e] * (1.0f / 2147483648.0f);
        else if (FMT == FD_PCM_U8) v = ((float)static_cast<const unsigned char *>(row)[e] - 128.0f) * (1.0f / 128.0f);
        else v = static_cast<const float *>(row)[e];
        s = c == 0 ? v : s + v;
    }
    return C == 1 ? s : __fdiv_rn(s, (float)C);
}

__device__ __forceinline__ const void *rs_row(const void *src, int fmt, long long elems)
{
    const long long bytes = fmt == FD_PCM_S16 ? 2 : (fmt == FD_PCM_U8 ? 1 : 4);
    return static_cast<const char *>(src) + elems * bytes;
}

template <int FMT>
__global__ void __launch_bounds__(256) k_resample(const void *__restrict__ src, float *__restrict__ dst, const float *__restrict__ table,
                                                  ResampleLens lens, int C, long long n_in, long long src_pitch, long long dst_pitch,
                                                  long long n_out_max, int up, int down, int half, int K, int Kp, int vec)
{
    __shared__ float xs[RS_CHUNK];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long valid = lens.v[b];
    const long long n_out = valid / down * up + (valid % down * up + down - 1) / down;
    const long long i0 = (long long)blockIdx.x * RS_TILE, i = i0 + tid;
    float *out = dst + (long long)b * dst_pitch;
    if (i0 >= n_out) {                                     // (the whole workgroup) behind the item's own length
        if (i < n_out_max) out[i] = 0.0f;
        return;
    }
    const void *row_src = rs_row(src, FMT, (long long)b * src_pitch);
    const long long i_last = (i0 + RS_TILE < n_out ? i0 + RS_TILE : n_out) - 1;
    // inputs of the tile: [jmax(i0) - K + 1, jmax(i_last)] cut to the item
    long long lo = (i0 * down + half) / up - (K - 1), hi = (i_last * down + half) / up + 1;
    lo = lo > 0 ? lo : 0;
    hi = hi < valid ? hi : valid;
    // this lane's output (a lane behind n_out computes i_last's again and stores nothing)
    const bool active = i < n_out;
    const long long a = (active ? i : i_last) * down + half;
    const long long js = a / up - (K - 1);                 // the input of row element 0
    const float *__restrict__ trow = table + (long long)(a % up) * Kp;
    float acc = 0.0f;
    for (long long c0 = vec ? (lo & ~3LL) : lo; c0 < hi; c0 += RS_CHUNK) {
        const long long c1 = c0 + RS_CHUNK < hi ? c0 + RS_CHUNK : hi;
        const int n = (int)(c1 - c0);
        __syncthreads();                                   // the previous piece has been read
        if (vec) {                                         // float mono, row and piece start 16-byte aligned
            const float *xr = static_cast<const float *>(row_src);
            for (int k = tid * 4; k < n; k += 1024) {
                if (c0 + k + 4 <= n_in) {
                    const float4 v = *reinterpret_cast<const float4 *>(xr + c0 + k);
                    xs[k] = v.x; xs[k + 1] = v.y; xs[k + 2] = v.z; xs[k + 3] = v.w;
                } else {
                    for (int e = 0; e < 4; ++e)
                        if (c0 + k + e < n_in) xs[k + e] = xr[c0 + k + e];
                }
            }
        } else {
            for (int k = tid; k < n; k += 256) xs[k] = rs_load<FMT>(row_src, c0 + k, C);
        }
        __syncthreads();
        // row elements whose input lies in [c0, c1)
        const long long d0 = c0 - js, d1 = c1 - js;
        const int rlo = d0 > 0 ? (d0 < K ? (int)d0 : K) : 0, rhi = d1 < K ? (d1 > 0 ? (int)d1 : 0) : K;
        const int off = rlo < rhi ? (int)(js - c0) : 0;    // row element r reads xs[off + r]; with rlo < rhi, -K < js - c0 < RS_CHUNK
        for (int r4 = rlo & ~3; r4 < rhi; r4 += 4) {
            const float4 t = *reinterpret_cast<const float4 *>(trow + r4);
            const int x0 = off + r4;
            if (r4 >= rlo && r4 + 4 <= rhi) {
                acc = fmaf(t.x, xs[x0], acc);
                acc = fmaf(t.y, xs[x0 + 1], acc);
                acc = fmaf(t.z, xs[x0 + 2], acc);
                acc = fmaf(t.w, xs[x0 + 3], acc);
            } else {
                if (r4 >= rlo && r4 < rhi) acc = fmaf(t.x, xs[x0], acc);
                if (r4 + 1 >= rlo && r4 + 1 < rhi) acc = fmaf(t.y, xs[x0 + 1], acc);
                if (r4 + 2 >= rlo && r4 + 2 < rhi) acc = fmaf(t.z, xs[x0 + 2], acc);
                if (r4 + 3 >= rlo && r4 + 3 < rhi) acc = fmaf(t.w, xs[x0 + 3], acc);
            }
        }
    }
    if (active) out[i] = acc;
    else if (i < n_out_max) out[i] = 0.0f;
}

// equal rates: conversion, down-mix and copy
template <int FMT>
__global__ void __launch_bounds__(256) k_resample_copy(const void *__restrict__ src, float *__restrict__ dst, ResampleLens lens, int C,
                                                       long long n_in, long long src_pitch, long long dst_pitch)
{
    const int b = blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_in) return;
    dst[(long long)b * dst_pitch + i] = i < lens.v[b] ? rs_load<FMT>(rs_row(src, FMT, (long long)b * src_pitch), i, C) : 0.0f;
}

template <int FMT>
static hipError_t resample_fmt(const Launch &L, const void *src, int C, int B, int64_t n_in, int64_t src_pitch, const int64_t *valid,
                               int up, int down, int half, int K, int Kp, int64_t n_out_max, const float *table, float *dst, int64_t dst_pitch)
{
    const bool copy = up == 1 && down == 1;
    for (int b0 = 0; b0 < B; b0 += RESAMPLE_ITEMS) {       // the items' lengths travel as kernel arguments: nothing to stage or to keep alive
        const int nb = B - b0 < RESAMPLE_ITEMS ? B - b0 : RESAMPLE_ITEMS;
        ResampleLens lens;
        for (int b = 0; b < RESAMPLE_ITEMS; ++b) lens.v[b] = b < nb ? (valid ? valid[b0 + b] : n_in) : 0;
        const void *s = static_cast<const char *>(src) + (int64_t)b0 * src_pitch * (FMT == FD_PCM_S16 ? 2 : (FMT == FD_PCM_U8 ? 1 : 4));
        float *d = dst + (int64_t)b0 * dst_pitch;
        if (copy) {
            FD_LAUNCH(L, "resample_copy", k_resample_copy<FMT>, dim3((unsigned)((n_in + 255) / 256), nb), dim3(256), 0, s, d, lens, C,
                      (long long)n_in, (long long)src_pitch, (long long)dst_pitch);
        } else {
            const int vec = FMT == FD_PCM_F32 && C == 1 && (reinterpret_cast<uintptr_t>(s) & 15) == 0 && src_pitch % 4 == 0;
            FD_LAUNCH(L, "resample", k_resample<FMT>, dim3((unsigned)((n_out_max + RS_TILE - 1) / RS_TILE), nb), dim3(256), 0, s, d, table,
                      lens, C, (long long)n_in, (long long)src_pitch, (long long)dst_pitch, (long long)n_out_max, up, down, half, K, Kp, vec);
        }
    }
    return hipSuccess;
}

hipError_t resample(const Launch &L, const void *src, int format, int C, int B, int64_t n_in, int64_t src_pitch, const int64_t *valid,
                    int up, int down, int half, int K, int Kp, int64_t n_out_max, const float *table, float *dst, int64_t dst_pitch)
{
    switch (format) {
    case FD_PCM_S16: return resample_fmt<FD_PCM_S16>(L, src, C, B, n_in, src_pitch, valid, up, down, half, K, Kp, n_out_max, table, dst, dst_pitch);
    case FD_PCM_S32: return resample_fmt<FD_PCM_S32>(L, src, C, B, n_in, src_pitch, valid, up, down, half, K, Kp, n_out_max, table, dst, dst_pitch);
    case FD_PCM_U8: return resample_fmt<FD_PCM_U8>(L, src, C, B, n_in, src_pitch, valid, up, down, half, K, Kp, n_out_max, table, dst, dst_pitch);
    default: return resample_fmt<FD_PCM_F32>(L, src, C, B, n_in, src_pitch, valid, up, down, half, K, Kp, n_out_max, table, dst, dst_pitch);
    }
}

}  // namespace fdk
