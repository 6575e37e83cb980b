// fd_wpack.h -- the ONE definition of the weight packs' layouts: for every pack of DevWeights the closed-form map from a destination
// position to the element of the folded reference-layout weight it holds, and the fp16 split of a value.  The host packer
// (fd_weights.cpp: fd_commit_weights) and the device packer (fd_kernels_wpack.hip: fd_refresh_weights_device) both include it, so the
// two images agree by construction.  Everything here is a pure function of its arguments.
#pragma once
#include <math.h>

#include "fd_internal.h"

namespace fdp {

// ---- fp16x2 form of a weight ---------------------------------------------------------------------------------------------------
// IEEE binary16 <-> binary32 in integer arithmetic (round to nearest even, subnormals kept): the weight pieces of the fp16x2 kernels.
__host__ __device__ inline uint32_t f32_bits(float x)
{
    union { float f; uint32_t u; } c;
    c.f = x;
    return c.u;
}
__host__ __device__ inline float f32_from_bits(uint32_t u)
{
    union { float f; uint32_t u; } c;
    c.u = u;
    return c.f;
}
__host__ __device__ inline uint16_t f16_from_f32(float x)
{
    uint32_t u = f32_bits(x);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    u &= 0x7FFFFFFFu;
    if (u > 0x7F800000u) return sign | 0x7E00u;                  // NaN
    if (u >= 0x477FF000u) return sign | 0x7C00u;                 // >= 65520 rounds to infinity
    if (u < 0x38800000u)                                         // below 2^-14: subnormal, a multiple of 2^-24
        return sign | (uint16_t)lrintf(f32_from_bits(u) * 16777216.0f);   // current rounding mode = nearest even; 1024 = smallest normal
    uint32_t hbits = (((u >> 23) - 112u) << 10) | ((u & 0x7FFFFFu) >> 13);
    const uint32_t rem = u & 0x1FFFu;
    if (rem > 0x1000u || (rem == 0x1000u && (hbits & 1u))) ++hbits;   // a carry into the exponent is the correct result
    return sign | (uint16_t)hbits;
}
__host__ __device__ inline float f32_from_f16(uint16_t hb)
{
    const uint32_t sign = (uint32_t)(hb & 0x8000u) << 16, exp = (hb >> 10) & 0x1Fu, man = hb & 0x3FFu;
    float v;
    if (exp == 0) v = (float)man * (1.0f / 16777216.0f);
    else if (exp == 31) v = f32_from_bits(0x7F800000u | (man << 13));
    else v = f32_from_bits(((exp + 112u) << 23) | (man << 13));
    return f32_from_bits(f32_bits(v) | sign);
}
// v = hi + 2^-11 lo, hi = fp16(v), lo = fp16((v - hi) * 2^11).  False when v does not fit the range the fp16-pipe kernels accept
// (|v| < 32768; a NaN does not): decided on the bits, so that no floating-point option of a build can change it.
__host__ __device__ inline bool split_f16(float v, uint16_t &hi, uint16_t &lo)
{
    hi = f16_from_f32(v);
    lo = f16_from_f32((v - f32_from_f16(hi)) * 2048.0f);
    return (f32_bits(v) & 0x7FFFFFFFu) < 0x47000000u;
}

// ---- fp32 MFMA operands: [mt][s4][lane][4], kk = 2*(4*s4 + r) + (lane >> 5) ------------------------------------------------------
// Position d of the A-operand pack of a conv weight [cout][cin][ks] (kk = tap*cin + ci) -> index into that weight
__host__ __device__ inline int pack_A_src(int d, int cin, int ks)
{
    const int ns4 = cin * ks / 8, r = d & 3, lane = (d >> 2) & 63, q = d >> 8, s4 = q % ns4, mt = q / ns4;
    const int o = mt * 32 + (lane & 31), kk = 2 * (4 * s4 + r) + (lane >> 5), tap = kk / cin, ci = kk % cin;
    return (o * cin + ci) * ks + tap;
}

// Position i of a [kg][64 lane][8 e] run of 32x32x16 fp16 operands: lane = row + 32*g holds the 8 consecutive k = 16*kg + 8*g + e.
struct Op16 { int row, k; };
__host__ __device__ inline Op16 op16(int i) { return {(i >> 3) & 31, 16 * (i >> 9) + 8 * ((i >> 8) & 1) + (i & 7)}; }

// fp16 pieces of a conv weight [cout][cin][ks] in 32x32x16 A-operand order [mt = out/32][piece][kg][lane = out%32 + 32*g][8],
// k = tap*cin + in: position i of row tile mt -> index into the weight
__host__ __device__ inline int pack_A_h2_src(int mt, int i, int cin, int ks)
{
    const Op16 q = op16(i);
    return ((mt * 32 + q.row) * cin + q.k % cin) * ks + q.k / cin;
}

// ---- ConvTranspose1d weight [in][out][2r] as per-phase operands, kk = sel*32 + i -------------------------------------------------
// sel 0: the nearer input position (jA), sel 1: the one before it (jB = jA - 1, tap + r)
__host__ __device__ inline int convt_tap(int r, int ph, int sel)
{
    const int pd = r / 2, kA = (ph < pd) ? ph + pd : ph - pd;
    return sel ? kA + r : kA;
}
// fp32 [ph][8 s4][lane][4]: position d -> index into the weight
__host__ __device__ inline int up_pack_src(int d, int r)
{
    const int q = d & 3, lane = (d >> 2) & 63, s4 = (d >> 8) & 7, ph = d >> 11;
    const int kk = 2 * (4 * s4 + q) + (lane >> 5), i = kk & 31, o = lane & 31;
    return (i * fd::C + o) * 2 * r + convt_tap(r, ph, kk >> 5);
}
// fp16 pieces [ph][piece][4 kg][64 lane = out + 32*g][8], k = 16*kg + 8*g + e = sel*32 + i: position i of phase ph -> index
__host__ __device__ inline int up_h2_src(int ph, int i, int r)
{
    const Op16 q = op16(i);
    return ((q.k & 31) * fd::C + q.row) * 2 * r + convt_tap(r, ph, q.k >> 5);
}

// ---- hop-8 LVC convs: 16x16x32 tiles [rt][tap][piece][64 lane][8] ------------------------------------------------------------------
// lane = out%16 + 16*g holds input channels 8g .. 8g+7 of one tap: position idx of tile rt_tap = rt*3 + tap -> index into [C][C][3]
__host__ __device__ inline int lvc_h16_src(int rt_tap, int idx)
{
    const int rt = rt_tap / 3, tap = rt_tap % 3, lane = idx >> 3, out = 16 * rt + (lane & 15), in = 8 * (lane >> 4) + (idx & 7);
    return (out * fd::C + in) * 3 + tap;
}

// ---- final_conv in the last LVC layer's register order: [mt*2 + hi][8 r][8] (7 taps + pad) --------------------------------------------
// channel = 16 mt + 4 hi + (r & 3) + 8 (r >> 2): position d -> index into [C][7], or -1 for the pad
__host__ __device__ inline int final_fuse_src(int d)
{
    const int k = d & 7, r = (d >> 3) & 7, part = d >> 6;
    return k == 7 ? -1 : (16 * (part >> 1) + 4 * (part & 1) + (r & 3) + 8 * (r >> 2)) * 7 + k;
}

// ---- the predictor GEMM's B operands: one column per packed-record position pp -----------------------------------------------------
__host__ __device__ inline void unpack_kernel_index(int p, int &layer, int &in, int &out, int &tap)
{
    layer = p / fd::KLAYER;
    const int q = p % fd::KLAYER, e = q & 7, lane = (q >> 3) & 63, mk = q >> 9;
    const int mt = mk / 6, kg = mk % 6, kk = kg * 16 + 8 * (lane >> 5) + e, row = lane & 31;
    tap = kk / fd::C; in = kk % fd::C;
    out = 16 * mt + (row & 15) + 32 * (row >> 4);      // inverse of kernel_tile / kernel_row
}
// The row behind packed column pp: of kernel_conv (pp < KW; the [layers,in,out,k] view, modules.py:333-338) or, *bias_conv set, of
// bias_conv (bias record [layer][mt][row] -> row layer*64 + out; view [layers,out], modules.py:339-342).  A row is [HID][3] weights
// and one bias.
__host__ __device__ inline int gemm_column_row(int pp, bool *bias_conv)
{
    *bias_conv = pp >= fd::KW;
    if (pp < fd::KW) {
        int layer, in, out, tap;
        unpack_kernel_index(pp, layer, in, out, tap);
        return ((layer * fd::C + in) * 2 * fd::C + out) * 3 + tap;
    }
    const int q = pp - fd::KW, layer = q >> 6, mt = (q >> 5) & 1, row = q & 31;
    return layer * 64 + 16 * mt + (row & 15) + 32 * (row >> 4);
}
// Where a position of a 32-column tile reads: which of the tile's columns, and which of that column's HID*3 weights.
struct TilePos { int col, widx; };
// fp32 [24 s4][lane][4] of a tile, kk = tap*64 + channel
__host__ __device__ inline TilePos gemm_pack_pos(int d)
{
    const int r = d & 3, lane = (d >> 2) & 63, s4 = d >> 8, kk = 2 * (4 * s4 + r) + (lane >> 5);
    return {lane & 31, (kk % fd::HID) * 3 + kk / fd::HID};
}
// fp16 pieces [12 kg][lane = col + 32*g][8] of a tile, k = tap*64 + channel
__host__ __device__ inline TilePos gemm_h2_pos(int i)
{
    const Op16 q = op16(i);
    return {q.row, (q.k % fd::HID) * 3 + q.k / fd::HID};
}
// Winograd F(2,3) over the frame axis (kernel_conv is a k = 3 convolution over frames, modules.py:315-318): per pair of output frames
//   y[2p] = m0 + m1 + m2,  y[2p+1] = m1 - m2 + m3  with  m_j = V_j . u_j (K = 64 each),
//   V0 = g0, V1 = (g0 + g1 + g2) / 2, V2 = (g0 - g1 + g2) / 2, V3 = -g2        (g_tap = the column's weights of that tap)
//   u0 = h[2p-1] - h[2p+1], u1 = h[2p] + h[2p+1], u2 = h[2p+1] - h[2p], u3 = h[2p] - h[2p+2]   (k_h_wino)
// fp16 pieces [16 kg][lane = col + 32*g][8] of a tile, k = 64 j + channel: position i -> column and V_j[channel], formed in double and
// rounded once (wino_value).  wrow(col): that column's [HID][3] weights.
__host__ __device__ inline float wino_value(int j, float w0, float w1, float w2)
{
    const double g0 = w0, g1 = w1, g2 = w2;
    switch (j) {
    case 0: return (float)g0;
    case 1: return (float)(0.5 * (g0 + g1 + g2));
    case 2: return (float)(0.5 * (g0 - g1 + g2));
    default: return (float)-g2;
    }
}
template <class Row> __host__ __device__ inline float gemm_w_value(int i, Row wrow)
{
    const Op16 q = op16(i);
    const float *w = wrow(q.row) + (q.k & 63) * 3;
    return wino_value(q.k >> 6, w[0], w[1], w[2]);
}

// ---- the six range flags as bits of one word (fd_get_weight_flags) --------------------------------------------------------------------
enum { OK_GEMM = 1, OK_GEMM_W = 2, OK_LVC = 4, OK_DBLOCK = 8, OK_CONVT = 16, OK_KPF = 32, OK_ALL = 63 };

}  // namespace fdp

// ---- the device packer's work lists (fd_kernels_wpack.hip; built by fd_refresh_weights_device) ----------------------------------------
namespace fdk {
// Weight norm of one tensor: dst[o][:] = v[o][:] * (g[o] / ||v[o]||), blocks [first_block, ...) take rows_per_block rows each
struct FoldJob { const float *v, *g; float *dst; int rows, per, rows_per_block, first_block; };
// One pack (or plain copy) of `n` destination values, 256 units of 16 destination bytes per block from first_block on
enum PackKind { WP_COPY = 0, WP_TRANSPOSE, WP_PACK_A, WP_UP_PACK, WP_FINAL_FUSE, WP_A_H2, WP_UP_H2, WP_H16 };
struct PackJob {
    const float *src;
    void *dst;
    int kind, n;
    int p0, p1;      // WP_TRANSPOSE: rows, cols of src; WP_PACK_A / WP_A_H2: cin, ks; WP_UP_PACK / WP_UP_H2: the upsampling ratio
    int inner;       // fp16 kinds: values per (outer, piece) of the [outer][piece][inner] destination
    int flag;        // fp16 kinds: the fdp::OK_* bit of the pack's kernel family
    int first_block, pad_;
};
// The predictor GEMM's operands of one LVC block, from the folded kernel_conv / bias_conv
struct GemmJob { const float *kc_w, *kc_b, *bc_w, *bc_b; float *pack, *bias; uint16_t *h2, *wino; };
struct GemmJobs { GemmJob blk[fd::NBLK]; };
constexpr int WPACK_FOLD_LDS = 64 * 193;      // floats of a fold block's row image: 64 rows of kernel_conv (192 + 1 pad)
inline int wpack_fold_rows(int per) { const int r = WPACK_FOLD_LDS / (per + 1); return r < 64 ? r : 64; }
// bad: one device word; the kernels OR the fdp::OK_* bit of a family into it when a value of that family does not fit fp16
hipError_t wpack_fold(const Launch &L, const FoldJob *jobs_dev, int n_jobs, int n_blocks);
hipError_t wpack_gather(const Launch &L, const PackJob *jobs_dev, int n_jobs, int n_blocks, unsigned *bad);
hipError_t wpack_gemm(const Launch &L, const GemmJobs &jobs, unsigned *bad);
}  // namespace fdk
