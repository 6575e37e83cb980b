// fd_kernels_pwg.hip -- Parallel WaveGAN's generator on the device (include/fastdiff_hip_ext.h: "Parallel WaveGAN", which defines the
// computation; the reference: vocoders/pwg.py over modules/parallel_wavegan).  Host side, images and scratch layout: fd_pwg.h.
//
//   k_pwg_front   grid (frame tiles of 64, row tiles of 64, B): the conditioning of the tile -- the caller's padded c, or the mel with the
//                 scaler and the edge replication applied by index clamp -- into LDS, then thread = (frame, 16 rows of one wave): the
//                 composed convolution W_aux_l conv_in, each output one fmaf chain over (channel, tap) -> G[b][l][128][T].
//   k_pwg_coef    grid (sample tiles of 256, B): per sample the coefficients of the frames q - 2 .. q + 2 that the up-sampling stages
//                 composed put on it, summed in float64 over the stage paths in ascending code; a path that leaves the item at any
//                 stage's rate contributes nothing -> K[b][5][L].
//   k_pwg_layer<FIRST, LAST>   grid (tiles of FD_PWG_TILE, B), 256 threads, one launch per residual block.  A wave takes 64 samples of the
//                 tile at a time, two column blocks of v_mfma_f32_32x32x2_f32, in two passes over the rows (32 of the tanh half with
//                 their 32 of the sigmoid half): 96 steps over (tap, channel pair) with the x operand read from x_l in memory (FIRST:
//                 formed from z) and zero outside [0, L_b); then the conditioning and the bias as further steps of the same contraction (k = a
//                 frame of G under the wave, times the sample's coefficient on it; k = the bias entry, times one);
//                 gate in registers; h through the wave's LDS slice into operand order, one column block at a time (the other
//                 waits in registers: 32 KB of LDS per workgroup, four workgroups per CU); 32 steps for out | skip per column block;
//                 x_{l+1} = (out + b + x_l) sqrt(1/2) to the other buffer (not LAST), skip read, added to, written (FIRST: written).
//   k_pwg_tail    grid (tiles of 128, B): relu(skip sqrt(1 / layers)) as the operand of the 64 x 64 product, relu, the 64-term dot with
//                 the last weights in register order, the two half waves added; zeros from L_b to hop T.
//   k_pwg_draw    the z of a call without z, for callers and tests that want to see it.
//
// Every sum has a fixed order that depends on the item's own length alone and there are no atomics, so a waveform is bit-identical
// alone, anywhere in a ragged batch and from call to call.  Nothing of an item behind its own frames is read.
#include "fd_internal.h"
#include "fd_kernels.h"
#include "fd_kernels_common.h"
#include "fd_pwg.h"

namespace fdk {

using fdk_fast::drow;
using fdk_fast::mfma32;

namespace {
constexpr int PRES = fdpwg::RES, PGATE = fdpwg::GATE, PAUX = fdpwg::AUX, PNEIGH = fdpwg::NEIGH;
constexpr int LAYER_WAVES_PER_SIMD = 2;      // the layer kernel's registers are held to this occupancy (measured: at 3 and 4 it spills and is 1.3x and 1.4x slower)
struct PwgStages { int n, hop, s[fdpwg::MAX_STAGES]; };

__device__ __forceinline__ float pwg_z(unsigned long long seed, unsigned long long id, long long pos)
{
    const float4 q = philox_normal4(seed, FD_PWG_PHILOX_STREAM, (uint64_t)(pos >> 2), id);
    return fdk_fast::f4c(q, (int)(pos & 3));
}
// k[j] for j = 0 .. 4, zero for any other j
__device__ __forceinline__ float pwg_pick(const float (&k)[fdpwg::NEIGH], int j)
{
    return j == 0 ? k[0] : (j == 1 ? k[1] : (j == 2 ? k[2] : (j == 3 ? k[3] : (j == 4 ? k[4] : 0.0f))));
}
}  // namespace
static_assert(sizeof(fd_pwg_config) == 112, "the size the header states");
static_assert(fdpwg::THREADS == 256 && fdpwg::WAVE_COLS == 64 && PRES == 64 && PGATE == 128, "the layer kernel is written for these");

__global__ void __launch_bounds__(256) k_pwg_front(const float *__restrict__ src, int padded, int has_scaler, const float *__restrict__ Wc,
                                                   const float *__restrict__ scaler, const long long *__restrict__ lens, int T, int w, int rows,
                                                   float *__restrict__ G)
{
    __shared__ float cs[PAUX][fdpwg::FRONT_FRAMES + 2 * FD_PWG_MAX_CONTEXT];
    const int b = blockIdx.z, t0 = blockIdx.x * fdpwg::FRONT_FRAMES;
    const int Tb = (int)own_len(lens, b, T);
    if (t0 >= Tb) return;
    const int K = 2 * w + 1, Tc = padded ? T + 2 * w : T, span = fdpwg::FRONT_FRAMES + 2 * w;
    const float *cb = src + (size_t)b * PAUX * Tc;
    for (int i = threadIdx.x; i < PAUX * span; i += 256) {
        const int m = i / span, j = i - m * span, f = t0 + j;      // f: a frame of the padded conditioning
        float v = 0.0f;
        if (f < Tb + 2 * w) {
            if (padded) v = cb[(size_t)m * Tc + f];
            else {
                v = cb[(size_t)m * Tc + min(max(f - w, 0), Tb - 1)];
                if (has_scaler) v = (v - scaler[m]) / scaler[PAUX + m];
            }
        }
        cs[m][j] = v;
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r0 = blockIdx.y * fdpwg::FRONT_ROWS + wv * 16, ld = PAUX * K;
    const float *Wr = Wc + (size_t)r0 * ld;
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    for (int m = 0; m < PAUX; ++m)
        for (int k = 0; k < K; ++k) {
            const float cv = cs[m][tx + k];
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = fmaf(Wr[(size_t)i * ld + m * K + k], cv, acc[i]);
        }
    const int t = t0 + tx;
    if (t < Tb) {
#pragma unroll
        for (int i = 0; i < 16; ++i) G[((size_t)b * rows + r0 + i) * T + t] = acc[i];
    }
}

__global__ void __launch_bounds__(256) k_pwg_coef(const float *__restrict__ phase, PwgStages st, const long long *__restrict__ lens, int T,
                                                  float *__restrict__ Kc)
{
    const int b = blockIdx.y;
    const long long L = (long long)st.hop * T, Lb = (long long)st.hop * own_len(lens, b, T);
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= Lb) return;
    double kk[PNEIGH] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int paths = 1;
    for (int i = 0; i < st.n; ++i) paths *= 3;
    const long long base0 = t / st.hop;
    for (int code = 0; code < paths; ++code) {
        long long q = t, len = Lb;
        double coef = 1.0;
        int cc = code;
        bool ok = true;
        for (int i = st.n - 1; i >= 0 && ok; --i) {
            const int s = st.s[i];
            const long long base = q / s;
            const int p = (int)(q - base * s), dsel = cc % 3;
            cc /= 3;
            coef *= (double)phase[(i * fdpwg::MAX_SCALE + p) * 3 + dsel];
            q = base + dsel - 1;
            len /= s;                                      // samples of the item at the rate below this stage
            ok = q >= 0 && q < len;
        }
        const long long j = q - base0 + 2;
        if (ok && j >= 0 && j < PNEIGH) kk[j] += coef;
    }
#pragma unroll
    for (int j = 0; j < PNEIGH; ++j) Kc[((size_t)b * PNEIGH + j) * L + t] = (float)kk[j];
}

template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(256, LAYER_WAVES_PER_SIMD) k_pwg_layer(const float *__restrict__ xin, const float *__restrict__ z, float *__restrict__ xout,
                                                   float *__restrict__ skip, const float *__restrict__ G, size_t g_item, const float *__restrict__ Kc,
                                                   const float *__restrict__ Wl, const float *__restrict__ w1, const float *__restrict__ b1,
                                                   const long long *__restrict__ lens, const unsigned long long *__restrict__ ids,
                                                   unsigned long long seed, int T, int hop, int d)
{
    __shared__ float hs[4][PRES][32];                       // a wave's h [64 channels][32 samples]: one column block at a time
    const int b = blockIdx.y;
    const int Tb = (int)own_len(lens, b, T);
    const int L = hop * T, Lb = hop * Tb, tile0 = blockIdx.x * fdpwg::TILE;
    if (tile0 >= Lb) return;                                // (uniform over the workgroup)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 31, hi = lane >> 5;
    const size_t item = (size_t)b * PRES * L;
    const float *bias = Wl + fdpwg::L_BIAS, *Wm = Wl + fdpwg::L_MIX, *mixb = Wl + fdpwg::L_MIXB;
    const float *Gb = G + (size_t)b * g_item;
    const unsigned long long id = (FIRST && ids) ? ids[b] : (unsigned long long)b;

    for (int part = 0; part < fdpwg::TILE / (4 * fdpwg::WAVE_COLS); ++part) {
        const int tw = tile0 + (part * 4 + wv) * fdpwg::WAVE_COLS;
        if (tile0 + part * 4 * fdpwg::WAVE_COLS >= Lb) break;      // (uniform over the workgroup)

        float zt[2][3];
        if (FIRST) {
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int pos = tw + cb * 32 + col + (j - 1) * d;
                    zt[cb][j] = 0.0f;
                    if (pos >= 0 && pos < Lb) zt[cb][j] = z ? z[(size_t)b * L + pos] : pwg_z(seed, id, pos);
                }
        }
        // the conditioning: the five coefficients of each of the lane's two samples, on the frames q - 2 .. q + 2 of its own frame q;
        // the wave's 64 samples lie under the frames F0 .. F0 + ne - 2, and entry ne - 1 of that list is the bias
        float kc[2][PNEIGH];
        int fq[2];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const int tt = min(tw + cb * 32 + col, Lb - 1);
            fq[cb] = tt / hop - 2;
#pragma unroll
            for (int j = 0; j < PNEIGH; ++j) kc[cb][j] = (Kc + (size_t)b * PNEIGH * L)[(unsigned)(j * L + tt)];
        }
        const int F0 = tw / hop - 2, ne = min(tw + fdpwg::WAVE_COLS - 1, Lb - 1) / hop + 2 - F0 + 2;

        // per tap: one base per step that is the same for every lane, and two 32-bit lane offsets; a position outside the item reads
        // the item's first sample instead and is then replaced by zero
        unsigned o0[3], o1[3];
        bool in0[3], in1[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int p0 = tw + col + (j - 1) * d, p1 = p0 + 32;
            in0[j] = p0 >= 0 && p0 < Lb;
            in1[j] = p1 >= 0 && p1 < Lb;
            o0[j] = (unsigned)(hi * L + (in0[j] ? p0 : 0));
            o1[j] = (unsigned)(hi * L + (in1[j] ? p1 : 0));
        }
        // (a zero the compiler cannot see through, made again for every part: addresses formed from it are not invariant over the parts,
        // so the several hundred of a pass are not all computed up front and kept in registers)
        const int zs = __builtin_amdgcn_readfirstlane(fdk_fast::opaque(0));
        const float *Wp = Wl + zs, *xp = xin + item + zs;
        // the operands of steps 4 c .. 4 c + 3 of pass ps (step = tap 32 + channel pair): the weights' two row blocks, x at the two columns
        auto fetch = [&](int c, int ps, float (&a0)[4], float (&a1)[4], float (&v0)[4], float (&v1)[4]) {
            const int j = c >> 3;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k2 = (c & 7) * 4 + i;
                const float *A = Wp + (j * 32 + k2) * 256 + ps * 64;
                a0[i] = A[(unsigned)lane];
                a1[i] = A[(unsigned)lane + 128u];
                if (FIRST) {
                    const int ch = 2 * k2 + hi;
                    v0[i] = in0[j] ? fmaf(w1[ch], zt[0][j], b1[ch]) : 0.0f;
                    v1[i] = in1[j] ? fmaf(w1[ch], zt[1][j], b1[ch]) : 0.0f;
                } else {
                    const float *xk = xp + (size_t)(2 * k2) * L;
                    const float x0 = xk[o0[j]], x1 = xk[o1[j]];
                    v0[i] = in0[j] ? x0 : 0.0f;
                    v1[i] = in1[j] ? x1 : 0.0f;
                }
            }
        };
        // 128 x 192, k = (tap, channel), two channels per step; in two passes over the rows: pass p holds rows 32 p .. 32 p + 31 of
        // the tanh half and of the sigmoid half, which gate each other in registers
        float hreg[2][16];                                  // h of the second column block, until the first has been through LDS
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            f32x16 acc[2][2];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[u][cb][r] = 0.0f;
            // (operands four steps at a time, the next four requested before the matrix pipe takes these: the loads come from L2 and
            // there are two waves on a SIMD to hide them behind)
            float ca0[4], ca1[4], cv0[4], cv1[4];
            fetch(0, ps, ca0, ca1, cv0, cv1);
#pragma unroll
            for (int c = 0; c < 24; ++c) {
                float na0[4], na1[4], nv0[4], nv1[4];
                if (c + 1 < 24) fetch(c + 1, ps, na0, na1, nv0, nv1);
                __builtin_amdgcn_sched_barrier(0);          // (or every load of the pass is moved to its top)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[0][0] = mfma32(ca0[i], cv0[i], acc[0][0]);
                    acc[0][1] = mfma32(ca0[i], cv1[i], acc[0][1]);
                    acc[1][0] = mfma32(ca1[i], cv0[i], acc[1][0]);
                    acc[1][1] = mfma32(ca1[i], cv1[i], acc[1][1]);
                }
                if (c + 1 < 24) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) { ca0[i] = na0[i]; ca1[i] = na1[i]; cv0[i] = nv0[i]; cv1[i] = nv1[i]; }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // ... and the conditioning and the bias as further steps of the same contraction: k = a frame of G under the wave (the
            // coefficient of a sample on it, zero off its five) or the bias entry (one)
            for (int s2 = 0; 2 * s2 < ne; ++s2) {
                const int e = 2 * s2 + hi, f = F0 + e, row = ps * 32 + col;
                const bool isf = e < ne - 1, isb = e == ne - 1, fv = isf && f >= 0 && f < Tb;
                const unsigned go = (unsigned)(row * T + min(max(f, 0), Tb - 1));
                const float g0 = Gb[go], g1 = Gb[go + (unsigned)(fdpwg::HALF * T)];
                const float a0 = isf ? g0 : (isb ? bias[row] : 0.0f);
                const float a1 = isf ? g1 : (isb ? bias[fdpwg::HALF + row] : 0.0f);
                const float bv0 = fv ? pwg_pick(kc[0], f - fq[0]) : (isb ? 1.0f : 0.0f);
                const float bv1 = fv ? pwg_pick(kc[1], f - fq[1]) : (isb ? 1.0f : 0.0f);
                acc[0][0] = mfma32(a0, bv0, acc[0][0]);
                acc[0][1] = mfma32(a0, bv1, acc[0][1]);
                acc[1][0] = mfma32(a1, bv0, acc[1][0]);
                acc[1][1] = mfma32(a1, bv1, acc[1][1]);
            }
            // the gate, in the result layout; h of the first column block into the wave's LDS slice
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float hv = tanhf(acc[0][cb][r]) * (1.0f / (1.0f + expf(-acc[1][cb][r])));
                    if (cb == 0) hs[wv][ps * 32 + drow(r, hi)][col] = hv;
                    else hreg[ps][r] = hv;
                }
        }
        __syncthreads();

        // 128 x 64: out over skip, one column block at a time
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            if (cb == 1) {
                __syncthreads();
#pragma unroll
                for (int ps = 0; ps < 2; ++ps)
#pragma unroll
                    for (int r = 0; r < 16; ++r) hs[wv][ps * 32 + drow(r, hi)][col] = hreg[ps][r];
                __syncthreads();
            }
            f32x16 o[4];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[rb][r] = 0.0f;
#pragma unroll 4
            for (int s = 0; s < 32; ++s) {
                const float bv = hs[wv][2 * s + hi][col];
                const float *A = Wm + s * 256;
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) o[rb] = mfma32(A[(unsigned)(lane + rb * 64)], bv, o[rb]);
            }
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) o[rb] = mfma32(hi ? 0.0f : mixb[rb * 32 + col], 1.0f, o[rb]);      // the two biases: one more step, times one
            const int t = tw + cb * 32 + col;
            if (t < Lb) {
                const float zc = FIRST ? zt[cb][1] : 0.0f;
#pragma unroll
                for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = rb * 32 + drow(r, hi);
                        const unsigned at = (unsigned)(row * L + t);
                        if (!LAST) {
                            const float xo = FIRST ? fmaf(w1[row], zc, b1[row]) : (xin + item)[at];
                            (xout + item)[at] = (o[rb][r] + xo) * 0.70710678118654752f;
                        }
                        (skip + item)[at] = FIRST ? o[rb + 2][r] : (skip + item)[at] + o[rb + 2][r];
                        if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // (four rows' loads in flight at a time, not all 32)
                    }
            }
        }
        __syncthreads();                                    // (the next part writes hs again)
    }
}

__global__ void __launch_bounds__(256) k_pwg_tail(const float *__restrict__ skip, const float *__restrict__ W1, const float *__restrict__ b1,
                                                  const float *__restrict__ w2, const float *__restrict__ b2, const long long *__restrict__ lens, int T,
                                                  int hop, float scale, float *__restrict__ wav, long long pitch)
{
    const int b = blockIdx.y;
    const int L = hop * T, Lb = hop * (int)own_len(lens, b, T);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 31, hi = lane >> 5;
    const int t = blockIdx.x * fdpwg::TAIL_COLS + wv * 32 + col;
    float *out = wav + (size_t)b * pitch;
    if ((int)(blockIdx.x * fdpwg::TAIL_COLS) >= Lb) {       // (uniform over the workgroup)
        if (hi == 0 && t < L) out[t] = 0.0f;
        return;
    }
    const float *sb = skip + (size_t)b * PRES * L;
    f32x16 o[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[rb][r] = 0.0f;
#pragma unroll 4
    for (int s = 0; s < 32; ++s) {
        const float v = t < Lb ? fmaxf(sb[(size_t)(2 * s + hi) * L + t] * scale, 0.0f) : 0.0f;
        const float *A = W1 + (size_t)s * 128 + lane;
        o[0] = mfma32(A[0], v, o[0]);
        o[1] = mfma32(A[64], v, o[1]);
    }
    float part = 0.0f;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = rb * 32 + drow(r, hi);
            part = fmaf(w2[row], fmaxf(o[rb][r] + b1[row], 0.0f), part);
        }
    const float tot = part + __shfl_xor(part, 32);          // (an add commutes: both half waves hold the same bits)
    if (hi == 0 && t < L) out[t] = t < Lb ? tot + b2[0] : 0.0f;
}

__global__ void __launch_bounds__(256) k_pwg_draw(const unsigned long long *__restrict__ ids, unsigned long long seed, long long L,
                                                  float *__restrict__ z, long long pitch)
{
    const int b = blockIdx.y;
    const long long i4 = (long long)blockIdx.x * 256 + threadIdx.x;
    if (4 * i4 >= L) return;
    const float4 q = philox_normal4(seed, FD_PWG_PHILOX_STREAM, (uint64_t)i4, ids ? ids[b] : (unsigned long long)b);
    float *o = z + (size_t)b * pitch + 4 * i4;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (4 * i4 + c < L) o[c] = fdk_fast::f4c(q, c);
}

hipError_t pwg_draw(const Launch &La, int B, long long L, unsigned long long seed, const unsigned long long *ids_dev, float *z_out, long long pitch)
{
    FD_LAUNCH(La, "pwg_draw", k_pwg_draw, dim3((unsigned)(((L + 3) / 4 + 255) / 256), (unsigned)B), dim3(256), 0, ids_dev, seed, L, z_out, pitch);
    return hipSuccess;
}

hipError_t pwg_generate(const Launch &La, const PwgNet &net, const float *src, int padded, int B, int T, const long long *lens_dev,
                        const unsigned long long *ids_dev, const float *z, unsigned long long seed, float *wav, long long pitch, void *scratch)
{
    const fd_pwg_config &c = net.cfg;
    const fdpwg::Image im = fdpwg::image(c);
    const int hop = fdpwg::hop(c), layers = c.layers, rows = PGATE * layers, L = hop * T;
    const fdpwg::Layout o = fdpwg::layout(layers, hop, B, T);
    char *p = static_cast<char *>(scratch);
    float *G = reinterpret_cast<float *>(p + o.G), *Kc = reinterpret_cast<float *>(p + o.K), *skip = reinterpret_cast<float *>(p + o.skip);
    float *x[2] = {reinterpret_cast<float *>(p + o.x[0]), reinterpret_cast<float *>(p + o.x[1])};
    const float *img = net.img;
    PwgStages st{};
    st.n = c.n_scales;
    st.hop = hop;
    for (int i = 0; i < c.n_scales; ++i) st.s[i] = c.upsample_scales[i];

    FD_LAUNCH(La, "pwg_front", k_pwg_front, dim3((unsigned)((T + fdpwg::FRONT_FRAMES - 1) / fdpwg::FRONT_FRAMES), (unsigned)(rows / fdpwg::FRONT_ROWS), (unsigned)B),
              dim3(256), 0, src, padded, net.has_scaler ? 1 : 0, img + im.front, img + im.scaler, lens_dev, T, (int)c.aux_context_window, rows, G);
    FD_LAUNCH(La, "pwg_coef", k_pwg_coef, dim3((unsigned)((L + 255) / 256), (unsigned)B), dim3(256), 0, img + im.phase, st, lens_dev, T, Kc);
    const dim3 grid((unsigned)((L + fdpwg::TILE - 1) / fdpwg::TILE), (unsigned)B);
    const size_t g_item = (size_t)rows * T;
    const float *w1 = img + im.first_w, *b1 = img + im.first_b;
    for (int l = 0; l < layers; ++l) {
        const float *Wl = img + im.layer + fdpwg::LAYER_FLOATS * l, *Gl = G + (size_t)l * PGATE * T;
        const float *xin = l ? x[(l - 1) & 1] : nullptr;
        float *xout = x[l & 1];
        const int d = fdpwg::dilation(c, l);
        const bool first = l == 0, last = l == layers - 1;
#define FD_PWG_LAYER(F, Z)                                                                                                                     \
    FD_LAUNCH(La, "pwg_layer", (k_pwg_layer<F, Z>), grid, dim3(fdpwg::THREADS), 0, xin, z, xout, skip, Gl, g_item, (const float *)Kc, Wl, w1, b1, lens_dev, \
              ids_dev, seed, T, hop, d)
        if (first && last) FD_PWG_LAYER(true, true);
        else if (first) FD_PWG_LAYER(true, false);
        else if (last) FD_PWG_LAYER(false, true);
        else FD_PWG_LAYER(false, false);
#undef FD_PWG_LAYER
    }
    FD_LAUNCH(La, "pwg_tail", k_pwg_tail, dim3((unsigned)((L + fdpwg::TAIL_COLS - 1) / fdpwg::TAIL_COLS), (unsigned)B), dim3(256), 0, (const float *)skip,
              img + im.tail_w1, img + im.tail_b1, img + im.tail_w2, img + im.tail_b2, lens_dev, T, hop, (float)sqrt(1.0 / layers), wav, pitch);
    return hipSuccess;
}

}  // namespace fdk
