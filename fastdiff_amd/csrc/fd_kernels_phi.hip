// fd_kernels_phi.hip -- the scheduling network (fastdiff_amd/noisepred.py: NoisePredictor; this project's own design, the reference calls
// a `noise_pred` it never defines), the pieces of one training step of it around the frozen denoiser (phi_loss, util.py:328-362) and the
// greedy schedule search (noise_scheduling, util.py:254-288) with its state in device memory.  include/fastdiff_hip_train.h, last section.
//
// Sums run in the fixed order of fd_kernels_sums.h; partial sums live in the handle's step scratch.
#include <algorithm>

#include "fd_kernels_sums.h"

// The scalars of the draws, the residual, the search's update and its scalars are defined operation by operation (torch evaluates them as
// separate passes): no multiply-add contraction in this file.  (fmaf() calls stay what they say.)
#pragma clang fp contract(off)

namespace fdk {
namespace {

// ---- band energies -------------------------------------------------------------------------------------------------------------------
// y[b,c,f] = bias[c] + sum_k W[c,k] x[b, 32 f + k] over F = L / 32 - 1 frames of 64 samples at stride 32; feat[b,c] = log(1e-6 + mean_f y^2).
// A workgroup takes BP_FRAMES = 8 * RUN frames of one item: thread (g = t & 7, c = t >> 3) holds row c of W in registers and walks the
// RUN frames of run g; the eight runs of a channel sit in neighbouring lanes and are joined by a three-level butterfly.  The x tile
// (BP_FRAMES * 32 + 32 floats) is loaded 16 bytes per lane into LDS, four floats of padding after every run of 512 so that the eight
// runs of a 16-byte read fall on distinct banks.
constexpr int BP_C = 32, BP_K = 64, BP_HOP = 32;
constexpr int BP_G = WG / BP_C;                   // 8 runs per workgroup
constexpr int BP_FRAMES = BP_G * RUN;             // 128
constexpr int BP_TILE = BP_FRAMES * BP_HOP + BP_HOP;                  // floats of x a workgroup reads
constexpr int BP_RUNF = RUN * BP_HOP;                                  // floats between two runs: 512
constexpr int BP_LDS = BP_TILE + 4 * (BP_TILE / BP_RUNF + 1);
static_assert(BP_G == 8 && (BP_RUNF & (BP_RUNF - 1)) == 0, "the butterfly and the padding assume 8 runs of a power-of-two length");

__device__ __forceinline__ int bp_pad(int p) { return p + 4 * (p / BP_RUNF); }

// the workgroup's x tile: floats [32 f0, 32 f0 + BP_TILE) of the item, those behind L left out (no frame reads them)
__device__ __forceinline__ void bp_load_tile(float *tile, const float *xb, int64_t f0, int64_t L)
{
    const float4 *src = reinterpret_cast<const float4 *>(xb + f0 * BP_HOP);
    const int64_t left = L - f0 * BP_HOP;
    for (int i = threadIdx.x; i < BP_TILE / 4; i += WG)
        if ((int64_t)i * 4 + 4 <= left) *reinterpret_cast<float4 *>(tile + bp_pad(4 * i)) = src[i];
    __syncthreads();
}

__device__ __forceinline__ void bp_load_row(float (&w)[BP_K], const float *W, int c)
{
#pragma unroll
    for (int k = 0; k < BP_K; ++k) w[k] = W[c * BP_K + k];
}

// float4 k4 of local frame lf: its two halves of 32 samples may lie on either side of a padding gap
__device__ __forceinline__ float4 bp_x4(const float *tile, int lf, int k4)
{
    return *reinterpret_cast<const float4 *>(tile + bp_pad((lf + (k4 >> 3)) * BP_HOP) + 4 * (k4 & 7));
}

// one y: the 64 products added in tap order, then the bias
__device__ __forceinline__ float bp_y(const float (&w)[BP_K], const float *tile, int lf, float bias)
{
    float s = 0.0f;
#pragma unroll
    for (int k4 = 0; k4 < BP_K / 4; ++k4) {
        const float4 v = bp_x4(tile, lf, k4);
        s = fmaf(w[4 * k4 + 0], v.x, s);
        s = fmaf(w[4 * k4 + 1], v.y, s);
        s = fmaf(w[4 * k4 + 2], v.z, s);
        s = fmaf(w[4 * k4 + 3], v.w, s);
    }
    return s + bias;
}

// the eight runs of a channel (lanes that differ in their low three bits): (r0 + r1) + (r2 + r3) + ..., in every lane
__device__ __forceinline__ float bp_join(float v)
{
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    return v;
}

// grid (P, B) -> partial[(b P + p) 32 + c] = sum of y^2 over the workgroup's frames
__global__ void __launch_bounds__(WG) k_bandpool_partial(const float *x, const float *W, const float *bias, int64_t L, int64_t F, int P, float *partial)
{
    __shared__ __attribute__((aligned(16))) float tile[BP_LDS];
    const int g = threadIdx.x & (BP_G - 1), c = threadIdx.x >> 3;
    const int64_t f0 = (int64_t)blockIdx.x * BP_FRAMES;
    bp_load_tile(tile, x + (int64_t)blockIdx.y * L, f0, L);
    float w[BP_K];
    bp_load_row(w, W, c);
    const float bc = bias[c];
    float acc = 0.0f;
#pragma unroll 1
    for (int j = 0; j < RUN; ++j) {
        const int lf = g * RUN + j;
        if (f0 + lf < F) {
            const float y = bp_y(w, tile, lf, bc);
            acc = fmaf(y, y, acc);
        }
    }
    acc = bp_join(acc);
    if (g == 0) partial[((int64_t)blockIdx.y * P + blockIdx.x) * BP_C + c] = acc;
}

// grid (B): thread (c = t & 31, q = t >> 5) adds the partial sums p = q, q + 8, ... of channel c serially, the eight results are joined
// by the same tree through LDS.  mode 0: out[b,c] = log(1e-6 + mean); mode 1: out[b,c] = mean (what the backward divides by).
__global__ void __launch_bounds__(WG) k_bandpool_final(const float *partial, int P, int64_t F, int mode, float *out)
{
    __shared__ float red[BP_G][BP_C];
    const int c = threadIdx.x & (BP_C - 1), q = threadIdx.x >> 5;
    const float *src = partial + (int64_t)blockIdx.x * P * BP_C;
    float acc = 0.0f;
    for (int p = q; p < P; p += BP_G) acc += src[(int64_t)p * BP_C + c];
    red[q][c] = acc;
    __syncthreads();
    if (q == 0) {
        const float total = ((red[0][c] + red[1][c]) + (red[2][c] + red[3][c])) + ((red[4][c] + red[5][c]) + (red[6][c] + red[7][c]));
        const float mean = (float)((double)total / (double)F);
        out[(int64_t)blockIdx.x * BP_C + c] = mode == 0 ? logf(1e-6f + mean) : mean;
    }
}

// grid (P, B): y recomputed, dy = coef[b,c] y with coef = dfeat 2 / (F (1e-6 + mean y^2)); a thread adds dy x[32 f + k] over its run for
// all 64 taps (and dy itself: the bias), the eight runs are joined, -> part[(b P + p)][c][0..64]
constexpr int BP_OUT = BP_K + 1;
__global__ void __launch_bounds__(WG) k_bandpool_backward(const float *x, const float *W, const float *bias, const float *dfeat, const float *msq,
                                                          int64_t L, int64_t F, int P, float *part)
{
    __shared__ __attribute__((aligned(16))) float tile[BP_LDS];
    const int g = threadIdx.x & (BP_G - 1), c = threadIdx.x >> 3;
    const int64_t f0 = (int64_t)blockIdx.x * BP_FRAMES;
    bp_load_tile(tile, x + (int64_t)blockIdx.y * L, f0, L);
    float w[BP_K], acc[BP_K];
    bp_load_row(w, W, c);
#pragma unroll
    for (int k = 0; k < BP_K; ++k) acc[k] = 0.0f;
    const float bc = bias[c];
    const int64_t bc_i = (int64_t)blockIdx.y * BP_C + c;
    const float coef = (dfeat[bc_i] * 2.0f) / ((float)F * (1e-6f + msq[bc_i]));
    float dbias = 0.0f;
#pragma unroll 1
    for (int j = 0; j < RUN; ++j) {
        const int lf = g * RUN + j;
        if (f0 + lf < F) {
            const float dy = coef * bp_y(w, tile, lf, bc);
            dbias += dy;
#pragma unroll
            for (int k4 = 0; k4 < BP_K / 4; ++k4) {
                const float4 v = bp_x4(tile, lf, k4);
                acc[4 * k4 + 0] = fmaf(dy, v.x, acc[4 * k4 + 0]);
                acc[4 * k4 + 1] = fmaf(dy, v.y, acc[4 * k4 + 1]);
                acc[4 * k4 + 2] = fmaf(dy, v.z, acc[4 * k4 + 2]);
                acc[4 * k4 + 3] = fmaf(dy, v.w, acc[4 * k4 + 3]);
            }
        }
    }
    float *dst = part + (((int64_t)blockIdx.y * P + blockIdx.x) * BP_C + c) * BP_OUT;
#pragma unroll
    for (int k = 0; k < BP_K; ++k) {
        const float v = bp_join(acc[k]);
        if (g == 0) dst[k] = v;
    }
    dbias = bp_join(dbias);
    if (g == 0) dst[BP_K] = dbias;
}

// grid (32 channels): thread (o = t & 63, q = t >> 6) adds the workgroup results n = q, q + 4, ... of tap o serially (items in order,
// an item's workgroups in order), then (q0 + q1) + (q2 + q3); the bias gradient the same way in threads o = 0 of a second round.
__global__ void __launch_bounds__(WG) k_bandpool_backward_final(const float *part, int64_t n, float *dW, float *db)
{
    __shared__ float red[4][BP_K];
    const int c = blockIdx.x, o = threadIdx.x & 63, q = threadIdx.x >> 6;
    for (int round = 0; round < 2; ++round) {
        const int col = round == 0 ? o : BP_K;
        float acc = 0.0f;
        if (round == 0 || o == 0)
            for (int64_t i = q; i < n; i += 4) acc += part[(i * BP_C + c) * BP_OUT + col];
        red[q][o] = acc;
        __syncthreads();
        if (q == 0) {
            const float total = (red[0][o] + red[1][o]) + (red[2][o] + red[3][o]);
            if (round == 0) dW[c * BP_K + o] = total;
            else if (o == 0) db[c] = total;
        }
        __syncthreads();
    }
}

// ---- the head ------------------------------------------------------------------------------------------------------------------------
// in = (feat[0..31], ln beta_next, ln delta2) -> h = swish(fc1 in + b1) -> u = fc2 h + b2 -> ratio = 1e-4 + (1 - 2e-4) sigmoid(u) ->
// beta_hat = min(beta_next, delta2) ratio.  One workgroup of 64 threads, thread j = hidden unit j with row j of fc1 in registers; items in
// order; the sum over the hidden units is the wave's butterfly.
constexpr int HD_IN = 34, HD_H = 64, HD_F = 32;

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + expf(-v)); }

struct HeadItem {
    float in[HD_IN];
    float a, s, hid, u, sig, scale;      // pre-activation of unit j, its sigmoid, swish; the logit, its sigmoid; min(beta_next, delta2)
};

__device__ __forceinline__ void head_item(HeadItem &I, const float *feat, float bn, float d2, const float (&w1)[HD_IN], float b1, float w2, float b2)
{
#pragma unroll
    for (int i = 0; i < HD_F; ++i) I.in[i] = feat[i];
    I.in[HD_F] = logf(bn);
    I.in[HD_F + 1] = logf(d2);
    float a = 0.0f;
#pragma unroll
    for (int i = 0; i < HD_IN; ++i) a = fmaf(w1[i], I.in[i], a);
    I.a = a + b1;
    I.s = sigmoidf_(I.a);
    I.hid = I.a * I.s;
    I.u = wave_sum(w2 * I.hid) + b2;
    I.sig = sigmoidf_(I.u);
    I.scale = fminf(bn, d2);
}

__global__ void __launch_bounds__(HD_H) k_npred_head_forward(const float *feat, const float *beta_next, const float *delta2, int R, const float *W1,
                                                             const float *b1, const float *W2, const float *b2, int B, float *beta_hat,
                                                             float *ratio)
{
    const int j = threadIdx.x;
    float w1[HD_IN];
#pragma unroll
    for (int i = 0; i < HD_IN; ++i) w1[i] = W1[j * HD_IN + i];
    const float b1j = b1[j], w2j = W2[j], b2v = b2[0];
    float total = 0.0f;
    for (int b = 0; b < B; ++b) {
        const int r = R == 1 ? 0 : b;
        HeadItem I;
        head_item(I, feat + (int64_t)b * HD_F, beta_next[r], delta2[r], w1, b1j, w2j, b2v);
        const float rt = 1e-4f + (1.0f - 2e-4f) * I.sig;
        total += rt;
        if (j == 0) {
            ratio[b] = rt;
            if (R != 1) beta_hat[b] = I.scale * rt;
        }
    }
    if (j == 0 && R == 1) beta_hat[0] = fminf(beta_next[0], delta2[0]) * (total / (float)B);
}

// R = B only.  dbeta_hat [B] -> dW1 [64, 34], db1 [64], dW2 [64], db2 [1], dfeat [B, 32]; sums over the items in item order.
__global__ void __launch_bounds__(HD_H) k_npred_head_backward(const float *feat, const float *beta_next, const float *delta2, const float *W1,
                                                              const float *b1, const float *W2, const float *b2, const float *dbeta, int B,
                                                              float *dW1, float *db1, float *dW2, float *db2, float *dfeat)
{
    const int j = threadIdx.x;
    float w1[HD_IN], g1[HD_IN];
#pragma unroll
    for (int i = 0; i < HD_IN; ++i) {
        w1[i] = W1[j * HD_IN + i];
        g1[i] = 0.0f;
    }
    const float b1j = b1[j], w2j = W2[j], b2v = b2[0];
    float gb1 = 0.0f, gw2 = 0.0f, gb2 = 0.0f;
    for (int b = 0; b < B; ++b) {
        HeadItem I;
        head_item(I, feat + (int64_t)b * HD_F, beta_next[b], delta2[b], w1, b1j, w2j, b2v);
        const float du = ((dbeta[b] * I.scale) * (1.0f - 2e-4f)) * (I.sig * (1.0f - I.sig));
        gw2 = fmaf(du, I.hid, gw2);
        gb2 += du;
        const float da = (du * w2j) * (I.s + I.a * (I.s * (1.0f - I.s)));
        gb1 += da;
#pragma unroll
        for (int i = 0; i < HD_IN; ++i) g1[i] = fmaf(da, I.in[i], g1[i]);
#pragma unroll
        for (int i = 0; i < HD_F; ++i) {
            const float v = wave_sum(w1[i] * da);
            if (j == 0) dfeat[(int64_t)b * HD_F + i] = v;
        }
    }
#pragma unroll
    for (int i = 0; i < HD_IN; ++i) dW1[j * HD_IN + i] = g1[i];
    db1[j] = gb1;
    dW2[j] = gw2;
    if (j == 0) db2[0] = gb2;
}

// ---- the draws of phi_loss -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WG) k_phi_draw(const float4 *x0, const float *alpha, uint32_t T_train, uint32_t tau, int64_t l4, int64_t n4,
                                                 unsigned long long seed, const fd_train_state *state, unsigned long long iter_host, float4 *x_t,
                                                 float4 *z, float *steps, float *beta_nxt, float *delta, float *delta2)
{
    const int64_t i4 = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (i4 >= n4) return;
    const unsigned long long it = step_iter(state, iter_host);
    const int64_t b = i4 / l4;
    const uint32_t ts = tau + (uint32_t)(((uint64_t)item_word(seed, 0xFFFFFFFAu, b, it) * (uint64_t)(T_train - 2u * tau)) >> 32);      // in [tau, T_train - tau)
    const float a = alpha[ts], an = alpha[ts + tau];
    const float q = an / a;
    const float d = sqrtf(1.0f - a * a);
    if (i4 == b * l4) {
        steps[b] = (float)ts;
        beta_nxt[b] = 1.0f - q * q;
        delta[b] = d;
        delta2[b] = d * d;
    }
    const float4 n = philox_normal4(seed, 0xFFFFFFF9u, (uint64_t)i4, it);
    const float4 x = x0[i4];
    z[i4] = n;
    x_t[i4] = noised4(a, d, x, n);
}

// ---- the residual of phi_loss ------------------------------------------------------------------------------------------------------------
// r = delta z - (beta_hat / delta) eps;  m[b] = mean r^2,  s[b] = mean r eps.  grid (P, B): a workgroup sums RS_SLOTS float4s of item b
// (a thread RUN / 4 of them: a run of RUN elements), the P results of an item lie together in the scratch (m behind s: two planes).
constexpr int RS_SLOTS = (RUN / 4) * WG;
static_assert(RUN % 4 == 0, "a thread's run is whole float4s");

__device__ __forceinline__ void rs_add(float &am, float &as, float zv, float ev, float d, float k)
{
    const float r = d * zv - k * ev;
    am = fmaf(r, r, am);
    as = fmaf(r, ev, as);
}

__global__ void __launch_bounds__(WG) k_phi_residual_partial(const float4 *eps, const float4 *z, const float *delta, const float *beta_hat, int64_t l4,
                                                             int P, float *part_m, float *part_s)
{
    const int b = blockIdx.y;
    const float d = delta[b];
    const float k = beta_hat[b] / d;
    const float4 *e4 = eps + (int64_t)b * l4, *z4 = z + (int64_t)b * l4;
    float am = 0.0f, as = 0.0f;
#pragma unroll
    for (int j = 0; j < RUN / 4; ++j) {
        const int64_t s = (int64_t)blockIdx.x * RS_SLOTS + (int64_t)j * WG + threadIdx.x;
        if (s < l4) {
            const float4 ev = e4[s], zv = z4[s];
            rs_add(am, as, zv.x, ev.x, d, k);
            rs_add(am, as, zv.y, ev.y, d, k);
            rs_add(am, as, zv.z, ev.z, d, k);
            rs_add(am, as, zv.w, ev.w, d, k);
        }
    }
    am = block_sum(am);
    as = block_sum(as);
    if (threadIdx.x == 0) {
        part_m[(int64_t)b * P + blockIdx.x] = am;
        part_s[(int64_t)b * P + blockIdx.x] = as;
    }
}

// grid (B, 2): y = 0 -> m, y = 1 -> s
__global__ void __launch_bounds__(WG) k_phi_residual_final(const float *part_m, const float *part_s, int P, int64_t n, float *m, float *s)
{
    const float total = final_sum((blockIdx.y == 0 ? part_m : part_s) + (int64_t)blockIdx.x * P, P);
    if (threadIdx.x == 0) (blockIdx.y == 0 ? m : s)[blockIdx.x] = (float)((double)total / (double)n);
}

// ---- the schedule search ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_sched_init(fd_sched_state *st, float betaN, float alphaN)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    fd_sched_state s;
    s.alpha_cur = alphaN;
    s.beta_cur = betaN;
    s.stopped = 0;
    s.n_found = 0;
    for (int i = 0; i < FD_SCHED_MAX_STEPS; ++i) s.found[i] = 0.0f;
    s.step = 0.0f;
    s.ddim = 0;
    for (int i = 0; i < 4; ++i) s.coef[i] = 0.0f;
    s.cond[0] = betaN;
    s.cond[1] = 1.0f;
    *st = s;
}

// map_noise_scale_to_time_step (util.py:394-404) on float32 values: the clamps, the first bracket, frac as a float32 difference and
// quotient, the sum in double
__device__ __forceinline__ float sched_map(float a, const float *alpha, int T)
{
    if (a < alpha[T - 1]) return (float)(T - 1);
    if (a > alpha[0]) return 0.0f;
    for (int t = 0; t < T - 1; ++t) {
        const float hi = alpha[t], lo = alpha[t + 1];
        if (lo <= a && a <= hi) {
            float frac = hi - a;
            frac = frac / (hi - lo);
            return (float)((double)t + (double)frac);
        }
    }
    return -1.0f;
}

__global__ void __launch_bounds__(64) k_sched_begin(fd_sched_state *st, const float *beta_hat, int n_hat, double rho, const float *alpha, int T_train,
                                                    int ddim, float *steps_out, int B)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (st->stopped) return;
    if (beta_hat) {
        float sum = 0.0f;
        for (int i = 0; i < n_hat; ++i) sum += beta_hat[i];
        const float beta = sum / (float)n_hat;
        if ((double)beta < rho) {
            st->stopped = 2;
            return;
        }
        st->beta_cur = beta;
    }
    const float a = st->alpha_cur, bc = st->beta_cur;
    const float step = sched_map(a, alpha, T_train);
    if (step >= 0.0f && st->n_found < FD_SCHED_MAX_STEPS) st->found[st->n_found++] = bc;
    st->step = step;
    for (int b = 0; b < B; ++b) steps_out[b] = step;
    st->ddim = ddim;
    if (!ddim) {
        st->coef[0] = bc / sqrtf(1.0f - a * a);
        st->coef[1] = sqrtf(1.0f - bc);
        st->coef[2] = st->coef[3] = 0.0f;
    } else {
        const float a_next = a / sqrtf(1.0f - bc);
        const float c1 = a_next / a;
        st->coef[0] = c1;
        st->coef[1] = -sqrtf(1.0f - a * a) * c1;
        st->coef[2] = sqrtf(1.0f - a_next * a_next);
        st->coef[3] = 0.0f;
    }
}

__device__ __forceinline__ float sched_ddpm(float x, float e, float c, float d) { return (x - c * e) / d; }
__device__ __forceinline__ float sched_ddim(float x, float e, float c1, float c2, float c3) { return (c1 * x + c2 * e) + c3 * e; }

__global__ void __launch_bounds__(WG) k_sched_update(const fd_sched_state *st, float4 *x, const float4 *eps, int64_t n4)
{
    if (st->stopped) return;
    const int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (i >= n4) return;
    const float c0 = st->coef[0], c1 = st->coef[1], c2 = st->coef[2];
    float4 v = x[i];
    const float4 e = eps[i];
    if (!st->ddim) {
        v.x = sched_ddpm(v.x, e.x, c0, c1);
        v.y = sched_ddpm(v.y, e.y, c0, c1);
        v.z = sched_ddpm(v.z, e.z, c0, c1);
        v.w = sched_ddpm(v.w, e.w, c0, c1);
    } else {
        v.x = sched_ddim(v.x, e.x, c0, c1, c2);
        v.y = sched_ddim(v.y, e.y, c0, c1, c2);
        v.z = sched_ddim(v.z, e.z, c0, c1, c2);
        v.w = sched_ddim(v.w, e.w, c0, c1, c2);
    }
    x[i] = v;
}

__global__ void __launch_bounds__(64) k_sched_advance(fd_sched_state *st, float *cond_out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (st->stopped) return;
    const float a = st->alpha_cur / sqrtf(1.0f - st->beta_cur);
    st->alpha_cur = a;
    if (a > 1.0f) {
        st->stopped = 1;
        return;
    }
    st->cond[0] = cond_out[0] = st->beta_cur;
    st->cond[1] = cond_out[1] = 1.0f - a * a;
}

}  // namespace

int64_t bandpool_blocks(int64_t L) { return (L / BP_HOP - 1 + BP_FRAMES - 1) / BP_FRAMES; }
size_t bandpool_scratch_floats(int B, int64_t L, bool backward)
{
    const size_t P = (size_t)bandpool_blocks(L);
    return (size_t)B * P * BP_C + (backward ? (size_t)B * BP_C + (size_t)B * P * BP_C * BP_OUT : 0);
}

hipError_t bandpool_forward(const Launch &L_, const float *x, const float *W, const float *bias, int B, int64_t L, float *feat, float *scratch)
{
    const int64_t F = L / BP_HOP - 1;
    const int P = (int)bandpool_blocks(L);
    FD_LAUNCH(L_, "bandpool_partial", k_bandpool_partial, dim3((unsigned)P, (unsigned)B), dim3(WG), 0, x, W, bias, L, F, P, scratch);
    FD_LAUNCH(L_, "bandpool_final", k_bandpool_final, dim3((unsigned)B), dim3(WG), 0, (const float *)scratch, P, F, 0, feat);
    return hipSuccess;
}

hipError_t bandpool_backward(const Launch &L_, const float *x, const float *W, const float *bias, const float *dfeat, int B, int64_t L, float *dW,
                             float *db, float *scratch)
{
    const int64_t F = L / BP_HOP - 1;
    const int P = (int)bandpool_blocks(L);
    float *partial = scratch, *msq = partial + (size_t)B * P * BP_C, *part = msq + (size_t)B * BP_C;
    FD_LAUNCH(L_, "bandpool_partial", k_bandpool_partial, dim3((unsigned)P, (unsigned)B), dim3(WG), 0, x, W, bias, L, F, P, partial);
    FD_LAUNCH(L_, "bandpool_final", k_bandpool_final, dim3((unsigned)B), dim3(WG), 0, (const float *)partial, P, F, 1, msq);
    FD_LAUNCH(L_, "bandpool_backward", k_bandpool_backward, dim3((unsigned)P, (unsigned)B), dim3(WG), 0, x, W, bias, dfeat, (const float *)msq, L, F, P,
              part);
    FD_LAUNCH(L_, "bandpool_backward_final", k_bandpool_backward_final, dim3(BP_C), dim3(WG), 0, (const float *)part, (int64_t)B * P, dW, db);
    return hipSuccess;
}

hipError_t npred_head_forward(const Launch &L_, const float *feat, const float *beta_next, const float *delta2, int R, const float *W1,
                              const float *b1, const float *W2, const float *b2, int B, float *beta_hat, float *ratio)
{
    FD_LAUNCH(L_, "npred_head_forward", k_npred_head_forward, dim3(1), dim3(HD_H), 0, feat, beta_next, delta2, R, W1, b1, W2, b2, B, beta_hat, ratio);
    return hipSuccess;
}

hipError_t npred_head_backward(const Launch &L_, const float *feat, const float *beta_next, const float *delta2, const float *W1, const float *b1,
                               const float *W2, const float *b2, const float *dbeta_hat, int B, float *dW1, float *db1, float *dW2, float *db2,
                               float *dfeat)
{
    FD_LAUNCH(L_, "npred_head_backward", k_npred_head_backward, dim3(1), dim3(HD_H), 0, feat, beta_next, delta2, W1, b1, W2, b2, dbeta_hat, B, dW1,
              db1, dW2, db2, dfeat);
    return hipSuccess;
}

hipError_t phi_draw(const Launch &L_, const float *x0, const float *alpha, int T_train, int tau, int B, int64_t len, uint64_t seed,
                    const fd_train_state *state, uint64_t iter_host, float *x_t, float *z, float *steps, float *beta_nxt, float *delta,
                    float *delta2)
{
    const int64_t l4 = len / 4, n4 = l4 * B;
    FD_LAUNCH(L_, "phi_draw", k_phi_draw, dim3((unsigned)((n4 + WG - 1) / WG)), dim3(WG), 0, reinterpret_cast<const float4 *>(x0), alpha,
              (uint32_t)T_train, (uint32_t)tau, l4, n4, (unsigned long long)seed, state, (unsigned long long)iter_host,
              reinterpret_cast<float4 *>(x_t), reinterpret_cast<float4 *>(z), steps, beta_nxt, delta, delta2);
    return hipSuccess;
}

int64_t phi_residual_blocks(int64_t len) { return (len / 4 + RS_SLOTS - 1) / RS_SLOTS; }

hipError_t phi_residual_forward(const Launch &L_, const float *eps, const float *z, const float *delta, const float *beta_hat, int B, int64_t len,
                                float *m, float *s, float *scratch)
{
    const int P = (int)phi_residual_blocks(len);
    float *part_m = scratch, *part_s = scratch + (size_t)B * P;
    FD_LAUNCH(L_, "phi_residual_partial", k_phi_residual_partial, dim3((unsigned)P, (unsigned)B), dim3(WG), 0, reinterpret_cast<const float4 *>(eps),
              reinterpret_cast<const float4 *>(z), delta, beta_hat, len / 4, P, part_m, part_s);
    FD_LAUNCH(L_, "phi_residual_final", k_phi_residual_final, dim3((unsigned)B, 2), dim3(WG), 0, (const float *)part_m, (const float *)part_s, P, len,
              m, s);
    return hipSuccess;
}

hipError_t sched_init(const Launch &L_, fd_sched_state *state, float betaN, float alphaN)
{
    FD_LAUNCH(L_, "sched_init", k_sched_init, dim3(1), dim3(1), 0, state, betaN, alphaN);
    return hipSuccess;
}

hipError_t sched_begin(const Launch &L_, fd_sched_state *state, const float *beta_hat, int n_hat, double rho, const float *alpha, int T_train,
                       int ddim, float *steps_out, int B)
{
    FD_LAUNCH(L_, "sched_begin", k_sched_begin, dim3(1), dim3(1), 0, state, beta_hat, n_hat, rho, alpha, T_train, ddim, steps_out, B);
    return hipSuccess;
}

hipError_t sched_update(const Launch &L_, fd_sched_state *state, float *x, const float *eps, int64_t n, float *cond_out)
{
    const int64_t n4 = n / 4;
    FD_LAUNCH(L_, "sched_update", k_sched_update, dim3((unsigned)((n4 + WG - 1) / WG)), dim3(WG), 0, (const fd_sched_state *)state,
              reinterpret_cast<float4 *>(x), reinterpret_cast<const float4 *>(eps), n4);
    FD_LAUNCH(L_, "sched_advance", k_sched_advance, dim3(1), dim3(1), 0, state, cond_out);
    return hipSuccess;
}

}  // namespace fdk
