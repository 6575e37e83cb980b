// fd_kernels_step.hip -- the rest of a training step around the denoiser's forward and backward (include/fastdiff_hip_train.h, last
// section): the batch cut from a device-resident corpus, the draws of theta_timestep_loss, the MSE loss both ways, and
// clip_grad_norm_ + non-finite guard + AdamW over all parameter tensors, and an optional moving average of them behind it.  Everything a step decides -- the step index of the draws, the clip coefficient, the bias corrections, whether the
// update is skipped -- is read from and written to device memory, so a captured step replays with fresh draws and no host round trip.
//
// Sums (loss, squared gradient norm, distances) run in the fixed order of fd_kernels_sums.h; partial sums live in the handle's step scratch.
//
// All memory-bound and small next to the step (15.3 M parameters: 7 streams of 61 MB; the loss: 3 of 2 MB).  Tensors of the optimizer
// are addressed element-wise, 256 consecutive floats per wave-group instruction: parameter and gradient tensors are views of arbitrary
// offset and length (a weight-norm g of 1 element next to a 24576 x 64 x 3 weight), so no 16-byte alignment can be assumed there.
#include <algorithm>

#include "fd_kernels_sums.h"

// sqrt(1 - a a) of the draws and the optimizer's update are defined operation by operation (torch evaluates them as separate
// element-wise passes): no multiply-add contraction in this file.  (fmaf() calls stay what they say.)
#pragma clang fp contract(off)

namespace fdk {
namespace {

// ---- the draws ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WG) k_train_draw(const float4 *x0, const float *alpha, uint32_t T_train, int64_t l4, int64_t n4,
                                                   unsigned long long seed, const fd_train_state *state, unsigned long long iter_host,
                                                   float4 *x_t, float4 *z, float *steps)
{
    const int64_t i4 = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (i4 >= n4) return;
    const unsigned long long it = step_iter(state, iter_host);
    const int64_t b = i4 / l4;
    const uint32_t ts = (uint32_t)(((uint64_t)item_word(seed, 0xFFFFFFFDu, b, it) * (uint64_t)T_train) >> 32);      // < T_train
    if (i4 == b * l4) steps[b] = (float)ts;
    const float a = alpha[ts];
    const float d = sqrtf(1.0f - a * a);
    const float4 q = philox_normal4(seed, 0xFFFFFFFEu, (uint64_t)i4, it);
    const float4 x = x0[i4];
    z[i4] = q;
    x_t[i4] = noised4(a, d, x, q);
}

// ---- the batch ---------------------------------------------------------------------------------------------------------------------
// A training batch cut from a device-resident corpus (include/fastdiff_hip_train.h: fd_train_collate; fastdiff_amd/corpus.py holds the
// arenas and the host twin of the choice).  Which utterance and which window slot b of step `it` takes is a pure function of
// (seed, it, b, rank, world, n, T_item - F), recomputed by every thread (a few dozen Philox calls, uniform over the workgroup).

// pi_e(j): a 4-round balanced Feistel network on 2k bits (4^k >= n > 4^(k-1)), walked along its cycle until it lands below n -- a
// bijection of [0, n) for every epoch e, evaluated per element.  Round function: word 0 of the generator keyed (seed, stream
// 0xFFFFFFFB, position = half ^ (round << 28), id = e); n <= 2^28 keeps the round number clear of the half.
__device__ __forceinline__ uint64_t collate_perm(uint64_t j, uint64_t n, unsigned long long seed, unsigned long long e)
{
    int k = 0;
    while (((uint64_t)1 << (2 * k)) < n) ++k;
    const uint32_t mask = ((uint32_t)1 << k) - 1u;
    uint64_t x = j;
    do {
        uint32_t l = (uint32_t)(x >> k), r = (uint32_t)x & mask;
#pragma unroll 1
        for (uint32_t round = 0; round < 4; ++round) {
            uint32_t w[4];
            philox_keyed(seed, 0xFFFFFFFBu, (uint64_t)(r ^ (round << 28)), e, w);
            const uint32_t t = l ^ (w[0] & mask);
            l = r;
            r = t;
        }
        x = ((uint64_t)l << k) | r;
    } while (x >= n);
    return x;
}

constexpr int CL_MELS = 80;                      // mel bins of a frame
constexpr int CL_TF = 64;                        // frames per transposed tile: one wave writes 64 consecutive floats of a mel row
constexpr int CL_LD = CL_MELS + 1;               // tile row stride: 81 = 17 mod 32, so the 64 frames of a column read fall on distinct banks
constexpr int CL_WAV4 = 4 * WG;                  // float4s of waveform a workgroup copies

// What a workgroup of either collater copies once its slot's first frame is known: workgroups [0, mel_tiles) one transposed mel tile
// each, the others CL_WAV4 float4s of waveform.  tile: CL_TF * CL_LD floats of LDS.
__device__ __forceinline__ void collate_copy(float *tile, const float *wav_arena, const float *mel_arena, int64_t frame0, int hop, int F, int b,
                                             int mel_tiles, float *wavs, float *mels)
{
    if ((int)blockIdx.x < mel_tiles) {
        const int f0 = (int)blockIdx.x * CL_TF;
        const int nf = min(CL_TF, F - f0);
        const float *src = mel_arena + (frame0 + f0) * CL_MELS;
        for (int e = threadIdx.x; e < nf * CL_MELS; e += WG) {
            const int f = e / CL_MELS;
            tile[f * CL_LD + (e - f * CL_MELS)] = src[e];
        }
        __syncthreads();
        float *dst = mels + (int64_t)b * CL_MELS * F + f0;
        const int f = threadIdx.x & 63;
        if (f < nf)
            for (int m = threadIdx.x >> 6; m < CL_MELS; m += WG / 64) dst[(int64_t)m * F + f] = tile[f * CL_LD + m];
    } else {
        const int64_t l4 = (int64_t)F * (hop / 4);
        const float4 *src = reinterpret_cast<const float4 *>(wav_arena + frame0 * hop);
        float4 *dst = reinterpret_cast<float4 *>(wavs) + (int64_t)b * l4;
        const int64_t base = (int64_t)((int)blockIdx.x - mel_tiles) * CL_WAV4 + threadIdx.x;
#pragma unroll
        for (int j = 0; j < CL_WAV4 / WG; ++j) {
            const int64_t i = base + (int64_t)j * WG;
            if (i < l4) dst[i] = src[i];
        }
    }
}

// what the two collaters receive alike
struct CollateArgs {
    const float *wav_arena, *mel_arena;
    const int64_t *frame_off;
    int64_t n_items;
    int hop, F, B;
    unsigned long long seed;
    const fd_train_state *state;
    unsigned long long iter_host;
    int mel_tiles;
    float *wavs, *mels;
    int64_t *picked;
};

// Slot b = blockIdx.y of step `it` once its item is known: the window start (stream 0xFFFFFFFC, id = it), the record in `picked`
// ((-1, -1) for a slot that is not active), the copy.  grid (mel tiles + waveform chunks, B).  Source of the mel: the contiguous [F, 80]
// block of the arena, read element-wise in order (coalesced), written into LDS row by row; destination [80, F]: a wave reads one
// column of the tile and writes 64 consecutive floats.
__device__ __forceinline__ void collate_slot(const CollateArgs &a, unsigned long long it, int64_t item, bool active)
{
    __shared__ float tile[CL_TF * CL_LD];
    const int b = blockIdx.y;
    const int64_t first = a.frame_off[item];
    const int64_t range = a.frame_off[item + 1] - first - a.F;      // the window starts in [0, range)
    const uint32_t w = item_word(a.seed, 0xFFFFFFFCu, b, it);
    const bool ok = range >= 1 && range < ((int64_t)1 << 32);       // (a table that breaks the corpus' filter: nothing is read)
    const int64_t start = ok ? (int64_t)(((uint64_t)w * (uint64_t)range) >> 32) : -1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.picked[2 * b] = active ? item : -1;
        a.picked[2 * b + 1] = active ? start : -1;
    }
    if (!ok) return;
    collate_copy(tile, a.wav_arena, a.mel_arena, first + start, a.hop, a.F, b, a.mel_tiles, a.wavs, a.mels);
}

// training: slot b of step `it` on rank r of w takes place g = (it B + b) w + r of the stream of epochs, item pi_epoch(g mod n)
__global__ void __launch_bounds__(WG) k_train_collate(const CollateArgs a, int rank, int world)
{
    const unsigned long long it = step_iter(a.state, a.iter_host);
    const uint64_t g = (it * (uint64_t)a.B + (uint64_t)blockIdx.y) * (uint64_t)world + (uint64_t)rank;
    const uint64_t epoch = g / (uint64_t)a.n_items;
    collate_slot(a, it, (int64_t)collate_perm(g % (uint64_t)a.n_items, (uint64_t)a.n_items, a.seed, epoch), true);
}

// The batch of an evaluation pass (include/fastdiff_hip_train.h: fd_eval_collate; TrainCorpus.eval_plan is the host twin): slot b of
// batch `it` is item g = it B + b itself, in order and without wrapping; the window start is the training collater's draw (same
// stream, position and word, the id = the batch index).  A slot behind the last item is cut from item n - 1 -- the forward then reads
// finite data -- and reported as (-1, -1): fd_eval_accumulate leaves it out.
__global__ void __launch_bounds__(WG) k_eval_collate(const CollateArgs a)
{
    const unsigned long long it = step_iter(a.state, a.iter_host);
    const uint64_t g = it * (uint64_t)a.B + (uint64_t)blockIdx.y;
    const bool active = g < (uint64_t)a.n_items;
    collate_slot(a, it, active ? (int64_t)g : a.n_items - 1, active);
}

// ---- the loss ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WG) k_mse_partial(const float *eps, const float *z, int64_t n, float *partial)
{
    const int64_t base = (int64_t)blockIdx.x * TILE + threadIdx.x;
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < RUN; ++j) {
        const int64_t i = base + (int64_t)j * WG;
        if (i < n) {
            const float d = eps[i] - z[i];
            acc = fmaf(d, d, acc);
        }
    }
    acc = block_sum(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(WG) k_mse_final(const float *partial, int64_t P, int64_t n, float *loss, fd_train_state *state)
{
    const float total = final_sum(partial, P);
    if (threadIdx.x == 0) {
        const float l = (float)((double)total / (double)n);
        *loss = l;
        if (state) state->loss = l;
    }
}

__global__ void __launch_bounds__(WG) k_mse_backward(const float *eps, const float *z, const float *dloss, int64_t n, float *deps)
{
    const float s = (float)(2.0 * (double)*dloss / (double)n);
    const int64_t base = (int64_t)blockIdx.x * TILE + threadIdx.x;
#pragma unroll
    for (int j = 0; j < RUN; ++j) {
        const int64_t i = base + (int64_t)j * WG;
        if (i < n) deps[i] = (eps[i] - z[i]) * s;
    }
}

// ---- an evaluation pass: per-item distances and the accumulators ---------------------------------------------------------------------
// fd_item_distance: out[i] = mean over item i's n elements of (a - b)^2 (kind 0) or |a - b| (kind 1).  grid (P, B): workgroup (p, i) sums
// 16-byte slots [p * ED_SLOTS, (p + 1) * ED_SLOTS) of item i, a thread RUN / 4 of them = a serial run of RUN elements, then block_sum; the P
// partial sums of an item lie together in the scratch and one final workgroup per item adds them (final_sum).  No workgroup touches two
// items.  The slots of an item are the ALIGNED float4s of the whole [B, n] array that it overlaps (n need not be a multiple of 4): a slot
// that lies wholly inside the item is one 16-byte load per operand, its first and last slot may be shared with a neighbour (or end
// behind the array) and are read element by element, the item's own elements only -- a neighbour's inf never enters the sum.
constexpr int ED_SLOTS = (RUN / 4) * WG;          // float4 slots per workgroup
static_assert(RUN % 4 == 0, "a thread's run is whole float4s");

__device__ __forceinline__ float dist_add(float acc, float x, float y, int kind)
{
    const float d = x - y;
    return kind == 0 ? fmaf(d, d, acc) : acc + fabsf(d);
}

__global__ void __launch_bounds__(WG) k_item_distance_partial(const float *a, const float *b, int64_t n, int kind, int P, float *partial)
{
    const int64_t lo = (int64_t)blockIdx.y * n, hi = lo + n;      // the item's elements in the whole array
    const int64_t s_lo = lo >> 2, s_hi = (hi + 3) >> 2;           // its slots
    const float4 *a4 = reinterpret_cast<const float4 *>(a), *b4 = reinterpret_cast<const float4 *>(b);
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < RUN / 4; ++j) {
        const int64_t s = s_lo + (int64_t)blockIdx.x * ED_SLOTS + (int64_t)j * WG + threadIdx.x;
        if (s >= s_hi) continue;
        const int64_t e = s << 2;
        if (e >= lo && e + 4 <= hi) {
            const float4 x = a4[s], y = b4[s];
            acc = dist_add(acc, x.x, y.x, kind);
            acc = dist_add(acc, x.y, y.y, kind);
            acc = dist_add(acc, x.z, y.z, kind);
            acc = dist_add(acc, x.w, y.w, kind);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (e + k >= lo && e + k < hi) acc = dist_add(acc, a[e + k], b[e + k], kind);
        }
    }
    acc = block_sum(acc);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * P + blockIdx.x] = acc;
}

__global__ void __launch_bounds__(WG) k_item_distance_final(const float *partial, int P, int64_t n, float *out)
{
    const float total = final_sum(partial + (int64_t)blockIdx.x * P, P);
    if (threadIdx.x == 0) out[blockIdx.x] = (float)((double)total / (double)n);
}

// fd_eval_accumulate: one workgroup.  Thread k < bins walks the slots in order and adds those of bin k; thread ACC_TOTAL walks them for
// the totals, the per-item output and the batch counter.  Every sum is therefore formed in slot order.  Whether a value takes part is
// decided on its bits (not_finite): the build lets the compiler drop ordinary NaN compares.
constexpr int ACC_TOTAL = FD_EVAL_MAX_BINS;
constexpr int ACC_WG = 2 * FD_EVAL_MAX_BINS;

__global__ void __launch_bounds__(ACC_WG) k_eval_accumulate(const float *values, const float *steps, const int64_t *picked, int B, int T_train,
                                                            int bins, fd_eval_state *acc, float *item_out, fd_train_state *advance)
{
    const int t = threadIdx.x;
    if (t == ACC_TOTAL) {
        double sum = acc->sum;
        uint64_t count = acc->count, bad = acc->nonfinite;
        for (int b = 0; b < B; ++b) {
            const int64_t item = picked[2 * b];
            if (item < 0) continue;
            const float v = values[b];
            if (item_out) item_out[item] = v;
            if (not_finite(v)) {
                ++bad;
            } else {
                sum += (double)v;
                ++count;
            }
        }
        acc->sum = sum;
        acc->count = count;
        acc->nonfinite = bad;
        if (advance) advance->iter += 1ull;
    } else if (steps && t < bins) {
        double sum = acc->bin_sum[t];
        uint64_t count = acc->bin_count[t];
        for (int b = 0; b < B; ++b) {
            if (picked[2 * b] < 0) continue;
            const float v = values[b], ts = steps[b];
            if (not_finite(v) || not_finite(ts)) continue;
            int64_t bin = ((int64_t)ts * bins) / T_train;
            bin = bin < 0 ? 0 : (bin >= bins ? bins - 1 : bin);      // (a step outside [0, T_train) lands in an end bin)
            if (bin != t) continue;
            sum += (double)v;
            ++count;
        }
        acc->bin_sum[t] = sum;
        acc->bin_count[t] = count;
    }
}

// ---- clip + guard + AdamW -------------------------------------------------------------------------------------------------------------
// The records travel as kernel arguments (<= AD_CHUNK per launch: 2.8 KB of the 4 KB a launch may carry), as weight_norm_multi's do.
// first_block: the first workgroup of each tensor (TILE elements per workgroup, no workgroup straddles two tensors).
constexpr int AD_CHUNK = 64;
struct AdamChunk {
    fd_adamw_item it[AD_CHUNK];
    int first_block[AD_CHUNK + 1];
    int n;
    int part0;      // this launch's first slot in the partial sums
    int last;       // the step's last launch: it advances the state
};

// what the final workgroup of the norm decides for the update launches (the head of the step scratch)
struct AdamDecision {
    float clip, decay, w1, beta2, w2, step_size, bc2_sqrt, eps;
    int skip;
};
constexpr int DEC_FLOATS = 16;
static_assert(sizeof(AdamDecision) <= DEC_FLOATS * sizeof(float), "the decision record's slot");

__global__ void __launch_bounds__(WG) k_adamw_norm(const AdamChunk c, float *partial, unsigned *flags)
{
    const int it = find_item(c, blockIdx.x);
    const float *g = c.it[it].g;
    const int64_t numel = c.it[it].numel;
    const int64_t base = (int64_t)(blockIdx.x - c.first_block[it]) * TILE + threadIdx.x;
    float acc = 0.0f;
    int bad = 0;
#pragma unroll
    for (int j = 0; j < RUN; ++j) {
        const int64_t i = base + (int64_t)j * WG;
        if (i < numel) {
            const float v = g[i];
            acc = fmaf(v, v, acc);
            bad |= not_finite(v) ? 1 : 0;
        }
    }
    acc = block_sum(acc);
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        partial[c.part0 + blockIdx.x] = acc;
        flags[c.part0 + blockIdx.x] = bad ? 1u : 0u;
    }
}

__device__ __forceinline__ double ipow(double x, unsigned long long t)      // x^t by squaring: a few double roundings
{
    double r = 1.0;
    while (t) {
        if (t & 1ull) r *= x;
        x *= x;
        t >>= 1;
    }
    return r;
}

__global__ void __launch_bounds__(WG) k_adamw_final(const float *partial, const unsigned *flags, int64_t P, const fd_adamw_hyper *hyper,
                                                    fd_train_state *state, AdamDecision *dec)
{
    int bad = 0;
    for (int64_t i = threadIdx.x; i < P; i += WG) bad |= (int)flags[i];
    const float total = final_sum(partial, P);
    bad = __syncthreads_or(bad);
    if (threadIdx.x != 0) return;
    const float norm = sqrtf(total);
    const fd_adamw_hyper hy = *hyper;
    const unsigned long long t = state->applied + 1ull;
    AdamDecision d;
    d.skip = (bad || not_finite(norm)) ? 1 : 0;
    const float coef = (float)hy.max_norm / (norm + 1e-6f);
    d.clip = (hy.max_norm != 0.0 && !d.skip && coef < 1.0f) ? coef : 1.0f;
    d.decay = (float)(1.0 - hy.lr * hy.weight_decay);
    d.w1 = (float)(1.0 - hy.beta1);
    d.beta2 = (float)hy.beta2;
    d.w2 = (float)(1.0 - hy.beta2);
    d.step_size = (float)(hy.lr / (1.0 - ipow(hy.beta1, t)));
    d.bc2_sqrt = (float)sqrt(1.0 - ipow(hy.beta2, t));
    d.eps = (float)hy.eps;
    *dec = d;
    state->grad_norm = norm;
}

__global__ void __launch_bounds__(WG) k_adamw_update(const AdamChunk c, const AdamDecision *dec, fd_train_state *state)
{
    const AdamDecision d = *dec;
    if (c.last && blockIdx.x == 0 && threadIdx.x == 0) {      // nothing else in this launch reads the state
        state->iter += 1ull;
        if (d.skip) state->skipped += 1ull; else state->applied += 1ull;
    }
    if (d.skip || (int)blockIdx.x >= c.first_block[c.n]) return;
    const int it = find_item(c, blockIdx.x);
    const float *g = c.it[it].g;
    float *p = c.it[it].p, *m = c.it[it].m, *v = c.it[it].v;
    const int64_t numel = c.it[it].numel;
    const int64_t base = (int64_t)(blockIdx.x - c.first_block[it]) * TILE + threadIdx.x;
#pragma unroll 4
    for (int j = 0; j < RUN; ++j) {
        const int64_t i = base + (int64_t)j * WG;
        if (i < numel) {
            const float gi = g[i] * d.clip;
            float pi = p[i] * d.decay, mi = m[i], vi = v[i];
            mi = mi + d.w1 * (gi - mi);
            vi = vi * d.beta2 + (d.w2 * gi) * gi;
            const float denom = sqrtf(vi) / d.bc2_sqrt + d.eps;
            pi = pi - (d.step_size * mi) / denom;
            p[i] = pi;
            m[i] = mi;
            v[i] = vi;
        }
    }
}

// ---- an exponential moving average of the parameters ---------------------------------------------------------------------------------
// fd_ema_multi (include/fastdiff_hip_train.h): e += w (p - e) over all tensors, behind the optimizer in stream order.  One thread decides
// -- whether the optimizer applied a step since the average last moved, and the weight of this update -- and stores that in the caller's
// fd_ema_state; the update launches only read it, as k_adamw_update reads k_adamw_final's record.  No scratch of the handle, no atomics.
// The records travel as kernel arguments (<= EMA_CHUNK per launch: 1.8 KB); TILE elements per workgroup, no workgroup straddles two
// tensors.
constexpr int EMA_CHUNK = 64;
struct EmaChunk {
    fd_ema_item it[EMA_CHUNK];
    int first_block[EMA_CHUNK + 1];
    int n;
};

__global__ void __launch_bounds__(64) k_ema_decide(const fd_ema_hyper *hyper, const fd_train_state *state, fd_ema_state *ema)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const fd_ema_hyper hy = *hyper;
    const unsigned long long updates = ema->updates, applied = state->applied;
    const int apply = applied > ema->seen_applied ? 1 : 0;
    double decay = hy.decay;
    if (hy.warmup != 0.0) {
        const double ramp = (1.0 + (double)updates) / (10.0 + (double)updates);
        decay = ramp < decay ? ramp : decay;
    }
    ema->w = (float)(1.0 - decay);
    ema->apply = apply;
    if (apply) {
        ema->seen_applied = applied;
        ema->updates = updates + 1ull;
    }
}

__device__ __forceinline__ float ema_step(float e, float p, float w) { return e + w * (p - e); }

__global__ void __launch_bounds__(WG) k_ema_update(const EmaChunk c, const fd_ema_state *ema)
{
    if (!ema->apply) return;
    const float w = ema->w;
    const int lo = find_item(c, blockIdx.x);
    const float *p = c.it[lo].p;
    float *e = c.it[lo].e;
    const int64_t numel = c.it[lo].numel;
    const int64_t tile0 = (int64_t)((int)blockIdx.x - c.first_block[lo]) * TILE;      // the tile's first element
    if (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(e)) & 15) == 0) {
        // 16 bytes per lane over the whole float4s of the tensor; its last numel % 4 elements one by one (they lie in the last tile)
        const float4 *p4 = reinterpret_cast<const float4 *>(p);
        float4 *e4 = reinterpret_cast<float4 *>(e);
        const int64_t n4 = numel >> 2;
        const int64_t base = (tile0 >> 2) + threadIdx.x;
#pragma unroll
        for (int j = 0; j < RUN / 4; ++j) {
            const int64_t i = base + (int64_t)j * WG;
            if (i < n4) {
                const float4 pv = p4[i];
                float4 ev = e4[i];
                ev.x = ema_step(ev.x, pv.x, w);
                ev.y = ema_step(ev.y, pv.y, w);
                ev.z = ema_step(ev.z, pv.z, w);
                ev.w = ema_step(ev.w, pv.w, w);
                e4[i] = ev;
            }
        }
        const int64_t t = (n4 << 2) + threadIdx.x;
        if (t < numel && t >= tile0 && t < tile0 + TILE) e[t] = ema_step(e[t], p[t], w);
    } else {
        const int64_t base = tile0 + threadIdx.x;
#pragma unroll 4
        for (int j = 0; j < RUN; ++j) {
            const int64_t i = base + (int64_t)j * WG;
            if (i < numel) e[i] = ema_step(e[i], p[i], w);
        }
    }
}

}  // namespace

size_t step_scratch_floats(int64_t blocks) { return (size_t)DEC_FLOATS + 2 * (size_t)blocks; }
int64_t mse_blocks(int64_t n) { return tiles(n); }
int64_t adamw_blocks(const fd_adamw_item *items, int n)
{
    int64_t blocks = 0;
    for (int i = 0; i < n; ++i)
        if (items[i].g) blocks += tiles(items[i].numel);
    return blocks;
}

hipError_t train_draw(const Launch &L_, const float *x0, const float *alpha, int T_train, int B, int64_t len, uint64_t seed,
                      const fd_train_state *state, uint64_t iter_host, float *x_t, float *z, float *steps)
{
    const int64_t l4 = len / 4, n4 = l4 * B;
    FD_LAUNCH(L_, "train_draw", k_train_draw, dim3((unsigned)((n4 + WG - 1) / WG)), dim3(WG), 0, reinterpret_cast<const float4 *>(x0), alpha,
              (uint32_t)T_train, l4, n4, (unsigned long long)seed, state, (unsigned long long)iter_host, reinterpret_cast<float4 *>(x_t),
              reinterpret_cast<float4 *>(z), steps);
    return hipSuccess;
}

hipError_t collate(const Launch &L_, bool eval, const float *wav_arena, const float *mel_arena, const int64_t *frame_off, int64_t n_items,
                   int hop, int F, int B, uint64_t seed, const fd_train_state *state, uint64_t iter_host, int rank, int world, float *wavs,
                   float *mels, int64_t *picked)
{
    const int mel_tiles = (F + CL_TF - 1) / CL_TF;
    const int64_t l4 = (int64_t)F * (hop / 4);
    const int wav_chunks = (int)((l4 + CL_WAV4 - 1) / CL_WAV4);
    const dim3 grid((unsigned)(mel_tiles + wav_chunks), (unsigned)B);
    const CollateArgs a = {wav_arena, mel_arena, frame_off, n_items, hop, F, B, (unsigned long long)seed, state, (unsigned long long)iter_host,
                           mel_tiles, wavs, mels, picked};
    if (eval) FD_LAUNCH(L_, "eval_collate", k_eval_collate, grid, dim3(WG), 0, a);
    else FD_LAUNCH(L_, "train_collate", k_train_collate, grid, dim3(WG), 0, a, rank, world);
    return hipSuccess;
}

// workgroups per item: the most slots an item of n elements overlaps (one more than n / 4 when its ends can lie inside slots)
int64_t item_distance_blocks(int64_t n)
{
    const int64_t slots = n % 4 == 0 ? n / 4 : (n + 3) / 4 + 1;
    return (slots + ED_SLOTS - 1) / ED_SLOTS;
}

hipError_t item_distance(const Launch &L_, const float *a, const float *b, int B, int64_t n, int kind, float *out, float *scratch)
{
    float *partial = scratch + DEC_FLOATS;
    const int P = (int)item_distance_blocks(n);
    FD_LAUNCH(L_, "item_distance_partial", k_item_distance_partial, dim3((unsigned)P, (unsigned)B), dim3(WG), 0, a, b, n, kind, P, partial);
    FD_LAUNCH(L_, "item_distance_final", k_item_distance_final, dim3((unsigned)B), dim3(WG), 0, (const float *)partial, P, n, out);
    return hipSuccess;
}

hipError_t eval_accumulate(const Launch &L_, const float *values, const float *steps, const int64_t *picked, int B, int T_train, int bins,
                           fd_eval_state *acc, float *item_out, fd_train_state *advance)
{
    FD_LAUNCH(L_, "eval_accumulate", k_eval_accumulate, dim3(1), dim3(ACC_WG), 0, values, steps, picked, B, T_train, bins, acc, item_out, advance);
    return hipSuccess;
}

hipError_t mse_forward(const Launch &L_, const float *eps, const float *z, int64_t n, float *loss, fd_train_state *state, float *scratch)
{
    float *partial = scratch + DEC_FLOATS;
    const int64_t P = tiles(n);
    FD_LAUNCH(L_, "mse_partial", k_mse_partial, dim3((unsigned)P), dim3(WG), 0, eps, z, n, partial);
    FD_LAUNCH(L_, "mse_final", k_mse_final, dim3(1), dim3(WG), 0, (const float *)partial, P, n, loss, state);
    return hipSuccess;
}

hipError_t mse_backward(const Launch &L_, const float *eps, const float *z, const float *dloss, int64_t n, float *deps)
{
    FD_LAUNCH(L_, "mse_backward", k_mse_backward, dim3((unsigned)tiles(n)), dim3(WG), 0, eps, z, dloss, n, deps);
    return hipSuccess;
}

// items: HOST memory
hipError_t adamw_multi(const Launch &L_, const fd_adamw_item *items, int n, const fd_adamw_hyper *hyper, fd_train_state *state, float *scratch)
{
    const int64_t P = adamw_blocks(items, n);
    AdamDecision *dec = reinterpret_cast<AdamDecision *>(scratch);
    float *partial = scratch + DEC_FLOATS;
    unsigned *flags = reinterpret_cast<unsigned *>(partial + P);
    // the tensors that took part, AD_CHUNK per launch
    std::vector<AdamChunk> chunks;
    int part0 = 0;
    for (int i = 0; i < n; ++i) {
        if (!items[i].g) continue;
        if (chunks.empty() || chunks.back().n == AD_CHUNK) {
            if (!chunks.empty()) part0 += chunks.back().first_block[AD_CHUNK];
            AdamChunk c;
            memset(&c, 0, sizeof(c));
            c.part0 = part0;
            chunks.push_back(c);
        }
        AdamChunk &c = chunks.back();
        c.it[c.n] = items[i];
        const int blocks = c.first_block[c.n] + (int)tiles(items[i].numel);
        for (int k = ++c.n; k <= AD_CHUNK; ++k) c.first_block[k] = blocks;
    }
    if (chunks.empty()) {      // no gradient at all: the norm is 0, the state still advances
        AdamChunk c;
        memset(&c, 0, sizeof(c));
        chunks.push_back(c);
    }
    chunks.back().last = 1;
    for (const AdamChunk &c : chunks)
        if (c.first_block[c.n] > 0) FD_LAUNCH(L_, "adamw_norm", k_adamw_norm, dim3((unsigned)c.first_block[c.n]), dim3(WG), 0, c, partial, flags);
    FD_LAUNCH(L_, "adamw_final", k_adamw_final, dim3(1), dim3(WG), 0, (const float *)partial, (const unsigned *)flags, P, hyper, state, dec);
    for (const AdamChunk &c : chunks)
        if (c.first_block[c.n] > 0 || c.last)
            FD_LAUNCH(L_, "adamw_update", k_adamw_update, dim3((unsigned)std::max(c.first_block[c.n], 1)), dim3(WG), 0, c, (const AdamDecision *)dec, state);
    return hipSuccess;
}

// items: HOST memory.  1 + ceil(n / EMA_CHUNK) launches.
hipError_t ema_multi(const Launch &L_, const fd_ema_item *items, int n, const fd_ema_hyper *hyper, const fd_train_state *state, fd_ema_state *ema)
{
    FD_LAUNCH(L_, "ema_decide", k_ema_decide, dim3(1), dim3(1), 0, hyper, state, ema);
    for (int i0 = 0; i0 < n; i0 += EMA_CHUNK) {
        EmaChunk c;
        memset(&c, 0, sizeof(c));
        c.n = std::min(EMA_CHUNK, n - i0);
        for (int k = 0; k < c.n; ++k) {
            c.it[k] = items[i0 + k];
            c.first_block[k + 1] = c.first_block[k] + (int)tiles(items[i0 + k].numel);
        }
        FD_LAUNCH(L_, "ema_update", k_ema_update, dim3((unsigned)c.first_block[c.n]), dim3(WG), 0, c, (const fd_ema_state *)ema);
    }
    return hipSuccess;
}

}  // namespace fdk
