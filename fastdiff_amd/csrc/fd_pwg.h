// fd_pwg.h -- host side of Parallel WaveGAN (include/fastdiff_hip_ext.h: "Parallel WaveGAN", which defines the computation): the
// configuration's refusals, the lengths, the tensors of a state dict with their sizes, the images fd_pwg_commit packs (the composed front
// convolution, the matrix instruction's operand order, the up-sampler's phase sums), the argument refusals and the scratch layout.  Plain
// C++ without the HIP runtime, so a stand-alone host program can include it.  tests/pwg_ref.py is the float64 oracle.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/fastdiff_hip_ext.h"

namespace fdpwg {

constexpr int RES = 64, GATE = 128, SKIP = 64, AUX = 80, HALF = GATE / 2;
constexpr int TILE = FD_PWG_TILE, THREADS = 256, WAVE_COLS = 64;      // a wave takes 64 samples at a time: two column blocks of the instruction
constexpr int MAX_B = 4096, MAX_T = FD_PWG_MAX_FRAMES, MAX_STAGES = FD_PWG_MAX_SCALES, MAX_SCALE = FD_PWG_MAX_SCALE;
constexpr int NEIGH = 5;                                               // frames q - 2 .. q + 2 under a sample of frame q
constexpr int FRONT_ROWS = 64, FRONT_FRAMES = 64;                      // outputs of one workgroup of the front kernel
constexpr int TAIL_COLS = 128;                                         // samples of one workgroup of the tail kernel
constexpr int MSG = 200;
static_assert((uint64_t)RES * FD_PWG_MAX_HOP * MAX_T * sizeof(float) <= (1ull << 32), "the layer kernel addresses an item's x with 32-bit byte offsets");
static_assert(TILE % ((THREADS / 64) * WAVE_COLS) == 0 && TILE % 256 == 0, "four waves of 64 samples, a whole number of times");

inline void default_config(fd_pwg_config *c)
{
    *c = fd_pwg_config{};
    c->in_channels = c->out_channels = 1; c->kernel_size = 3; c->layers = 30; c->stacks = 3;
    c->residual_channels = RES; c->gate_channels = GATE; c->skip_channels = SKIP; c->aux_channels = AUX; c->aux_context_window = 2;
    c->bias = 1; c->upsample_conditional_features = 1; c->upsample_net = FD_PWG_CONV_IN_UPSAMPLE;
    c->n_scales = 4;
    for (int i = 0; i < 4; ++i) c->upsample_scales[i] = 4;
    c->interpolate_nearest = 1; c->freq_axis_kernel_size = 1;
}

inline int hop(const fd_pwg_config &c)
{
    int h = 1;
    for (int i = 0; i < c.n_scales; ++i) h *= c.upsample_scales[i];
    return h;
}
inline int dilation(const fd_pwg_config &c, int layer) { return 1 << (layer % (c.layers / c.stacks)); }

// null = the specialised path takes it, else the field and its value in msg
inline const char *refusal(const fd_pwg_config &c, char (&msg)[MSG])
{
#define FD_PWG_WANT(field, want)                                                                                             \
    if (c.field != (want)) { snprintf(msg, MSG, #field " = %d: only %d is built", (int)c.field, (int)(want)); return msg; }
    FD_PWG_WANT(in_channels, 1) FD_PWG_WANT(out_channels, 1) FD_PWG_WANT(kernel_size, 3)
    FD_PWG_WANT(residual_channels, RES) FD_PWG_WANT(gate_channels, GATE) FD_PWG_WANT(skip_channels, SKIP) FD_PWG_WANT(aux_channels, AUX)
    FD_PWG_WANT(bias, 1) FD_PWG_WANT(use_causal_conv, 0) FD_PWG_WANT(upsample_conditional_features, 1)
    FD_PWG_WANT(use_pitch_embed, 0) FD_PWG_WANT(use_nsf, 0) FD_PWG_WANT(upsample_net, FD_PWG_CONV_IN_UPSAMPLE)
    FD_PWG_WANT(upsample_activation, 0) FD_PWG_WANT(interpolate_nearest, 1) FD_PWG_WANT(freq_axis_kernel_size, 1)
#undef FD_PWG_WANT
    if (c.layers < 1 || c.layers > FD_PWG_MAX_LAYERS) { snprintf(msg, MSG, "layers = %d outside 1 .. %d", c.layers, FD_PWG_MAX_LAYERS); return msg; }
    if (c.stacks < 1 || c.layers % c.stacks != 0) { snprintf(msg, MSG, "stacks = %d does not divide layers = %d", c.stacks, c.layers); return msg; }
    if (c.layers / c.stacks > 10) {
        snprintf(msg, MSG, "stacks = %d with layers = %d: dilation %lld above %d", c.stacks, c.layers, 1ll << (c.layers / c.stacks - 1), FD_PWG_MAX_DILATION);
        return msg;
    }
    if (c.aux_context_window < 0 || c.aux_context_window > FD_PWG_MAX_CONTEXT) {
        snprintf(msg, MSG, "aux_context_window = %d outside 0 .. %d", c.aux_context_window, FD_PWG_MAX_CONTEXT);
        return msg;
    }
    if (c.n_scales < 1 || c.n_scales > MAX_STAGES) { snprintf(msg, MSG, "upsample_scales: %d scales outside 1 .. %d", c.n_scales, MAX_STAGES); return msg; }
    for (int i = 0; i < c.n_scales; ++i)
        if (c.upsample_scales[i] < 2 || c.upsample_scales[i] > MAX_SCALE) {
            snprintf(msg, MSG, "upsample_scales[%d] = %d outside 2 .. %d", i, c.upsample_scales[i], MAX_SCALE);
            return msg;
        }
    if (hop(c) > FD_PWG_MAX_HOP) { snprintf(msg, MSG, "upsample_scales: hop = %d above %d", hop(c), FD_PWG_MAX_HOP); return msg; }
    return nullptr;
}

inline int64_t samples(const fd_pwg_config &c, int64_t frames)
{
    char msg[MSG];
    return (refusal(c, msg) || frames < 0) ? -1 : (int64_t)hop(c) * frames;
}
inline int64_t receptive_field(const fd_pwg_config &c)
{
    char msg[MSG];
    if (refusal(c, msg)) return -1;
    int64_t sum = 0;
    for (int l = 0; l < c.layers; ++l) sum += dilation(c, l);
    return 2 * sum + 1;
}

// The tensors of the state dict after weight-norm removal, in the reference's order, with their element counts
struct Tensor { std::string name; size_t n; };
inline std::vector<Tensor> tensors(const fd_pwg_config &c)
{
    std::vector<Tensor> t;
    const int K = 2 * c.aux_context_window + 1;
    t.push_back({"first_conv.weight", (size_t)RES});
    t.push_back({"first_conv.bias", (size_t)RES});
    t.push_back({"upsample_net.conv_in.weight", (size_t)AUX * AUX * K});
    for (int i = 0; i < c.n_scales; ++i) t.push_back({"upsample_net.upsample.up_layers." + std::to_string(2 * i + 1) + ".weight", (size_t)2 * c.upsample_scales[i] + 1});
    for (int l = 0; l < c.layers; ++l) {
        const std::string p = "conv_layers." + std::to_string(l) + ".";
        t.push_back({p + "conv.weight", (size_t)GATE * RES * 3});
        t.push_back({p + "conv.bias", (size_t)GATE});
        t.push_back({p + "conv1x1_aux.weight", (size_t)GATE * AUX});
        t.push_back({p + "conv1x1_out.weight", (size_t)RES * HALF});
        t.push_back({p + "conv1x1_out.bias", (size_t)RES});
        t.push_back({p + "conv1x1_skip.weight", (size_t)SKIP * HALF});
        t.push_back({p + "conv1x1_skip.bias", (size_t)SKIP});
    }
    t.push_back({"last_conv_layers.1.weight", (size_t)SKIP * SKIP});
    t.push_back({"last_conv_layers.1.bias", (size_t)SKIP});
    t.push_back({"last_conv_layers.3.weight", (size_t)SKIP});
    t.push_back({"last_conv_layers.3.bias", (size_t)1});
    return t;
}

// The device image, in floats from its start.  A matrix W [rows][k] in the exact-fp32 instruction's A-operand order: step s = k / 2,
// row block rb = row / 32, lane = (row & 31) + 32 (k & 1) -> [s][rb][lane]: a wave reads its 64 operands of one step as 256 bytes.
struct Image {
    size_t front;                  // [128 layers][80 (2 w + 1)]: W_aux_l conv_in, index (channel, tap)
    size_t first_w, first_b;       // [64] each
    size_t layer;                  // per layer LAYER_FLOATS: conv [96][4][64] (k = tap 64 + channel), bias [128], out | skip [32][4][64], bias [128]
    size_t tail_w1, tail_b1, tail_w2, tail_b2;      // [32][2][64], [64], [64], [1]
    size_t phase;                  // [MAX_STAGES][MAX_SCALE][3]: the sums of a stage's taps that fall on the neighbours q - 1, q, q + 1 at phase p
    size_t scaler;                 // mean [80], scale [80]
    size_t total;
};
constexpr size_t CONV_FLOATS = 96 * 4 * 64, MIX_FLOATS = 32 * 4 * 64, LAYER_FLOATS = CONV_FLOATS + GATE + MIX_FLOATS + GATE;
constexpr size_t L_CONV = 0, L_BIAS = CONV_FLOATS, L_MIX = CONV_FLOATS + GATE, L_MIXB = CONV_FLOATS + GATE + MIX_FLOATS;
inline Image image(const fd_pwg_config &c)
{
    Image o{};
    size_t at = 0;
    auto take = [&](size_t n) { const size_t p = at; at = (at + n + 63) & ~(size_t)63; return p; };
    o.front = take((size_t)GATE * c.layers * AUX * (2 * c.aux_context_window + 1));
    o.first_w = take(RES); o.first_b = take(RES);
    o.layer = take(LAYER_FLOATS * c.layers);
    o.tail_w1 = take(32 * 2 * 64); o.tail_b1 = take(SKIP); o.tail_w2 = take(SKIP); o.tail_b2 = take(1);
    o.phase = take((size_t)MAX_STAGES * MAX_SCALE * 3);
    o.scaler = take(2 * AUX);
    o.total = at;
    return o;
}
// W [rows][ld] (element (row, k) at W[row * ld + kmap(k)]) -> dst [K / 2][rows / 32][64]
template <class KMap>
inline void pack_a(float *dst, const float *W, int rows, int K, int ld, KMap kmap)
{
    const int RB = rows / 32;
    for (int k = 0; k < K; ++k)
        for (int row = 0; row < rows; ++row)
            dst[((size_t)(k >> 1) * RB + (row >> 5)) * 64 + (row & 31) + 32 * (k & 1)] = W[(size_t)row * ld + kmap(k)];
}
// stage taps [2 s + 1] -> [s][3]: at phase p the taps k < s - p fall on the neighbour q - 1, s - p <= k < 2 s - p on q, the rest on q + 1
inline void phase_sums(const float *taps, int s, float *dst)
{
    for (int p = 0; p < s; ++p) {
        double a[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k <= 2 * s; ++k) a[k < s - p ? 0 : (k < 2 * s - p ? 1 : 2)] += (double)taps[k];
        for (int j = 0; j < 3; ++j) dst[p * 3 + j] = (float)a[j];
    }
}

// null = accepted, else what is wrong, with the value, in msg (the pointers are the caller's to check)
inline const char *call_refusal(int hop_, int B, int T, int64_t wav_pitch, char (&msg)[MSG])
{
    if (B < 1 || B > MAX_B) { snprintf(msg, MSG, "B = %d items outside 1 .. %d", B, MAX_B); return msg; }
    if (T < 1 || T > MAX_T) { snprintf(msg, MSG, "T = %d frames outside 1 .. %d", T, MAX_T); return msg; }
    if (wav_pitch < (int64_t)hop_ * T) {
        snprintf(msg, MSG, "wav_pitch = %lld is less than the %lld samples of T = %d frames", (long long)wav_pitch, (long long)hop_ * T, T);
        return msg;
    }
    return nullptr;
}

// The scratch buffer, slots one after the other, each starting on a 256-byte border: lens [B] int64, ids [B] uint64, G [B][layers][128][T]
// float, K [B][5][L] float, two x buffers and skip [B][64][L] float
struct Layout { size_t lens, ids, G, K, x[2], skip, total; };
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline Layout layout(int layers, int hop_, int B, int T)
{
    Layout o{};
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t p = at; at = align256(at + bytes); return p; };
    const size_t bl = (size_t)B * (size_t)T * (size_t)hop_;
    o.lens = take(sizeof(int64_t) * (size_t)B);
    o.ids = take(sizeof(uint64_t) * (size_t)B);
    o.G = take(sizeof(float) * (size_t)B * layers * GATE * (size_t)T);
    o.K = take(sizeof(float) * bl * NEIGH);
    o.x[0] = take(sizeof(float) * bl * RES);
    o.x[1] = take(sizeof(float) * bl * RES);
    o.skip = take(sizeof(float) * bl * SKIP);
    o.total = at;
    return o;
}

}  // namespace fdpwg
