// fd_internal.h -- shared between the host side (fd_api.cpp, fd_weights.cpp) and the kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <string.h>
#include <map>
#include <string>
#include <vector>

#include "../../include/fastdiff_hip.h"
#include "../../include/fastdiff_hip_ext.h"
#include "../../include/fastdiff_hip_train.h"
#include "fd_loudness.h"
#include "fd_trim.h"
#include "fd_stoi.h"
#include "fd_pitch.h"
#include "fd_spectral.h"
#include "fd_gl.h"
#include "fd_nnls.h"
#include "fd_bins.h"
#include "fd_mcd.h"

// ---------------------------------------------------------------------------------------------
// Fixed architecture of this build (modules/FastDiff/config/base.yaml:21-33).  fd_create rejects
// anything else: the four dataset YAMLs of the reference never change the network shape.
// ---------------------------------------------------------------------------------------------
namespace fd {
constexpr int C = 32;          // inner_channels
constexpr int COND = 80;       // cond_channels
constexpr int HID = 64;        // kpnet_hidden_channels
constexpr int NBLK = 3;
constexpr int LAYERS = 4;      // lvc_layers_each_block
constexpr int HOPT = 256;      // prod(upsample_ratios)
constexpr int E_IN = 128, E_MID = 512, E_OUT = 512;
constexpr int KLAYER = 2 * C * C * 3;        // 6144 predicted-kernel floats per (frame, layer)
constexpr int KW = KLAYER * LAYERS;          // 24576
constexpr int KB = 2 * C * LAYERS;           // 256 predicted biases per frame
constexpr int KREC = KW + KB;                // 24832 floats: one frame's packed record
__host__ __device__ constexpr int ratio(int n) { return n == 2 ? 4 : 8; }        // upsample_ratios [8,8,4]
__host__ __device__ constexpr int hop(int n) { return n == 0 ? 8 : (n == 1 ? 64 : 256); }
__host__ __device__ constexpr int down_factor(int d) { return d == 0 ? 4 : 8; }   // reversed ratios (FastDiff_model.py:63)

// Packed position of predicted-kernel element K[layer][in][out][tap] inside a frame record.
// The record of one (frame, layer) is laid out as the A operand of v_mfma_f32_32x32x2_f32:
//   [mt][s4 = step/4][lane][r = step%4],  step = kk/2, lane = row + 32*(kk%2), kk = tap*32 + in
// so a lane fetches four consecutive k-steps of its row with one 16-byte load.  The 64 output channels are
// split over the two 32-row tiles so that each tile is closed under the gate (modules.py:217): gate channel
// ch = out%32 has its sigmoid input (out < 32) and its tanh input (out >= 32) in the SAME tile, 16 rows apart:
//   mt = ch/16,  row = ch%16 + 16*(out/32).
// In the MFMA result a lane then holds both halves of a channel (registers r and r+8), so sigmoid*tanh needs no
// cross-lane traffic, and for hop 256 a wave needs only ONE of the two tiles (48 instead of 96 operand registers).
__host__ __device__ inline int kernel_row(int out) { return (out & 15) + 16 * (out >> 5); }
__host__ __device__ inline int kernel_tile(int out) { return (out & 31) >> 4; }
__host__ __device__ inline int kernel_index(int layer, int in, int out, int tap)
{
    // A operand of a 32x32x16 MFMA: lane = row + 32*g holds the 8 consecutive k = 16*kg + 8*g + e, k = tap*32 + in
    const int kk = tap * C + in, kg = kk >> 4, g = (kk >> 3) & 1, e = kk & 7;
    const int mt = kernel_tile(out), lane = kernel_row(out) + 32 * g;
    return layer * KLAYER + ((mt * 6 + kg) * 64 + lane) * 8 + e;
}
// Position of predicted bias (layer, out): same [mt][row] order as the kernel rows.
__host__ __device__ inline int bias_index(int layer, int out) { return KW + layer * 64 + kernel_tile(out) * 32 + kernel_row(out); }
}  // namespace fd

// ---------------------------------------------------------------------------------------------
// Device-side weights
// ---------------------------------------------------------------------------------------------
struct ConvW {
    const float *w = nullptr;   // folded, reference layout [out][in][k]  (ConvTranspose: [in][out][k]; Linear: [out][in])
    const float *b = nullptr;
};

struct DevWeights {
    // reference-layout (naive kernels, VALU kernels)
    ConvW first, final_;
    struct { ConvW res, conv[3]; } down[fd::NBLK];
    struct { ConvW fc_t, up, kp_in, kp_res[6], kc, bc, convs[fd::LAYERS]; } blk[fd::NBLK];
    // embed MLP, transposed [in][out] so thread-per-output reads are coalesced
    const float *fc_t1_T = nullptr, *fc_t1_b = nullptr, *fc_t2_T = nullptr, *fc_t2_b = nullptr;
    const float *fc_t_T[fd::NBLK] = {}, *fc_t_b[fd::NBLK] = {};
    const float *embed_table = nullptr;           // [64] fp32 frequencies
    // MFMA A-operand packs ([mt][s4][lane][4], kk = tap*Cin + in)
    const float *down_pack[fd::NBLK][4] = {};     // conv0..2 (K=96), res 1x1 (K=32)
    const uint16_t *down_h2[fd::NBLK][4] = {};    // the same as two fp16 pieces: [piece][kg][64 lane][8]
    bool dblock_f16_ok = false;
    const float *lvc_conv_pack[fd::NBLK][fd::LAYERS] = {};
    const uint16_t *lvc_conv_h2[fd::NBLK][fd::LAYERS] = {};   // the same as two fp16 pieces: [piece][6 kg][64 lane][8], k = tap*32 + in
    const uint16_t *lvc_conv_h16[fd::LAYERS] = {};        // block 0 (hop 8): A operands of v_mfma_f32_16x16x32_f16: [row tile 2][tap 3][piece 2][64 lane][8]
    bool lvc_f16_ok = false;                      // every LVC conv weight fits the fp16 range
    const float *kp_in_pack[fd::NBLK] = {};       // 80->64 k5: 2 mt x 50 s4
    const float *kp_res_pack[fd::NBLK][6] = {};   // 64->64 k3: 2 mt x 24 s4
    const uint16_t *kp_in_h2[fd::NBLK] = {};      // the same as fp16 pieces: [2 mt][piece][25 kg][64 lane][8]
    const uint16_t *kp_res_h2[fd::NBLK][6] = {};  //                          [2 mt][piece][12 kg][64 lane][8]
    bool kpf_f16_ok = false;
    const float *gemm_pack[fd::NBLK] = {};        // kernel_conv+bias_conv as MFMA B operand: [776 ptile][24 s4][64][4]
    const float *gemm_bias[fd::NBLK] = {};        // [24832] conv biases in packed order
    const uint16_t *gemm_h2_pack[fd::NBLK] = {};  // same weights as two fp16 pieces (w1, (w-w1)*2^11): [776 ptile][2][12 kg][64 lane][8]
    bool gemm_f16_ok = false;                     // every GEMM weight fits the fp16 range
    // the same weights transformed for Winograd F(2,3) over the frame axis of kernel_conv (k_kp_gemm_w): per packed column four K = 64
    // blocks g0, (g0+g1+g2)/2, (g0-g1+g2)/2, -g2 (formed in double, rounded to fp32, split): [776 ptile][2 pieces][16 kg][64 lane][8]
    const uint16_t *gemm_w_pack[fd::NBLK] = {};
    bool gemm_w_ok = false;                       // ... and every transformed weight fits the fp16 range
    const float *up_pack[fd::NBLK] = {};          // ConvTranspose as per-phase A operands: [r phases][8 s4][64][4]
    const uint16_t *up_h2[fd::NBLK] = {};         // ConvTranspose per-phase slices as fp16 pieces: [ph][piece][4 kg][64 lane][8]
    bool convt_f16_ok = false;
    const float *final_fuse = nullptr;            // final_conv weights in the last LVC layer's register order: [mt*2 + hi][8 r][8] (7 taps + pad)
    const int *kc_perm = nullptr;                 // [24576] reference kernel_conv row -> packed position
    const int *bc_perm = nullptr;                 // [256] reference bias_conv row -> position inside the bias part
};

// ---------------------------------------------------------------------------------------------
// Per-call step description read by kernels from device memory (so a captured graph is pointer-free)
// ---------------------------------------------------------------------------------------------
struct StepParams {
    fd_step table[1024];
    const float *z;        // injected noise [N,B,L] or null
    float *seq;            // trajectory [N+1,B,L] or null
    unsigned long long seed;
    int n_steps;
    int ddim;
    int step_idx;          // advanced on device at the end of every captured step
    int l4;                // samples / 4 of one (padded) utterance of this call: splits a flat float4 index into (utterance, offset)
    const unsigned long long *uids;   // [B] per-utterance noise stream ids (fd_set_noise_streams) or null: see philox_normal4
    int l4_io;             // samples / 4 of one utterance as the CALLER lays it out (x_T, z, seq_out, out): == l4 unless the call's frames were
                           // rounded up to a bucket (fd_context::t_bucket); also what a Philox draw's position is counted in
    long long n4_io;       // B * l4_io: one step's stride in z / seq_out
    const long long *offs4;   // [B] or null (with uids only): where utterance b's samples start inside a longer utterance, in float4s --
                              // a draw is keyed on off4 + offs4[b], so a window of fd_sample_span draws what the whole utterance does
};

enum Stage { ST_EMBED = 0, ST_FIRST, ST_DBLOCK, ST_KP_FRONT, ST_KP_GEMM, ST_CONVT, ST_LVC, ST_FINAL, ST_COUNT };

// Everything that decides which kernels a denoiser step (or a captured piece of steps) enqueues and with which arguments.  A captured
// graph is keyed on (B, T, steps, StepMode).  fd_context::mode holds the option values; a call copies it and fills in its own fields.
// Nobody but plan_step (fd_plan.h) reads the pipe bits, the fusion switches and fp32_mask: the drivers read the StepPlan it returns.
struct StepMode {
    // options
    bool fast[ST_COUNT] = {true, true, true, true, true, true, true, true};   // "kernels.<stage>" = fast | naive
    bool gemm_f16 = true;        // kp_gemm on the fp16 matrix pipe with the 2-piece operand split
    bool gemm_wino = true;       // option "gemm_form" = "winograd" | "direct": ... as Winograd F(2,3) over the frame axis (2/3 of the matrix work)
    bool gemm_tile16 = true;     // option "gemm_tile" = "16" | "32": the Winograd form's item on 16x16x32 matrix tiles (two row tiles of 16 pairs; a
                                 // row tile behind the utterance's end is skipped) or on 32x32x16 ones (k_kp_gemm_w<TILE>)
    bool lvc_f16 = true;         // LVC layers (hop 64, 256) likewise
    bool conv_f16 = true;        // DBlocks, ConvTranspose upsamplers and the predictor front likewise
    bool lvc_h8_mfma = true;     // option "lvc_h8" = "mfma": the hop-8 layers on 16x16x32 fp16 tiles (k_lvc_h8m) | "valu" (k_lvc_h8)
    bool fuse_final = true;      // option "fuse_final": final_conv inside the last LVC layer
    bool fuse_up = true;         // option "fuse_up": the ConvTranspose of blocks 1 and 2 inside their first LVC layer (when both stages run
                                 // fp16x2-only, i.e. under fallback = host or a forced mask without them).  Same bits, one launch and one
                                 // round trip of x less per block: B=1 -5.2 %, B=8 -2.6 %
    bool fuse_advance = true;    // option "fuse_advance": between two steps of one graph / launch sequence the end-of-step bookkeeping
                                 // (k_advance) rides in the next step's first kernel instead of a launch of its own
    bool keep_taps = false;      // option "taps"
    // per call.  How a stage that has an fp16x2 kernel is launched (fd_plan.h: Pipe):
    //   inline_fallback  the fp32 kernel is enqueued right behind the fp16x2 one and exits at once unless that one raised its flag
    //                    (fully asynchronous, works inside a captured graph; ~2 us per stage and step)
    //   !inline_fallback only the fp16x2 kernel; flags accumulate in the sticky words of range_flag and the HOST redoes the work with
    //                    fp32_mask set (option fallback = host: fd_sample_check)
    //   fp32_mask        bit i set: the stage whose flag word is i (fd::flags) runs its fp32 kernel outright
    unsigned fp32_mask = 0;
    bool inline_fallback = true;
    bool ragged = false;         // the call's `lens` are in Workspace::lens_dev (a ragged batch)
    // hoisted predictor (fd_context::hoist_mode): the kernels of hoist_np reverse steps are predicted by ONE front + GEMM launch pair
    // (batch entry n * B + b = step n of utterance b), in front of the call's steps -- or, hoist_chunk (a schedule of more than 8 steps),
    // in front of each captured piece of up to 8 steps, over the piece's own steps (rows step_idx .. step_idx + 7 of the embedding
    // table, read through the device step counter).  hoist_np = 1: each step runs its own predictor
    int hoist_np = 1;
    bool hoist_chunk = false;

    bool operator==(const StepMode &o) const
    {
        for (int i = 0; i < ST_COUNT; ++i)
            if (fast[i] != o.fast[i]) return false;
        return gemm_f16 == o.gemm_f16 && gemm_wino == o.gemm_wino && gemm_tile16 == o.gemm_tile16 && lvc_f16 == o.lvc_f16 && conv_f16 == o.conv_f16 &&
               lvc_h8_mfma == o.lvc_h8_mfma && fuse_final == o.fuse_final && fuse_up == o.fuse_up && fuse_advance == o.fuse_advance &&
               keep_taps == o.keep_taps && fp32_mask == o.fp32_mask && inline_fallback == o.inline_fallback && ragged == o.ragged &&
               hoist_np == o.hoist_np && hoist_chunk == o.hoist_chunk;
    }
};

#include "fd_plan.h"

struct Workspace {
    int B = 0;                  // capacity: utterances (per-utterance arrays),
    int64_t frames = 0;         //           B*T frames (activations, predicted kernels),
    int64_t rows = 0;           //           B*gx_rows(T) rows of the GEMM's fp16 image
    float *noise = nullptr;     // [1024][B][3][80]
    float *embed_h2 = nullptr;  // [max(1024, B)][512] second MLP layer of the step embedding, between the two embed kernels
    float *a[4] = {};           // a0..a3
    float *kp_h0 = nullptr, *kp_hA = nullptr, *kp_hB = nullptr;   // [3][B][64][T]
    float *kpack = nullptr;     // [3][B][T][KREC]
    float *h_f16 = nullptr;     // fp16 piece image of the predictor hidden state: [3][B][64*ceil(T/64)+2 rows][2 pieces][64] x 2 B
    int *lens_dev = nullptr;    // [B] valid frames per utterance of the current call (ragged batches)
    unsigned long long *uid_dev = nullptr;   // [B] noise stream ids of the current call (fd_set_noise_streams)
    long long *off_dev = nullptr;            // [B] Philox position offsets (float4s) of the current call (StepParams::offs4)
    float *xsave = nullptr;     // [B][L] x at the start of the call / of the current graph chunk (option fallback = host: what a redo starts from)
    int *range_flag = nullptr;  // (128 words) the fp16-range flags of the stages, of this step, the previous one and the call: fd::flags (fd_plan.h)
    float *xA = nullptr, *xB = nullptr;                           // [B][32][L] ping-pong
    float *xtap[fd::NBLK] = {}; // block outputs kept for fd_read_tap
    int64_t pframes = 0, prows = 0, plens = 0;   // capacity of the predictor's buffers (kp_h*, kpack, mel_rep / h_f16 / lens_dev): frames, image
                                                 // rows and utterances x the reverse steps predicted at once (StepMode::hoist_np), tracked on
                                                 // their own so that a large batch and a hoisted small one do not multiply
    float *mel_rep = nullptr;   // [N][B][80][T] the mel once per reverse step: the hoisted predictor's batch
    float *mel = nullptr;       // [B][80][T] library-owned copy used by the sampler graph
    float *x = nullptr;         // [B][L] running x_t of the sampler
    float *eps_acc = nullptr;   // [B][L] final_conv sums written by the last LVC layer (k_lvc_h2 FINAL); all zero between steps
    float *steps = nullptr;     // [B] step values for fd_forward
    StepParams *params = nullptr;
    size_t bytes = 0;
};

struct ProfEntry { std::string name; hipEvent_t e0, e1; };
struct Scratch { float *p = nullptr; size_t bytes = 0; };      // a device buffer of the handle that grows on demand

// Constant tables of the mel front-end (fd_kernels_mel.hip; fd_griffin_lim and the MCD read them too), built in double precision at the first call that needs them.
struct MelTables {
    const float *tab = nullptr;      // cos[1024], sin[1024] of 2*pi*i/1024, periodic Hann window [1024]
    const int *fb_lo = nullptr, *fb_n = nullptr, *fb_off = nullptr;      // per mel filter: first FFT bin, #bins, offset into fb_w
    const float *fb_w = nullptr;     // the non-zero weights of librosa.filters.mel(22050, 1024, 80, fmin, fmax), filter after filter
};
enum MelVariant { MEL_PWG = 0, MEL_TACOTRON = 1, MEL_VARIANTS = 2 };

// A parameter as fd_commit_weights folds it (weight-norm applied, reference layout) and the configuration-generic path that takes them
// (fd_generic.hip: any architecture the reference constructor accepts, on runtime-shaped kernels; gen == nullptr for base.yaml's
// architecture, which runs on the tuned kernel set).
struct FoldedParam { std::vector<float> w, b; };
// A weight set as host bytes (fd_weights.cpp builds it, fd_commit_weights uploads it with one allocation and one copy): every piece at
// a 256-byte-aligned offset, with the pointer field that receives its device address.
struct WeightImage {
    std::vector<char> bytes;
    std::vector<std::pair<const void **, size_t>> fields;      // (destination pointer field, offset into bytes)
    template <class T> void add(const T *&dst, const std::vector<T> &v)
    {
        const size_t off = (bytes.size() + 255) & ~(size_t)255;
        bytes.resize(off + v.size() * sizeof(T));
        memcpy(bytes.data() + off, v.data(), v.size() * sizeof(T));
        fields.push_back({reinterpret_cast<const void **>(&dst), off});
    }
};
namespace fdg {
struct Net;
int validate(const fd_config &c, std::string &why);
int create(fd_context *c);
void destroy(fd_context *c);
int hop_total(const fd_context *c);
int pack_weights(fd_context *c, const std::map<std::string, FoldedParam> &f, WeightImage &img);   // its weights, fields = the Net's pointers
int forward(fd_context *c, const float *x, const float *mel, const float *steps, int B, int T, const int *lens, float *eps_out, hipStream_t stream);
int sample(fd_context *c, const float *mel, int B, int T, const int *lens, const fd_step *table, int N, int ddim, const float *x_T, const float *z,
           unsigned long long seed, const std::vector<unsigned long long> &ids, float *out, float *seq_out, hipStream_t stream);
}  // namespace fdg

struct fd_context {
    fd_config cfg;
    fdg::Net *gen = nullptr;                  // set for a configuration other than base.yaml's: every compute call goes to fd_generic.hip
    int device = 0;
    int num_cus = 256;
    std::string err;
    bool committed = false;
    StepMode mode;                            // the options among the mode's fields; the per-call ones stay at their defaults here
    bool use_graph = true;
    int profile = 0;                          // option "profile": 0 off | 1 the kernels' own begin / end timestamps | 2 ("events") stream events around each launch
    std::vector<unsigned long long> noise_ids; // fd_set_noise_streams: consumed by the next fd_sample
    std::vector<long long> noise_offs;       // fd_sample_span (fd_api_span.cpp): each window's first sample / 4 in the utterance, consumed
                                             // with noise_ids (empty: every draw counted from the utterance's start)
    bool host_fallback = true;                // option "fallback" = "host" (default; settled inside fd_sample unless defer_check) | "graph"
    std::map<std::string, std::pair<std::vector<int64_t>, std::vector<float>>> raw;   // host copies from fd_set_weight
    void *weight_arena = nullptr;            // the one device allocation behind the committed weights (DevWeights or fdg::Net)
    size_t weight_bytes = 0;                 // ... and its size (fd_get_weight_image)
    DevWeights w;
    // fd_refresh_weights_device (fd_weights.cpp) rebuilds the arena in place on a stream.  Its work lists and the word its kernels OR
    // the out-of-range families into live in refresh_dev (allocated by the first refresh); the word is copied to refresh_bad (pinned)
    // behind the kernels, and the first inference call after a refresh waits for refresh_done alone and looks at it
    // (fd_settle_refresh) before it chooses a kernel family: w.*_ok are stale while refresh_pending.
    void *refresh_dev = nullptr;
    size_t refresh_dev_bytes = 0;
    unsigned *refresh_bad = nullptr;
    hipEvent_t refresh_done = nullptr;
    bool refresh_pending = false;
    long long n_refreshes = 0, n_refresh_graph_drops = 0;
    Workspace ws;
    bool lvc_dx_gather = true;               // option lvc_dx = gather | copy: the frames path's dx kernel reads kernel_conv's frames (fd_kernels_train.hip)
    // the step embedding and the three fc_t rows of every reverse step depend on the schedule's t values and the weights only: kept from
    // the previous fd_sample when those are unchanged (two launches per call)
    std::vector<float> embed_t;
    int embed_B = 0;
    bool embed_valid = false;
    bool embed_cache = true;                 // option "embed_cache"
    MelTables mel[MEL_VARIANTS];             // [MEL_PWG]: fmin 80, fmax 7600; [MEL_TACOTRON]: fmin 0, fmax 8000 (twiddles/window shared)
    int mel_variant = MEL_PWG;               // option "mel"
    std::vector<float> mel_bank[MEL_VARIANTS];   // the dense [80][513] bank each front-end uses (host copy: fd_get_mel_filterbank)
    bool mel_bank_user[MEL_VARIANTS] = {false, false};   // supplied through fd_set_mel_filterbank (else the restated default)
    // Every constant table uploaded so far, owned here and freed at fd_destroy (fd_api_ext.cpp: upload_table): mel, resampler ratios,
    // STOI, spectral, the pseudo-inverses of both mel inversions, NNLS banks, the MCD's DCT.  The members that point into it are made at
    // the first call that needs them, never inside a stream capture (first_use / refresh; but see ensure_mel_tables).
    std::vector<void *> tables;
    // a table keyed on the caller's host values: the values last uploaded and their device image (refresh: made again when they differ)
    struct KeyedTable { std::vector<float> host; const float *dev = nullptr; };
    std::map<std::pair<int, int>, const float *> resample_tabs;      // fd_resample's polyphase tables by reduced ratio (up, down); fd_stoi_measure's too
    int last_B = 0, last_T = 0;
    hipStream_t cap_stream = nullptr;
    // Calls on one handle share the workspace, the embedding rows and the pending range check: they are ordered by the stream they run
    // on.  When a caller moves to another stream (fd_forward / fd_sample), a pending check is settled on the old stream and the new
    // stream waits for everything the old one still holds (follow_stream in fd_api.cpp).
    hipStream_t last_stream = nullptr;
    bool have_last_stream = false;
    hipEvent_t ev_switch = nullptr;          // the tail of the handle's last compute call (fd_api.cpp: mark_tail / follow_stream)
    bool tail_marked = false;
    // The predictor (front + GEMM) sees the mel and the step embedding only -- never x -- so for a short schedule on a small batch all N
    // steps' kernels are predicted by ONE pair of launches in front of the loop (StepMode::hoist_np): at B = 1 the front's seven-layer
    // latency chain and the GEMM's fill are paid once per call instead of once per step.
    // option "hoist" = auto (B * T <= 4096 frames, N >= 2) | on | off
    int hoist_mode = 1;                       // 0 off, 1 auto, 2 on
    // captured denoiser steps, one per (B, T, steps, mode): micro-batches of different padded length alternate without re-capturing
    struct StepGraph { int B, T, steps; StepMode mode; hipGraph_t graph; hipGraphExec_t exec; unsigned long long last_use; };   // `steps` denoiser steps per launch
    std::vector<StepGraph> graphs;           // at most max_graphs, least recently used evicted
    unsigned long long graph_clock = 0;
    // An evicted graph may still be running: it is parked here with an event recorded behind everything enqueued so far and destroyed
    // by a later call once that event has completed (no stream-wide wait on the eviction path).
    struct RetiredGraph { hipGraph_t graph; hipGraphExec_t exec; hipEvent_t done; };
    std::vector<RetiredGraph> retired;
    int max_graphs = 64;                     // option "graph_cache"
    // The reference CLI vocodes one utterance per call with a different length each time (FastDiff.py:97-103, base.yaml:53): a graph
    // keyed on the exact T would be captured once per utterance.  fd_sample therefore rounds the frames of its OWN buffers up to a
    // multiple of t_bucket (option "t_bucket", 0 / 1 = off) and runs the call with `lens` -- whose contract already is "as if the
    // utterance were alone and lens[b] frames long", bit for bit -- so one graph serves every length of a bucket; the caller's
    // tensors keep their own dense layout (StepParams::l4_io).
    int t_bucket = 32;
    long long n_graph_captures = 0, n_graph_hits = 0, n_graph_evictions = 0;
    bool defer_check = false;                // option "defer_check": fd_sample returns with its range check still pending (tickets)
    // Pinned staging ring for everything a call uploads from the host (step table, lens, noise stream ids, valid counts): a slot
    // is rewritten only after the event recorded behind its last upload has completed, so no call waits for the stream and no
    // asynchronous copy ever reads memory the next call has already overwritten.
    static constexpr int STAGE_SLOTS = 8;
    struct StageSlot { char *host = nullptr; size_t cap = 0; hipEvent_t done = nullptr; };
    StageSlot stage[STAGE_SLOTS];
    unsigned stage_next = 0;
    // Everything fd_sample was called with (host arrays copied): what a redo of a call of up to 8 steps starts from again
    struct SampleArgs {
        const float *mel = nullptr;
        int B = 0, T = 0, N = 0, ddim = 0;
        bool has_lens = false;
        std::vector<int> lens;
        std::vector<fd_step> table;
        const float *x_T = nullptr, *z = nullptr;
        unsigned long long seed = 0;
        float *out = nullptr, *seq_out = nullptr;
        hipStream_t stream = nullptr;
        std::vector<unsigned long long> ids;
        std::vector<long long> offs;                        // (with ids) StepParams::offs4
    };
    // option fallback = host: the fd_sample call whose range flags have not been looked at yet (fd_sample_check / fd_sample_settle).
    //   lazy (schedules of up to 8 steps = one graph launch): the NEXT fd_sample enqueues its own work first and looks at this call's
    //   flags afterwards, so the host's wait falls on a busy GPU; a flagged call is then run again as a whole from `args`;
    //   otherwise (longer schedules, checked every 8 steps): redone from `xsave`, steps [first, first + count).
    struct PendingCall {
        bool active = false;
        bool lazy = false;
        int slot = 0;                                       // which of the two flag buffers / events
        long long ticket = 0;
        int B = 0, T = 0, N = 0, first = 0, count = 0;      // steps [first, first + count) were enqueued without fallbacks; T: frames of the
        int T_io = 0;                                       // library's buffers (bucketed), T_io: the caller's
        float *out = nullptr;
        hipStream_t stream = nullptr;
        StepMode mode;                                      // a piece of a long schedule: the mode it was enqueued with
        SampleArgs args;
    } pending;
    long long ticket_counter = 0;            // one per fd_sample
    // fd_get_counter: the last long call's 8-step pieces (enqueued / run again after a flag / enqueued with stages already on fp32 and
    // with which), and the short calls run again as a whole since fd_create
    long long n_pieces = 0, n_pieces_redone = 0, n_pieces_fp32 = 0, n_calls_redone = 0;
    unsigned call_fp32_mask = 0;
    long long redone_ring[16] = {};          // tickets of the calls that had to be redone (0 = none), newest overwrite oldest
    unsigned redone_next = 0;
    int *flags_host = nullptr;               // pinned, 2 x 32 words: the sticky flags of the pending call(s)
    hipEvent_t flags_done = nullptr, flags_done2 = nullptr;
    void *scratch = nullptr;                 // 64 KB device scratch (abs-max words, ...)
    // the training operators' buffers, grown on demand (fd_api_train.cpp): three, so a captured graph's pointers change only with its own
    Scratch lvc_scratch;                     // the LVC operator's frame-major kernel copy (fd_lvc_forward / fd_lvc_backward)
    Scratch kconv_scratch;                   // the partial sums of fd_kconv_backward* and fd_input_conv_backward*
    Scratch cconv_scratch;                   // per-workgroup partial sums of fd_conv32 / conv7 / upsample backward's dW / db
    Scratch span_scratch;                    // a window batch of fd_sample_span / fd_sample_spans: window records, mel, injected x_T / z, x_0
    Scratch ring_scratch;                    // fd_mel_ring_append's chunk records
    long long n_span_batches = 0, n_span_windows = 0;   // fd_get_counter: fd_sample calls / windows made by the span entry points
    Scratch loud_scratch;                    // fd_loudness_measure / _normalize: peak words, lengths, tile states, partial sums, block powers
    Scratch stoi_scratch;                    // fd_stoi_measure: lengths, the 10 kHz signals, frame energies, src, band amplitudes, segment partials
    const float *stoi_tab = nullptr;         // its window and twiddles (csrc/fd_stoi.h: tables)
    Scratch pitch_scratch;                   // fd_pitch_track / _compare: the device copies of valid [B] and frames [B]
    Scratch spectral_scratch;                // fd_spectral_measure: lengths, then the frame partials of every resolution
    std::map<std::pair<int, int>, const float *> spectral_tabs;      // its window and twiddles by (nfft, win) (csrc/fd_spectral.h: tables)
    Scratch gl_scratch;                      // fd_griffin_lim: lengths, stream ids, transposed amplitudes, two frame buffers, frame sums (csrc/fd_gl.h: layout)
    KeyedTable gl_pinv[MEL_VARIANTS];        // fd_mel_to_linear: the pseudo-inverse [513][80] last used with each variant
    Scratch nnls_scratch;                    // fd_mel_to_linear_nnls: lengths and frame sums (csrc/fd_nnls.h: layout)
    // ... per variant: the bank last used with its device table (fdn::table) and L, and the pseudo-inverse last used.  Its own slots, apart
    // from gl_pinv: callers of the two inversions that alternate with different matrices would otherwise upload at every call.
    struct NnlsBank { KeyedTable bank, pinv; double L = 0.0; } nnls_bank[MEL_VARIANTS];
    Scratch bins_scratch;                    // fd_bins_pass: per chunk the counts, inertia, moved, nonfinite and sums (csrc/fd_bins.h: layout)
    Scratch mcd_scratch;                     // fd_cepstra / fd_dtw / fd_mcd_measure: counts, bottom rows, direction codes, records, cepstra (fd_kernels_mcd.hip: layout)
    const float *mcd_dct = nullptr;          // their DCT table [40][80] (csrc/fd_mcd.h: dct_table); their front-end's tables: `mel`
    Scratch pwg_scratch;                     // fd_pwg_generate: lengths, stream ids, G, the up-sampling coefficients, two x buffers, skip (csrc/fd_pwg.h: layout)
    Scratch trim_scratch;                    // fd_trim_silences / fd_trim_levels: lengths, window levels, prefix tables (fd_kernels_trim.hip: layout)
    Scratch step_scratch;                    // fd_mse_forward / fd_adamw_multi: per-workgroup partial sums and the optimizer's per-step scalars
    std::vector<ProfEntry> prof_pending;
    std::vector<hipEvent_t> event_pool;
    std::map<std::string, std::pair<int64_t, double>> prof_acc;
};

// Arguments of one denoiser step (all device pointers)
struct StepIO {
    const float *x_in;     // [B][L] current x_t
    const float *mel;      // [B][80][T]
    const float *steps;    // [B] (forward mode) -- ignored in sampler mode (table[step_idx].t)
    float *eps_out;        // forward mode: eps destination; sampler mode: null (x updated in place)
    int sampler;           // 0 = fd_forward, 1 = fd_sample step
    int hoist_step = 0;    // hoisted predictor (StepMode::hoist_np > 1): which B entries of its kpack batch this step reads
    bool advance = false;  // the first kernel does the previous step's end-of-step bookkeeping (StepMode::fuse_advance)
};

// kernels (fd_kernels_*.hip) -- each returns hipError from launch
namespace fdk {
struct Launch {
    fd_context *ctx;
    hipStream_t stream;
    bool capturing;
    const StepMode *mode = nullptr;   // what the denoiser step's launchers read, and the plan resolved from it (fd_plan.h: plan_step);
    const StepPlan *plan = nullptr;   // left out (null) by the paths that launch no step
    const int *lens() const { return mode->ragged ? ctx->ws.lens_dev : nullptr; }
    // block n's records of this step; with a hoisted predictor the batch behind kpack is hoist_np * B entries and this step's are the
    // hoist_step-th B of them
    const float *kpack(int n, const StepIO &io, int B, int T) const
    {
        return ctx->ws.kpack + ((int64_t)n * mode->hoist_np + io.hoist_step) * B * T * fd::KREC;
    }
    Twin twin(int word, bool f16_on = true) const { return twin_of(*plan, word, ctx->ws.range_flag, f16_on); }
};
hipError_t embed(const Launch &L, const StepIO &io, int B, int n_steps);
hipError_t advance_step(const Launch &L);
hipError_t clear_range_flags(const Launch &L, int set_step = 0);     // before the first step of a call / of a redo: step counter := set_step
hipError_t mel_frontend(const Launch &L, const float *wav, int B, int64_t n_samples, float *mel, int T);
hipError_t init_noise(const Launch &L, float *x, int B, int l4, int l4_io, unsigned long long seed, const unsigned long long *uids,
                      const long long *offs4 = nullptr);
// fd_sample_span's window batch (fd_kernels_span.hip): window b covers utterance frames [start[b], start[b] + len[b])
constexpr int SPAN_MAX_WINDOWS = 8;
struct SpanWindows {
    int n;                               // windows in the batch
    long long start[SPAN_MAX_WINDOWS];   // first frame of the window in the utterance
    int len[SPAN_MAX_WINDOWS];           // frames of the window (<= the batch's padded length Wp)
    long long c0[SPAN_MAX_WINDOWS];      // first frame of the window's centre (what the scatter copies) ...
    int clen[SPAN_MAX_WINDOWS];          // ... and its frames
};
// caller's mel [80][mel_frames] (frames from mel_first), x_T [mel_frames*256], z [nz][mel_frames*256] -> [n][80][Wp], [n][Wp*256],
// [nz][n][Wp*256]; zero where a window reaches outside the caller's frames or behind its own length.  One launch.
hipError_t span_gather(const Launch &L, const SpanWindows &w, int Wp, const float *mel, const float *x_T, const float *z, int nz,
                       long long mel_first, long long mel_frames, float *mel_w, float *x_w, float *z_w);
// x_0 of the windows [n][Wp*256] -> the caller's out over frames [t0, ...): each window's centre.  One launch.
hipError_t span_scatter(const Launch &L, const SpanWindows &w, int Wp, const float *x_w, long long t0, float *out);
// fd_sample_spans' window batch: windows of MANY utterances, each with its own source (a plain buffer or a ring) and destination.  The
// records lie in device memory (uploaded through the handle's pinned staging ring), one per batch item.
struct SpanRec {
    const float *src;                    // channel c, utterance frame f at src[c * pitch + col(f)]
    float *dst;                          // where the window's centre goes: its span's out + (c0 - t0) * 256
    long long pitch, cap;                // cap 0: col(f) = f - mel_first; > 0: col(f) = f % cap
    long long mel_first, mel_frames;     // the utterance frames the source holds
    long long start, c0;                 // first frame of the window / of its centre
    int len, clen;                       // frames of the window (<= Wp) / of its centre
    long long pad_;                      // (80 bytes: a multiple of 16)
};
constexpr int SPANS_MAX_WINDOWS = 32;
// recs [n] device.  gather: -> mel_w [n][80][Wp]; scatter: x_w [n][Wp*256] -> each record's dst.  One launch each.
hipError_t spans_gather(const Launch &L, const SpanRec *recs, int n, int Wp, float *mel_w);
hipError_t spans_scatter(const Launch &L, const SpanRec *recs, int n, int Wp, int max_clen, const float *x_w);
// chunks [n] device (max_frames = the longest): frame first_frame + i of src -> column (first_frame + i) % cap of each ring row
hipError_t ring_append(const Launch &L, const fd_ring_chunk *chunks, int n, long long max_frames);
hipError_t copy_rows(const Launch &L, float *dst, int64_t dpitch, const float *src, int64_t spitch, int width, int rows, int reps = 1,
                     int64_t rep_stride = 0);
hipError_t peak_normalize_int16(const Launch &L, const float *wav, int B, int64_t len, int16_t *pcm, const long long *valid_dev);
// fd_resample (fd_kernels_resample.hip).  The frames that count of up to RESAMPLE_ITEMS items are a kernel argument; a larger batch is
// one launch per RESAMPLE_ITEMS items.  valid: HOST [B] or null; table: device [up][Kp] (csrc/fd_resample.h), unused for up = down = 1.
constexpr int RESAMPLE_ITEMS = 64;
struct ResampleLens { long long v[RESAMPLE_ITEMS]; };
hipError_t resample(const Launch &L, const void *src, int format, int C, int B, int64_t n_in, int64_t src_pitch, const int64_t *valid,
                    int up, int down, int half, int K, int Kp, int64_t n_out_max, const float *table, float *dst, int64_t dst_pitch);
// How the tools below lay out their scratch buffers: slots one after the other, each starting on a 256-byte border.
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
struct Carve { size_t at = 0; size_t take(size_t bytes) { const size_t o = at; at = align256(at + bytes); return o; } };      // at: bytes taken so far
// fd_loudness_measure / fd_loudness_normalize (fd_kernels_loudness.hip).  scratch: loudness_scratch_bytes(B, L, rate) bytes of the handle's
// loudness buffer; valid_dev: null or loudness_valid_slot() of that buffer, filled by the caller; rec: device [B] or null (a slot of the
// buffer); the filter and its powers (csrc/fd_loudness.h) are kernel arguments.
constexpr int LOUDNESS_SEGS = 24;      // 100 ms segments a tile can touch: 16384 / 799 + 2 at the lowest rate, 8000 Hz
using LoudnessFilter = fdl::Filter;
size_t loudness_scratch_bytes(int B, int64_t L, int rate);
long long *loudness_valid_slot(void *scratch, int B, int64_t L, int rate);
hipError_t loudness(const Launch &L_, const float *wav, int B, int64_t L, const long long *valid_dev, int rate, const LoudnessFilter &F,
                    bool normalize, double target, fd_loudness *rec, float *out_f32, int16_t *out_pcm, void *scratch);
// fd_stoi_measure (fd_kernels_stoi.hip).  x, y: [B] rows `pitch` floats apart AT 10 kHz (the caller's, or the x10 / y10 slots of the
// scratch buffer after the internal resample); n10: the longest row; lens_dev: null (every row n10 samples) or the lens slot, filled by
// the caller with each row's own 10 kHz length; tab: device copy of fds::tables; rec: device [B].
struct StoiBands { int lo[fds::BANDS], hi[fds::BANDS]; };
struct StoiSlots { long long *lens; float *x10, *y10; long long pitch10; };
size_t stoi_scratch_bytes(int B, int64_t n10, bool resampled);
StoiSlots stoi_slots(void *scratch, int B, int64_t n10, bool resampled);
hipError_t stoi(const Launch &L_, const float *x, const float *y, long long pitch, int B, int64_t n10, const long long *lens_dev,
                const float *tab, const StoiBands &bd, fd_stoi *rec, void *scratch, bool resampled);
// fd_pitch_track / fd_pitch_compare (fd_kernels_pitch.hip).  lens_dev / frames_dev: null (every row L samples / `pitch` frames) or device
// [B]; lg: fdp::lags of cfg, which the caller has validated.
hipError_t pitch_track(const Launch &L_, const float *wav, long long pitch, int B, int64_t L, const long long *lens_dev,
                       const fd_pitch_config &cfg, const fdp::Lags &lg, float *f0, float *aper, long long out_pitch);
hipError_t pitch_compare(const Launch &L_, const float *f0_ref, const float *f0_deg, long long pitch, int B, const long long *frames_dev,
                         fd_pitch *rec);
// fd_spectral_measure (fd_kernels_spectral.hip).  x, y: [B] rows `pitch` floats apart; lens_dev: null (every row L samples) or the lens
// slot of the scratch buffer; c: a configuration the caller has validated (fdx::refusal); tabs[r]: device copy of fdx::tables(nfft[r], win[r]).
size_t spectral_scratch_bytes(int B, int64_t L, const fd_spectral_config &c);
long long *spectral_lens_slot(void *scratch);
hipError_t spectral(const Launch &L_, const float *x, const float *y, long long pitch, int B, int64_t L, const long long *lens_dev,
                    const fd_spectral_config &c, const float *const *tabs, fd_spectral *rec, void *scratch);
// fd_griffin_lim / fd_mel_to_linear (fd_kernels_gl.hip).  lens_dev / ids_dev: null (every item T frames / id = b) or the slots of the
// scratch buffer, filled by the caller; tab: the mel front-end's table (cos, sin, window); scratch: gl_scratch_bytes(B, T) bytes.
struct GlSlots { long long *lens; unsigned long long *ids; };
size_t gl_scratch_bytes(int B, int T);
GlSlots gl_slots(void *scratch, int B, int T);
hipError_t griffin_lim(const Launch &L_, const float *amp, const float *angles, int B, int T, const long long *lens_dev,
                       const unsigned long long *ids_dev, int n_iters, unsigned long long seed, const float *tab, float *wav, long long pitch,
                       fd_gl *rec, void *scratch);
hipError_t mel_to_linear(const Launch &L_, const float *mel, int B, int T, const float *pinv_dev, int variant, float *amp);
// fd_pwg_generate / fd_pwg_draw (fd_kernels_pwg.hip).  net: a committed generator (img: its device image, csrc/fd_pwg.h: image);
// lens_dev / ids_dev as above; src: the mel or the padded c; z: device [B][hop T] or null; scratch: fdpwg::layout(...).total bytes.
struct PwgNet { const float *img; fd_pwg_config cfg; bool has_scaler; };
hipError_t pwg_generate(const Launch &L_, const PwgNet &net, const float *src, int padded, int B, int T, const long long *lens_dev,
                        const unsigned long long *ids_dev, const float *z, unsigned long long seed, float *wav, long long pitch, void *scratch);
hipError_t pwg_draw(const Launch &L_, int B, long long L, unsigned long long seed, const unsigned long long *ids_dev, float *z_out, long long pitch);
// fd_mel_to_linear_nnls (fd_kernels_nnls.hip).  lens_dev: null or the lens slot of the scratch buffer (nnls_scratch_bytes(B, T) bytes);
// tab_dev: device copy of fdn::fill_table(bank); step: fdn::step(L); rec: device [B] or null.
size_t nnls_scratch_bytes(int B, int T);
long long *nnls_lens_slot(void *scratch);
hipError_t mel_to_linear_nnls(const Launch &L_, const float *mel, int B, int T, const long long *lens_dev, const float *pinv_dev,
                              const float *tab_dev, float step, int variant, int n_iters, float *amp, fd_nnls *rec, void *scratch);
// fd_bins_pass (fd_kernels_bins.hip).  Every pointer on the device; scratch: bins_scratch_bytes(N, K, D, cent_out != null) bytes.
size_t bins_scratch_bytes(long long N, int K, int D, bool update);
hipError_t bins_pass(const Launch &L_, const float *x, long long N, int D, long long ld, const float *shift, const float *scale, const float *cent,
                     int K, int *assign_io, float *cent_out, fd_bins *rec, void *scratch);
// fd_cepstra / fd_dtw / fd_mcd_measure (fd_kernels_mcd.hip).  The handle's one buffer for the three: mcd_scratch_bytes(B, bot_pitch = the
// pitch of b's rows, code_stride = bytes of direction codes per pair or 0, the floats of the two cepstra or 0); the count slots 0 .. 3 lie
// in front whatever the rest.  Counts: null (every row whole) or a slot filled by the caller; dct: device copy of fdm::dct_table.
size_t mcd_scratch_bytes(int B, long long bot_pitch, long long code_stride, long long cep_floats_a, long long cep_floats_b);
long long *mcd_count_slot(void *scratch, int which);
float *mcd_cep_slot(void *scratch, int B, long long bot_pitch, long long code_stride, long long cep_floats_a, long long cep_floats_b, int which);
fd_dtw_rec *mcd_rec_slot(void *scratch, int B, long long bot_pitch, long long code_stride);
hipError_t cepstra(const Launch &L_, const float *wav, int B, long long L, const long long *lens_dev, int n_coef, const float *dct, float *cep,
                   long long T_pitch);
hipError_t dtw(const Launch &L_, const float *a, const float *b, int B, int D, long long ld, long long pitch_a, long long pitch_b,
               const long long *fa_dev, const long long *fb_dev, fd_dtw_rec *rec, int *align, long long align_pitch, long long code_stride, void *scratch);
hipError_t mcd_finish(const Launch &L_, const float *ca, const float *cb, int B, int D, long long pitch_a, long long pitch_b, const long long *fa_dev,
                      const long long *fb_dev, const long long *na_dev, long long Lc, const long long *nb_dev, long long Ld, const fd_dtw_rec *dtw_rec,
                      fd_mcd *rec);
// fd_trim_silences / fd_trim_levels (fd_kernels_trim.hip).  W, Mp: the window and the windows of L samples (fdtr::windows); M_grid: the
// windows of the longest row, which the levels' grid covers; valid_dev: null or the valid slot of the scratch buffer (trim_scratch_bytes(B, Mp)
// bytes), filled by the caller; p: parameters the caller has validated (fdtr::refusal).
size_t trim_scratch_bytes(int B, int64_t Mp);
long long *trim_valid_slot(void *scratch);
hipError_t trim_levels(const Launch &L_, const float *wav, int B, int64_t L, const long long *valid_dev, int64_t W, int64_t M_grid, double *levels,
                       int64_t pitch, bool fill_tail);
hipError_t trim(const Launch &L_, const float *wav, int B, int64_t L, const long long *valid_dev, const fd_trim_params &p, int64_t W, int64_t Mp,
                int64_t M_grid, float *out, int *out_valid, unsigned char *flags, fd_trim *rec, void *scratch);
}  // namespace fdk

// profiling-aware launch helper.  Option profile = 1: the launch goes through hipExtLaunchKernelGGL with a start and a stop event, which
// receive the dispatch's own begin / end timestamps (what rocprofv3 --kernel-trace reports) -- nothing is put between two launches, so
// the kernels run back to back as in the replayed graph.  profile = events: hipEventRecord in front of and behind each launch (two
// barrier packets per kernel: the gaps let the previous kernel's dirty lines drain, the numbers come out 3-5 % shorter).
bool fd_prof_stamps(const fdk::Launch &L, const char *name, hipEvent_t *e0, hipEvent_t *e1);
void fd_prof_begin(const fdk::Launch &L, const char *name);
void fd_prof_end(const fdk::Launch &L);

#define FD_LAUNCH(L, name, kernel, grid, block, shmem, ...)                                  \
    do {                                                                                     \
        hipEvent_t ev0__ = nullptr, ev1__ = nullptr;                                         \
        if (fd_prof_stamps(L, name, &ev0__, &ev1__)) {                                       \
            hipExtLaunchKernelGGL(kernel, grid, block, shmem, (L).stream, ev0__, ev1__, 0, __VA_ARGS__); \
        } else {                                                                             \
            fd_prof_begin(L, name);                                                          \
            hipLaunchKernelGGL(kernel, grid, block, shmem, (L).stream, __VA_ARGS__);         \
            fd_prof_end(L);                                                                  \
        }                                                                                    \
        hipError_t e__ = hipGetLastError();                                                  \
        if (e__ != hipSuccess) return e__;                                                   \
    } while (0)
