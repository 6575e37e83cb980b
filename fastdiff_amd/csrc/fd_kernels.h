// fd_kernels.h -- internal: per-stage entry points of the naive and the fast (MFMA) kernel sets, and the reference kernels behind the
// naive set and the generic path.
#pragma once
#include "fd_internal.h"

// Geometry of the predictor GEMM's fp16 piece images (fd_kernels_kp.hip), shared by the kernels that write and read them and the host
// code that sizes the workspace behind them (fd_api.cpp): one definition, so that a DMA never reads behind the allocation.
namespace fdk_fast {
constexpr int GX_CT = 4;                          // direct form: frame tiles (of 32) per item
constexpr int GX_ROWB = 2 * 128;                  // bytes per row (frame) of its image: [piece][64 ch] fp16
constexpr int GW_PAIRS = 32;                      // Winograd form: pairs per item (64 frames)
constexpr int GW_ROWB = 1024;                     // bytes per pair row: [4 j][2 pieces][64 ch] fp16
__host__ __device__ inline int gx_rows(int T) { return ((T + GX_CT * 32 - 1) / (GX_CT * 32)) * (GX_CT * 32) + 2; }   // image rows per (block, utterance)
__host__ __device__ inline int gw_pairs(int T) { return ((T + 2 * GW_PAIRS - 1) / (2 * GW_PAIRS)) * GW_PAIRS; }      // image rows (pairs) per (block, entry)

// The Winograd form's item on 16 x 16 x 32 matrix tiles (k_kp_gemm_w<16>): an item is 2 row tiles (rt) of 16 pairs x 2 column tiles (ct) of
// 16 record positions, a K = 64 product 2 steps (ks) of K = 32.  Lane = (r or n = lane & 15, g = lane >> 4).  The lane maps live here so
// that tools/gemm16_index_check.cpp walks the very arithmetic the kernel runs.
// A operand: byte offset of lane's 16 B inside the row tile's window, piece q, step ks (+ 16 rt GW_ROWB + 256 j for row tile and sub-row)
__host__ __device__ inline int gw16_a_off(int lane, int q, int ks)
{
    const int r = lane & 15, g = lane >> 4;
    return r * GW_ROWB + (((8 * q + 4 * ks + g) ^ r) << 4);
}
// B operand: float4 index into a block's gemm_w_pack ([ptile][piece][16 kg][lane = col + 32 hi][8]) for sub-row j, step ks, column tile ct
__host__ __device__ inline int gw16_b_idx(int ptile, int q, int j, int ks, int ct, int lane)
{
    const int kh = 4 * ks + (lane >> 4);      // 8-value group of the K = 64 product: kg = 4 j + kh / 2, hi = kh % 2
    return ((ptile * 2 + q) * 16 + 4 * j + (kh >> 1)) * 64 + 32 * (kh & 1) + 16 * ct + (lane & 15);
}
// D: register i of tile (rt, ct) holds pair row 16 rt + gw16_d_pair and position gw16_d_pos of the 32-column tile
__host__ __device__ inline int gw16_d_pair(int lane, int i) { return 4 * (lane >> 4) + i; }
__host__ __device__ inline int gw16_d_pos(int lane, int ct) { return 16 * ct + (lane & 15); }
// Stores of a whole row tile.  The odd 16-lane rows of the ct = 0 register have changed places with the even rows of the ct = 1 register:
// register i of part 0 (the former ct = 0 register) / part 1 then holds pair row 16 rt + 4 part + i + 8 (lane >> 5), position lane & 31.
// Float offsets inside the item's 64 records: a per-lane part and a wave-uniform one.
__host__ __device__ inline unsigned gw16_st_lane_off(int lane) { return (unsigned)(16 * (lane >> 5)) * (unsigned)fd::KREC + (unsigned)(lane & 31); }
__host__ __device__ inline int gw16_st_row_off(int rt, int part, int i, int odd) { return (2 * (16 * rt + 4 * part + i) + odd) * fd::KREC; }
}  // namespace fdk_fast

namespace fdk {
// naive set (fd_kernels_naive.hip)
hipError_t naive_first_conv(const Launch &L, const StepIO &io, int B, int T);
hipError_t naive_dblock(const Launch &L, int d, int B, int T);
hipError_t naive_kp_front(const Launch &L, const StepIO &io, int B, int T);
hipError_t naive_kp_gemm(const Launch &L, int B, int T);
hipError_t naive_convt(const Launch &L, int n, const float *x_in, float *x_out, int B, int Lin);
hipError_t naive_lvc_layer(const Launch &L, int n, int layer, float *x, const float *skip, float *y, int B, int T);
hipError_t naive_final_eps(const Launch &L, const float *x32, float *eps, int B, int T);
hipError_t naive_update(const Launch &L, float *x, const float *eps, int64_t n);
// fast set (fd_kernels_first_final / _dblock / _kp / _convt / _lvc .hip)
hipError_t fast_first_conv(const Launch &L, const StepIO &io, int B, int T);
hipError_t fast_dblock(const Launch &L, int d, int B, int T, const float *audio);
hipError_t fast_kp_front(const Launch &L, const StepIO &io, int B, int T);
hipError_t fast_kp_gemm(const Launch &L, int B, int T);
hipError_t fast_convt(const Launch &L, int n, const float *x_in, float *x_out, int B, int Lin);
// up: layer 0 of block n >= 1 with the block's ConvTranspose inside it -- x_in is then the block's input (fp16x2-only launches)
hipError_t fast_lvc_layer(const Launch &L, const StepIO &io, int n, int layer, const float *x_in, const float *skip, float *x_out, int B, int T,
                          bool up = false);
hipError_t fast_final(const Launch &L, const StepIO &io, const float *x32, int B, int T);
// the LVC operator with its gradients (fd_kernels_train.hip)
// scratch: B*T*Cin*Cout*ks floats when lvc_op_needs_scratch (the model's shape: matrix-pipe kernels), else unused
bool lvc_op_needs_scratch(int Cin, int Cout, int ks, int hop);
// kbs / dkbs: floats between two utterances of K / dK (0 = a tensor of its own; the model's shape also takes one layer's slice of a
// [B, layers, Cin, Cout, ks, T] tensor)
// frames (the model's shape): K / dK are frame-major ([T][6144] per utterance, fd_frame_order.h: K in ORDER_FWD, dK in ORDER_DK) as
// kconv_forward / kconv_backward with frames = true write / read them; kbs / dkbs are then the floats between two utterances of those
hipError_t lvc_op_forward(const Launch &L, const float *x, const float *K, const float *bias, float *out, int B, int Cin, int Cout, int ks,
                          int T, int hop, float *scratch, int64_t kbs = 0, bool frames = false, int64_t bbs = 0);
hipError_t lvc_op_backward(const Launch &L, const float *x, const float *K, const float *dout, float *dx, float *dK, float *dbias, int B,
                           int Cin, int Cout, int ks, int T, int hop, float *scratch, int64_t kbs = 0, int64_t dkbs = 0, bool frames = false,
                           int64_t dbbs = 0);      // bbs / dbbs (frames only): floats between two utterances of bias / dbias (0 = Cout * T)
// the gate + residual of an LVC layer, one pass forward and one backward (modules.py:217)
hipError_t gate_forward(const Launch &L, const float *x, const float *y, float *out, int B, int C, int64_t len);
hipError_t gate_backward(const Launch &L, const float *y, const float *dout, float *dy, int B, int C, int64_t len);
// a skip tensor's fan-out on the training path (fd_kernels_train.hip): out[r, j] = x[r, j f] (the DBlock's nearest pick), and the sum of
// the gradients that come back: dx = g[0] + g[1] + g[2] + g[3] + scatter(gp) (null pointers = absent); rows = B * C
hipError_t fan_pick(const Launch &L, const float *x, float *out, int rows, int64_t len, int f);
hipError_t fan_sum(const Launch &L, const float *const g[4], const float *gp, float *dx, int rows, int64_t len, int f);
// the KernelPredictor's kernel_conv (Conv1d 64 -> M, k3) forward and backward for the training path (fd_kernels_kconv.hip);
// scratch: kconv_scratch_floats(B, M, T) floats for the backward's partial sums
bool kconv_supported(int M, int T);
size_t kconv_scratch_floats(int B, int M, int T);
// frames (M a multiple of 6144 = M / 6144 layers of the LVC operator's kernels): out is [B][layers][T][6144] with every frame in the
// operator's forward operand order, dout the same shape in its dK accumulator order (fd_frame_order.h) -- the LVC kernels then read /
// write the predictor's tensors where they lie
bool kconv_frames_supported(int M, int T);
// post / y (M <= 512: the predictor's small convolutions): out = leaky_relu(conv, post); the backward is given that output (y) and
// takes dout as the gradient behind the activation
bool kconv_act_supported(int M, int T);
hipError_t kconv_forward(const Launch &L, const float *h, const float *W, const float *bias, float *out, int B, int M, int T, bool frames = false,
                         float post = 1.0f);
hipError_t kconv_backward(const Launch &L, const float *h, const float *W, const float *dout, float *dh, float *dW, float *dbias, int B, int M,
                          int T, float *scratch, bool frames = false, const float *y = nullptr, float post = 1.0f, float in_slope = 1.0f);
// the weight / bias gradients of n <= 8 small convolutions of ONE shape (M <= 512) in two launches (the six pairs of the predictor's residual
// stack, once its dx chain has run); y[i] != null: dout[i] is masked with that activated output; scratch: kconv_w_multi_scratch_floats()
size_t kconv_w_multi_scratch_floats(int n, int B, int M);
hipError_t kconv_backward_w_multi(const Launch &L, int n, const float *const *h, const float *const *dout, const float *const *y, float post, int B,
                                  int M, int T, float *const *dW, float *const *dbias, float *scratch);
// n <= 8 independent convolutions of one shape side by side in one launch each (the three KernelPredictors' front ends; a single
// convolution is n = 1): forward of small convolutions, one step of their dx chains (kconv_backward's dh part), the input convolution
// both ways.  Host arrays of device pointers.
hipError_t kconv_forward_multi(const Launch &L, int n, const float *const *h, const float *const *W, const float *const *bias, float *const *out, int B,
                               int M, int T, float post);
// in_slope != 1 (a chain of such pairs): h is the activated output of the pair below and dh comes out multiplied by that activation's
// mask (h > 0 ? 1 : in_slope), i.e. as the gradient in front of it
size_t kconv_x_multi_scratch_floats(int n, int B, int M, int T);
hipError_t kconv_backward_x_multi(const Launch &L, int n, const float *const *h, const float *const *W, const float *const *y, const float *const *dout,
                                  float *const *dh, int B, int M, int T, float post, float in_slope, float *scratch);
// the predictor's input convolution with its activation: leaky_relu(Conv1d(80 -> 64, k5, pad 2), post) (modules.py:292-295), T <= 128;
// the backward takes the activated output y; scratch: input_conv_multi_scratch_floats(n, B) floats
hipError_t input_conv_forward_multi(const Launch &L, int n, const float *const *x, const float *const *w, const float *const *bias, float *const *out,
                                    int B, int T, float post);
size_t input_conv_multi_scratch_floats(int n, int B);
hipError_t input_conv_backward_multi(const Launch &L, int n, const float *const *x, const float *const *w, const float *const *y, const float *const *dy,
                                     float *const *dx, float *const *dw, float *const *db, int B, int T, float post, float *scratch);
// one layer's "x (+ skip) -> leaky_relu -> dilated Conv1d(32 -> 32, k3) -> bias -> (leaky_relu)" forward and backward for the training
// path (fd_kernels_cconv.hip); scratch: cconv_scratch_floats() floats for the per-workgroup partial sums of dW / db
bool cconv_supported(int dil, int64_t len);
size_t cconv_scratch_floats(const Launch &L, int dil, int B, int64_t len);
hipError_t cconv_forward(const Launch &L, const float *x, const float *skip, const float *w, const float *bias, float *xs_out, float *y, int B,
                         int64_t len, int dil, float pre, float post);
hipError_t cconv_backward(const Launch &L, const float *xs, const float *y, const float *w, const float *dy, const float *gxs, float *dxs,
                          float *dw, float *db, int B, int64_t len, int dil, float pre, float post, float *scratch);
// first_audio_conv (which = 0: Conv1d 1 -> 32, k7) and final_conv (which = 1: Conv1d 32 -> 1, k7) of the training path
size_t conv7_scratch_floats(const Launch &L, int B, int64_t len);
hipError_t conv7_forward(const Launch &L, int which, const float *x, const float *w, const float *bias, float *y, int B, int64_t len);
hipError_t conv7_backward(const Launch &L, int which, const float *x, const float *w, const float *dy, float *dx, float *dw, float *db, int B,
                          int64_t len, float *scratch);
// the block's up-sampler on the training path: leaky_relu(x, 0.2) -> ConvTranspose1d(32, 32, 2 r, stride r, padding r / 2), r = 4 or 8
size_t convt_scratch_floats(const Launch &L, int r, int B, int64_t len_in);
hipError_t convt_forward(const Launch &L, const float *x, const float *w, const float *bias, float *y, int B, int64_t len_in, int r);
hipError_t convt_backward(const Launch &L, const float *x, const float *w, const float *dy, float *dx, float *dw, float *db, int B, int64_t len_in,
                          int r, float *scratch);
// torch._weight_norm(v, g, 0) on [rows, cols] views and its backward for n tensors in ceil(n / 28) launches (fd_kernels_cconv.hip): items
// in HOST memory (include/fastdiff_hip.h: fd_wn_item), passed on as kernel arguments
hipError_t weight_norm_multi(const Launch &L, const fd_wn_item *items, int n, bool backward);
// the rest of a training step (fd_kernels_step.hip; include/fastdiff_hip_train.h): the draws, the loss, clip + guard + AdamW.
// scratch: step_scratch_floats(mse_blocks(n) or adamw_blocks(items, n)) floats of the handle's step scratch
size_t step_scratch_floats(int64_t blocks);
int64_t mse_blocks(int64_t n);
int64_t adamw_blocks(const fd_adamw_item *items, int n);
hipError_t train_draw(const Launch &L, const float *x0, const float *alpha, int T_train, int B, int64_t len, uint64_t seed,
                      const fd_train_state *state, uint64_t iter_host, float *x_t, float *z, float *steps);
// one launch, no scratch: slot b's utterance and window chosen on the device, waveform copied, mel block transposed to [80, F].  eval:
// the batch of an evaluation pass (fd_eval_collate: items in order, rank / world not read), else a training batch (fd_train_collate)
hipError_t collate(const Launch &L, bool eval, const float *wav_arena, const float *mel_arena, const int64_t *frame_off, int64_t n_items,
                   int hop, int F, int B, uint64_t seed, const fd_train_state *state, uint64_t iter_host, int rank, int world, float *wavs,
                   float *mels, int64_t *picked);
// the rest of an evaluation pass (include/fastdiff_hip_train.h: fd_item_distance, fd_eval_accumulate).  item_distance's scratch:
// step_scratch_floats(B * item_distance_blocks(n)) floats of the handle's step scratch
int64_t item_distance_blocks(int64_t n);
hipError_t item_distance(const Launch &L, const float *a, const float *b, int B, int64_t n, int kind, float *out, float *scratch);
hipError_t eval_accumulate(const Launch &L, const float *values, const float *steps, const int64_t *picked, int B, int T_train, int bins,
                           fd_eval_state *acc, float *item_out, fd_train_state *advance);
hipError_t mse_forward(const Launch &L, const float *eps, const float *z, int64_t n, float *loss, fd_train_state *state, float *scratch);
hipError_t mse_backward(const Launch &L, const float *eps, const float *z, const float *dloss, int64_t n, float *deps);
hipError_t adamw_multi(const Launch &L, const fd_adamw_item *items, int n, const fd_adamw_hyper *hyper, fd_train_state *state, float *scratch);
// e += w (p - e) over n tensors behind the optimizer (fd_ema_multi): one deciding thread, then ceil(n / 64) update launches; no scratch
hipError_t ema_multi(const Launch &L, const fd_ema_item *items, int n, const fd_ema_hyper *hyper, const fd_train_state *state, fd_ema_state *ema);
// the scheduling network, the pieces of its training step and the schedule search (fd_kernels_phi.hip; include/fastdiff_hip_train.h, last
// section).  scratch: bandpool_scratch_floats(B, L, backward) / 2 B phi_residual_blocks(L) floats of the handle's step scratch
size_t bandpool_scratch_floats(int B, int64_t L, bool backward);
hipError_t bandpool_forward(const Launch &L_, const float *x, const float *W, const float *bias, int B, int64_t L, float *feat, float *scratch);
hipError_t bandpool_backward(const Launch &L_, const float *x, const float *W, const float *bias, const float *dfeat, int B, int64_t L, float *dW,
                             float *db, float *scratch);
hipError_t npred_head_forward(const Launch &L_, const float *feat, const float *beta_next, const float *delta2, int R, const float *W1,
                              const float *b1, const float *W2, const float *b2, int B, float *beta_hat, float *ratio);
hipError_t npred_head_backward(const Launch &L_, const float *feat, const float *beta_next, const float *delta2, const float *W1, const float *b1,
                               const float *W2, const float *b2, const float *dbeta_hat, int B, float *dW1, float *db1, float *dW2, float *db2,
                               float *dfeat);
hipError_t phi_draw(const Launch &L_, const float *x0, const float *alpha, int T_train, int tau, int B, int64_t len, uint64_t seed,
                    const fd_train_state *state, uint64_t iter_host, float *x_t, float *z, float *steps, float *beta_nxt, float *delta,
                    float *delta2);
int64_t phi_residual_blocks(int64_t len);
hipError_t phi_residual_forward(const Launch &L_, const float *eps, const float *z, const float *delta, const float *beta_hat, int B, int64_t len,
                                float *m, float *s, float *scratch);
hipError_t sched_init(const Launch &L_, fd_sched_state *state, float betaN, float alphaN);
hipError_t sched_begin(const Launch &L_, fd_sched_state *state, const float *beta_hat, int n_hat, double rho, const float *alpha, int T_train,
                       int ddim, float *steps_out, int B);
hipError_t sched_update(const Launch &L_, fd_sched_state *state, float *x, const float *eps, int64_t n, float *cond_out);
}  // namespace fdk

// The exact-fp32 reference kernels (fd_generic.hip): one thread per output, runtime shapes, fp32 multiply-adds in a fixed order.  The
// generic path runs any configuration on them; the naive set (option kernels[.<stage>] = naive) runs base.yaml's on the tuned workspace.
// A Launch with ctx set (the naive set) goes through FD_LAUNCH under the given name; ctx == null (the generic path) launches plain on
// L.stream, unprofiled.
namespace fdg {
// y[b][o][t] = post(bias[o] + sum_{c,k} w[o][c][k] * pre(xin(b, c, t + k*dil - dil*(K-1)/2))) (+ res[b][o][t]),  K odd
//   xin(b, c, p) = 0 outside [0, Lout), else x[b][c][p * in_stride] (+ in_add[b][c]: the predictor's `c + noise`, modules.py:203 --
//   added to the signal, not to its zero padding).  in_stride > 1 reads every in_stride-th sample: nearest-neighbour down-sampling by
//   an integer factor (DiffusionDBlock, modules.py:127-134) without materialising the picked sequence.
//   lens (nullable) / spf: utterance b is lens[b] * spf output samples long; behind that nothing is computed and nothing is read.
struct ConvArgs {
    const float *x, *w, *bias;
    float *y;
    int B, Cin, Cout, K;
    int64_t Lx, Lout;                  // row lengths of x and y
    int dil = 1, in_stride = 1;
    float pre = 1.0f, post = 1.0f;     // leaky ReLU slopes, 1 = identity
    const float *in_add = nullptr;     // in_add[s * in_add_step + b * in_add_b + c], s = *step (device: the sampler's graphs) or 0
    int64_t in_add_b = 0, in_add_step = 0;
    const int *step = nullptr;
    const float *res = nullptr;
    const int *lens = nullptr;
    int spf = 1;
    int rec = 0, rec_off = 0;          // rec > 0: y[(b*Lout + t)*rec + rec_off + (perm ? perm[o] : o)] (the naive kernel_conv's records)
    const int *perm = nullptr;
    ConvArgs(const ConvW &cw, const float *x_, float *y_, int B_, int Cin_, int Cout_, int K_, int64_t L)
        : x(x_), w(cw.w), bias(cw.b), y(y_), B(B_), Cin(Cin_), Cout(Cout_), K(K_), Lx(L), Lout(L) {}
};
hipError_t conv1d(const fdk::Launch &L, const char *name, const ConvArgs &a);
// ConvTranspose1d(C, C, 2r, stride r, padding r/2 + r%2, output_padding r%2) of leaky_relu(x, 0.2): [B][C][Lin] -> [B][C][Lin*r]
hipError_t convt(const fdk::Launch &L, const char *name, const ConvW &up, const float *x, float *y, int B, int C, int r, int64_t Lin,
                 const int *lens, int spf_in);
// DiffusionDBlock (modules.py:116-134) on x [B][C][Lin], f = the down-sampling factor: res = Conv1x1(x) at every f-th sample; h = the
// picked x through three (lrelu 0.2, conv k3 dilation 1, 2, 4); out = h + res.  tmp: res, h after the first and the second conv.
hipError_t dblock(const fdk::Launch &L, const ConvW &res, const ConvW conv[3], const float *x, int64_t Lin, int f, float *const tmp[3],
                  float *out, int B, int C, const int *lens, int spf);
// the KernelPredictor's front (modules.py:292-318): `in` = its input conv k5 + lrelu 0.1 on c + noise into h0 = in.y, then six (conv
// k, lrelu 0.1) with h0 added behind the last: h0 -> ha -> hb -> ha -> hb -> ha -> hb, the result in hb
hipError_t kp_front(const fdk::Launch &L, const ConvArgs &in, const ConvW res[6], int k, float *ha, float *hb);
// one LVC layer (modules.py:208-217), in place on x [B][C][T*hop]: x += skip; y = lrelu(conv_{ks, dilation 3^layer}(lrelu(x, 0.2)), 0.2);
// x += sigmoid(z[ch]) * tanh(z[ch + C]) with z the location-variable convolution of y by the layer's predicted kernels
struct LvcArgs {
    float *x;
    const float *skip;
    float *y;                          // scratch [B][C][T*hop]
    // packed: kernels = the block's records [B][T][fd::KREC] (fd::kernel_index / bias_index: C = 32, ks = 3), biases unused;
    // else the reference layout as kernel_conv / bias_conv leave it, [B][layers*C*2C*ks][T] / [B][layers*2C][T] (modules.py:333-338)
    bool packed;
    const float *kernels, *biases;
    int B, C, ks, layers, layer, hop, T;
    const int *lens;
};
hipError_t lvc_layer(const fdk::Launch &L, const ConvW &conv, const LvcArgs &a);
}  // namespace fdg
