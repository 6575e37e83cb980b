/*
 * fastdiff_hip_train.h -- libfastdiff_hip.so: the training-side operators: the denoiser's layers as
 * differentiable forward / backward pairs in the reference's own tensor layouts, so that theta_timestep_loss
 * (modules/FastDiff/module/util.py:291-325) runs on HIP kernels under PyTorch autograd (fastdiff_amd/train.py, lvc_op.py).
 * Not part of the inference boundary.  Conventions: fastdiff_hip.h; every call is asynchronous on `stream`.
 */
#ifndef FASTDIFF_HIP_TRAIN_H
#define FASTDIFF_HIP_TRAIN_H

#include "fastdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Training side: TimeAware_LVCBlock.location_variable_convolution (modules/FastDiff/module/modules.py:220-253,
 * dilation = 1 as at its only call site, modules.py:216) as a differentiable operator in the reference's own tensor layouts, so that
 * theta_timestep_loss (util.py:291-325) can differentiate through it while the rest of the module stays on PyTorch autograd:
 *   out[b,o,q] = bias[b,o,q/hop] + sum_{i,k} xpad[b,i,q+k-(ks-1)/2] * kernel[b,i,o,k,q/hop]
 *   x [B,Cin,T*hop]   kernel [B,Cin,Cout,ks,T]   bias [B,Cout,T]   out, dout [B,Cout,T*hop]      (all device, float32, contiguous)
 * fd_lvc_backward writes the gradients whose pointer is not NULL: dx (needs kernel), dkernel and dbias (need x).
 * Any handle of the device will do (it supplies the device, the error text and, for the model's own shape -- Cin 32, Cout 64, ks 3,
 * hop 8 / 64 / 256, which runs on the fp32 matrix instruction -- a scratch buffer of B*T*Cin*Cout*ks floats for the frame-major copy of
 * the kernels: calls on one handle must therefore be ordered on one stream, as autograd orders a forward and its backward);
 * Cin*Cout*ks <= 8192, ks odd. */
FD_API int fd_lvc_forward(fd_handle h, const float *x, const float *kernel, const float *bias, int B, int Cin, int Cout, int ks, int T,
                          int hop, float *out, void *stream);
FD_API int fd_lvc_backward(fd_handle h, const float *x, const float *kernel, const float *dout, int B, int Cin, int Cout, int ks, int T,
                           int hop, float *dx, float *dkernel, float *dbias, void *stream);
/* The same with a batch stride on the predicted kernel and on its gradient (floats between two utterances; 0 = Cin*Cout*ks*T, a tensor
 * of its own): one layer's slice [:, i] of the predictor's [B, layers, Cin, Cout, ks, T] output -- and of the gradient buffer of that
 * shape -- is used where it lies, without a contiguous copy each way (the model's shape only: 32 -> 64, k3, hop 8 / 64 / 256). */
FD_API int fd_lvc_forward_strided(fd_handle h, const float *x, const float *kernel, int64_t kernel_bstride, const float *bias, int B, int Cin,
                                  int Cout, int ks, int T, int hop, float *out, void *stream);
FD_API int fd_lvc_backward_strided(fd_handle h, const float *x, const float *kernel, int64_t kernel_bstride, const float *dout, int B, int Cin,
                                   int Cout, int ks, int T, int hop, float *dx, float *dkernel, int64_t dkernel_bstride, float *dbias,
                                   void *stream);

/* KernelPredictor.kernel_conv (modules/FastDiff/module/modules.py:315-318,330-331: Conv1d(64 -> M, kernel 3, padding 1) with
 * M = lvc_layers * in * 2 in * 3 = 24576) for the training path, in the reference's layouts: x [B,64,T], weight [M,64,3] (after
 * weight-norm), bias [M], out / dout [B,M,T] (device, float32, contiguous); the three gradients whose pointer is not NULL are written
 * (dx needs weight; dweight and dbias need x).  fp32 matrix instruction throughout.  M a multiple of 128, 1 <= T <= 128 (the
 * reference trains on crops of 100 frames: base.yaml:50-51) -- anything else returns FD_ERR_UNSUPPORTED and the caller keeps its own
 * convolution. */
FD_API int fd_kconv_forward(fd_handle h, const float *x, const float *weight, const float *bias, int B, int M, int T, float *out, void *stream);
FD_API int fd_kconv_backward(fd_handle h, const float *x, const float *weight, const float *dout, int B, int M, int T, float *dx,
                             float *dweight, float *dbias, void *stream);
/* The same with the activation the predictor puts behind its small convolutions (modules.py:296-314: Conv1d, LeakyReLU(0.1)) inside:
 * out = leaky_relu(conv, post_slope); the backward takes that output (y) and dout = the gradient behind the activation.  M <= 512
 * (input and residual convolutions: M = 64); post_slope = 1 is the plain convolution (y may then be NULL).
 * in_slope (a chain of such pairs, e.g. the six of the predictor's residual stack, where x is itself the activated output of the
 * pair below and has no other reader): dx comes out multiplied by THAT activation's mask (x > 0 ? 1 : in_slope), i.e. as the
 * gradient in front of it, and the pair below is then called with post_slope = 1 on that gradient; 1 = dx as it is. */
FD_API int fd_kconv_forward_act(fd_handle h, const float *x, const float *weight, const float *bias, int B, int M, int T, float post_slope,
                                float *out, void *stream);
FD_API int fd_kconv_backward_act(fd_handle h, const float *x, const float *weight, const float *y, const float *dout, int B, int M, int T,
                                 float post_slope, float in_slope, float *dx, float *dweight, float *dbias, void *stream);
/* The weight and bias gradients of n <= 8 such convolutions of ONE shape in two launches: x, dout, y, dweight, dbias are HOST arrays of n
 * device pointers (y[i] = NULL: dout[i] is already the gradient in front of the activation; y = NULL: none is masked).  For the six pairs
 * of the predictor's residual stack once its dx chain (fd_kconv_backward_act with dweight = dbias = NULL) has run: one launch of
 * 6 x B workgroups instead of six latency-bound launches of B. */
FD_API int fd_kconv_backward_w_multi(fd_handle h, int n, const float *const *x, const float *const *dout, const float *const *y, int B, int M,
                                     int T, float post_slope, float *const *dweight, float *const *dbias, void *stream);

/* A skip tensor's fan-out on the training path (FastDiff_model.py:91-98): x [rows = B*C, L] is read by the DiffusionDBlock below it, which
 * begins by picking every factor-th column (F.interpolate to L / factor, nearest: modules.py:128-131), and as `audio_down` by the four
 * layers of the LVC block at its rate (modules.py:209).  fd_fan_forward: picked [rows, L / factor] = x[:, ::factor].  fd_fan_backward:
 * dx = g0 + g1 + g2 + g3 + scatter(gpicked) in one pass (any of the five may be NULL = no gradient from that reader); under autograd
 * the same is a zero-fill, a strided scatter and four full-size additions.  L a multiple of factor. */
FD_API int fd_fan_forward(fd_handle h, const float *x, int rows, int64_t L, int factor, float *picked, void *stream);
FD_API int fd_fan_backward(fd_handle h, const float *g0, const float *g1, const float *g2, const float *g3, const float *gpicked, int rows,
                           int64_t L, int factor, float *dx, void *stream);

/* KernelPredictor.input_conv (modules.py:292-295: Conv1d(80 -> 64, kernel 5, padding 2), LeakyReLU(0.1)) for the training path as one
 * operator each way: x [B,80,T], weight [64,80,5], bias [64], out / y / dout [B,64,T] (device, float32, contiguous), 1 <= T <= 128;
 * out = leaky_relu(conv, post_slope); the backward takes that output (y) and dout = the gradient behind the activation, and writes the
 * gradients whose pointer is not NULL (dweight / dbias: per-utterance partial sums added in a fixed order). */
FD_API int fd_input_conv_forward(fd_handle h, const float *x, const float *weight, const float *bias, int B, int T, float post_slope, float *out,
                                 void *stream);
FD_API int fd_input_conv_backward(fd_handle h, const float *x, const float *weight, const float *y, const float *dout, int B, int T,
                                  float post_slope, float *dx, float *dweight, float *dbias, void *stream);

/* Side by side: n <= 8 INDEPENDENT convolutions of one shape in one launch each.  The network's three KernelPredictors have identical
 * front ends -- input convolution, then six Conv1d(64, 64, 3) + LeakyReLU pairs -- on different weights and inputs; each is a chain
 * of latency-bound launches of B workgroups, the three together the same chain with 3 B.  Every pointer argument is a HOST array of n
 * device pointers (the library passes them on as kernel arguments); shapes and meaning per item as in the one-convolution entry
 * points above.  fd_kconv_backward_x_multi is one step of n dx chains (dx only: the weight gradients come from
 * fd_kconv_backward_w_multi once the chains have run); y[i] / dweight[i] / dbias[i] may be NULL where the single entry point allows it. */
FD_API int fd_kconv_forward_act_multi(fd_handle h, int n, const float *const *x, const float *const *weight, const float *const *bias, int B,
                                      int M, int T, float post_slope, float *const *out, void *stream);
FD_API int fd_kconv_backward_x_multi(fd_handle h, int n, const float *const *x, const float *const *weight, const float *const *y,
                                     const float *const *dout, int B, int M, int T, float post_slope, float in_slope, float *const *dx,
                                     void *stream);
FD_API int fd_input_conv_forward_multi(fd_handle h, int n, const float *const *x, const float *const *weight, const float *const *bias, int B,
                                       int T, float post_slope, float *const *out, void *stream);
FD_API int fd_input_conv_backward_multi(fd_handle h, int n, const float *const *x, const float *const *weight, const float *const *y,
                                        const float *const *dout, int B, int T, float post_slope, float *const *dx, float *const *dweight,
                                        float *const *dbias, void *stream);

/* The same two operators joined without the reference's tensor in between ("frames").  The reference hands the predicted kernels from
 * kernel_conv to the location-variable convolution as [B, layers, 32, 64, 3, T] (modules.py:333-338; T innermost), which the matrix
 * kernels of the operator have to transpose into frame-major order before use (and the gradient back): three passes over 6144*B*T
 * floats per layer and training step that exist only because of that layout.  Here kernel_conv writes
 *     frames [B, layers, T, 6144]      (M = layers * 6144; one frame = the operator's forward operand order)
 * and reads the gradient in the same shape (one frame = the operator's dK accumulator order), and the operator takes one layer's
 * [T, 6144] block per utterance where it lies: kernel_frames / dkernel_frames point at utterance 0's block of the layer, *_bstride =
 * floats between two utterances (layers * T * 6144); bias / dbias [64, T] per utterance likewise take the floats between two utterances
 * (0 = 64 * T; layers * 64 * T for one layer's slice of bias_conv's [B, layers, 64, T] output).  Both orders are permutations of the 6144 coefficients of a frame, internal to
 * this library (csrc/fd_frame_order.h); fastdiff_amd.lvc_op.frames_to_reference / reference_to_frames convert for inspection.  Same
 * shapes and limits as above (operator: 32 -> 64 channels, k 3, hop 8 / 64 / 256; kernel_conv: M a multiple of 6144, 1 <= T <= 128);
 * results equal those of the entry points above bit for bit (same products, same summation order), except kernel_conv's dx, whose sum
 * over the M rows runs frame group by frame group instead of row by row (float32 rounding apart). */
FD_API int fd_kconv_forward_frames(fd_handle h, const float *x, const float *weight, const float *bias, int B, int M, int T, float *frames,
                                   void *stream);
FD_API int fd_kconv_backward_frames(fd_handle h, const float *x, const float *weight, const float *dframes, int B, int M, int T, float *dx,
                                    float *dweight, float *dbias, void *stream);
FD_API int fd_lvc_forward_frames(fd_handle h, const float *x, const float *kernel_frames, int64_t kernel_bstride, const float *bias,
                                 int64_t bias_bstride, int B, int T, int hop, float *out, void *stream);
FD_API int fd_lvc_backward_frames(fd_handle h, const float *x, const float *kernel_frames, int64_t kernel_bstride, const float *dout, int B,
                                  int T, int hop, float *dx, float *dkernel_frames, int64_t dkernel_bstride, float *dbias,
                                  int64_t dbias_bstride, void *stream);

/* The gate of an LVC layer with its residual (modules.py:217) for the training path: out = x + sigmoid(y[:, :C]) * tanh(y[:, C:]),
 * x, out, dout [B,C,L], y, dy [B,2C,L] (device, float32, contiguous).  Under autograd the reference runs twelve elementwise kernels
 * for this line (four forward, eight backward), each moving the layer's whole tensor through HBM; these are one pass each way.
 * d out / d x is the identity, so fd_gate_backward only produces dy. */
FD_API int fd_gate_forward(fd_handle h, const float *x, const float *y, int B, int C, int64_t L, float *out, void *stream);
FD_API int fd_gate_backward(fd_handle h, const float *y, const float *dout, int B, int C, int64_t L, float *dy, void *stream);

/* The two 7-tap convolutions at the ends of the network on the training path: which = 0 first_audio_conv = Conv1d(1, 32, 7, padding 3)
 * (FastDiff_model.py:34-36,89): x [B,1,L] -> y [B,32,L], weight [32,1,7]; which = 1 final_conv = Conv1d(32, 1, 7, padding 3)
 * (FastDiff_model.py:67-68,100): x [B,32,L] -> y [B,1,L], weight [1,32,7].  L a multiple of 4.  backward writes dx (nullable),
 * dweight and dbias (each nullable) from x, the folded weight and dy; sums in a fixed order. */
FD_API int fd_conv7_forward(fd_handle h, int which, const float *x, const float *weight, const float *bias, int B, int64_t L, float *y,
                            void *stream);
FD_API int fd_conv7_backward(fd_handle h, int which, const float *x, const float *weight, const float *dy, int B, int64_t L, float *dx,
                             float *dweight, float *dbias, void *stream);

/* The block's up-sampler on the training path: `self.upsample(F.leaky_relu(x, 0.2))`, upsample = ConvTranspose1d(32, 32, 2 r, stride r,
 * padding r / 2) (modules/FastDiff/module/modules.py:163-166,205-206), ratio r = 4 or 8:  x [B,32,Lin] -> y [B,32,Lin*r]; weight
 * [32 in, 32 out, 2 r] (torch's ConvTranspose1d layout, no weight-norm), bias [32].  backward: from x, weight, dy it writes dx (the
 * activation's mask applied), dweight, dbias (each nullable); sums in a fixed order. */
FD_API int fd_upsample_forward(fd_handle h, const float *x, const float *weight, const float *bias, int B, int64_t Lin, int ratio, float *y,
                               void *stream);
FD_API int fd_upsample_backward(fd_handle h, const float *x, const float *weight, const float *dy, int B, int64_t Lin, int ratio, float *dx,
                                float *dweight, float *dbias, void *stream);

/* Weight-norm of the training path: every Conv1d of the model carries torch.nn.utils.weight_norm (FastDiff_model.py:71-72,115-122), i.e.
 * its forward evaluates w = torch._weight_norm(v, g, 0): w[r, :] = v[r, :] * g[r] / ||v[r, :]|| on the [rows = out channels, cols = in * k]
 * view.  forward also leaves ||v[r]|| in norm [rows] for the backward, which turns dw into dv [rows, cols] and dg [rows]. */
FD_API int fd_weight_norm_forward(fd_handle h, const float *v, const float *g, int64_t rows, int cols, float *w, float *norm, void *stream);
FD_API int fd_weight_norm_backward(fd_handle h, const float *v, const float *g, const float *norm, const float *dw, int64_t rows, int cols,
                                   float *dv, float *dg, void *stream);
/* The same for n parameter tensors in ceil(n / 28) launches each way (the model has 53 weight-normed convolutions: 106 launches of a
 * few microseconds per training step otherwise).  items: n records in HOST memory -- the library passes them on as kernel arguments, so
 * nothing is uploaded and a captured graph depends on no table's lifetime; every pointer inside is a device pointer: forward reads
 * v, g and writes w, norm; backward reads v, g, norm, dw and writes dv, dg (dw == NULL: that weight took no part in the loss, its dv and
 * dg are zeroed). */
typedef struct fd_wn_item {
    const float *v, *g;      /* [rows, cols], [rows] */
    float *w, *norm;         /* [rows, cols], [rows] */
    const float *dw;         /* [rows, cols] or NULL */
    float *dv, *dg;          /* [rows, cols], [rows] */
    int64_t rows;
    int32_t cols, reserved;
} fd_wn_item;
FD_API int fd_weight_norm_multi_forward(fd_handle h, const fd_wn_item *items, int n, void *stream);
FD_API int fd_weight_norm_multi_backward(fd_handle h, const fd_wn_item *items, int n, void *stream);

/* The denoiser's 21 small convolutions on the training path -- DiffusionDBlock.conv[0..2] applied as `layer(F.leaky_relu(x, 0.2))`
 * (modules/FastDiff/module/modules.py:120-125,136-137) and TimeAware_LVCBlock.convs[0..3] applied as `x += audio_down;
 * y = F.leaky_relu(conv(F.leaky_relu(x, 0.2)), 0.2)` (modules.py:183-187,209-212) -- as one differentiable operator:
 *   xs = x (+ skip);   y = post(bias + conv1d(pre(xs), weight, dilation, padding = dilation)),   pre / post = leaky_relu with the given
 *   slope, slope 1 = no activation.   x, skip, xs, y, dy, gxs, dxs [B,32,L];  weight [32,32,3] (folded: the caller applies weight-norm),
 *   bias [32];  L a multiple of 4, dilation one of 1, 2, 3, 4, 9, 27.
 * forward: skip may be NULL (then xs = x and xs_out may be NULL); with a skip xs_out receives x + skip (the layer's gate reads it).
 * backward: xs = the convolution's un-activated input (x + skip, or x), y = the forward's output (its sign is the post-activation's
 * mask), gxs (nullable) = the gradient that reached xs from its other readers; writes dxs = gxs + pre'(xs) * (W^T * (dy * post'(y)))
 * (the gradient of x and of skip alike), dweight [32,32,3], dbias [32] (each nullable).  Sums are formed in a fixed order. */
FD_API int fd_conv32_forward(fd_handle h, const float *x, const float *skip, const float *weight, const float *bias, int B, int64_t L,
                             int dilation, float pre_slope, float post_slope, float *xs_out, float *y, void *stream);
FD_API int fd_conv32_backward(fd_handle h, const float *xs, const float *y, const float *weight, const float *dy, const float *gxs, int B,
                              int64_t L, int dilation, float pre_slope, float post_slope, float *dxs, float *dweight, float *dbias,
                              void *stream);

/* The rest of a training step (FastDiffTask._training_step, FastDiff.py:44-49; theta_timestep_loss, util.py:291-325; base_task.py:231-233;
 * FastDiff.py:121-125) around the forward and backward above: the draws of a step, the loss, the global gradient norm with its clip, the
 * non-finite guard and AdamW -- with every per-step quantity in DEVICE memory, so that a whole step is one graph replay that draws anew,
 * and the host never waits for it.  Sums run in a fixed order (per-thread runs of FD_STEP_RUN elements, a tree inside the workgroup,
 * per-workgroup partial sums in a scratch buffer of the handle, one final workgroup): no floating-point atomics, two runs agree bit for
 * bit.  Calls on one handle must be ordered on one stream, and the first call at a larger size must not sit inside a graph capture (the
 * scratch buffer grows then: refused with FD_ERR_STATE, here and in the operators above).  Growing frees the old buffer: a graph captured earlier on this handle has its address baked in and must
 * not be replayed after a LARGER fd_mse_forward / fd_adamw_multi call on the same handle (capture again) -- as with the scratch buffers
 * of the backward operators above.  At most 2^36 elements per call.
 *
 * fd_train_state: 32 bytes of device memory owned by the caller (zero it before the first step).  Only kernels write it. */
typedef struct fd_train_state {
    uint64_t iter;        /* steps drawn so far: the id slot of the step's Philox draws */
    uint64_t applied;     /* optimizer steps applied (AdamW's `step`) */
    uint64_t skipped;     /* optimizer steps skipped because a gradient was not finite */
    float grad_norm;      /* global L2 norm of the gradients of the last step, before clipping */
    float loss;           /* loss of the last step */
} fd_train_state;
#define FD_STEP_RUN 16     /* elements a thread adds up serially in the sums of this section (the rest of a sum is a tree) */

/* The draws of theta_timestep_loss (util.py:312-318) on the device: x0 [B,1,L] -> steps [B,1] (float, as the network takes them),
 * z [B,1,L] ~ N(0, I) and x_t = alpha[ts] * x0 + sqrt(1 - alpha[ts]^2) * z, every operation rounded on its own (what torch evaluates on
 * the same z, bit for bit).  With `it` = state ? state->iter (read on the device: a replay draws anew) : iter_host,
 *   ts[b] = (w * T_train) >> 32 (64-bit product), w = word b & 3 of Philox4x32-10 keyed (seed, stream 0xFFFFFFFD, position b >> 2, id it),
 *   z[b,t] = component (b L + t) & 3 of the generator's normal4 keyed (seed, stream 0xFFFFFFFE, position (b L + t) >> 2, id it)
 * (oracle/philox.py is the host twin).  alpha: device [T_train]; L a multiple of 4; x0, x_t, z 16-byte aligned. */
FD_API int fd_train_draw(fd_handle h, const float *x0, const float *alpha, int T_train, int B, int64_t L, uint64_t seed,
                         const fd_train_state *state, uint64_t iter_host, float *x_t, float *z, float *steps, void *stream);

/* The batch of a step, cut on the device from a corpus that lives there (what VocoderDataset.__getitem__ + collater,
 * tasks/vocoder/dataset_utils.py:80-160, build on the host; fastdiff_amd/corpus.py: TrainCorpus holds the arenas, TrainCorpus.plan is the
 * host twin of the choice).  One launch, no scratch buffer of the handle, no atomics.
 *   wav_arena [sum T_i * hop]   mel_arena [sum T_i, 80] (frame-major)   frame_off [n_items + 1] = the frame prefix sums   (device)
 *   wavs [B,1,F*hop]   mels [B,80,F]   picked [B,2] = (item, start frame) per slot                                          (device)
 * Every item must be longer than the window, T_i > F (a slot whose item is not gets start = -1 and is left unwritten).
 * With `it` = state ? state->iter (read on the device: a replay cuts a new batch) : iter_host, slot b takes
 *   g = (it B + b) world + rank (mod 2^64),   e = g / n_items,   item = pi_e(g % n_items),
 *   start = (w * (T_item - F)) >> 32 (64-bit product), w = word b & 3 of Philox4x32-10 keyed (seed, stream 0xFFFFFFFC, position b >> 2, id it),
 * pi_e = a 4-round balanced Feistel network on 2k bits (k the smallest with 4^k >= n_items; halves hi = x >> k, lo = x & (2^k - 1);
 * a round: (hi, lo) <- (lo, hi ^ (F & (2^k - 1))), F = word 0 of Philox keyed (seed, stream 0xFFFFFFFB, position lo ^ (round << 28),
 * id e)), applied again while the value is >= n_items: a bijection of [0, n_items) per epoch e.
 * hop a multiple of 4; n_items <= 2^28; wav_arena, wavs 16-byte aligned. */
FD_API int fd_train_collate(fd_handle h, const float *wav_arena, const float *mel_arena, const int64_t *frame_off, int64_t n_items, int hop,
                            int F, int B, uint64_t seed, const fd_train_state *state, uint64_t iter_host, int rank, int world, float *wavs,
                            float *mels, int64_t *picked, void *stream);

/* nn.MSELoss() (util.py:307,325) and its backward: *loss = mean((eps - z)^2) (also into state->loss when state is not NULL);
 * deps = *dloss * 2 (eps - z) / n.  loss, dloss: device scalars. */
FD_API int fd_mse_forward(fd_handle h, const float *eps, const float *z, int64_t n, float *loss, fd_train_state *state, void *stream);
FD_API int fd_mse_backward(fd_handle h, const float *eps, const float *z, const float *dloss, int64_t n, float *deps, void *stream);

/* torch.nn.utils.clip_grad_norm_(params, max_norm) (norm type 2), the reference's NaN-gradient guard (trainer.py:320-327) and
 * torch.optim.AdamW.step() (amsgrad = False) for n parameter tensors in 2 ceil(n / 64) + 1 launches.  items: n records in HOST memory,
 * passed on as kernel arguments (as fd_wn_item); g == NULL: the parameter took no part in the step and is left alone.  hyper: DEVICE
 * memory (a learning-rate schedule is a copy of 8 bytes between replays); max_norm == 0: no clipping.
 *   norm = ||all g||_2 -> state->grad_norm;   c = max_norm ? min(1, max_norm / (norm + 1e-6)) : 1;   t = state->applied + 1
 *   norm finite:  g' = c g;  p *= 1 - lr wd;  m += (1 - beta1) (g' - m);  v = beta2 v + (1 - beta2) g'^2;
 *                 p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps);   state->applied += 1
 *   else:         no p, m or v is written;   state->skipped += 1
 * and state->iter += 1 either way, in the last launch (behind every read of it in stream order). */
typedef struct fd_adamw_item {
    float *p;             /* [numel] parameter */
    const float *g;       /* [numel] gradient, or NULL */
    float *m, *v;         /* [numel] exp_avg, exp_avg_sq */
    int64_t numel;
} fd_adamw_item;
typedef struct fd_adamw_hyper {
    double lr, beta1, beta2, eps, weight_decay, max_norm;      /* doubles, as torch keeps them: 1 - beta2 is then the optimizer's own */
} fd_adamw_hyper;
FD_API int fd_adamw_multi(fd_handle h, const fd_adamw_item *items, int n, const fd_adamw_hyper *hyper, fd_train_state *state, void *stream);

/* An exponential moving average of n parameter tensors (fastdiff_amd/ema.py: ParamEMA; the reference has none), in 1 + ceil(n / 64)
 * launches behind fd_adamw_multi in stream order.  It reads fd_train_state and never writes it; no scratch buffer of the handle, no
 * atomics.  items: n records in HOST memory, passed on as kernel arguments (as fd_adamw_item); p and e must not overlap.  Tensors whose
 * p and e are both 16-byte aligned are read and written 16 bytes per lane, the others element by element.  With u = ema->updates as it
 * stands before the call, in double precision:
 *   apply   = state->applied > ema->seen_applied      (a step the non-finite guard skipped did not advance `applied`: nothing moves)
 *   decay_t = warmup != 0 ? min(decay, (1 + u) / (10 + u)) : decay;      w = (float)(1 - decay_t)
 *   apply:    e = e + w * (p - e) for every element, each operation rounded on its own;
 *             ema->seen_applied = state->applied;  ema->updates = u + 1
 * ema->w and ema->apply are stored either way (what the update launches read). */
typedef struct fd_ema_item {
    const float *p;       /* [numel] parameter */
    float *e;             /* [numel] its average */
    int64_t numel;
} fd_ema_item;
typedef struct fd_ema_hyper {
    double decay, warmup; /* DEVICE memory, as fd_adamw_hyper: a decay schedule is a copy of 8 bytes between replays */
} fd_ema_hyper;
typedef struct fd_ema_state { /* 24 bytes of DEVICE memory owned by the caller (zero it first).  Only kernels write it. */
    uint64_t updates;      /* updates applied so far */
    uint64_t seen_applied; /* state->applied at the last one */
    float w;               /* 1 - decay_t of the last call */
    int32_t apply;         /* whether the last call moved the average */
} fd_ema_state;
FD_API int fd_ema_multi(fd_handle h, const fd_ema_item *items, int n, const fd_ema_hyper *hyper, const fd_train_state *state,
                        fd_ema_state *ema, void *stream);

/* An evaluation pass over a held-out corpus on the device (fastdiff_amd/validate.py: Validator): every item exactly once,
 * windows and draws a pure function of (seed, batch index), everything accumulated in device memory.  A pass keeps an fd_train_state
 * of its own whose `iter` is the batch index (zeroed at the start of a pass); fd_train_draw is used as it is on that state and seed.
 *
 * fd_eval_collate: the batch of an evaluation pass; arguments and limits as fd_train_collate (no rank / world: the held-out loader is
 * neither shuffled nor sharded, vocoder_base.py:29).  With `it` = state ? state->iter : iter_host, slot b stands at g = it B + b
 * (< 2^64) and takes
 *   g <  n_items: item g,           picked[b] = (g, start)
 *   g >= n_items: item n_items - 1, picked[b] = (-1, -1)      (inactive: filled so that the forward reads finite data)
 *   start = (w * (T_item - F)) >> 32, w = word b & 3 of Philox4x32-10 keyed (seed, stream 0xFFFFFFFC, position b >> 2, id it)
 * -- the training collater's start draw; no new stream.  TrainCorpus.eval_plan is the host twin. */
FD_API int fd_eval_collate(fd_handle h, const float *wav_arena, const float *mel_arena, const int64_t *frame_off, int64_t n_items, int hop,
                           int F, int B, uint64_t seed, const fd_train_state *state, uint64_t iter_host, float *wavs, float *mels,
                           int64_t *picked, void *stream);

/* out[i] = mean over item i's n elements of (a - b)^2 (kind 0) or |a - b| (kind 1); a, b [B, n] (device, float32, contiguous, the
 * arrays 16-byte aligned; n need not be a multiple of 4), out [B].  Sums as above in this section: a thread adds a run of FD_STEP_RUN
 * elements (four 16-byte loads per operand; only an item's first and last 16 bytes are read element-wise where n or the item's
 * offset is no multiple of 4), a tree inside the workgroup, per-workgroup partial sums in the handle's step scratch, one final
 * workgroup per item.  A workgroup never touches two items: a non-finite element spoils its own item's value only.  No atomics; two runs agree bit
 * for bit.  B n < 2^36. */
FD_API int fd_item_distance(fd_handle h, const float *a, const float *b, int B, int64_t n, int kind, float *out, void *stream);

/* The accumulators of a pass: caller-owned device memory, zeroed before the pass; only fd_eval_accumulate writes it. */
#define FD_EVAL_MAX_BINS 64
typedef struct fd_eval_state {
    double sum;                              /* of the finite values of active slots, added in slot order */
    uint64_t count;                          /* how many */
    uint64_t nonfinite;                      /* active slots whose value was inf or NaN (not added anywhere) */
    uint64_t reserved;
    double bin_sum[FD_EVAL_MAX_BINS];        /* the same per bin of the diffusion step */
    uint64_t bin_count[FD_EVAL_MAX_BINS];
} fd_eval_state;

/* One launch of one workgroup.  For every slot b with picked[b][0] >= 0, in slot order: item_out[picked[b][0]] = values[b] (item_out
 * nullable); a finite values[b] is added (as double) to acc->sum with count += 1 and, when steps is not NULL, to bin
 * (ts * bins) / T_train, ts = (integer) steps[b] as fd_train_draw writes it; a non-finite one only counts in acc->nonfinite.  Inactive
 * slots contribute nothing.  advance (nullable): the pass's fd_train_state; its `iter` += 1, behind every read of it in stream order
 * (as fd_adamw_multi does for a training step).  1 <= bins <= FD_EVAL_MAX_BINS; T_train >= 1. */
FD_API int fd_eval_accumulate(fd_handle h, const float *values, const float *steps, const int64_t *picked, int B, int T_train, int bins,
                              fd_eval_state *acc, float *item_out, fd_train_state *advance, void *stream);

/* The scheduling network and what surrounds it (fastdiff_amd/noisepred.py: NoisePredictor, phistep.py: PhiStep, sampler.noise_scheduling
 * with search = "device").  The reference calls a `noise_pred` (util.py:284,356) that it never defines: the network below is
 * this project's own, in BDDM's form beta_hat = min(beta_next, delta^2) * sigma_phi(x).  Sums as above in this section: runs of
 * FD_STEP_RUN, a fixed tree, per-workgroup results in the handle's step scratch, one final workgroup; no workgroup touches two items, no
 * floating-point atomics, two runs agree bit for bit.  Calls on one handle are ordered on one stream; the first call at a new size must
 * not sit inside a graph capture.
 *
 * Band energies.  x [B, L] (16-byte aligned, L a multiple of 32, L >= 64), W [32, 64], b [32], F = L / 32 - 1 frames of 64 samples at
 * stride 32, no padding:
 *   y[b,c,f] = b[c] + sum_k W[c,k] x[b, 32 f + k]   (one sum of 64 products in tap order, then the bias)
 *   feat[b,c] = log(1e-6 + mean_f y[b,c,f]^2)                                                                        feat [B, 32]
 * x is read 16 bytes per lane.  The backward recomputes y:  dy = dfeat[b,c] 2 y / (F (1e-6 + mean y^2)),
 * dW[c,k] = sum_{b,f} dy x[b, 32 f + k], db[c] = sum_{b,f} dy (items in order, frames in order).  No dx: x is data.  L < 2^31. */
FD_API int fd_bandpool_forward(fd_handle h, const float *x, const float *W, const float *b, int B, int64_t L, float *feat, void *stream);
FD_API int fd_bandpool_backward(fd_handle h, const float *x, const float *W, const float *b, const float *dfeat, int B, int64_t L, float *dW,
                                float *db, void *stream);

/* The head, one workgroup (thread j = hidden unit j; sums over items in item order):
 *   in[b] = (feat[b, 0..31], ln beta_next[r], ln delta2[r])      r = b (R = B) or 0 (R = 1: the condition is broadcast)
 *   h = swish(W1 in + b1)   u = W2 h + b2   ratio[b] = 1e-4 + (1 - 2e-4) sigmoid(u)         W1 [64, 34], b1 [64], W2 [1, 64], b2 [1]
 *   R = B: beta_hat[b] = min(beta_next[b], delta2[b]) ratio[b];    R = 1: beta_hat[0] = min(beta_next, delta2) (sum_b ratio[b]) / B
 * beta_hat [R], ratio [B].  The backward (R = B only) takes dbeta_hat [B] and writes dW1, db1, dW2, db2 and dfeat [B, 32]. */
FD_API int fd_npred_head_forward(fd_handle h, const float *feat, const float *beta_next, const float *delta2, int R, const float *W1,
                                 const float *b1, const float *W2, const float *b2, int B, float *beta_hat, float *ratio, void *stream);
FD_API int fd_npred_head_backward(fd_handle h, const float *feat, const float *beta_next, const float *delta2, const float *W1, const float *b1,
                                  const float *W2, const float *b2, const float *dbeta_hat, int B, float *dW1, float *db1, float *dW2,
                                  float *db2, float *dfeat, void *stream);

/* The draws of phi_loss (util.py:340-350) on the device; arguments as fd_train_draw plus tau, T_train > 2 tau.  With `it` as there,
 *   ts[b] = tau + ((w * (T_train - 2 tau)) >> 32), w = word b & 3 of Philox4x32-10 keyed (seed, stream 0xFFFFFFFA, position b >> 2, id it)
 *   z[b,t] = component (b L + t) & 3 of the generator's normal4 keyed (seed, stream 0xFFFFFFF9, position (b L + t) >> 2, id it)
 *   a = alpha[ts], a' = alpha[ts + tau]:  beta_nxt = 1 - (a' / a)^2,  delta = sqrt(1 - a^2),  delta2 = delta delta,  x_t = a x0 + delta z
 * every operation rounded on its own.  steps, beta_nxt, delta, delta2: [B]. */
FD_API int fd_phi_draw(fd_handle h, const float *x0, const float *alpha, int T_train, int tau, int B, int64_t L, uint64_t seed,
                       const fd_train_state *state, uint64_t iter_host, float *x_t, float *z, float *steps, float *beta_nxt, float *delta,
                       float *delta2, void *stream);

/* The residual of phi_loss: with r = delta[b] z - (beta_hat[b] / delta[b]) eps, m[b] = mean_t r^2 and s[b] = mean_t r eps.  eps, z [B, L]
 * (16-byte aligned, L a multiple of 4); delta, beta_hat, m, s [B].  d m[b] / d beta_hat[b] = (-2 / delta[b]) s[b]. */
FD_API int fd_phi_residual_forward(fd_handle h, const float *eps, const float *z, const float *delta, const float *beta_hat, int B, int64_t L,
                                   float *m, float *s, void *stream);

/* The greedy schedule search (noise_scheduling, util.py:254-288) with its state in device memory: caller-owned, written only by kernels. */
#define FD_SCHED_MAX_STEPS 64
typedef struct fd_sched_state {
    float alpha_cur, beta_cur;
    int32_t stopped;                       /* 0 running, 1 alpha > 1, 2 beta < rho */
    int32_t n_found;
    float found[FD_SCHED_MAX_STEPS];       /* the accepted betas, in the order of the search (the schedule is their reverse) */
    float step;                            /* the current step, as written to steps_out */
    int32_t ddim;
    float coef[4];                         /* DDPM: c, d;  "ddim": c1, c2, c3 */
    float cond[2];                         /* (beta_cur, 1 - alpha_cur^2) as last written to cond_out */
} fd_sched_state;
/* state := (alphaN, betaN), running, nothing found. */
FD_API int fd_sched_init(fd_handle h, fd_sched_state *state, float betaN, float alphaN, void *stream);
/* One thread.  While running: a pending beta_hat [n_hat] (NULL: none) gives beta = (sum in order) / n_hat; (double) beta < rho stops the
 * search (stopped = 2), else beta_cur = beta.  Still running: step = map_noise_scale_to_time_step(alpha_cur, alpha) (util.py:394-404: the
 * clamps, the first bracket alpha[t+1] <= a <= alpha[t], frac as a float32 difference and quotient, (float)((double) t + (double) frac),
 * -1 without a bracket); step >= 0 appends beta_cur to found; steps_out[0..B) = step; the update's coefficients as float32 scalars:
 *   DDPM:   c = beta_cur / sqrt(1 - alpha_cur^2), d = sqrt(1 - beta_cur)
 *   "ddim": a_next = alpha_cur / sqrt(1 - beta_cur), c1 = a_next / alpha_cur, c2 = -sqrt(1 - alpha_cur^2) c1, c3 = sqrt(1 - a_next^2) */
FD_API int fd_sched_begin(fd_handle h, fd_sched_state *state, const float *beta_hat, int n_hat, double rho, const float *alpha, int T_train,
                          int ddim, float *steps_out, int B, void *stream);
/* While running: x = (x - c eps) / d  or  x = (c1 x + c2 eps) + c3 eps  over n elements (16 bytes per lane, every operation rounded on its
 * own; n a multiple of 4), then in a launch of its own alpha_cur = alpha_cur / sqrt(1 - beta_cur); alpha_cur > 1 stops the search
 * (stopped = 1), else cond_out = (beta_cur, 1 - alpha_cur^2).  Once stopped, x and cond_out are left untouched. */
FD_API int fd_sched_update(fd_handle h, fd_sched_state *state, float *x, const float *eps, int64_t n, float *cond_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FASTDIFF_HIP_TRAIN_H */
