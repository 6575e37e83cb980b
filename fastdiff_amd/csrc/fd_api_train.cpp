// fd_api_train.cpp -- host side of the training operators of include/fastdiff_hip_train.h: argument checks, scratch
// buffers and launches of fd_kernels_train / _kconv / _cconv.hip.  Nothing here is on the inference path.
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>

#include "fd_kernels.h"
#include "fd_host.h"

#define FD_TRY(expr)                        \
    do {                                    \
        const int rc__ = (expr);            \
        if (rc__ != FD_OK) return rc__;     \
    } while (0)

// The backward passes add up partial sums, and the LVC operator's matrix-pipe kernels read the predicted kernels frame-major, through
// scratch buffers kept on the handle (fd_context: lvc_scratch, kconv_scratch, cconv_scratch, step_scratch), reserved by run_scratch
// (fd_host.h) before the launch: grown when a call needs more, which is refused inside a stream capture.

static bool slope_ok(float s) { return s > 0.0f && s <= 1.0f; }      // a leaky-relu slope: (0, 1], 1 = no activation

static int check_batch(fd_handle h, int B, const char *who)
{
    if (B <= 0 || B > 65535) FD_FAIL(h, FD_ERR_INVALID, "%s: B=%d", who, B);
    return FD_OK;
}

// the host arrays of device pointers of the *_multi entry points: every list given and none of its n items null
static int check_lists(fd_handle h, int n, std::initializer_list<const void *> lists, const char *who)
{
    for (const void *list : lists) {
        const void *const *l = reinterpret_cast<const void *const *>(list);
        if (!l) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer list", who);
        for (int i = 0; i < n; ++i)
            if (!l[i]) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer in item %d", who, i);
    }
    return FD_OK;
}

static int check_multi(fd_handle h, int n, int B, std::initializer_list<const void *> lists, const char *who)
{
    if (n < 1 || n > 8) FD_FAIL(h, FD_ERR_INVALID, "%s: n=%d outside 1..8", who, n);
    FD_TRY(check_batch(h, B, who));
    return check_lists(h, n, lists, who);
}

extern "C" {

static int check_lvc_op(fd_handle h, int B, int Cin, int Cout, int ks, int T, int hop, const char *who)
{
    if (B <= 0 || Cin <= 0 || Cout <= 0 || T <= 0 || hop <= 0 || ks <= 0 || (ks & 1) == 0)
        FD_FAIL(h, FD_ERR_INVALID, "%s: B=%d Cin=%d Cout=%d ks=%d T=%d hop=%d must be positive, ks odd", who, B, Cin, Cout, ks, T, hop);
    if ((int64_t)Cin * Cout * ks > 8192 || Cout > 256)
        FD_FAIL(h, FD_ERR_UNSUPPORTED, "%s: Cin*Cout*ks = %lld > 8192 (or Cout > 256) has no kernel", who, (long long)Cin * Cout * ks);
    if ((int64_t)B * std::max(Cin, Cout) * T * hop >= (int64_t)1 << 31)
        FD_FAIL(h, FD_ERR_INVALID, "%s: tensor too large for one call", who);
    if (B > 65535 || std::max(Cin, Cout) > 65535) FD_FAIL(h, FD_ERR_INVALID, "%s: B, channels <= 65535", who);
    return FD_OK;
}

// The operator's frame-major copy of the predicted kernels (B*T*Cin*Cout*ks floats), for the shapes whose kernels read one; else 0 floats
// and a null pointer
static size_t lvc_scratch_floats(int B, int Cin, int Cout, int ks, int T, int hop)
{
    return fdk::lvc_op_needs_scratch(Cin, Cout, ks, hop) ? (size_t)B * T * Cin * Cout * ks : 0;
}

// a batch stride of the operator's kernel / dkernel: 0 or the tensor's own size, or, for the model's shape, anything beyond that
static bool lvc_stride_ok(int64_t st, int Cin, int Cout, int ks, int T, int hop)
{
    const int64_t own = (int64_t)Cin * Cout * ks * T;
    return st == 0 || st == own || (st > own && fdk::lvc_op_needs_scratch(Cin, Cout, ks, hop));
}

int fd_lvc_forward_strided(fd_handle h, const float *x, const float *kernel, int64_t kernel_bstride, const float *bias, int B, int Cin, int Cout,
                           int ks, int T, int hop, float *out, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!x || !kernel || !bias || !out) FD_FAIL(h, FD_ERR_INVALID, "fd_lvc_forward: null pointer");
    FD_TRY(check_lvc_op(h, B, Cin, Cout, ks, T, hop, "fd_lvc_forward"));
    if (!lvc_stride_ok(kernel_bstride, Cin, Cout, ks, T, hop))
        FD_FAIL(h, FD_ERR_UNSUPPORTED, "fd_lvc_forward: a batch-strided kernel (stride %lld) needs the model's shape (32 -> 64, k3, hop 8 / 64 / 256)", (long long)kernel_bstride);
    const size_t floats = lvc_scratch_floats(B, Cin, Cout, ks, T, hop);
    return run_scratch(h, stream, "fd_lvc_forward", h->lvc_scratch, floats, [&](const fdk::Launch &L, float *scratch) {
        return fdk::lvc_op_forward(L, x, kernel, bias, out, B, Cin, Cout, ks, T, hop, floats ? scratch : nullptr, kernel_bstride);
    });
}

int fd_lvc_forward(fd_handle h, const float *x, const float *kernel, const float *bias, int B, int Cin, int Cout, int ks, int T, int hop,
                   float *out, void *stream)
{
    return fd_lvc_forward_strided(h, x, kernel, 0, bias, B, Cin, Cout, ks, T, hop, out, stream);
}

int fd_lvc_backward_strided(fd_handle h, const float *x, const float *kernel, int64_t kernel_bstride, const float *dout, int B, int Cin, int Cout,
                            int ks, int T, int hop, float *dx, float *dkernel, int64_t dkernel_bstride, float *dbias, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!dout || ((dkernel || dbias) && !x) || (dx && !kernel)) FD_FAIL(h, FD_ERR_INVALID, "fd_lvc_backward: null pointer");
    FD_TRY(check_lvc_op(h, B, Cin, Cout, ks, T, hop, "fd_lvc_backward"));
    for (int64_t st : {kernel_bstride, dkernel_bstride})
        if (!lvc_stride_ok(st, Cin, Cout, ks, T, hop))
            FD_FAIL(h, FD_ERR_UNSUPPORTED, "fd_lvc_backward: a batch-strided kernel / dkernel (stride %lld) needs the model's shape (32 -> 64, k3, hop 8 / 64 / 256)", (long long)st);
    const size_t floats = lvc_scratch_floats(B, Cin, Cout, ks, T, hop);
    return run_scratch(h, stream, "fd_lvc_backward", h->lvc_scratch, floats, [&](const fdk::Launch &L, float *scratch) {
        return fdk::lvc_op_backward(L, x, kernel, dout, dx, dkernel, dbias, B, Cin, Cout, ks, T, hop, floats ? scratch : nullptr, kernel_bstride, dkernel_bstride);
    });
}

int fd_lvc_backward(fd_handle h, const float *x, const float *kernel, const float *dout, int B, int Cin, int Cout, int ks, int T, int hop,
                    float *dx, float *dkernel, float *dbias, void *stream)
{
    return fd_lvc_backward_strided(h, x, kernel, 0, dout, B, Cin, Cout, ks, T, hop, dx, dkernel, 0, dbias, stream);
}

// kernel_conv of the KernelPredictor (training path).  The backward adds up partial sums (row slices for dx, utterance ranges for
// dweight / dbias, each in a fixed order) in the kconv scratch buffer.
static int check_act(fd_handle h, int M, int T, float post, const char *who)
{
    if (!slope_ok(post)) FD_FAIL(h, FD_ERR_INVALID, "%s: the leaky-relu slope must lie in (0, 1] (1 = no activation), got %g", who, post);
    if (post != 1.0f && !fdk::kconv_act_supported(M, T)) FD_FAIL(h, FD_ERR_UNSUPPORTED, "%s: the fused activation covers M <= 512 (the predictor's small convolutions), got M=%d", who, M);
    return FD_OK;
}

// M and T of the *_multi forms (the predictor's small convolutions)
static int check_small(fd_handle h, int M, int T, const char *who)
{
    if (!fdk::kconv_act_supported(M, T)) FD_FAIL(h, FD_ERR_UNSUPPORTED, "%s: M=%d (a multiple of 32, <= 512) and T=%d (1..128) only", who, M, T);
    return FD_OK;
}

int fd_kconv_forward_act(fd_handle h, const float *x, const float *weight, const float *bias, int B, int M, int T, float post_slope, float *out,
                         void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!x || !weight || !bias || !out) FD_FAIL(h, FD_ERR_INVALID, "fd_kconv_forward: null pointer");
    FD_TRY(check_batch(h, B, "fd_kconv_forward"));
    if (!fdk::kconv_supported(M, T)) FD_FAIL(h, FD_ERR_UNSUPPORTED, "fd_kconv_forward: M=%d (a multiple of 32) and T=%d (1..128) only", M, T);
    FD_TRY(check_act(h, M, T, post_slope, "fd_kconv_forward"));
    return run(h, stream, "fd_kconv_forward", [&](const fdk::Launch &L) { return fdk::kconv_forward(L, x, weight, bias, out, B, M, T, false, post_slope); });
}

int fd_kconv_forward(fd_handle h, const float *x, const float *weight, const float *bias, int B, int M, int T, float *out, void *stream)
{
    return fd_kconv_forward_act(h, x, weight, bias, B, M, T, 1.0f, out, stream);
}

int fd_kconv_backward_act(fd_handle h, const float *x, const float *weight, const float *y, const float *dout, int B, int M, int T,
                          float post_slope, float in_slope, float *dx, float *dweight, float *dbias, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!dout || ((dweight || dbias) && !x) || (dx && !weight)) FD_FAIL(h, FD_ERR_INVALID, "fd_kconv_backward: null pointer");
    FD_TRY(check_batch(h, B, "fd_kconv_backward"));
    if (!fdk::kconv_supported(M, T)) FD_FAIL(h, FD_ERR_UNSUPPORTED, "fd_kconv_backward: M=%d (a multiple of 32) and T=%d (1..128) only", M, T);
    FD_TRY(check_act(h, M, T, post_slope, "fd_kconv_backward"));
    if (post_slope != 1.0f && !y) FD_FAIL(h, FD_ERR_INVALID, "fd_kconv_backward: a fused activation needs the forward's output y");
    if (!slope_ok(in_slope)) FD_FAIL(h, FD_ERR_INVALID, "fd_kconv_backward: in_slope must lie in (0, 1], got %g", in_slope);
    if (in_slope != 1.0f && dx && !x) FD_FAIL(h, FD_ERR_INVALID, "fd_kconv_backward: in_slope needs x");
    return run_scratch(h, stream, "fd_kconv_backward", h->kconv_scratch, fdk::kconv_scratch_floats(B, M, T), [&](const fdk::Launch &L, float *scratch) {
        return fdk::kconv_backward(L, x, weight, dout, dx, dweight, dbias, B, M, T, scratch, false, post_slope != 1.0f ? y : nullptr, post_slope, in_slope);
    });
}

int fd_kconv_backward(fd_handle h, const float *x, const float *weight, const float *dout, int B, int M, int T, float *dx, float *dweight,
                      float *dbias, void *stream)
{
    return fd_kconv_backward_act(h, x, weight, nullptr, dout, B, M, T, 1.0f, 1.0f, dx, dweight, dbias, stream);
}

int fd_kconv_backward_w_multi(fd_handle h, int n, const float *const *x, const float *const *dout, const float *const *y, int B, int M, int T,
                              float post_slope, float *const *dweight, float *const *dbias, void *stream)
{
    const char *who = "fd_kconv_backward_w_multi";
    if (!h) return FD_ERR_INVALID;
    if (!x || !dout || (!dweight && !dbias)) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    FD_TRY(check_multi(h, n, B, {}, who));
    FD_TRY(check_small(h, M, T, who));
    FD_TRY(check_act(h, M, T, post_slope, who));
    FD_TRY(check_lists(h, n, {x, dout}, who));
    return run_scratch(h, stream, who, h->kconv_scratch, fdk::kconv_w_multi_scratch_floats(n, B, M), [&](const fdk::Launch &L, float *scratch) {
        return fdk::kconv_backward_w_multi(L, n, x, dout, y, post_slope, B, M, T, dweight, dbias, scratch);
    });
}

int fd_kconv_forward_act_multi(fd_handle h, int n, const float *const *x, const float *const *weight, const float *const *bias, int B, int M, int T,
                               float post_slope, float *const *out, void *stream)
{
    const char *who = "fd_kconv_forward_act_multi";
    if (!h) return FD_ERR_INVALID;
    FD_TRY(check_multi(h, n, B, {x, weight, bias, out}, who));
    FD_TRY(check_small(h, M, T, who));
    FD_TRY(check_act(h, M, T, post_slope, who));
    return run(h, stream, who, [&](const fdk::Launch &L) { return fdk::kconv_forward_multi(L, n, x, weight, bias, out, B, M, T, post_slope); });
}

int fd_kconv_backward_x_multi(fd_handle h, int n, const float *const *x, const float *const *weight, const float *const *y, const float *const *dout,
                              int B, int M, int T, float post_slope, float in_slope, float *const *dx, void *stream)
{
    const char *who = "fd_kconv_backward_x_multi";
    if (!h) return FD_ERR_INVALID;
    FD_TRY(check_multi(h, n, B, {weight, dout, dx}, who));
    FD_TRY(check_small(h, M, T, who));
    FD_TRY(check_act(h, M, T, post_slope, who));
    if (!slope_ok(in_slope)) FD_FAIL(h, FD_ERR_INVALID, "%s: in_slope must lie in (0, 1], got %g", who, in_slope);
    if (in_slope != 1.0f) FD_TRY(check_lists(h, n, {x}, who));
    if (post_slope != 1.0f && !y) FD_FAIL(h, FD_ERR_INVALID, "%s: a fused activation needs the forward's outputs y", who);
    return run_scratch(h, stream, who, h->kconv_scratch, fdk::kconv_x_multi_scratch_floats(n, B, M, T), [&](const fdk::Launch &L, float *scratch) {
        return fdk::kconv_backward_x_multi(L, n, x, weight, post_slope != 1.0f ? y : nullptr, dout, dx, B, M, T, post_slope, in_slope, scratch);
    });
}

// The predictor's input convolution (80 -> 64, k5) with its activation (fd_kernels_kconv.hip: k_ic_*); per-utterance partial sums of
// the weight gradient in the kconv scratch buffer.  The single entry points are the n = 1 case of the _multi ones.
static int check_input_conv(fd_handle h, int B, int T, float post, const char *who)
{
    FD_TRY(check_batch(h, B, who));
    if (T < 1 || T > 128) FD_FAIL(h, FD_ERR_UNSUPPORTED, "%s: T=%d (1..128) only", who, T);
    if (!slope_ok(post)) FD_FAIL(h, FD_ERR_INVALID, "%s: the leaky-relu slope must lie in (0, 1] (1 = no activation), got %g", who, post);
    return FD_OK;
}

static int input_conv_forward(fd_handle h, int n, const float *const *x, const float *const *weight, const float *const *bias, int B, int T,
                              float post_slope, float *const *out, void *stream, const char *who)
{
    FD_TRY(check_input_conv(h, B, T, post_slope, who));
    return run(h, stream, who, [&](const fdk::Launch &L) { return fdk::input_conv_forward_multi(L, n, x, weight, bias, out, B, T, post_slope); });
}

// dx / dweight / dbias: null = not wanted (a list, or the one pointer of the single form)
static int input_conv_backward(fd_handle h, int n, const float *const *x, const float *const *weight, const float *const *y, const float *const *dout,
                               int B, int T, float post_slope, float *const *dx, float *const *dweight, float *const *dbias, void *stream, const char *who)
{
    return run_scratch(h, stream, who, h->kconv_scratch, fdk::input_conv_multi_scratch_floats(n, B), [&](const fdk::Launch &L, float *scratch) {
        return fdk::input_conv_backward_multi(L, n, x, weight, y, dout, dx, dweight, dbias, B, T, post_slope, scratch);
    });
}

int fd_input_conv_forward_multi(fd_handle h, int n, const float *const *x, const float *const *weight, const float *const *bias, int B, int T,
                                float post_slope, float *const *out, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    FD_TRY(check_multi(h, n, B, {x, weight, bias, out}, "fd_input_conv_forward_multi"));
    return input_conv_forward(h, n, x, weight, bias, B, T, post_slope, out, stream, "fd_input_conv_forward_multi");
}

int fd_input_conv_backward_multi(fd_handle h, int n, const float *const *x, const float *const *weight, const float *const *y, const float *const *dout,
                                 int B, int T, float post_slope, float *const *dx, float *const *dweight, float *const *dbias, void *stream)
{
    const char *who = "fd_input_conv_backward_multi";
    if (!h) return FD_ERR_INVALID;
    FD_TRY(check_multi(h, n, B, {x, weight, y, dout}, who));
    FD_TRY(check_input_conv(h, B, T, post_slope, who));
    if (dx) FD_TRY(check_lists(h, n, {dx}, who));
    return input_conv_backward(h, n, x, weight, y, dout, B, T, post_slope, dx, dweight, dbias, stream, who);
}

int fd_input_conv_forward(fd_handle h, const float *x, const float *weight, const float *bias, int B, int T, float post_slope, float *out, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!x || !weight || !bias || !out) FD_FAIL(h, FD_ERR_INVALID, "fd_input_conv_forward: null pointer");
    return input_conv_forward(h, 1, &x, &weight, &bias, B, T, post_slope, &out, stream, "fd_input_conv_forward");
}

int fd_input_conv_backward(fd_handle h, const float *x, const float *weight, const float *y, const float *dout, int B, int T, float post_slope,
                           float *dx, float *dweight, float *dbias, void *stream)
{
    const char *who = "fd_input_conv_backward";
    if (!h) return FD_ERR_INVALID;
    if (!dout || !y || ((dweight || dbias) && !x) || (dx && !weight)) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    FD_TRY(check_input_conv(h, B, T, post_slope, who));
    return input_conv_backward(h, 1, &x, &weight, &y, &dout, B, T, post_slope, dx ? &dx : nullptr, dweight ? &dweight : nullptr,
                               dbias ? &dbias : nullptr, stream, who);
}

// weight-norm of n tensors (fd_kernels_cconv.hip); the single entry points are one item
static int weight_norm(fd_handle h, const fd_wn_item *items, int n, void *stream, bool backward, const char *who)
{
    if (!items) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    if (n <= 0 || n > 4096) FD_FAIL(h, FD_ERR_INVALID, "%s: n=%d", who, n);
    for (int i = 0; i < n; ++i) {
        const fd_wn_item &I = items[i];
        if (I.rows <= 0 || I.cols <= 0 || I.rows > ((int64_t)1 << 31) || !I.v || !I.g || !I.norm || (backward ? (!I.dv || !I.dg) : !I.w))
            FD_FAIL(h, FD_ERR_INVALID, "%s: item %d: rows=%lld cols=%d or a null pointer", who, i, (long long)I.rows, I.cols);
    }
    return run(h, stream, who, [&](const fdk::Launch &L) { return fdk::weight_norm_multi(L, items, n, backward); });
}

int fd_weight_norm_multi_forward(fd_handle h, const fd_wn_item *items, int n, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    return weight_norm(h, items, n, stream, false, "fd_weight_norm_multi_forward");
}

int fd_weight_norm_multi_backward(fd_handle h, const fd_wn_item *items, int n, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    return weight_norm(h, items, n, stream, true, "fd_weight_norm_multi_backward");
}

static int check_wn_rows(fd_handle h, int64_t rows, int cols, const char *who)
{
    if (rows <= 0 || cols <= 0 || rows > ((int64_t)1 << 31)) FD_FAIL(h, FD_ERR_INVALID, "%s: rows=%lld cols=%d", who, (long long)rows, cols);
    return FD_OK;
}

int fd_weight_norm_forward(fd_handle h, const float *v, const float *g, int64_t rows, int cols, float *w, float *norm, void *stream)
{
    const char *who = "fd_weight_norm_forward";
    if (!h) return FD_ERR_INVALID;
    if (!v || !g || !w || !norm) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    FD_TRY(check_wn_rows(h, rows, cols, who));
    const fd_wn_item item = {v, g, w, norm, nullptr, nullptr, nullptr, rows, cols, 0};
    return weight_norm(h, &item, 1, stream, false, who);
}

int fd_weight_norm_backward(fd_handle h, const float *v, const float *g, const float *norm, const float *dw, int64_t rows, int cols, float *dv,
                            float *dg, void *stream)
{
    const char *who = "fd_weight_norm_backward";
    if (!h) return FD_ERR_INVALID;
    if (!v || !g || !norm || !dw || !dv || !dg) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    FD_TRY(check_wn_rows(h, rows, cols, who));
    const fd_wn_item item = {v, g, nullptr, const_cast<float *>(norm), dw, dv, dg, rows, cols, 0};
    return weight_norm(h, &item, 1, stream, true, who);
}

// A skip tensor's fan-out (fd_kernels_train.hip: k_fan_*).
static int check_fan(fd_handle h, int rows, int64_t L, int factor, const char *who)
{
    if (rows <= 0 || rows > 65535 || L <= 0 || factor < 1 || L % factor != 0) FD_FAIL(h, FD_ERR_INVALID, "%s: rows=%d L=%lld factor=%d", who, rows, (long long)L, factor);
    return FD_OK;
}

int fd_fan_forward(fd_handle h, const float *x, int rows, int64_t L, int factor, float *picked, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!x || !picked) FD_FAIL(h, FD_ERR_INVALID, "fd_fan_forward: null pointer");
    FD_TRY(check_fan(h, rows, L, factor, "fd_fan_forward"));
    return run(h, stream, "fd_fan_forward", [&](const fdk::Launch &La) { return fdk::fan_pick(La, x, picked, rows, L, factor); });
}

int fd_fan_backward(fd_handle h, const float *g0, const float *g1, const float *g2, const float *g3, const float *gpicked, int rows, int64_t L,
                    int factor, float *dx, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!dx) FD_FAIL(h, FD_ERR_INVALID, "fd_fan_backward: null pointer");
    FD_TRY(check_fan(h, rows, L, factor, "fd_fan_backward"));
    const float *g[4] = {g0, g1, g2, g3};
    return run(h, stream, "fd_fan_backward", [&](const fdk::Launch &La) { return fdk::fan_sum(La, g, gpicked, dx, rows, L, factor); });
}

// "frames": kernel_conv and the operator joined through frame-major tensors (include/fastdiff_hip.h)
static int check_kconv_frames(fd_handle h, int B, int M, int T, const char *who)
{
    FD_TRY(check_batch(h, B, who));
    if (!fdk::kconv_frames_supported(M, T)) FD_FAIL(h, FD_ERR_UNSUPPORTED, "%s: M=%d (a multiple of 6144) and T=%d (1..128) only", who, M, T);
    return FD_OK;
}

int fd_kconv_forward_frames(fd_handle h, const float *x, const float *weight, const float *bias, int B, int M, int T, float *frames, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!x || !weight || !bias || !frames) FD_FAIL(h, FD_ERR_INVALID, "fd_kconv_forward_frames: null pointer");
    FD_TRY(check_kconv_frames(h, B, M, T, "fd_kconv_forward_frames"));
    return run(h, stream, "fd_kconv_forward_frames", [&](const fdk::Launch &L) { return fdk::kconv_forward(L, x, weight, bias, frames, B, M, T, true); });
}

int fd_kconv_backward_frames(fd_handle h, const float *x, const float *weight, const float *dframes, int B, int M, int T, float *dx,
                             float *dweight, float *dbias, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!dframes || ((dweight || dbias) && !x) || (dx && !weight)) FD_FAIL(h, FD_ERR_INVALID, "fd_kconv_backward_frames: null pointer");
    FD_TRY(check_kconv_frames(h, B, M, T, "fd_kconv_backward_frames"));
    return run_scratch(h, stream, "fd_kconv_backward_frames", h->kconv_scratch, fdk::kconv_scratch_floats(B, M, T), [&](const fdk::Launch &L, float *scratch) {
        return fdk::kconv_backward(L, x, weight, dframes, dx, dweight, dbias, B, M, T, scratch, true);
    });
}

static int check_frames_stride(fd_handle h, int64_t st, int T, const char *who)
{
    if (st < (int64_t)T * 6144 || st % 4 != 0) FD_FAIL(h, FD_ERR_INVALID, "%s: a frame stride of %lld floats (at least T * 6144, a multiple of 4)", who, (long long)st);
    return FD_OK;
}

static int check_lvc_frames(fd_handle h, int B, int T, int hop, const char *who)
{
    FD_TRY(check_lvc_op(h, B, 32, 64, 3, T, hop, who));
    if (!fdk::lvc_op_needs_scratch(32, 64, 3, hop)) FD_FAIL(h, FD_ERR_UNSUPPORTED, "%s: hop 8 / 64 / 256 only, got %d", who, hop);
    return FD_OK;
}

int fd_lvc_forward_frames(fd_handle h, const float *x, const float *kernel_frames, int64_t kernel_bstride, const float *bias, int64_t bias_bstride,
                          int B, int T, int hop, float *out, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!x || !kernel_frames || !bias || !out) FD_FAIL(h, FD_ERR_INVALID, "fd_lvc_forward_frames: null pointer");
    FD_TRY(check_lvc_frames(h, B, T, hop, "fd_lvc_forward_frames"));
    FD_TRY(check_frames_stride(h, kernel_bstride, T, "fd_lvc_forward_frames"));
    if (bias_bstride != 0 && bias_bstride < (int64_t)64 * T) FD_FAIL(h, FD_ERR_INVALID, "fd_lvc_forward_frames: bias stride %lld < 64 * T", (long long)bias_bstride);
    return run(h, stream, "fd_lvc_forward_frames", [&](const fdk::Launch &L) {
        return fdk::lvc_op_forward(L, x, kernel_frames, bias, out, B, 32, 64, 3, T, hop, nullptr, kernel_bstride, true, bias_bstride);
    });
}

int fd_lvc_backward_frames(fd_handle h, const float *x, const float *kernel_frames, int64_t kernel_bstride, const float *dout, int B, int T,
                           int hop, float *dx, float *dkernel_frames, int64_t dkernel_bstride, float *dbias, int64_t dbias_bstride, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!dout || ((dkernel_frames || dbias) && !x) || (dx && !kernel_frames)) FD_FAIL(h, FD_ERR_INVALID, "fd_lvc_backward_frames: null pointer");
    FD_TRY(check_lvc_frames(h, B, T, hop, "fd_lvc_backward_frames"));
    if (dx) FD_TRY(check_frames_stride(h, kernel_bstride, T, "fd_lvc_backward_frames"));
    if (dkernel_frames) FD_TRY(check_frames_stride(h, dkernel_bstride, T, "fd_lvc_backward_frames"));
    if (dbias && dbias_bstride != 0 && dbias_bstride < (int64_t)64 * T) FD_FAIL(h, FD_ERR_INVALID, "fd_lvc_backward_frames: dbias stride %lld < 64 * T", (long long)dbias_bstride);
    const size_t floats = dx && !h->lvc_dx_gather ? lvc_scratch_floats(B, 32, 64, 3, T, hop) : 0;      // option lvc_dx = copy: the dx kernel's operand order
    return run_scratch(h, stream, "fd_lvc_backward_frames", h->lvc_scratch, floats, [&](const fdk::Launch &L, float *scratch) {
        return fdk::lvc_op_backward(L, x, kernel_frames, dout, dx, dkernel_frames, dbias, B, 32, 64, 3, T, hop, floats ? scratch : nullptr,
                                    kernel_bstride, dkernel_bstride, true, dbias_bstride);
    });
}

// The small convolutions of the training path (fd_kernels_cconv.hip).  The backward's per-workgroup partial sums live in the cconv
// scratch buffer.
static int check_conv32(fd_handle h, int B, int64_t L, int dil, float pre, float post, const char *who)
{
    if (B <= 0 || B > 65535 || L <= 0) FD_FAIL(h, FD_ERR_INVALID, "%s: B=%d L=%lld", who, B, (long long)L);
    if (!slope_ok(pre) || !slope_ok(post))
        FD_FAIL(h, FD_ERR_INVALID, "%s: leaky-relu slopes must lie in (0, 1] (1 = no activation), got %g / %g", who, pre, post);
    if (!fdk::cconv_supported(dil, L))
        FD_FAIL(h, FD_ERR_UNSUPPORTED, "%s: dilation %d (1, 2, 3, 4, 9, 27) and a length that is a multiple of 4 only, got L=%lld", who, dil, (long long)L);
    if ((int64_t)B * 32 * L >= (int64_t)1 << 40) FD_FAIL(h, FD_ERR_INVALID, "%s: tensor too large", who);
    return FD_OK;
}

int fd_conv32_forward(fd_handle h, const float *x, const float *skip, const float *weight, const float *bias, int B, int64_t L, int dilation,
                      float pre_slope, float post_slope, float *xs_out, float *y, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!x || !weight || !bias || !y || (skip && !xs_out)) FD_FAIL(h, FD_ERR_INVALID, "fd_conv32_forward: null pointer (xs_out is needed with a skip)");
    FD_TRY(check_conv32(h, B, L, dilation, pre_slope, post_slope, "fd_conv32_forward"));
    return run(h, stream, "fd_conv32_forward", [&](const fdk::Launch &La) {
        return fdk::cconv_forward(La, x, skip, weight, bias, xs_out, y, B, L, dilation, pre_slope, post_slope);
    });
}

int fd_conv32_backward(fd_handle h, const float *xs, const float *y, const float *weight, const float *dy, const float *gxs, int B, int64_t L,
                       int dilation, float pre_slope, float post_slope, float *dxs, float *dweight, float *dbias, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!xs || !y || !weight || !dy) FD_FAIL(h, FD_ERR_INVALID, "fd_conv32_backward: null pointer");
    FD_TRY(check_conv32(h, B, L, dilation, pre_slope, post_slope, "fd_conv32_backward"));
    return run_scratch(h, stream, "fd_conv32_backward", h->cconv_scratch, fdk::cconv_scratch_floats({h, nullptr, false}, dilation, B, L), [&](const fdk::Launch &La, float *scratch) {
        return fdk::cconv_backward(La, xs, y, weight, dy, gxs, dxs, dweight, dbias, B, L, dilation, pre_slope, post_slope, scratch);
    });
}

static int check_conv7(fd_handle h, int which, int B, int64_t L, const char *who)
{
    if ((which != 0 && which != 1) || B <= 0 || B > 65535 || L < 4 || L % 4 != 0 || L >= ((int64_t)1 << 25))
        FD_FAIL(h, FD_ERR_UNSUPPORTED, "%s: which=%d (0 first_audio_conv, 1 final_conv), B=%d, L=%lld (a multiple of 4)", who, which, B, (long long)L);
    return FD_OK;
}

int fd_conv7_forward(fd_handle h, int which, const float *x, const float *weight, const float *bias, int B, int64_t L, float *y, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!x || !weight || !bias || !y) FD_FAIL(h, FD_ERR_INVALID, "fd_conv7_forward: null pointer");
    FD_TRY(check_conv7(h, which, B, L, "fd_conv7_forward"));
    return run(h, stream, "fd_conv7_forward", [&](const fdk::Launch &La) { return fdk::conv7_forward(La, which, x, weight, bias, y, B, L); });
}

int fd_conv7_backward(fd_handle h, int which, const float *x, const float *weight, const float *dy, int B, int64_t L, float *dx, float *dweight,
                      float *dbias, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!x || !weight || !dy) FD_FAIL(h, FD_ERR_INVALID, "fd_conv7_backward: null pointer");
    FD_TRY(check_conv7(h, which, B, L, "fd_conv7_backward"));
    return run_scratch(h, stream, "fd_conv7_backward", h->cconv_scratch, fdk::conv7_scratch_floats({h, nullptr, false}, B, L), [&](const fdk::Launch &La, float *scratch) {
        return fdk::conv7_backward(La, which, x, weight, dy, dx, dweight, dbias, B, L, scratch);
    });
}

static int check_upsample(fd_handle h, int B, int64_t Lin, int ratio, const char *who)
{
    if ((ratio != 4 && ratio != 8) || B <= 0 || B > 65535 || Lin < 1 || Lin * ratio >= ((int64_t)1 << 25))
        FD_FAIL(h, FD_ERR_UNSUPPORTED, "%s: ratio %d (4 or 8), B=%d, Lin=%lld", who, ratio, B, (long long)Lin);
    return FD_OK;
}

int fd_upsample_forward(fd_handle h, const float *x, const float *weight, const float *bias, int B, int64_t Lin, int ratio, float *y, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!x || !weight || !bias || !y) FD_FAIL(h, FD_ERR_INVALID, "fd_upsample_forward: null pointer");
    FD_TRY(check_upsample(h, B, Lin, ratio, "fd_upsample_forward"));
    return run(h, stream, "fd_upsample_forward", [&](const fdk::Launch &La) { return fdk::convt_forward(La, x, weight, bias, y, B, Lin, ratio); });
}

int fd_upsample_backward(fd_handle h, const float *x, const float *weight, const float *dy, int B, int64_t Lin, int ratio, float *dx, float *dweight,
                         float *dbias, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!x || !weight || !dy) FD_FAIL(h, FD_ERR_INVALID, "fd_upsample_backward: null pointer");
    FD_TRY(check_upsample(h, B, Lin, ratio, "fd_upsample_backward"));
    return run_scratch(h, stream, "fd_upsample_backward", h->cconv_scratch, fdk::convt_scratch_floats({h, nullptr, false}, ratio, B, Lin), [&](const fdk::Launch &La, float *scratch) {
        return fdk::convt_backward(La, x, weight, dy, dx, dweight, dbias, B, Lin, ratio, scratch);
    });
}

static int check_gate(fd_handle h, int B, int C, int64_t L, const char *who)
{
    if (B <= 0 || C <= 0 || L <= 0 || B > 65535 || C > 65535) FD_FAIL(h, FD_ERR_INVALID, "%s: B=%d C=%d L=%lld", who, B, C, (long long)L);
    return FD_OK;
}

int fd_gate_forward(fd_handle h, const float *x, const float *y, int B, int C, int64_t L, float *out, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!x || !y || !out) FD_FAIL(h, FD_ERR_INVALID, "fd_gate_forward: null pointer");
    FD_TRY(check_gate(h, B, C, L, "fd_gate_forward"));
    return run(h, stream, "fd_gate_forward", [&](const fdk::Launch &La) { return fdk::gate_forward(La, x, y, out, B, C, L); });
}

int fd_gate_backward(fd_handle h, const float *y, const float *dout, int B, int C, int64_t L, float *dy, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!y || !dout || !dy) FD_FAIL(h, FD_ERR_INVALID, "fd_gate_backward: null pointer");
    FD_TRY(check_gate(h, B, C, L, "fd_gate_backward"));
    return run(h, stream, "fd_gate_backward", [&](const fdk::Launch &La) { return fdk::gate_backward(La, y, dout, dy, B, C, L); });
}

// The rest of a training step (fd_kernels_step.hip): the draws, the loss, clip + guard + AdamW.  Partial sums and the optimizer's
// per-step scalars live in the step scratch buffer.
static bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// B rows of L floats that the kernels read 16 bytes per lane
static int check_len4(fd_handle h, int B, int64_t L, const char *who)
{
    FD_TRY(check_batch(h, B, who));
    if (L < 4 || L % 4 != 0 || (int64_t)B * L >= ((int64_t)1 << 36)) FD_FAIL(h, FD_ERR_INVALID, "%s: L=%lld (a multiple of 4)", who, (long long)L);
    return FD_OK;
}

int fd_train_draw(fd_handle h, const float *x0, const float *alpha, int T_train, int B, int64_t L, uint64_t seed, const fd_train_state *state,
                  uint64_t iter_host, float *x_t, float *z, float *steps, void *stream)
{
    const char *who = "fd_train_draw";
    if (!h) return FD_ERR_INVALID;
    if (!x0 || !alpha || !x_t || !z || !steps) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    if (T_train < 1) FD_FAIL(h, FD_ERR_INVALID, "%s: T_train=%d", who, T_train);
    FD_TRY(check_len4(h, B, L, who));
    if (!aligned(x0, 16) || !aligned(x_t, 16) || !aligned(z, 16) || !aligned(state, 8))
        FD_FAIL(h, FD_ERR_INVALID, "%s: x0, x_t and z must be 16-byte aligned, state 8-byte aligned", who);
    return run(h, stream, who, [&](const fdk::Launch &La) { return fdk::train_draw(La, x0, alpha, T_train, B, L, seed, state, iter_host, x_t, z, steps); });
}

// fd_train_collate, and fd_eval_collate (eval: the batch in item order; rank / world neither checked nor read)
static int collate(fd_handle h, const char *who, bool eval, const float *wav_arena, const float *mel_arena, const int64_t *frame_off, int64_t n_items,
                   int hop, int F, int B, uint64_t seed, const fd_train_state *state, uint64_t iter_host, int rank, int world, float *wavs, float *mels,
                   int64_t *picked, void *stream)
{
    if (!h) return FD_ERR_INVALID;
    if (!wav_arena || !mel_arena || !frame_off || !wavs || !mels || !picked) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    FD_TRY(check_batch(h, B, who));
    if (n_items < 1 || n_items > ((int64_t)1 << 28)) FD_FAIL(h, FD_ERR_INVALID, "%s: n_items=%lld (1..2^28)", who, (long long)n_items);
    if (hop < 4 || hop % 4 != 0 || F < 1 || (int64_t)F * hop >= ((int64_t)1 << 31))
        FD_FAIL(h, FD_ERR_INVALID, "%s: hop=%d (a multiple of 4), F=%d", who, hop, F);
    if (!eval && (world < 1 || rank < 0 || rank >= world)) FD_FAIL(h, FD_ERR_INVALID, "%s: rank=%d of world=%d", who, rank, world);
    if (!aligned(wav_arena, 16) || !aligned(wavs, 16) || !aligned(frame_off, 8) || !aligned(picked, 8) || !aligned(state, 8))
        FD_FAIL(h, FD_ERR_INVALID, "%s: wav_arena and wavs must be 16-byte aligned, frame_off, picked and state 8-byte aligned", who);
    return run(h, stream, who, [&](const fdk::Launch &La) {
        return fdk::collate(La, eval, wav_arena, mel_arena, frame_off, n_items, hop, F, B, seed, state, iter_host, rank, world, wavs, mels, picked);
    });
}

int fd_train_collate(fd_handle h, const float *wav_arena, const float *mel_arena, const int64_t *frame_off, int64_t n_items, int hop, int F, int B,
                     uint64_t seed, const fd_train_state *state, uint64_t iter_host, int rank, int world, float *wavs, float *mels,
                     int64_t *picked, void *stream)
{
    return collate(h, "fd_train_collate", false, wav_arena, mel_arena, frame_off, n_items, hop, F, B, seed, state, iter_host, rank, world, wavs, mels,
                   picked, stream);
}

static int check_mse(fd_handle h, int64_t n, const char *who)
{
    if (n < 1 || n >= ((int64_t)1 << 36)) FD_FAIL(h, FD_ERR_INVALID, "%s: n=%lld", who, (long long)n);      // (2^24 workgroups)
    return FD_OK;
}

int fd_mse_forward(fd_handle h, const float *eps, const float *z, int64_t n, float *loss, fd_train_state *state, void *stream)
{
    const char *who = "fd_mse_forward";
    if (!h) return FD_ERR_INVALID;
    if (!eps || !z || !loss || !aligned(state, 8)) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer (or a state that is not 8-byte aligned)", who);
    FD_TRY(check_mse(h, n, who));
    return run_scratch(h, stream, who, h->step_scratch, fdk::step_scratch_floats(fdk::mse_blocks(n)), [&](const fdk::Launch &La, float *scratch) {
        return fdk::mse_forward(La, eps, z, n, loss, state, scratch);
    });
}

int fd_mse_backward(fd_handle h, const float *eps, const float *z, const float *dloss, int64_t n, float *deps, void *stream)
{
    const char *who = "fd_mse_backward";
    if (!h) return FD_ERR_INVALID;
    if (!eps || !z || !dloss || !deps) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    FD_TRY(check_mse(h, n, who));
    return run(h, stream, who, [&](const fdk::Launch &La) { return fdk::mse_backward(La, eps, z, dloss, n, deps); });
}

int fd_adamw_multi(fd_handle h, const fd_adamw_item *items, int n, const fd_adamw_hyper *hyper, fd_train_state *state, void *stream)
{
    const char *who = "fd_adamw_multi";
    if (!h) return FD_ERR_INVALID;
    if (!items || !hyper || !state || !aligned(hyper, 8) || !aligned(state, 8))
        FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer (hyper and state: device memory, 8-byte aligned)", who);
    if (n <= 0 || n > 65536) FD_FAIL(h, FD_ERR_INVALID, "%s: n=%d", who, n);
    for (int i = 0; i < n; ++i) {
        const fd_adamw_item &I = items[i];
        if (I.numel <= 0 || I.numel >= ((int64_t)1 << 32) || !I.p || !I.m || !I.v)
            FD_FAIL(h, FD_ERR_INVALID, "%s: item %d: numel=%lld or a null pointer", who, i, (long long)I.numel);
    }
    if (fdk::adamw_blocks(items, n) > ((int64_t)1 << 24))      // (workgroup indices are int; 2^36 elements is far beyond any model here)
        FD_FAIL(h, FD_ERR_UNSUPPORTED, "%s: more than 2^24 workgroups of %d elements in one call", who, FD_STEP_RUN * 256);
    return run_scratch(h, stream, who, h->step_scratch, fdk::step_scratch_floats(fdk::adamw_blocks(items, n)), [&](const fdk::Launch &La, float *scratch) {
        return fdk::adamw_multi(La, items, n, hyper, state, scratch);
    });
}

int fd_ema_multi(fd_handle h, const fd_ema_item *items, int n, const fd_ema_hyper *hyper, const fd_train_state *state, fd_ema_state *ema,
                 void *stream)
{
    const char *who = "fd_ema_multi";
    if (!h) return FD_ERR_INVALID;
    if (!items || !hyper || !state || !ema || !aligned(hyper, 8) || !aligned(state, 8) || !aligned(ema, 8))
        FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer (hyper, state and ema: device memory, 8-byte aligned)", who);
    if (n <= 0 || n > 65536) FD_FAIL(h, FD_ERR_INVALID, "%s: n=%d", who, n);
    for (int i = 0; i < n; ++i) {
        const fd_ema_item &I = items[i];
        if (I.numel <= 0 || I.numel >= ((int64_t)1 << 32) || !I.p || !I.e || !aligned(I.p, 4) || !aligned(I.e, 4))
            FD_FAIL(h, FD_ERR_INVALID, "%s: item %d: numel=%lld, a null pointer or one that is not 4-byte aligned", who, i, (long long)I.numel);
    }
    return run(h, stream, who, [&](const fdk::Launch &La) { return fdk::ema_multi(La, items, n, hyper, state, ema); });
}

// An evaluation pass (fd_kernels_step.hip): the batch in item order, per-item distances, accumulators in device memory.
int fd_eval_collate(fd_handle h, const float *wav_arena, const float *mel_arena, const int64_t *frame_off, int64_t n_items, int hop, int F, int B,
                    uint64_t seed, const fd_train_state *state, uint64_t iter_host, float *wavs, float *mels, int64_t *picked, void *stream)
{
    return collate(h, "fd_eval_collate", true, wav_arena, mel_arena, frame_off, n_items, hop, F, B, seed, state, iter_host, 0, 1, wavs, mels, picked, stream);
}

int fd_item_distance(fd_handle h, const float *a, const float *b, int B, int64_t n, int kind, float *out, void *stream)
{
    const char *who = "fd_item_distance";
    if (!h) return FD_ERR_INVALID;
    if (!a || !b || !out) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    FD_TRY(check_batch(h, B, who));
    if (n < 1 || (int64_t)B * n >= ((int64_t)1 << 36) || (kind != 0 && kind != 1))
        FD_FAIL(h, FD_ERR_INVALID, "%s: n=%lld, kind=%d (0 squared, 1 absolute)", who, (long long)n, kind);
    if (!aligned(a, 16) || !aligned(b, 16)) FD_FAIL(h, FD_ERR_INVALID, "%s: a and b must be 16-byte aligned", who);
    const size_t floats = fdk::step_scratch_floats((int64_t)B * fdk::item_distance_blocks(n));
    return run_scratch(h, stream, who, h->step_scratch, floats, [&](const fdk::Launch &La, float *scratch) {
        return fdk::item_distance(La, a, b, B, n, kind, out, scratch);
    });
}

int fd_eval_accumulate(fd_handle h, const float *values, const float *steps, const int64_t *picked, int B, int T_train, int bins,
                       fd_eval_state *acc, float *item_out, fd_train_state *advance, void *stream)
{
    const char *who = "fd_eval_accumulate";
    if (!h) return FD_ERR_INVALID;
    if (!values || !picked || !acc) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    FD_TRY(check_batch(h, B, who));
    if (bins < 1 || bins > FD_EVAL_MAX_BINS || T_train < 1)
        FD_FAIL(h, FD_ERR_INVALID, "%s: bins=%d (1..%d), T_train=%d", who, bins, FD_EVAL_MAX_BINS, T_train);
    if (!aligned(picked, 8) || !aligned(acc, 8) || !aligned(advance, 8))
        FD_FAIL(h, FD_ERR_INVALID, "%s: picked, acc and advance must be 8-byte aligned", who);
    return run(h, stream, who, [&](const fdk::Launch &La) {
        return fdk::eval_accumulate(La, values, steps, picked, B, T_train, bins, acc, item_out, advance);
    });
}

// The scheduling network, the pieces of its training step and the schedule search (fd_kernels_phi.hip).
static int check_npred(fd_handle h, int B, int R, const char *who)
{
    FD_TRY(check_batch(h, B, who));
    if (R != B && R != 1) FD_FAIL(h, FD_ERR_INVALID, "%s: R=%d (B=%d or 1)", who, R, B);
    return FD_OK;
}

static int check_bandpool(fd_handle h, const float *x, int B, int64_t L, const char *who)
{
    FD_TRY(check_batch(h, B, who));
    if (L < 64 || L % 32 != 0 || L >= ((int64_t)1 << 31)) FD_FAIL(h, FD_ERR_INVALID, "%s: L=%lld (a multiple of 32, at least 64)", who, (long long)L);
    if (!aligned(x, 16)) FD_FAIL(h, FD_ERR_INVALID, "%s: x must be 16-byte aligned", who);
    return FD_OK;
}

int fd_bandpool_forward(fd_handle h, const float *x, const float *W, const float *b, int B, int64_t L, float *feat, void *stream)
{
    const char *who = "fd_bandpool_forward";
    if (!h) return FD_ERR_INVALID;
    if (!x || !W || !b || !feat) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    FD_TRY(check_bandpool(h, x, B, L, who));
    return run_scratch(h, stream, who, h->step_scratch, fdk::bandpool_scratch_floats(B, L, false), [&](const fdk::Launch &La, float *scratch) {
        return fdk::bandpool_forward(La, x, W, b, B, L, feat, scratch);
    });
}

int fd_bandpool_backward(fd_handle h, const float *x, const float *W, const float *b, const float *dfeat, int B, int64_t L, float *dW, float *db,
                         void *stream)
{
    const char *who = "fd_bandpool_backward";
    if (!h) return FD_ERR_INVALID;
    if (!x || !W || !b || !dfeat || !dW || !db) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    FD_TRY(check_bandpool(h, x, B, L, who));
    return run_scratch(h, stream, who, h->step_scratch, fdk::bandpool_scratch_floats(B, L, true), [&](const fdk::Launch &La, float *scratch) {
        return fdk::bandpool_backward(La, x, W, b, dfeat, B, L, dW, db, scratch);
    });
}

int fd_npred_head_forward(fd_handle h, const float *feat, const float *beta_next, const float *delta2, int R, const float *W1, const float *b1,
                          const float *W2, const float *b2, int B, float *beta_hat, float *ratio, void *stream)
{
    const char *who = "fd_npred_head_forward";
    if (!h) return FD_ERR_INVALID;
    if (!feat || !beta_next || !delta2 || !W1 || !b1 || !W2 || !b2 || !beta_hat || !ratio) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    FD_TRY(check_npred(h, B, R, who));
    return run(h, stream, who, [&](const fdk::Launch &La) { return fdk::npred_head_forward(La, feat, beta_next, delta2, R, W1, b1, W2, b2, B, beta_hat, ratio); });
}

int fd_npred_head_backward(fd_handle h, const float *feat, const float *beta_next, const float *delta2, const float *W1, const float *b1,
                           const float *W2, const float *b2, const float *dbeta_hat, int B, float *dW1, float *db1, float *dW2, float *db2,
                           float *dfeat, void *stream)
{
    const char *who = "fd_npred_head_backward";
    if (!h) return FD_ERR_INVALID;
    if (!feat || !beta_next || !delta2 || !W1 || !b1 || !W2 || !b2 || !dbeta_hat || !dW1 || !db1 || !dW2 || !db2 || !dfeat)
        FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    FD_TRY(check_batch(h, B, who));
    return run(h, stream, who, [&](const fdk::Launch &La) {
        return fdk::npred_head_backward(La, feat, beta_next, delta2, W1, b1, W2, b2, dbeta_hat, B, dW1, db1, dW2, db2, dfeat);
    });
}

int fd_phi_draw(fd_handle h, const float *x0, const float *alpha, int T_train, int tau, int B, int64_t L, uint64_t seed, const fd_train_state *state,
                uint64_t iter_host, float *x_t, float *z, float *steps, float *beta_nxt, float *delta, float *delta2, void *stream)
{
    const char *who = "fd_phi_draw";
    if (!h) return FD_ERR_INVALID;
    if (!x0 || !alpha || !x_t || !z || !steps || !beta_nxt || !delta || !delta2) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    if (tau < 0 || T_train < 1 || (int64_t)T_train <= 2 * (int64_t)tau) FD_FAIL(h, FD_ERR_INVALID, "%s: T_train=%d must exceed 2 tau=%d", who, T_train, 2 * tau);
    FD_TRY(check_len4(h, B, L, who));
    if (!aligned(x0, 16) || !aligned(x_t, 16) || !aligned(z, 16) || !aligned(state, 8))
        FD_FAIL(h, FD_ERR_INVALID, "%s: x0, x_t and z must be 16-byte aligned, state 8-byte aligned", who);
    return run(h, stream, who, [&](const fdk::Launch &La) {
        return fdk::phi_draw(La, x0, alpha, T_train, tau, B, L, seed, state, iter_host, x_t, z, steps, beta_nxt, delta, delta2);
    });
}

int fd_phi_residual_forward(fd_handle h, const float *eps, const float *z, const float *delta, const float *beta_hat, int B, int64_t L, float *m,
                            float *s, void *stream)
{
    const char *who = "fd_phi_residual_forward";
    if (!h) return FD_ERR_INVALID;
    if (!eps || !z || !delta || !beta_hat || !m || !s) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    FD_TRY(check_len4(h, B, L, who));
    if (!aligned(eps, 16) || !aligned(z, 16)) FD_FAIL(h, FD_ERR_INVALID, "%s: eps and z must be 16-byte aligned", who);
    return run_scratch(h, stream, who, h->step_scratch, 2 * (size_t)B * (size_t)fdk::phi_residual_blocks(L), [&](const fdk::Launch &La, float *scratch) {
        return fdk::phi_residual_forward(La, eps, z, delta, beta_hat, B, L, m, s, scratch);
    });
}

int fd_sched_init(fd_handle h, fd_sched_state *state, float betaN, float alphaN, void *stream)
{
    const char *who = "fd_sched_init";
    if (!h) return FD_ERR_INVALID;
    if (!state || !aligned(state, 4)) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    return run(h, stream, who, [&](const fdk::Launch &La) { return fdk::sched_init(La, state, betaN, alphaN); });
}

int fd_sched_begin(fd_handle h, fd_sched_state *state, const float *beta_hat, int n_hat, double rho, const float *alpha, int T_train, int ddim,
                   float *steps_out, int B, void *stream)
{
    const char *who = "fd_sched_begin";
    if (!h) return FD_ERR_INVALID;
    if (!state || !alpha || !steps_out) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    FD_TRY(check_batch(h, B, who));
    if (T_train < 1 || (beta_hat && n_hat < 1)) FD_FAIL(h, FD_ERR_INVALID, "%s: T_train=%d, n_hat=%d", who, T_train, n_hat);
    return run(h, stream, who, [&](const fdk::Launch &La) { return fdk::sched_begin(La, state, beta_hat, n_hat, rho, alpha, T_train, ddim ? 1 : 0, steps_out, B); });
}

int fd_sched_update(fd_handle h, fd_sched_state *state, float *x, const float *eps, int64_t n, float *cond_out, void *stream)
{
    const char *who = "fd_sched_update";
    if (!h) return FD_ERR_INVALID;
    if (!state || !x || !eps || !cond_out) FD_FAIL(h, FD_ERR_INVALID, "%s: null pointer", who);
    if (n < 4 || n % 4 != 0 || n >= ((int64_t)1 << 36) || !aligned(x, 16) || !aligned(eps, 16))
        FD_FAIL(h, FD_ERR_INVALID, "%s: n=%lld (a multiple of 4), x and eps 16-byte aligned", who, (long long)n);
    return run(h, stream, who, [&](const fdk::Launch &La) { return fdk::sched_update(La, state, x, eps, n, cond_out); });
}

}  // extern "C"
