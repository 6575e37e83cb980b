"""The location-variable convolution as a differentiable operator on the MI355X.

`location_variable_convolution(x, kernel, bias, dilation, hop_size)` has the signature, tensor layouts and assert of
`TimeAware_LVCBlock.location_variable_convolution` (modules/FastDiff/module/modules.py:220-253); forward and backward run as HIP
kernels behind the C ABI (fd_lvc_forward / fd_lvc_backward, include/fastdiff_hip.h), everything around it stays on PyTorch autograd.
Binding it in the reference is one line:

    TimeAware_LVCBlock.location_variable_convolution = lambda self, x, k, b, d, h: fastdiff_amd.location_variable_convolution(x, k, b, d, h)

which puts the twelve LVC calls of every training forward/backward (theta_timestep_loss, util.py:291-325) on these kernels.
There is no CPU path: CPU tensors raise.
"""
import ctypes as ct

import threading

import torch

from . import _capi

_handles = {}
_handles_lock = threading.Lock()


def _handle(device):
    """One library handle per device: it supplies the device, the error text and the scratch buffers the backward kernels sum their
    partial results in (grown with hipFree + hipMalloc on first use of a larger shape).  Consequence, as for any handle of the library:
    the operators of this module must be ordered on ONE stream per device -- what torch.autograd does for a forward and its backward --
    and their first call at a larger shape is refused inside a graph capture (warm up before capturing).  Two models
    training concurrently on one device from different threads or streams need a process each."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _handles:
        with _handles_lock:
            if idx not in _handles:
                lib = _capi.load()
                cfg = _capi.FdConfig()
                lib.fd_default_config(ct.byref(cfg))
                h = ct.c_void_p()
                _capi.check(lib, None, lib.fd_create(ct.byref(cfg), idx, ct.byref(h)), "fd_create")
                _handles[idx] = h
    return _capi.load(), _handles[idx]


def _stream(device):
    return ct.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptrs(ts):
    """A ctypes array of the tensors' device pointers (None -> NULL): the host-side pointer lists of the *_multi entry points."""
    return (ct.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _arg(a):
    if isinstance(a, torch.Tensor):
        return a.data_ptr()
    if isinstance(a, (list, tuple)):
        return _ptrs(a)
    return a      # None (NULL), or a number


def _call(dev, fn, label, *args):
    """lib.<fn>(handle, *args, stream) on the handle and the current stream of `dev`, its status checked under `label`: a tensor goes in
    as its device pointer, a list of tensors as a _ptrs() array, None as NULL."""
    lib, h = _handle(dev)
    return _capi.check(lib, h, getattr(lib, fn)(h, *[_arg(a) for a in args], _stream(dev)), label)


def _f32(*ts):
    """The inputs as contiguous float32 tensors (what the kernels read; None stays None)."""
    return [None if t is None else t.contiguous().float() for t in ts]


def _cast_back(ctx, *grads):
    """The gradients in the types of the inputs they belong to (ctx.in_dtypes), as autograd requires; None stays None."""
    return tuple(None if g is None else g.to(t) for g, t in zip(grads, ctx.in_dtypes))


def _flat(pairs):
    """[a_1, b_1, a_2, b_2, ...] of the pairs (a_i, b_i): how the operators over many convolutions take their tensors (*args of apply)."""
    return [t for pair in pairs for t in pair]


def _out_grads(gout, shape, dev):
    """The gradients of a node's outputs as contiguous float32 tensors; an output that took no part in the loss (None): zeros, one
    tensor of `shape` shared by all of them."""
    zero = torch.zeros(shape, device=dev, dtype=torch.float32) if any(t is None for t in gout) else None
    return [(zero if t is None else t).contiguous().float() for t in gout]


def _batch_strided(k):
    """True if k [B, Cin, Cout, ks, T] is contiguous apart from its batch stride (one layer's slice of a [B, layers, ...] tensor)."""
    _, ci, co, ks, T = k.shape
    return k.stride()[1:] == (co * ks * T, ks * T, T, 1) and k.stride(0) >= ci * co * ks * T


class _LVC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, bias, hop_size, grad_slot=None):
        if not (x.is_cuda and kernel.is_cuda and bias.is_cuda):
            raise RuntimeError("fastdiff_amd.location_variable_convolution runs only on a HIP device (no CPU fallback)")
        # the kernels compute in float32 (the reference trains in float32); other floating types are converted on the way in and
        # the gradients go back in each input's own type, as autograd requires
        ctx.in_dtypes = (x.dtype, kernel.dtype, bias.dtype)
        # split_layers (below) hands out slices of the predictor's [B, layers, ...] output and a slot for the gradient of each
        ctx.grad_slot = grad_slot
        B, Cin, L = x.shape
        _, _, Cout, ks, T = kernel.shape
        model_shape = (Cin, Cout, ks) == (32, 64, 3) and int(hop_size) in (8, 64, 256)
        x, bias = _f32(x, bias)
        # a layer's slice stays where it lies, and its gradient may go into the shared slot, only for the shape whose kernels take a
        # batch stride (fd_lvc_*_strided: the model's own); every other shape runs on a contiguous copy and owns its gradient
        ctx.strided_ok = kernel.dtype == torch.float32 and model_shape and _batch_strided(kernel)
        if not ctx.strided_ok:
            kernel = kernel.contiguous().float()
        out = torch.empty((B, Cout, L), device=x.device, dtype=torch.float32)
        _call(x.device, "fd_lvc_forward_strided", "fd_lvc_forward", x, kernel, kernel.stride(0), bias, B, Cin, Cout, ks, T, int(hop_size), out)
        ctx.save_for_backward(x, kernel)
        ctx.hop = int(hop_size)
        return out.to(ctx.in_dtypes[0])

    @staticmethod
    def backward(ctx, dout):
        x, kernel = ctx.saved_tensors
        dout = dout.contiguous().float()
        B, Cin, L = x.shape
        _, _, Cout, ks, T = kernel.shape
        need_x, need_k, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dx = torch.empty_like(x) if need_x else None
        dk = None
        if need_k:
            slot = ctx.grad_slot
            if slot is not None and ctx.strided_ok:      # this layer's slice of the shared gradient buffer
                holder, i, shape = slot
                if holder.get("buf") is None:
                    holder["buf"] = torch.empty(shape, device=x.device, dtype=torch.float32)
                dk = holder["buf"][:, i]
            else:
                dk = torch.empty(kernel.shape, device=x.device, dtype=torch.float32)
        db = torch.empty((B, Cout, T), device=x.device, dtype=torch.float32) if need_b else None
        _call(x.device, "fd_lvc_backward_strided", "fd_lvc_backward", x, kernel, kernel.stride(0), dout, B, Cin, Cout, ks, T, ctx.hop, dx, dk,
              0 if dk is None else dk.stride(0), db)
        return _cast_back(ctx, dx, dk, db) + (None, None)


class _SplitLayers(torch.autograd.Function):
    """kernels [B, layers, Cin, Cout, ks, T] -> the `layers` slices kernels[:, i] (what the reference takes with `kernels[:, i, ...]`,
    modules.py:213-214), without a copy either way: the location-variable convolution reads a slice where it lies (batch-strided) and
    writes that layer's gradient into its slice of ONE buffer of the whole shape, which is then this node's gradient as it stands.
    (torch's own unbind / select give contiguous copies to the operator and stack the four gradients: 0.5 ms per training step.)"""

    @staticmethod
    def forward(ctx, k, holder):
        ctx.holder = holder
        return tuple(k[:, i] for i in range(k.shape[1]))

    @staticmethod
    def backward(ctx, *grads):
        buf = ctx.holder.get("buf")
        ctx.holder["buf"] = None
        if buf is not None and all(g is not None and g.data_ptr() == buf[:, i].data_ptr() and g.stride() == buf[:, i].stride() and g.dtype == buf.dtype
                                   for i, g in enumerate(grads)):
            return buf, None
        ref = next(g for g in grads if g is not None)
        return torch.stack([g if g is not None else torch.zeros_like(ref) for g in grads], 1), None


def split_layers(kernels):
    """(slices, slots): the per-layer slices kernels[:, i] of the predictor's kernels [B, layers, Cin, Cout, ks, T] and, for each, the
    `grad_slot` to hand to location_variable_convolution together with it."""
    holder = {"buf": None}
    slices = _SplitLayers.apply(kernels, holder)
    return slices, tuple((holder, i, tuple(kernels.shape)) for i in range(kernels.shape[1]))


class _Gate(torch.autograd.Function):
    """out = x + sigmoid(y[:, :C]) * tanh(y[:, C:]) (modules.py:217), one HIP pass forward (fd_gate_forward) and one backward."""

    @staticmethod
    def forward(ctx, x, y):
        if not (x.is_cuda and y.is_cuda):
            raise RuntimeError("fastdiff_amd.gated_residual runs only on a HIP device (no CPU fallback)")
        ctx.in_dtypes = (x.dtype, y.dtype)
        x, y = _f32(x, y)
        B, C, L = x.shape
        assert tuple(y.shape) == (B, 2 * C, L), "gate: y must hold the sigmoid half and the tanh half of every channel of x"
        out = torch.empty_like(x)
        _call(x.device, "fd_gate_forward", "fd_gate_forward", x, y, B, C, L, out)
        ctx.save_for_backward(y)
        return out.to(ctx.in_dtypes[0])

    @staticmethod
    def backward(ctx, dout):
        (y,) = ctx.saved_tensors
        dy = None
        if ctx.needs_input_grad[1]:
            g = dout.contiguous().float()
            B, C2, L = y.shape
            dy = torch.empty_like(y)
            _call(y.device, "fd_gate_backward", "fd_gate_backward", y, g, B, C2 // 2, L, dy)
            dy = dy.to(ctx.in_dtypes[1])
        return (dout if ctx.needs_input_grad[0] else None), dy


def gated_residual(x, y):
    """x + sigmoid(y[:, :C]) * tanh(y[:, C:]) for x [B, C, L], y [B, 2C, L]: the last line of an LVC layer (modules.py:217) as one
    differentiable operator."""
    return _Gate.apply(x, y)


class _KConv(torch.autograd.Function):
    """KernelPredictor.kernel_conv (modules.py:315-318,330-331: Conv1d(64 -> M, k3, pad 1)) forward and backward on fp32-MFMA HIP
    kernels (fd_kconv_forward / fd_kconv_backward), the reference's layouts.  post_slope != 1 (M <= 512): the LeakyReLU the predictor
    puts behind its small convolutions (modules.py:296-314) inside the same launches (fd_kconv_forward_act / fd_kconv_backward_act)."""

    @staticmethod
    def forward(ctx, x, weight, bias, post_slope=1.0):
        ctx.in_dtypes = (x.dtype, weight.dtype, bias.dtype)
        x, weight, bias = _f32(x, weight, bias)
        B, _, T = x.shape
        M = weight.shape[0]
        out = torch.empty((B, M, T), device=x.device, dtype=torch.float32)
        _call(x.device, "fd_kconv_forward_act", "fd_kconv_forward", x, weight, bias, B, M, T, float(post_slope), out)
        ctx.post = float(post_slope)
        if ctx.post != 1.0:
            ctx.save_for_backward(x, weight, out)
        else:
            ctx.save_for_backward(x, weight)
        return out.to(ctx.in_dtypes[0])

    @staticmethod
    def backward(ctx, dout):
        x, weight = ctx.saved_tensors[:2]
        y = ctx.saved_tensors[2] if ctx.post != 1.0 else None
        dout = dout.contiguous().float()
        B, _, T = x.shape
        M = weight.shape[0]
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        dx = torch.empty_like(x) if need_x else None
        dw = torch.empty_like(weight) if need_w else None
        db = torch.empty((M,), device=x.device, dtype=torch.float32) if need_b else None
        _call(x.device, "fd_kconv_backward_act", "fd_kconv_backward", x, weight, y, dout, B, M, T, ctx.post, 1.0, dx, dw, db)
        return _cast_back(ctx, dx, dw, db) + (None,)


class _SkipFan(torch.autograd.Function):
    """A skip tensor's fan-out (FastDiff_model.py:91-98): returns (x[..., ::factor] for the DiffusionDBlock below, whose nearest
    F.interpolate picks exactly those columns (modules.py:128-131), and four aliases of x for the four layers of the LVC block that
    adds it as audio_down).  Backward: the five gradients in one pass (fd_fan_backward) instead of autograd's zero-fill + strided
    scatter + four full-size additions."""

    @staticmethod
    def forward(ctx, x, factor):
        assert x.dtype == torch.float32 and x.dim() == 3 and x.shape[-1] % int(factor) == 0
        x = x.contiguous()
        B, C, L = x.shape
        picked = torch.empty((B, C, L // int(factor)), device=x.device, dtype=torch.float32)
        _call(x.device, "fd_fan_forward", "fd_fan_forward", x, B * C, L, int(factor), picked)
        ctx.factor, ctx.shape = int(factor), (B, C, L)
        return (picked,) + tuple(x.view_as(x) for _ in range(4))

    @staticmethod
    def backward(ctx, gp, *gs):
        B, C, L = ctx.shape
        ref = next((g for g in (gp,) + gs if g is not None), None)
        if ref is None:
            return None, None
        dx = torch.empty((B, C, L), device=ref.device, dtype=torch.float32)
        _call(ref.device, "fd_fan_backward", "fd_fan_backward", *_f32(*gs, gp), B * C, L, ctx.factor, dx)
        return dx, None


def skip_fan_supported(x, factor):
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[-1] % int(factor) == 0 and x.shape[0] * x.shape[1] <= 65535


def skip_fan(x, factor):
    """(x[..., ::factor], x, x, x, x) for a skip tensor x [B, C, L]: the picked columns for the DBlock below and one alias of x per
    layer of the LVC block that adds it; the gradients of all five come back through one kernel."""
    return _SkipFan.apply(x, factor)


class _InputConv(torch.autograd.Function):
    """KernelPredictor.input_conv (modules.py:292-295): leaky_relu(Conv1d(80 -> 64, k5, padding 2), slope), forward and backward on HIP
    kernels (fd_input_conv_forward / fd_input_conv_backward)."""

    @staticmethod
    def forward(ctx, x, weight, bias, post_slope):
        ctx.in_dtypes = (x.dtype, weight.dtype, bias.dtype)
        x, weight, bias = _f32(x, weight, bias)
        B, _, T = x.shape
        y = torch.empty((B, 64, T), device=x.device, dtype=torch.float32)
        _call(x.device, "fd_input_conv_forward", "fd_input_conv_forward", x, weight, bias, B, T, float(post_slope), y)
        ctx.post = float(post_slope)
        ctx.save_for_backward(x, weight, y)
        return y.to(ctx.in_dtypes[0])

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        dy = dy.contiguous().float()
        B, _, T = x.shape
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        dx = torch.empty_like(x) if need_x else None
        dw = torch.empty_like(weight) if need_w else None
        db = torch.empty(64, device=x.device, dtype=torch.float32) if need_b else None
        _call(x.device, "fd_input_conv_backward", "fd_input_conv_backward", x, weight, y, dy, B, T, ctx.post, dx, dw, db)
        return _cast_back(ctx, dx, dw, db) + (None,)


def input_conv_supported(x, weight):
    """The predictor's input convolution as the model builds it: weight [64, 80, 5] on a HIP tensor [B, 80, T], T <= 128."""
    return x.is_cuda and x.dim() == 3 and x.shape[1] == 80 and tuple(weight.shape) == (64, 80, 5) and 1 <= x.shape[2] <= 128


def input_conv(x, weight, bias, post_slope=0.1):
    """leaky_relu(conv1d(x [B,80,T], weight [64,80,5], bias, padding=2), post_slope) as a differentiable HIP operator."""
    return _InputConv.apply(x, weight, bias, post_slope)


class _KConvStack(torch.autograd.Function):
    """A chain of `Conv1d(64, 64, 3, padding 1), LeakyReLU(slope)` pairs -- the predictor's residual stack (modules.py:297-314) -- as ONE
    autograd node: n forward launches with the activation in the store; in the backward the gradient that a pair hands down is
    multiplied by the mask of the pair below as it is written (fd_kconv_backward_act: in_slope), so only the top pair's two
    latency-bound launches read an activation mask.  Inputs: x [B, 64, T], then weight_1, bias_1, ..., weight_n, bias_n."""

    @staticmethod
    def forward(ctx, x, slope, *params):
        n = len(params) // 2
        ctx.in_dtype = x.dtype
        ctx.slope, ctx.n = float(slope), n
        hs = _f32(x)
        ws = _f32(*params[0::2])
        B, _, T = hs[0].shape
        for j in range(n):
            out = torch.empty((B, 64, T), device=x.device, dtype=torch.float32)
            _call(x.device, "fd_kconv_forward_act", "fd_kconv_forward", hs[-1], ws[j], params[2 * j + 1].contiguous().float(), B, 64, T, ctx.slope, out)
            hs.append(out)
        ctx.save_for_backward(*hs, *ws)
        return hs[-1].to(ctx.in_dtype)

    @staticmethod
    def backward(ctx, dout):
        n = ctx.n
        hs, ws = ctx.saved_tensors[:n + 1], ctx.saved_tensors[n + 1:]
        B, _, T = hs[0].shape
        g = dout.contiguous().float()
        gs = [None] * n
        # the dx chain first: pair j's gradient in front of its activation (the top pair masks dout with its own output, every other
        # pair receives it masked from the pair above) ...
        for j in range(n - 1, -1, -1):
            top, bottom = j == n - 1, j == 0
            gs[j] = g
            if bottom and not ctx.needs_input_grad[0]:
                g = None
                break
            dx = torch.empty_like(hs[j])
            _call(dout.device, "fd_kconv_backward_act", "fd_kconv_backward", hs[j], ws[j], hs[j + 1] if top else None, g, B, 64, T,
                  ctx.slope if top else 1.0, 1.0 if bottom else ctx.slope, dx, None, None)
            g = dx
        # ... then the weight and bias gradients of all pairs in two launches
        want = [j for j in range(n) if ctx.needs_input_grad[2 + 2 * j] or ctx.needs_input_grad[3 + 2 * j]]
        grads = [None] * (2 * n)
        for c0 in range(0, len(want), 8):
            js = want[c0:c0 + 8]
            dws = [torch.empty_like(ws[j]) if ctx.needs_input_grad[2 + 2 * j] else None for j in js]
            dbs = [torch.empty(64, device=gs[0].device, dtype=torch.float32) if ctx.needs_input_grad[3 + 2 * j] else None for j in js]
            _call(dout.device, "fd_kconv_backward_w_multi", "fd_kconv_backward_w_multi", len(js), [hs[j] for j in js], [gs[j] for j in js],
                  [hs[j + 1] if j == n - 1 else None for j in js], B, 64, T, ctx.slope, dws, dbs)
            for j, dw, db in zip(js, dws, dbs):
                grads[2 * j], grads[2 * j + 1] = dw, db
        return (None if g is None else g.to(ctx.in_dtype), None) + tuple(grads)


class _PredictorFronts(torch.autograd.Function):
    """The front ends of P KernelPredictors side by side (modules.py:292-314,328-329): for each, c = leaky_relu(input_conv(x)),
    r = residual stack(c) (n pairs of Conv1d(64, 64, 3) + LeakyReLU), output c + r.  The P chains are independent and each launch of one
    is latency-bound (B workgroups); here every step of the chain is ONE launch for all P (fd_*_multi: the pointers of the P
    convolutions as kernel arguments), forward and backward.  Inputs: slope, n, x_1 .. x_P, then per predictor w_in, b_in, w_1, b_1,
    ..., w_n, b_n.  Same kernels as input_conv / kernel_conv_stack: same bits."""

    @staticmethod
    def forward(ctx, slope, n, *args):
        P = len(args) // (2 * n + 3)
        xs = _f32(*args[:P])
        par = _f32(*args[P:])
        per = 2 * n + 2
        win, bin_ = [par[p * per] for p in range(P)], [par[p * per + 1] for p in range(P)]
        ws = [[par[p * per + 2 + 2 * j] for p in range(P)] for j in range(n)]
        bs = [[par[p * per + 3 + 2 * j] for p in range(P)] for j in range(n)]
        B, _, T = xs[0].shape
        dev = xs[0].device
        H = [torch.empty((P, B, 64, T), device=dev, dtype=torch.float32) for _ in range(n + 1)]      # H[0] = c, H[j] = output of pair j
        _call(dev, "fd_input_conv_forward_multi", "fd_input_conv_forward_multi", P, xs, win, bin_, B, T, float(slope), H[0].unbind(0))
        for j in range(n):
            _call(dev, "fd_kconv_forward_act_multi", "fd_kconv_forward_act_multi", P, H[j].unbind(0), ws[j], bs[j], B, 64, T, float(slope),
                  H[j + 1].unbind(0))
        out = H[0] + H[n]
        ctx.save_for_backward(*xs, *win, *[w for wj in ws for w in wj], *H)
        ctx.slope, ctx.n, ctx.P = float(slope), n, P
        return tuple(out.unbind(0))

    @staticmethod
    def backward(ctx, *gout):
        n, P, slope = ctx.n, ctx.P, ctx.slope
        sv = ctx.saved_tensors
        xs, win = sv[:P], sv[P:2 * P]
        ws = [sv[2 * P + j * P:2 * P + (j + 1) * P] for j in range(n)]
        H = sv[2 * P + n * P:]
        B, _, T = xs[0].shape
        dev = xs[0].device
        gtop = g = _out_grads(gout, (B, 64, T), dev)
        gs = [None] * n            # gs[j]: the gradients in front of pair j's activation (P tensors); the top pair's is masked in the kernels
        cur = g
        for j in range(n - 1, -1, -1):
            top, bottom = j == n - 1, j == 0
            gs[j] = cur
            DX = torch.empty((P, B, 64, T), device=dev, dtype=torch.float32)
            _call(dev, "fd_kconv_backward_x_multi", "fd_kconv_backward_x_multi", P, H[j].unbind(0), ws[j], H[n].unbind(0) if top else None, cur, B, 64, T,
                  slope if top else 1.0, 1.0 if bottom else slope, DX.unbind(0))
            cur = list(DX.unbind(0))
        # weight and bias gradients of all P * n pairs, eight per call
        flat = [(p, j) for p in range(P) for j in range(n)]
        dW = {k: torch.empty_like(ws[k[1]][k[0]]) for k in flat}
        dB = {k: torch.empty(64, device=dev, dtype=torch.float32) for k in flat}
        for c0 in range(0, len(flat), 8):
            ks = flat[c0:c0 + 8]
            _call(dev, "fd_kconv_backward_w_multi", "fd_kconv_backward_w_multi", len(ks), [H[j][p] for p, j in ks], [gs[j][p] for p, j in ks],
                  [H[n][p] if j == n - 1 else None for p, j in ks], B, 64, T, slope, [dW[k] for k in ks], [dB[k] for k in ks])
        # c has two readers, the stack and the sum: dc = dx of the bottom pair + the output's gradient
        torch._foreach_add_(cur, gtop)
        need_x = any(ctx.needs_input_grad[2:2 + P])
        DXin = torch.empty((P, B, 80, T), device=dev, dtype=torch.float32) if need_x else None
        dwin = [torch.empty_like(w) for w in win]
        dbin = [torch.empty(64, device=dev, dtype=torch.float32) for _ in range(P)]
        _call(dev, "fd_input_conv_backward_multi", "fd_input_conv_backward_multi", P, xs, win, H[0].unbind(0), cur, B, T, slope,
              None if DXin is None else DXin.unbind(0), dwin, dbin)
        grads = [None, None] + ([None] * P if DXin is None else list(DXin.unbind(0)))
        for p in range(P):
            grads += [dwin[p], dbin[p]]
            for j in range(n):
                grads += [dW[(p, j)], dB[(p, j)]]
        return tuple(grads)


def predictor_fronts(xs, input_convs, stacks, slope):
    """[leaky_relu(input_conv_p(x_p)) + stack_p(.) for p] for P predictors at once: xs = P tensors [B, 80, T]; input_convs = P pairs
    (weight [64, 80, 5], bias); stacks = P lists of n pairs (weight [64, 64, 3], bias); one launch per chain step for all P."""
    n = len(stacks[0])
    return list(_PredictorFronts.apply(slope, n, *xs, *_flat(pair for ic, st in zip(input_convs, stacks) for pair in (ic, *st))))


class _KConvSide(torch.autograd.Function):
    """P independent small convolutions of one shape -- conv1d(x_p [B,64,T], w_p [M,64,3], b_p, padding 1), M <= 512: the three
    predictors' bias_conv -- with one launch per kernel for all P (fd_kconv_forward_act_multi, fd_kconv_backward_x_multi,
    fd_kconv_backward_w_multi).  Inputs: x_1 .. x_P, w_1, b_1, ..., w_P, b_P."""

    @staticmethod
    def forward(ctx, *args):
        P = len(args) // 3
        xs, ws, bs = _f32(*args[:P]), _f32(*args[P::2]), _f32(*args[P + 1::2])
        B, _, T = xs[0].shape
        M = ws[0].shape[0]
        dev = xs[0].device
        out = torch.empty((P, B, M, T), device=dev, dtype=torch.float32)
        _call(dev, "fd_kconv_forward_act_multi", "fd_kconv_forward_act_multi", P, xs, ws, bs, B, M, T, 1.0, out.unbind(0))
        ctx.save_for_backward(*xs, *ws)
        ctx.P = P
        return tuple(out.unbind(0))

    @staticmethod
    def backward(ctx, *gout):
        P = ctx.P
        xs, ws = ctx.saved_tensors[:P], ctx.saved_tensors[P:]
        B, _, T = xs[0].shape
        M = ws[0].shape[0]
        dev = xs[0].device
        g = _out_grads(gout, (B, M, T), dev)
        DX = torch.empty((P, B, 64, T), device=dev, dtype=torch.float32) if any(ctx.needs_input_grad[:P]) else None
        if DX is not None:
            _call(dev, "fd_kconv_backward_x_multi", "fd_kconv_backward_x_multi", P, None, ws, None, g, B, M, T, 1.0, 1.0, DX.unbind(0))
        dws = [torch.empty_like(w) for w in ws]
        dbs = [torch.empty(M, device=dev, dtype=torch.float32) for _ in range(P)]
        _call(dev, "fd_kconv_backward_w_multi", "fd_kconv_backward_w_multi", P, xs, g, None, B, M, T, 1.0, dws, dbs)
        grads = [None] * P if DX is None else list(DX.unbind(0))
        for dw, db in zip(dws, dbs):
            grads += [dw, db]
        return tuple(grads)


def kernel_conv1d_side_by_side(xs, weights, biases):
    """[conv1d(x_p, w_p, b_p, padding=1) for p] for P <= 8 inputs [B, 64, T] and weights [M, 64, 3] of one shape (M <= 512), one launch
    per kernel for all P."""
    return list(_KConvSide.apply(*xs, *_flat(zip(weights, biases))))


def kernel_conv_stack(x, weights, biases, slope):
    """leaky_relu(conv1d(., w_j, b_j, padding=1), slope) applied n times in a row to x [B, 64, T] (every w_j [64, 64, 3]) as one
    differentiable HIP operator: the predictor's residual stack without its Dropout(p = 0) modules."""
    return _KConvStack.apply(x, slope, *_flat(zip(weights, biases)))


class _Conv7(torch.autograd.Function):
    """first_audio_conv (which = 0: Conv1d(1, 32, 7, padding 3)) / final_conv (which = 1: Conv1d(32, 1, 7, padding 3)), FastDiff_model.py:
    34-36,67-68, forward and backward on HIP kernels (fd_conv7_forward / fd_conv7_backward)."""

    @staticmethod
    def forward(ctx, x, weight, bias, which):
        ctx.in_dtypes = (x.dtype, weight.dtype, bias.dtype)
        x, weight, bias = _f32(x, weight, bias)
        B, _, L = x.shape
        y = torch.empty((B, 32 if which == 0 else 1, L), device=x.device, dtype=torch.float32)
        _call(x.device, "fd_conv7_forward", "fd_conv7_forward", int(which), x, weight, bias, B, L, y)
        ctx.save_for_backward(x, weight)
        ctx.which = int(which)
        return y.to(ctx.in_dtypes[0])

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous().float()
        B, _, L = x.shape
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        dx = torch.empty_like(x) if need_x else None
        dw = torch.empty_like(weight) if need_w else None
        db = torch.empty(32 if ctx.which == 0 else 1, device=x.device, dtype=torch.float32) if need_b else None
        _call(x.device, "fd_conv7_backward", "fd_conv7_backward", ctx.which, x, weight, dy, B, L, dx, dw, db)
        return _cast_back(ctx, dx, dw, db) + (None,)


def conv7_supported(x, weight):
    """first_audio_conv ([32,1,7] on [B,1,L]) or final_conv ([1,32,7] on [B,32,L]) on a HIP tensor whose length is a multiple of 4."""
    return (x.is_cuda and x.dim() == 3 and x.shape[2] % 4 == 0 and 4 <= x.shape[2] < (1 << 25) and
            ((tuple(weight.shape) == (32, 1, 7) and x.shape[1] == 1) or (tuple(weight.shape) == (1, 32, 7) and x.shape[1] == 32)))


def conv7(x, weight, bias):
    """conv1d(x, weight, bias, padding=3) for the model's first_audio_conv / final_conv as a differentiable HIP operator."""
    return _Conv7.apply(x, weight, bias, 0 if weight.shape[0] == 32 else 1)


class _Upsample(torch.autograd.Function):
    """`upsample(F.leaky_relu(x, 0.2))` of an LVC block (modules.py:163-166,205-206): activation + ConvTranspose1d(32, 32, 2 r, stride r,
    padding r / 2) forward and backward on HIP kernels (fd_upsample_forward / fd_upsample_backward)."""

    @staticmethod
    def forward(ctx, x, weight, bias, ratio):
        ctx.in_dtypes = (x.dtype, weight.dtype, bias.dtype)
        x, weight, bias = _f32(x, weight, bias)
        B, _, Lin = x.shape
        y = torch.empty((B, 32, Lin * int(ratio)), device=x.device, dtype=torch.float32)
        _call(x.device, "fd_upsample_forward", "fd_upsample_forward", x, weight, bias, B, Lin, int(ratio), y)
        ctx.save_for_backward(x, weight)
        ctx.ratio = int(ratio)
        return y.to(ctx.in_dtypes[0])

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous().float()
        B, _, Lin = x.shape
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        dx = torch.empty_like(x) if need_x else None
        dw = torch.empty_like(weight) if need_w else None
        db = torch.empty(32, device=x.device, dtype=torch.float32) if need_b else None
        _call(x.device, "fd_upsample_backward", "fd_upsample_backward", x, weight, dy, B, Lin, ctx.ratio, dx, dw, db)
        return _cast_back(ctx, dx, dw, db) + (None,)


def upsample_supported(x, m):
    """An LVC block's up-sampler as the model builds it: ConvTranspose1d(32, 32, 2 r, stride r, padding r / 2), r = 4 or 8, on a HIP tensor."""
    r = m.stride[0]
    return (x.is_cuda and x.dim() == 3 and x.shape[1] == 32 and isinstance(m, torch.nn.ConvTranspose1d) and r in (4, 8) and
            tuple(m.weight.shape) == (32, 32, 2 * r) and m.padding == (r // 2,) and m.output_padding == (0,) and m.dilation == (1,))


def upsample(x, weight, bias, ratio):
    """conv_transpose1d(leaky_relu(x, 0.2), weight, bias, stride=ratio, padding=ratio // 2) for weight [32, 32, 2 * ratio] as a
    differentiable HIP operator."""
    return _Upsample.apply(x, weight, bias, ratio)


class _WeightNorm(torch.autograd.Function):
    """w = torch._weight_norm(v, g, 0) (what torch.nn.utils.weight_norm's hook evaluates on every forward, FastDiff_model.py:115-122)
    as one HIP launch forward (fd_weight_norm_forward) and one backward (fd_weight_norm_backward)."""

    @staticmethod
    def forward(ctx, v, g):
        v, g = v.contiguous(), g.contiguous()
        rows, cols = v.shape[0], v.numel() // v.shape[0]
        w = torch.empty_like(v)
        norm = torch.empty(rows, device=v.device, dtype=torch.float32)
        _call(v.device, "fd_weight_norm_forward", "fd_weight_norm_forward", v, g, rows, cols, w, norm)
        ctx.save_for_backward(v, g, norm)
        return w

    @staticmethod
    def backward(ctx, dw):
        v, g, norm = ctx.saved_tensors
        dw = dw.contiguous().float()
        rows, cols = v.shape[0], v.numel() // v.shape[0]
        dv, dg = torch.empty_like(v), torch.empty_like(g)
        _call(v.device, "fd_weight_norm_backward", "fd_weight_norm_backward", v, g, norm, dw, rows, cols, dv, dg)
        return dv, dg


def weight_norm(v, g):
    """torch._weight_norm(v, g, 0) for float32 HIP tensors (g of shape [out, 1, ...]) as a differentiable HIP operator; anything else
    goes to torch."""
    if v.is_cuda and v.dtype == torch.float32 and g.dtype == torch.float32 and g.numel() == v.shape[0]:
        return _WeightNorm.apply(v, g)
    return torch._weight_norm(v, g, 0)


class _WeightNormAll(torch.autograd.Function):
    """w_i = torch._weight_norm(v_i, g_i, 0) for ALL weight-normed convolutions of the module in one or two launches each way
    (fd_weight_norm_multi_forward / _backward; inputs v_1, g_1, v_2, g_2, ...).  The w_i are views of one flat buffer, and so are the
    gradients dv_i / dg_i (which become the parameters' .grad).  The host work per call is a few vectorised numpy statements and two
    torch.split calls: in eager mode this operator sits at the very end of the backward, where nothing hides it."""

    @staticmethod
    def forward(ctx, *vg):
        import numpy as np
        n = len(vg) // 2
        vs, gs = [t.contiguous() for t in vg[0::2]], [t.contiguous() for t in vg[1::2]]
        dev = vs[0].device
        rows = np.array([v.shape[0] for v in vs], dtype=np.int64)
        numel = np.array([v.numel() for v in vs], dtype=np.int64)
        ow, on = np.concatenate(([0], np.cumsum(numel)[:-1])), np.concatenate(([0], np.cumsum(rows)[:-1]))
        W = torch.empty(int(numel.sum()), device=dev, dtype=torch.float32)
        N = torch.empty(int(rows.sum()), device=dev, dtype=torch.float32)
        tab = np.zeros(n, dtype=_capi.record("fd_wn_item"))
        tab["v"] = [v.data_ptr() for v in vs]
        tab["g"] = [g.data_ptr() for g in gs]
        tab["w"] = W.data_ptr() + 4 * ow
        tab["norm"] = N.data_ptr() + 4 * on
        tab["rows"] = rows
        tab["cols"] = numel // rows
        _call(dev, "fd_weight_norm_multi_forward", "fd_weight_norm_multi_forward", tab.ctypes.data, n)
        ctx.save_for_backward(N, *vs, *gs)
        ctx.tab, ctx.ow, ctx.on, ctx.sizes = tab, ow, on, (numel.tolist(), rows.tolist())
        return tuple(w.view(v.shape) for w, v in zip(W.split(ctx.sizes[0]), vs))

    @staticmethod
    def backward(ctx, *dws):
        n = len(dws)
        N, vs, gs = ctx.saved_tensors[0], ctx.saved_tensors[1:1 + n], ctx.saved_tensors[1 + n:]
        dev = N.device
        DV = torch.empty(sum(ctx.sizes[0]), device=dev, dtype=torch.float32)
        DG = torch.empty(sum(ctx.sizes[1]), device=dev, dtype=torch.float32)
        dws = [None if d is None else d.contiguous().float() for d in dws]      # (kept alive until the launch is enqueued)
        tab = ctx.tab.copy()
        tab["dw"] = [0 if d is None else d.data_ptr() for d in dws]
        tab["dv"] = DV.data_ptr() + 4 * ctx.ow
        tab["dg"] = DG.data_ptr() + 4 * ctx.on
        _call(dev, "fd_weight_norm_multi_backward", "fd_weight_norm_multi_backward", tab.ctypes.data, n)
        out = []
        for dv, dg, v, g in zip(DV.split(ctx.sizes[0]), DG.split(ctx.sizes[1]), vs, gs):
            out.append(dv.view(v.shape))
            out.append(dg.view(g.shape))
        return tuple(out)


def weight_norm_all(pairs):
    """[torch._weight_norm(v, g, 0) for (v, g) in pairs] for float32 HIP tensors, all in one differentiable operator (one or two
    launches each way whatever the number of tensors)."""
    return list(_WeightNormAll.apply(*_flat(pairs)))


class _Conv32(torch.autograd.Function):
    """xs = x (+ skip); y = post(bias + conv1d(pre(xs), weight, dilation, padding = dilation)) -- one of the denoiser's 21 small
    convolutions with everything the reference wraps around it (modules.py:136-137 and 209-212), forward in one HIP pass
    (fd_conv32_forward) and backward in one pass plus a fixed-order reduction of the weight / bias gradients (fd_conv32_backward)."""

    @staticmethod
    def forward(ctx, x, skip, weight, bias, dilation, pre_slope, post_slope):
        ctx.in_dtypes = (x.dtype, None if skip is None else skip.dtype, weight.dtype, bias.dtype)
        x, skip, weight, bias = _f32(x, skip, weight, bias)
        B, _, L = x.shape
        y = torch.empty_like(x)
        xs = x if skip is None else torch.empty_like(x)
        _call(x.device, "fd_conv32_forward", "fd_conv32_forward", x, skip, weight, bias, B, L, int(dilation), float(pre_slope), float(post_slope),
              None if skip is None else xs, y)
        ctx.save_for_backward(xs, y, weight)
        ctx.cfg = (int(dilation), float(pre_slope), float(post_slope), skip is not None)
        ctx.set_materialize_grads(False)                 # an output nobody differentiates arrives as None, not as a tensor of zeros
        if skip is None:
            return y.to(ctx.in_dtypes[0])
        return xs.to(ctx.in_dtypes[0]), y.to(ctx.in_dtypes[0])

    @staticmethod
    def backward(ctx, *grads):
        xs, y, weight = ctx.saved_tensors
        dilation, pre, post, has_skip = ctx.cfg
        gxs, gy = (grads if has_skip else (None, grads[0]))
        B, _, L = xs.shape
        need_x = ctx.needs_input_grad[0] or (has_skip and ctx.needs_input_grad[1])
        need_w, need_b = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        if gy is None:                                   # y had no reader: only the pass-through of xs is left
            d = gxs
            dw = torch.zeros_like(weight) if need_w else None
            db = torch.zeros(32, device=xs.device) if need_b else None
        else:
            gy, gxs = _f32(gy, gxs)
            d = torch.empty_like(xs) if need_x else None
            dw = torch.empty_like(weight) if need_w else None
            db = torch.empty(32, device=xs.device, dtype=torch.float32) if need_b else None
            _call(xs.device, "fd_conv32_backward", "fd_conv32_backward", xs, y, weight, gy, gxs, B, L, dilation, pre, post, d, dw, db)
        dx = d if ctx.needs_input_grad[0] else None
        ds = d if has_skip and ctx.needs_input_grad[1] else None
        return _cast_back(ctx, dx, ds, dw, db) + (None, None, None)


def conv32_supported(x, weight, dilation):
    """The shapes the HIP operator covers: 32 -> 32 channels, kernel 3, dilation 1 / 2 / 3 / 4 / 9 / 27 (every small convolution of
    the model), a length that is a multiple of 4."""
    return (x.is_cuda and x.dim() == 3 and x.shape[1] == 32 and tuple(weight.shape) == (32, 32, 3) and int(dilation) in (1, 2, 3, 4, 9, 27)
            and x.shape[2] % 4 == 0 and 4 <= x.shape[2] < (1 << 25))


def conv32(x, weight, bias, dilation, skip=None, pre_slope=0.2, post_slope=1.0):
    """One small convolution of the denoiser as the reference applies it, as a differentiable HIP operator:
        xs = x + skip (when a skip is given);   y = leaky_relu_post(bias + conv1d(leaky_relu_pre(xs), weight, dilation=d, padding=d))
    with slope 1.0 = no activation.  DiffusionDBlock: conv32(x, w, b, d) (modules.py:136-137); TimeAware_LVCBlock layer i:
    xs, y = conv32(x, w, b, 3 ** i, skip=audio_down, post_slope=0.2) (modules.py:209-212).  Returns y, or (xs, y) with a skip.
    weight is the folded weight (torch._weight_norm of the module's weight_v / weight_g under weight-norm)."""
    return _Conv32.apply(x, skip, weight, bias, dilation, pre_slope, post_slope)


def kernel_conv_supported(x, weight):
    """The shapes the HIP kernels cover: 64 input channels, kernel 3, a multiple of 32 output channels (kernel_conv 24576, bias_conv
    256, the predictor's residual convolutions 64), at most 128 frames (the reference trains on crops of 100: base.yaml:50-51)."""
    return (x.is_cuda and x.dim() == 3 and weight.dim() == 3 and x.shape[1] == 64 and tuple(weight.shape[1:]) == (64, 3)
            and weight.shape[0] % 32 == 0 and 1 <= x.shape[2] <= 128)


def kernel_conv1d(x, weight, bias, post_slope=1.0):
    """leaky_relu(conv1d(x [B,64,T], weight [M,64,3], bias [M], padding=1), post_slope) -> [B,M,T] as a differentiable HIP operator
    (the predictor's kernel_conv, and with post_slope = 0.1 and M = 64 its residual convolutions with their activation); shapes outside
    kernel_conv_supported(), or an activation on M > 512, are refused by the library (FD_ERR_UNSUPPORTED)."""
    return _KConv.apply(x, weight, bias, post_slope)


def lvc_operator_supported(in_channels, out_channels, kernel_size):
    """The shapes fd_lvc_forward / fd_lvc_backward have kernels for (fd_api.cpp: check_lvc_op): the coefficient block of a frame fits
    the operator's staging (Cin * Cout * ks <= 8192, Cout <= 256) -- with ks = 3 that is inner_channels <= 36."""
    return in_channels * out_channels * kernel_size <= 8192 and out_channels <= 256 and kernel_size % 2 == 1


def _lvc_torch(x, kernel, bias, hop_size):
    """out[b, o, l * hop + s] = bias[b, o, l] + sum_{i, k} xpad[b, i, l * hop + s + k] * kernel[b, i, o, k, l] (modules.py:220-253 with
    dilation 1) on torch ops, differentiable by autograd: for the configurations the constructor accepts but the HIP operator has no
    kernel for (a frame's coefficient block beyond its staging: inner_channels > 36) -- a correctness path, like fd_generic.hip's."""
    B, Cin, L = x.shape
    _, _, Cout, ks, T = kernel.shape
    pad = (ks - 1) // 2
    win = torch.nn.functional.pad(x, (pad, pad)).unfold(2, hop_size + 2 * pad, hop_size).unfold(3, ks, 1)      # [B, Cin, T, hop, ks]
    out = torch.einsum("bilsk,biokl->bols", win, kernel) + bias.unsqueeze(-1)
    return out.reshape(B, Cout, L)


def location_variable_convolution(x, kernel, bias, dilation=1, hop_size=256, grad_slot=None):
    """(batch, in_channels, in_length), (batch, in_channels, out_channels, kernel_size, kernel_length), (batch, out_channels,
    kernel_length) -> (batch, out_channels, in_length); same assert as the reference (modules.py:236).  dilation must be 1: it is
    the only value the model ever passes (modules.py:216).  grad_slot (train.py only): see split_layers.
    Shapes outside the HIP operator's limits (lvc_operator_supported) run on torch ops (_lvc_torch) -- still on the device, still
    differentiable; a shared gradient slot is then not used (autograd owns the gradient of that layer's slice)."""
    batch, in_channels, in_length = x.shape
    batch, in_channels, out_channels, kernel_size, kernel_length = kernel.shape
    assert in_length == (kernel_length * hop_size), "length of (x, kernel) is not matched"
    if dilation != 1:
        raise NotImplementedError("location_variable_convolution: the HIP operator implements dilation = 1 (modules.py:216)")
    if not lvc_operator_supported(in_channels, out_channels, kernel_size):
        if not x.is_cuda:
            raise RuntimeError("fastdiff_amd.location_variable_convolution runs only on a HIP device (no CPU fallback)")
        return _lvc_torch(x, kernel, bias, int(hop_size))
    return _LVC.apply(x, kernel, bias, hop_size, grad_slot)


# ---- "frames": kernel_conv and the operator joined through frame-major tensors (include/fastdiff_hip.h: fd_kconv_*_frames, fd_lvc_*_frames) ----

FRAME = 32 * 64 * 3      # coefficients per frame of the model's operator


def frame_order(order):
    """LongTensor [6144]: position e of a frame -> row (i * 64 + o) * 3 + k of the reference's [32, 64, 3] coefficient block, for
    order = "forward" (the frames kernel_conv writes: the operator's forward operand order) or "grad" (the frames of the gradient: its
    dK accumulator order).  The Python statement of csrc/fd_frame_order.h: row_of, for tests and inspection."""
    e = torch.arange(FRAME)
    j, lane, grp = e & 3, (e >> 2) & 63, e >> 8
    l31, hi = lane & 31, lane >> 5
    if order == "forward":
        mt, sq = grp // 12, grp % 12
        kidx = 2 * (4 * sq + j) + hi
        o, k, i = 32 * mt + l31, kidx >> 5, kidx & 31
    elif order == "grad":
        g, t6 = grp & 3, grp >> 2
        mt = t6 // 3
        k, o, i = t6 - 3 * mt, 32 * mt + 8 * g + 4 * hi + j, l31
    else:
        raise ValueError("frame_order: order must be 'forward' or 'grad'")
    return (i * 64 + o) * 3 + k


def frames_to_reference(frames, order="forward"):
    """frames [B, layers, T, 6144] -> the reference's kernels [B, layers, 32, 64, 3, T] (modules.py:333-338)."""
    B, nl, T, _ = frames.shape
    out = torch.empty((B, nl, FRAME, T), device=frames.device, dtype=frames.dtype)
    out[:, :, frame_order(order).to(frames.device)] = frames.transpose(2, 3)
    return out.view(B, nl, 32, 64, 3, T)


def reference_to_frames(kernels, order="forward"):
    """the reference's kernels [B, layers, 32, 64, 3, T] -> frames [B, layers, T, 6144]."""
    B, nl = kernels.shape[:2]
    T = kernels.shape[-1]
    return kernels.reshape(B, nl, FRAME, T)[:, :, frame_order(order).to(kernels.device)].transpose(2, 3).contiguous()


class _KConvFrames(torch.autograd.Function):
    """kernel_conv writing the LVC operator's frames directly (fd_kconv_forward_frames) and reading the gradient as frames
    (fd_kconv_backward_frames): out [B, M / 6144, T, 6144]."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.in_dtypes = (x.dtype, weight.dtype, bias.dtype)
        x, weight, bias = _f32(x, weight, bias)
        B, _, T = x.shape
        M = weight.shape[0]
        out = torch.empty((B, M // FRAME, T, FRAME), device=x.device, dtype=torch.float32)
        _call(x.device, "fd_kconv_forward_frames", "fd_kconv_forward_frames", x, weight, bias, B, M, T, out)
        ctx.save_for_backward(x, weight)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight = ctx.saved_tensors
        dout = dout.contiguous().float()
        B, _, T = x.shape
        M = weight.shape[0]
        need_x, need_w, need_b = ctx.needs_input_grad
        dx = torch.empty_like(x) if need_x else None
        dw = torch.empty_like(weight) if need_w else None
        db = torch.empty((M,), device=x.device, dtype=torch.float32) if need_b else None
        _call(x.device, "fd_kconv_backward_frames", "fd_kconv_backward_frames", x, weight, dout, B, M, T, dx, dw, db)
        return _cast_back(ctx, dx, dw, db)


def kernel_conv_frames_supported(x, weight):
    """kernel_conv_supported() and a whole number of the operator's layers in the output channels (kernel_conv: 4 x 6144)."""
    return kernel_conv_supported(x, weight) and weight.shape[0] % FRAME == 0 and x.dtype == weight.dtype == torch.float32


def kernel_conv1d_frames(x, weight, bias):
    """The predictor's kernel_conv with its result as frames [B, layers, T, 6144] (frames_to_reference() gives the reference's tensor)."""
    return _KConvFrames.apply(x, weight, bias)


class _LVCFrames(torch.autograd.Function):
    """The location-variable convolution on one layer's frames: kernel [B, T, 6144] = frames[:, i] of kernel_conv1d_frames and bias
    [B, 64, T] = bias_conv's output [:, i] (both batch-strided, used where they lie); their gradients are written into the layer's
    slices of the shared buffers of split_layers (grad_slot, bias_slot).
    INVARIANT of the frames pair: the gradient this node returns for `kernel` is in the operator's GRADIENT element order, not the
    forward tensor's, and _KConvFrames.backward (fd_kconv_backward_frames) is its only legal consumer -- the frames tensor is an
    internal edge between kernel_conv1d_frames and this node, created and consumed inside train._kernel_predictor / _lvc_block.  Do not
    attach hooks, retain_grad or a second reader to it, and do not ask torch.autograd.grad for it: take
    lvc_op.frames_to_reference(frames) (a real tensor in the reference's layout, with an ordinary gradient) for anything of that kind."""

    @staticmethod
    def forward(ctx, x, kernel, bias, hop_size, grad_slot, bias_slot):
        if not (x.is_cuda and kernel.is_cuda and bias.is_cuda):
            raise RuntimeError("fastdiff_amd.location_variable_convolution_frames runs only on a HIP device (no CPU fallback)")
        ctx.in_dtypes = (x.dtype, bias.dtype)
        ctx.grad_slot, ctx.bias_slot = grad_slot, bias_slot
        B, _, L = x.shape
        T = kernel.shape[1]
        # (the stride of a dimension of size 1 means nothing and torch reports what it likes there)
        assert kernel.dtype == torch.float32 and tuple(kernel.shape) == (B, T, FRAME) and kernel.stride(2) == 1 and \
            (T == 1 or kernel.stride(1) == FRAME) and (B == 1 or kernel.stride(0) >= T * FRAME), "frames [B, T, 6144]"
        assert L == T * int(hop_size), "length of (x, kernel) is not matched"
        ctx.kbs = kernel.stride(0) if B > 1 else T * FRAME
        x = x.contiguous().float()
        # a layer's slice of bias_conv's [B, layers, 64, T] output is read where it lies
        if not (bias.dtype == torch.float32 and tuple(bias.shape) == (B, 64, T) and (T == 1 or bias.stride(2) == 1) and bias.stride(1) == T and
                (B == 1 or bias.stride(0) >= 64 * T)):
            bias = bias.contiguous().float()
        bbs = bias.stride(0) if B > 1 else 64 * T
        out = torch.empty((B, 64, L), device=x.device, dtype=torch.float32)
        _call(x.device, "fd_lvc_forward_frames", "fd_lvc_forward_frames", x, kernel, ctx.kbs, bias, bbs, B, T, int(hop_size), out)
        ctx.save_for_backward(x, kernel)
        ctx.hop = int(hop_size)
        return out.to(ctx.in_dtypes[0])

    @staticmethod
    def backward(ctx, dout):
        x, kernel = ctx.saved_tensors
        dout = dout.contiguous().float()
        B, _, L = x.shape
        T = kernel.shape[1]
        need_x, need_k, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dx = torch.empty_like(x) if need_x else None

        def slot_or_new(slot, shape):      # this layer's slice of a shared gradient buffer (split_layers), or a tensor of its own
            if slot is None:
                return torch.empty(shape, device=x.device, dtype=torch.float32)
            holder, i, full = slot
            if holder.get("buf") is None:
                holder["buf"] = torch.empty(full, device=x.device, dtype=torch.float32)
            return holder["buf"][:, i]

        dk = slot_or_new(ctx.grad_slot, (B, T, FRAME)) if need_k else None
        db = slot_or_new(ctx.bias_slot if ctx.in_dtypes[1] == torch.float32 else None, (B, 64, T)) if need_b else None
        _call(x.device, "fd_lvc_backward_frames", "fd_lvc_backward_frames", x, kernel, ctx.kbs, dout, B, T, ctx.hop, dx, dk,
              0 if dk is None else (dk.stride(0) if B > 1 else T * FRAME), db, 0 if db is None else (db.stride(0) if B > 1 else 64 * T))
        dx, db = _cast_back(ctx, dx, db)
        return dx, dk, db, None, None, None


def location_variable_convolution_frames(x, kernel_frames, bias, hop_size, grad_slot=None, bias_slot=None):
    """location_variable_convolution for x [B, 32, L], one layer's frames [B, T, 6144] (forward order) and bias [B, 64, T]; the gradient
    with respect to the frames comes back in the "grad" order (what kernel_conv1d_frames' backward reads).  grad_slot / bias_slot: the
    slots split_layers hands out with the slices of the frames / of bias_conv's [B, layers, 64, T] output."""
    return _LVCFrames.apply(x, kernel_frames, bias, hop_size, grad_slot, bias_slot)


# ---------------------------------------------------------------------------------------------------------------------------------
# The rest of a training step (include/fastdiff_hip_train.h, last section): the draws, the loss, clip + guard + AdamW
# ---------------------------------------------------------------------------------------------------------------------------------
TS_STREAM, Z_STREAM = 0xFFFFFFFD, 0xFFFFFFFE      # the Philox streams of a training step's ts and z


AdamWHyper = _capi.struct("fd_adamw_hyper")


def new_state(name, device, dtype=torch.int64):
    """A zeroed C struct `name` (include/fastdiff_hip_train.h) in device memory, as whole words of `dtype`."""
    return torch.zeros(_capi.record(name).itemsize // dtype.itemsize, dtype=dtype, device=device)


def pack_state(name, dtype=torch.int64, **values):
    """The C struct `name` with `values` in the fields they name and zero elsewhere, as a host tensor of `dtype` words: what a state
    tensor's copy_ takes."""
    import numpy as np
    r = np.zeros(1, _capi.record(name))
    for k, v in values.items():
        r[k] = v
    return torch.from_numpy(r.view(np.uint8)).view(dtype)


def state_field(t, name, field):
    """The one-element view, in the field's own type, of scalar `field` of the C struct `name` that the state tensor `t` holds."""
    ftype, offset = _capi.record(name).fields[field][:2]
    return t.view(getattr(torch, ftype.name))[offset // ftype.itemsize:][:1]


def _is_state(t, name, dtype=torch.int64):
    return t.dtype == dtype and t.is_contiguous() and t.numel() * t.element_size() == _capi.record(name).itemsize


def _read_state(t, name):
    """The tensor's bytes on the host as the one record `name`, read by field name (synchronises)."""
    return t.cpu().numpy().view(_capi.record(name))[0]


def new_train_state(device):
    """A zeroed fd_train_state in device memory, as int64 words."""
    return new_state("fd_train_state", device)


def read_train_state(state):
    """fd_train_state -> dict (synchronises)."""
    r = _read_state(state, "fd_train_state")
    return {"iter": int(r["iter"]), "applied": int(r["applied"]), "skipped": int(r["skipped"]), "grad_norm": float(r["grad_norm"]),
            "loss": float(r["loss"])}


def train_draw(x0, alpha, T_train, seed=0, iteration=0, state=None, out=None):
    """The draws of theta_timestep_loss (util.py:312-318) on the device (fd_train_draw): x0 [B, 1, L] (L a multiple of 4), alpha [T_train]
    on the same device -> (x_t, z, steps [B, 1] float32).  The step index that keys the draws is state's `iter` (read on the device when
    the kernel runs: a captured call draws anew on every replay) or, without a state, `iteration`.  out: (x_t, z, steps) to write into."""
    if not x0.is_cuda:
        raise RuntimeError("fastdiff_amd.lvc_op.train_draw runs only on a HIP device (no CPU fallback)")
    x0, alpha = _f32(x0, alpha)
    B, L = x0.shape[0], x0.numel() // x0.shape[0]
    assert alpha.numel() == int(T_train) and alpha.device == x0.device, "alpha: [T_train] on the device of the audio"
    x_t, z, steps = out if out is not None else (torch.empty_like(x0), torch.empty_like(x0), torch.empty((B, 1), device=x0.device, dtype=torch.float32))
    _call(x0.device, "fd_train_draw", "fd_train_draw", x0, alpha, int(T_train), B, L, int(seed) & 0xFFFFFFFFFFFFFFFF, state,
          int(iteration) & 0xFFFFFFFFFFFFFFFF, x_t, z, steps)
    return x_t, z, steps


def _collate(fn, corpus, batch_size, seed, iteration, state, out, *tail):
    """train_collate and eval_collate: entry point `fn`, whose arguments between the step index and the outputs are `tail`."""
    if not corpus.wav.is_cuda:
        raise RuntimeError(f"fastdiff_amd.lvc_op.{fn[3:]} runs only on a HIP device (no CPU fallback): corpus.to(device) uploads the corpus")
    dev, B, F, hop = corpus.wav.device, int(batch_size), corpus.frames, corpus.hop_size
    if out is None:
        out = (torch.empty((B, 80, F), device=dev, dtype=torch.float32), torch.empty((B, 1, F * hop), device=dev, dtype=torch.float32),
               torch.empty((B, 2), device=dev, dtype=torch.int64))
    mels, wavs, picked = out
    for t, shape, dtype in ((mels, (B, 80, F), torch.float32), (wavs, (B, 1, F * hop), torch.float32), (picked, (B, 2), torch.int64)):
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.device == dev, "out: (mels [B, 80, F], wavs [B, 1, F hop], picked [B, 2] int64)"
    assert state is None or state.device == dev
    _call(dev, fn, fn, corpus.wav, corpus.mel, corpus.frame_off, corpus.n_items, hop, F, B, int(seed) & 0xFFFFFFFFFFFFFFFF, state,
          int(iteration) & 0xFFFFFFFFFFFFFFFF, *tail, wavs, mels, picked)
    return mels, wavs, picked


def train_collate(corpus, batch_size, seed=0, iteration=0, state=None, rank=0, world_size=1, out=None):
    """The batch of a step cut on the device from a corpus.TrainCorpus that lies there (fd_train_collate) -> (mels [B, 80, F], wavs
    [B, 1, F * hop], picked [B, 2] int64 = (item, start frame) per slot; corpus.plan(...) gives the same picks on the host).  The step
    index is state's `iter` (read on the device: a captured call cuts a new batch on every replay) or, without a state, `iteration`;
    rank / world_size: slot b stands at position (it B + b) world_size + rank of the endless item order.  out: (mels, wavs, picked)."""
    return _collate("fd_train_collate", corpus, batch_size, seed, iteration, state, out, int(rank), int(world_size))


class _MSE(torch.autograd.Function):
    """nn.MSELoss() (util.py:307,325) as one fixed-order sum forward (fd_mse_forward) and one pass backward (fd_mse_backward); z is the
    target: it receives no gradient."""

    @staticmethod
    def forward(ctx, eps, z, state):
        ctx.in_dtypes = (eps.dtype,)
        eps, z = _f32(eps, z)
        assert eps.shape == z.shape
        loss = torch.empty((), device=eps.device, dtype=torch.float32)
        _call(eps.device, "fd_mse_forward", "fd_mse_forward", eps, z, eps.numel(), loss, state)
        ctx.save_for_backward(eps, z)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        eps, z = ctx.saved_tensors
        deps = torch.empty_like(eps)
        _call(eps.device, "fd_mse_backward", "fd_mse_backward", eps, z, dloss.contiguous().float(), eps.numel(), deps)
        return _cast_back(ctx, deps) + (None, None)


def mse_loss(eps, z, state=None):
    """mean((eps - z)^2) on the HIP kernels, differentiable in eps; state (a new_train_state tensor) also receives the loss."""
    if not (eps.is_cuda and z.is_cuda):
        raise RuntimeError("fastdiff_amd.lvc_op.mse_loss runs only on a HIP device (no CPU fallback)")
    return _MSE.apply(eps, z, state)


def adamw_multi(items, hyper, state):
    """clip_grad_norm_ + non-finite guard + AdamW.step() over all tensors (fd_adamw_multi).  items: [(p, g or None, m, v)] float32
    contiguous HIP tensors; hyper: a device tensor holding an AdamWHyper; state: a new_train_state tensor."""
    import numpy as np
    tab = np.zeros(len(items), dtype=_capi.record("fd_adamw_item"))
    for i, (p, g, m, v) in enumerate(items):
        assert p.is_contiguous() and m.is_contiguous() and v.is_contiguous() and p.dtype == m.dtype == v.dtype == torch.float32
        assert g is None or (g.is_contiguous() and g.dtype == torch.float32 and g.numel() == p.numel())
        row = tab[i]
        row["p"], row["g"], row["m"], row["v"], row["numel"] = p.data_ptr(), 0 if g is None else g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
    _call(state.device, "fd_adamw_multi", "fd_adamw_multi", tab.ctypes.data, len(items), hyper, state)


def new_ema_state(device):
    """A zeroed fd_ema_state in device memory, as int64 words."""
    return new_state("fd_ema_state", device)


def read_ema_state(ema_state):
    """fd_ema_state -> dict (synchronises)."""
    r = _read_state(ema_state, "fd_ema_state")
    return {"updates": int(r["updates"]), "seen_applied": int(r["seen_applied"]), "w": float(r["w"]), "apply": int(r["apply"])}


def ema_multi(items, hyper, state, ema_state):
    """e += w (p - e) over all tensors, behind adamw_multi on the same stream (fd_ema_multi).  items: [(p, e)] float32 contiguous HIP
    tensors of equal size that do not overlap; hyper: a device tensor of two float64 (fd_ema_hyper: decay, warmup); state: the
    new_train_state tensor the optimizer advances (only read); ema_state: a new_ema_state tensor.  Nothing moves unless the
    optimizer applied a step since the last update.  Does not synchronise."""
    import numpy as np
    dev = ema_state.device
    assert _is_state(hyper, "fd_ema_hyper", torch.float64) and hyper.device == dev, "hyper: an fd_ema_hyper as float64 on the device"
    assert _is_state(state, "fd_train_state") and state.device == dev, "state: a new_train_state tensor on the device"
    assert _is_state(ema_state, "fd_ema_state") and ema_state.is_cuda, "ema_state: a new_ema_state tensor"
    tab = np.zeros(len(items), dtype=_capi.record("fd_ema_item"))
    for i, (p, e) in enumerate(items):
        assert p.is_contiguous() and e.is_contiguous() and p.dtype == e.dtype == torch.float32 and p.numel() == e.numel()
        assert p.device == dev and e.device == dev
        row = tab[i]
        row["p"], row["e"], row["numel"] = p.data_ptr(), e.data_ptr(), p.numel()
    _call(dev, "fd_ema_multi", "fd_ema_multi", tab.ctypes.data, len(items), hyper, state, ema_state)


# ---------------------------------------------------------------------------------------------------------------------------------
# An evaluation pass (include/fastdiff_hip_train.h: fd_eval_collate, fd_item_distance, fd_eval_accumulate; fastdiff_amd/validate.py)
# ---------------------------------------------------------------------------------------------------------------------------------
EVAL_MAX_BINS = _capi.FD_EVAL_MAX_BINS


def new_eval_state(device):
    """A zeroed fd_eval_state in device memory, as int64 words."""
    return new_state("fd_eval_state", device)


def read_eval_state(acc, bins=EVAL_MAX_BINS):
    """fd_eval_state -> {"sum", "count", "nonfinite", "bin_sum" [bins] float64, "bin_count" [bins] int64} (synchronises)."""
    r = _read_state(acc, "fd_eval_state")
    return {"sum": float(r["sum"]), "count": int(r["count"]), "nonfinite": int(r["nonfinite"]), "bin_sum": r["bin_sum"][:bins].copy(),
            "bin_count": r["bin_count"][:bins].astype("int64")}


def eval_collate(corpus, batch_size, seed=0, iteration=0, state=None, out=None):
    """The batch of an evaluation pass cut on the device (fd_eval_collate) -> (mels [B, 80, F], wavs [B, 1, F * hop], picked [B, 2] int64):
    slot b of batch `it` is item it B + b itself; a slot behind the last item is filled from the last item and reported as (-1, -1).
    corpus.eval_plan(it, B, seed) gives the same picks on the host.  The batch index is state's `iter` (read on the device) or, without
    a state, `iteration`.  out: (mels, wavs, picked) to write into."""
    return _collate("fd_eval_collate", corpus, batch_size, seed, iteration, state, out)


def item_distance(a, b, kind=0, out=None):
    """out[i] = mean over item i of (a - b)^2 (kind 0) or |a - b| (kind 1) for a, b [B, ...] (fd_item_distance): fixed-order sums, two
    calls agree bit for bit, an item's value depends on that item's elements alone."""
    if not (a.is_cuda and b.is_cuda):
        raise RuntimeError("fastdiff_amd.lvc_op.item_distance runs only on a HIP device (no CPU fallback)")
    a, b = _f32(a, b)
    assert a.shape == b.shape and a.dim() >= 1 and a.numel() > 0 and kind in (0, 1)
    B = a.shape[0]
    if out is None:
        out = torch.empty(B, device=a.device, dtype=torch.float32)
    assert tuple(out.shape) == (B,) and out.dtype == torch.float32 and out.is_contiguous() and out.device == a.device
    _call(a.device, "fd_item_distance", "fd_item_distance", a, b, B, a.numel() // B, int(kind), out)
    return out


def eval_accumulate(values, picked, acc, steps=None, T_train=1, bins=1, item_out=None, advance=None):
    """Add the values [B] of a batch's active slots (picked [B, 2] from eval_collate) to the fd_eval_state `acc` in slot order
    (fd_eval_accumulate); with steps [B] also to bin (ts bins) // T_train; item_out[item] = value; advance: the pass's train state,
    whose batch index goes up by one behind this call."""
    dev, B = values.device, values.numel()
    for t, n, dtype in ((values, B, torch.float32), (steps, B, torch.float32), (picked, 2 * B, torch.int64), (item_out, None, torch.float32)):
        assert t is None or (t.is_cuda and t.device == dev and t.dtype == dtype and t.is_contiguous() and n in (None, t.numel())), \
            "eval_accumulate: contiguous HIP tensors of one device: values / steps [B] float32, picked [B, 2] int64"
    for t, name in ((acc, "fd_eval_state"), (advance, "fd_train_state")):
        assert t is None or (t.is_cuda and t.device == dev and _is_state(t, name)), f"eval_accumulate: {name} as int64 words on the device of the values"
    _call(dev, "fd_eval_accumulate", "fd_eval_accumulate", values, steps, picked, B, int(T_train), int(bins), acc, item_out, advance)


# ---------------------------------------------------------------------------------------------------------------------------------
# The scheduling network, the pieces of its training step and the schedule search (include/fastdiff_hip_train.h, last section;
# fastdiff_amd/noisepred.py, phistep.py, sampler.noise_scheduling(search="device"))
# ---------------------------------------------------------------------------------------------------------------------------------
PHI_TS_STREAM, PHI_Z_STREAM = 0xFFFFFFFA, 0xFFFFFFF9      # the Philox streams of phi_loss's ts and z


class _BandPool(torch.autograd.Function):
    """feat[b, c] = log(1e-6 + mean_f (bias[c] + sum_k W[c, k] x[b, 32 f + k])^2) (fd_bandpool_forward / _backward); x is data: it
    receives no gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x, weight, bias = _f32(x, weight, bias)
        B, L = x.shape
        assert tuple(weight.shape) == (32, 64) and tuple(bias.shape) == (32,)
        feat = torch.empty((B, 32), device=x.device, dtype=torch.float32)
        _call(x.device, "fd_bandpool_forward", "fd_bandpool_forward", x, weight, bias, B, L, feat)
        ctx.save_for_backward(x, weight, bias)
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        x, weight, bias = ctx.saved_tensors
        dW, db = torch.empty_like(weight), torch.empty_like(bias)
        _call(x.device, "fd_bandpool_backward", "fd_bandpool_backward", x, weight, bias, dfeat.contiguous().float(), x.shape[0], x.shape[1], dW, db)
        return None, dW, db


def band_pool(x, weight, bias):
    """The band energies of NoisePredictor: x [B, L] (L a multiple of 32, >= 64), weight [32, 64], bias [32] -> feat [B, 32]."""
    if not x.is_cuda:
        raise RuntimeError("fastdiff_amd.lvc_op.band_pool runs only on a HIP device (no CPU fallback)")
    assert x.dim() == 2 and x.shape[1] >= 64 and x.shape[1] % 32 == 0, "x [B, L] with L a multiple of 32, at least 64"
    return _BandPool.apply(x, weight, bias)


class _NPredHead(torch.autograd.Function):
    """The 34 -> 64 -> 1 head of NoisePredictor (fd_npred_head_forward / _backward) -> (beta_hat [R], ratio [B]); only beta_hat carries a
    gradient, to feat and the four parameter tensors.  The condition is data."""

    @staticmethod
    def forward(ctx, feat, beta_next, delta2, w1, b1, w2, b2):
        feat, beta_next, delta2, w1, b1, w2, b2 = _f32(feat, beta_next, delta2, w1, b1, w2, b2)
        B, R = feat.shape[0], beta_next.numel()
        assert delta2.numel() == R and R in (1, B) and tuple(w1.shape) == (64, 34) and w2.numel() == 64
        beta_hat = torch.empty(R, device=feat.device, dtype=torch.float32)
        ratio = torch.empty(B, device=feat.device, dtype=torch.float32)
        _call(feat.device, "fd_npred_head_forward", "fd_npred_head_forward", feat, beta_next, delta2, R, w1, b1, w2, b2, B, beta_hat, ratio)
        ctx.save_for_backward(feat, beta_next, delta2, w1, b1, w2, b2)
        ctx.mark_non_differentiable(ratio)
        return beta_hat, ratio

    @staticmethod
    def backward(ctx, dbeta, _dratio):
        feat, beta_next, delta2, w1, b1, w2, b2 = ctx.saved_tensors
        B = feat.shape[0]
        if beta_next.numel() != B:
            raise RuntimeError("NoisePredictor: one condition for a batch of several items (R = 1) is a no_grad form")
        dfeat = torch.empty_like(feat)
        dw1, db1, dw2, db2 = (torch.empty_like(t) for t in (w1, b1, w2, b2))
        _call(feat.device, "fd_npred_head_backward", "fd_npred_head_backward", feat, beta_next, delta2, w1, b1, w2, b2, dbeta.contiguous().float(), B,
              dw1, db1, dw2, db2, dfeat)
        return dfeat, None, None, dw1, db1, dw2, db2


def npred_head(feat, beta_next, delta2, w1, b1, w2, b2):
    if not feat.is_cuda:
        raise RuntimeError("fastdiff_amd.lvc_op.npred_head runs only on a HIP device (no CPU fallback)")
    return _NPredHead.apply(feat, beta_next, delta2, w1, b1, w2, b2)


def phi_draw(x0, alpha, T_train, tau, seed=0, iteration=0, state=None, out=None):
    """The draws of phi_loss (util.py:340-350) on the device (fd_phi_draw): x0 [B, 1, L] -> (x_t, z, steps [B, 1], beta_nxt [B, 1],
    delta [B, 1], delta2 [B, 1]); the step index as in train_draw.  out: the six tensors to write into."""
    if not x0.is_cuda:
        raise RuntimeError("fastdiff_amd.lvc_op.phi_draw runs only on a HIP device (no CPU fallback)")
    x0, alpha = _f32(x0, alpha)
    B, L = x0.shape[0], x0.numel() // x0.shape[0]
    assert alpha.numel() == int(T_train) and alpha.device == x0.device, "alpha: [T_train] on the device of the audio"
    if out is None:
        out = (torch.empty_like(x0), torch.empty_like(x0)) + tuple(torch.empty((B, 1), device=x0.device, dtype=torch.float32) for _ in range(4))
    x_t, z, steps, beta_nxt, delta, delta2 = out
    _call(x0.device, "fd_phi_draw", "fd_phi_draw", x0, alpha, int(T_train), int(tau), B, L, int(seed) & 0xFFFFFFFFFFFFFFFF, state,
          int(iteration) & 0xFFFFFFFFFFFFFFFF, x_t, z, steps, beta_nxt, delta, delta2)
    return x_t, z, steps, beta_nxt, delta, delta2


def phi_draw_plan(seed, it, B, T_train, tau):
    """The host twin of fd_phi_draw's step choice: ts [B] int64, each in [tau, T_train - tau)."""
    import numpy as np
    T_train, tau = int(T_train), int(tau)
    if T_train <= 2 * tau:
        raise ValueError(f"phi_draw_plan: T_train={T_train} must exceed 2 tau={2 * tau}")
    from .corpus import _words
    b = np.arange(int(B), dtype=np.uint64)
    w = np.stack(_words(seed, PHI_TS_STREAM, b >> np.uint64(2), np.uint64(int(it) & 0xFFFFFFFFFFFFFFFF)), axis=-1)[np.arange(int(B)), (b & np.uint64(3)).astype(np.int64)]
    return (tau + ((w * np.uint64(T_train - 2 * tau)) >> np.uint64(32))).astype(np.int64)


class _PhiResidual(torch.autograd.Function):
    """m[b] = mean_t (delta z - (beta_hat / delta) eps)^2 on fixed-order sums (fd_phi_residual_forward); the backward is
    dbeta_hat[b] = dm[b] (-2 / delta[b]) s[b] with s[b] = mean_t r eps from the same pass.  Only beta_hat receives a gradient."""

    @staticmethod
    def forward(ctx, eps, z, delta, beta_hat):
        ctx.hat_shape = beta_hat.shape
        eps, z, delta, beta_hat = _f32(eps, z, delta, beta_hat)
        B = eps.shape[0]
        assert eps.shape == z.shape and delta.numel() == B and beta_hat.numel() == B
        m, s = (torch.empty(B, device=eps.device, dtype=torch.float32) for _ in range(2))
        _call(eps.device, "fd_phi_residual_forward", "fd_phi_residual_forward", eps, z, delta, beta_hat, B, eps.numel() // B, m, s)
        ctx.save_for_backward(delta, s)
        return m

    @staticmethod
    def backward(ctx, dm):
        delta, s = ctx.saved_tensors
        return None, None, None, (dm * (-2.0 / delta.view(-1)) * s).view(ctx.hat_shape)


def phi_residual(eps, z, delta, beta_hat):
    """eps, z [B, 1, L] (L a multiple of 4), delta, beta_hat [B]-like -> m [B]; differentiable in beta_hat."""
    if not (eps.is_cuda and z.is_cuda):
        raise RuntimeError("fastdiff_amd.lvc_op.phi_residual runs only on a HIP device (no CPU fallback)")
    return _PhiResidual.apply(eps, z, delta, beta_hat)


SCHED_MAX_STEPS = _capi.FD_SCHED_MAX_STEPS


def new_sched_state(device, betaN, alphaN):
    """An fd_sched_state in device memory (int32 words), initialised on the device (fd_sched_init)."""
    state = new_state("fd_sched_state", device, torch.int32)
    lib, h = _handle(device)
    _capi.check(lib, h, lib.fd_sched_init(h, state.data_ptr(), float(betaN), float(alphaN), _stream(device)), "fd_sched_init")
    return state


def read_sched_state(state):
    """fd_sched_state -> dict (synchronises: the one read of a search)."""
    r = _read_state(state, "fd_sched_state")
    n = int(r["n_found"])
    return {"alpha_cur": float(r["alpha_cur"]), "beta_cur": float(r["beta_cur"]), "stopped": int(r["stopped"]), "n_found": n,
            "found": r["found"][:n].copy(), "step": float(r["step"])}


def sched_begin(state, beta_hat, rho, alpha, ddim, steps_out):
    dev = state.device
    if beta_hat is not None:
        assert beta_hat.is_cuda and beta_hat.dtype == torch.float32 and beta_hat.is_contiguous() and beta_hat.numel() >= 1
    lib, h = _handle(dev)
    _capi.check(lib, h, lib.fd_sched_begin(h, state.data_ptr(), None if beta_hat is None else beta_hat.data_ptr(),
                                           0 if beta_hat is None else beta_hat.numel(), float(rho), alpha.data_ptr(), alpha.numel(), int(bool(ddim)),
                                           steps_out.data_ptr(), steps_out.numel(), _stream(dev)), "fd_sched_begin")


def sched_update(state, x, eps, cond_out):
    assert x.is_contiguous() and eps.is_contiguous() and x.dtype == eps.dtype == torch.float32 and x.shape == eps.shape
    assert cond_out.numel() == 2 and cond_out.dtype == torch.float32 and cond_out.is_contiguous()
    _call(state.device, "fd_sched_update", "fd_sched_update", state, x, eps, x.numel(), cond_out)
