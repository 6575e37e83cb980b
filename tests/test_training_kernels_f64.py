"""The training step's large matrix products against float64 references that share nothing with the HIP kernels.

kernel_conv with M > 512 (the KernelPredictor's kernel_conv, Conv1d(64 -> 24576, k3, pad 1), modules.py:315-318,330-331) runs on the
large-M kernels of csrc/fd_kernels_kconv.hip: k_kc_fwd, k_kc_dw + k_kc_dw_sum, k_kc_dh + k_kc_dh_fold.  Elsewhere the suite compares
them with each other (frames form vs reference layout) or samples them inside a whole training step; here every element of out, dx,
dW and dbias is compared with an explicit im2col product in float64 (run on the device: rocBLAS DGEMM), at shapes chosen to reach
each range / slice split of the launchers, the idle waves of a last 128-row workgroup and every column-tile edge.  The location-variable
convolution is checked the same way at the training shape (B = 20, T = 100) against oracle/torch_eager.py's unfold + einsum form.

CPU tests pin both references (to F.conv1d and its autograd, to oracle/lvc_grad.py) and show that the comparison helper rejects an
error just above its bar at the positions where these kernels go wrong."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

OUT_BAR, GRAD_BAR = 2e-6, 3e-6      # test_lvc_op.py: test_kernel_conv_operator_forward_and_backward_match_torch_autograd
LVC_BAR = 3e-6                      # test_lvc_op.py: test_matrix_pipe_kernels_against_the_numpy_oracle_at_ragged_sizes
LARGE = {"kconv_forward", "kconv_backward_w", "kconv_backward_w_sum", "kconv_backward_h", "kconv_backward_h_fold"}
SMALL = {"kconv_forward_small", "kconv_backward_w_small"}


# ---- references ---------------------------------------------------------------------------------------------------------------

def _hcol(h):
    """h [B, 64, T] -> Hcol [B, 192, T] with Hcol[b, c * 3 + k, t] = h[b, c, t + k - 1] (zero outside [0, T))."""
    B, C, T = h.shape
    return F.pad(h, (1, 1)).unfold(2, 3, 1).permute(0, 1, 3, 2).reshape(B, 3 * C, T)


def kconv_ref(h, W, bias):
    """conv1d(h, W, bias, padding=1) as W [M, 192] @ Hcol + bias, in the inputs' type (float64 here)."""
    return W.reshape(W.shape[0], -1) @ _hcol(h) + bias[:, None]


def kconv_ref_backward(h, W, dout):
    """(dx, dW, dbias) of kconv_ref for the output gradient dout [B, M, T]."""
    B, C, T = h.shape
    M = W.shape[0]
    hc = _hcol(h)
    dW = torch.einsum("bpt,bkt->pk", dout, hc).reshape(M, C, 3)
    G = F.pad((W.reshape(M, -1).t() @ dout).view(B, C, 3, T), (1, 1))      # G[b, c, k, t + 1] = sum_p W[p, c, k] dout[b, p, t]
    dx = G[:, :, 0, 2:] + G[:, :, 1, 1:-1] + G[:, :, 2, :-2]                 # dx[t] = sum_k G[k, t - k + 1]
    return dx, dW, dout.sum((0, 2))


def lvc_ref(x, K, bias, dout, hop):
    """(out, dx, dK, dbias) of the location-variable convolution in float64: oracle/torch_eager.py's unfold + einsum under autograd."""
    from torch_eager import EagerFastDiff
    x, K, bias = (t.double().requires_grad_(True) for t in (x, K, bias))
    out = EagerFastDiff.lvc(x, K, bias, hop)
    out.backward(dout.double())
    return out.detach(), x.grad, K.grad, bias.grad


def rel_err(got, want):
    """max |got - want| over every element, relative to max(1, max |want|), in float64."""
    want = want.double()
    return float((got.double() - want).abs().max()) / max(1.0, float(want.abs().max()))


def check(name, got, want, bar):
    assert tuple(got.shape) == tuple(want.shape), (name, tuple(got.shape), tuple(want.shape))
    err = rel_err(got, want.to(got.device))
    print(f"  {name}: {err:.2e} (bar {bar:.0e})")
    assert err < bar, (name, err, bar)
    return err


# ---- the launchers' splits (fd_kernels_kconv.hip: pick_ranges, dh_slices), restated to name what a shape reaches -------------------

def _pick_ranges(per_range, units, max_ranges, slots):
    best, best_cost = 1, None
    for n in range(1, min(units, max_ranges) + 1):
        cost = -(-per_range * n // slots) * -(-units // n)
        if best_cost is None or cost < best_cost:
            best, best_cost = n, cost
    return best


def _ranges(units, n):
    chunk = -(-units // n)
    return [min(chunk, units - i) for i in range(0, units, chunk)]


def _dh_slices(M, per_slice, slots):
    chunks, best, nks = M // 32, None, 1
    for k in range(1, min(64, chunks) + 1):
        if chunks % k == 0:
            cost = -(-k * per_slice // slots) * (chunks // k)
            if best is None or cost < best:
                best, nks = cost, k
    return nks


def splits(M, B, slots=512):
    """(utterance ranges of the forward, utterance ranges of dW, row slices of dh) of kernel_conv at M > 512; slots = 2 x CUs."""
    gx = -(-M // 128)
    return _ranges(B, _pick_ranges(gx, B, 16, slots)), _ranges(B, _pick_ranges(gx, B, 8, slots)), _dh_slices(M, B, slots)


# (M, B, T): every branch of the large-M path at slots = 512 (256 CUs); test_the_cases_reach_the_splits_they_are_chosen_for pins it
KCONV_CASES = [(544, 3, 33),        # 1 live wave of 4 in the last workgroup; dh 17 slices of 32 rows; k_kc_dw<false, false>; nct = 2
               (544, 20, 100),      # dW in 7 ranges of 3, the last holds 2; forward in 10 ranges of 2
               (800, 37, 127),      # 1 live wave; forward ranges of 3, the last holds 1; nct = 4, ragged last tile
               (640, 1, 1),         # one frame, both neighbours zero
               (6144, 7, 64),       # k_kc_dw<true, false>; exactly 2 full column tiles
               (24576, 3, 65),      # forward and dW ranges of 2 + 1; one column of the third tile
               (24576, 20, 100),    # the training shape: 5 ranges of 4, dh in 24 slices of 1024 rows
               (24576, 2, 128),     # T at the limit: 4 full tiles, dh in 64 slices
               (544, 2, 2), (800, 3, 3), (640, 2, 5), (6144, 3, 31), (24576, 2, 32)]      # T % 4 and T % 32 next to a boundary


def test_the_cases_reach_the_splits_they_are_chosen_for():
    assert splits(544, 3) == ([1, 1, 1], [1, 1, 1], 17)
    assert splits(544, 20)[:2] == ([2] * 10, [3] * 6 + [2])
    assert splits(800, 37)[0] == [3] * 12 + [1]
    assert splits(24576, 3)[:2] == ([2, 1], [2, 1])
    assert splits(24576, 20) == ([4] * 5, [4] * 5, 24)
    assert splits(24576, 2)[2] == 64
    assert {M % 128 for M, _, _ in KCONV_CASES} == {0, 32}                     # 32: one live wave in the last workgroup
    assert {T % 4 for _, _, T in KCONV_CASES} == {0, 1, 2, 3}
    assert {T % 32 for _, _, T in KCONV_CASES} >= {0, 1, 2, 3, 5, 31}


# ---- CPU: the references are what they claim, and the helper rejects what the bars are there for ---------------------------------

@pytest.mark.parametrize("B,M,T", [(2, 96, 7), (3, 64, 1)])
def test_im2col_reference_equals_conv1d_and_its_autograd(B, M, T):
    g = torch.Generator().manual_seed(B * 100 + T)
    x, w, b = torch.randn(B, 64, T, generator=g, dtype=torch.float64), torch.randn(M, 64, 3, generator=g, dtype=torch.float64), \
        torch.randn(M, generator=g, dtype=torch.float64)
    dout = torch.randn(B, M, T, generator=g, dtype=torch.float64)
    x64, w64, b64 = (t.clone().requires_grad_(True) for t in (x, w, b))
    ref = F.conv1d(x64, w64, b64, padding=1)
    ref.backward(dout)
    assert torch.allclose(kconv_ref(x, w, b), ref.detach(), rtol=0, atol=1e-12)
    for got, want in zip(kconv_ref_backward(x, w, dout), (x64.grad, w64.grad, b64.grad)):
        assert got.shape == want.shape and torch.allclose(got, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("hop", [8, 64, 256])
def test_eager_lvc_reference_equals_the_numpy_oracle(hop):
    import lvc_grad as lg
    rng = np.random.default_rng(hop)
    B, T = 2, 3
    x, K = rng.standard_normal((B, 32, T * hop)), rng.standard_normal((B, 32, 64, 3, T))
    b, d = rng.standard_normal((B, 64, T)), rng.standard_normal((B, 64, T * hop))
    got = lvc_ref(*(torch.from_numpy(a) for a in (x, K, b, d)), hop)
    want = (lg.lvc_forward(x, K, b, hop),) + lg.lvc_backward(x, K, d, hop)
    for name, g_, w_ in zip(("out", "dx", "dK", "dbias"), got, want):
        assert g_.shape == w_.shape and np.abs(g_.numpy() - w_).max() <= 1e-12 * max(1.0, np.abs(w_).max()), name


@pytest.mark.parametrize("which", ["out", "dx", "dW"])
def test_the_bars_reject_one_element_just_beyond_them(which):
    """The float32 image of a float64 reference passes; one element moved by 1.01 x the bar fails -- at the last frame, the last row and
    an utterance of the last range (B = 20, T = 100 with M = 544: the forward in ten ranges of 2)."""
    B, M, T = 20, 544, 100
    g = torch.Generator().manual_seed(7)
    x, w = torch.randn(B, 64, T, generator=g, dtype=torch.float64), torch.randn(M, 64, 3, generator=g, dtype=torch.float64) / 14.0
    bias, dout = torch.randn(M, generator=g, dtype=torch.float64), torch.randn(B, M, T, generator=g, dtype=torch.float64)
    dx, dW, _ = kconv_ref_backward(x, w, dout)
    ref, bar = {"out": (kconv_ref(x, w, bias), OUT_BAR), "dx": (dx, GRAD_BAR), "dW": (dW, GRAD_BAR)}[which]
    b_last = B - splits(M, B)[0][-1]      # first utterance of the forward's last range
    places = {"out": [(0, 5, T - 1), (1, M - 1, 3), (b_last, 100, 50)],
              "dx": [(0, 5, T - 1), (B - 1, 63, 40)],
              "dW": [(M - 1, 63, 2), (M - 1, 0, 0)]}[which]
    good = ref.float()
    check(which, good, ref, bar)
    step = 1.01 * bar * max(1.0, float(ref.abs().max()))
    for idx in places:
        for sign in (1.0, -1.0):
            bad = ref.clone()
            bad[idx] += sign * step
            with pytest.raises(AssertionError):
                check(which, bad.float(), ref, bar)
        half = ref.clone()
        half[idx] += 0.5 * step
        check(which, half, ref, bar)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def launched_kernels():
    """{launch label: count} of the operator handle's launches inside the block (option profile = 1), restored to off afterwards."""
    from fastdiff_amd import _capi, lvc_op
    lib, h = lvc_op._handle(torch.device("cuda"))
    torch.cuda.synchronize()
    lib.fd_reset_profile(h)
    assert lib.fd_set_option(h, b"profile", b"1") == 0
    names = {}
    try:
        yield names
        torch.cuda.synchronize()
        stats = (_capi.FdKernelStat * 128)()
        n = lib.fd_get_profile(h, stats, 128)
        names.update({stats[i].name.decode(): int(stats[i].launches) for i in range(min(n, 128))})
    finally:
        assert lib.fd_set_option(h, b"profile", b"0") == 0
        lib.fd_reset_profile(h)


def _kconv_inputs(M, B, T, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, 64, T, generator=g, device="cuda")
    w = torch.randn(M, 64, 3, generator=g, device="cuda") / 14.0
    bias = torch.randn(M, generator=g, device="cuda")
    return x, w, bias


def _kconv_f64(x, w, bias, dout):
    x, w, bias, dout = (t.double() for t in (x, w, bias, dout))
    return (kconv_ref(x, w, bias),) + kconv_ref_backward(x, w, dout)


def _check_kconv(got, ref):
    for name, g_, r_, bar in zip(("out", "dx", "dW", "dbias"), got, ref, (OUT_BAR, GRAD_BAR, GRAD_BAR, GRAD_BAR)):
        check(name, g_, r_, bar)


def _kconv_run(x, w, bias, dout):
    import fastdiff_amd
    xg, wg, bg = (t.clone().requires_grad_(True) for t in (x, w, bias))
    out = fastdiff_amd.kernel_conv1d(xg, wg, bg)
    out.backward(dout)
    return out.detach(), xg.grad, wg.grad, bg.grad


@pytest.mark.gpu
@pytest.mark.parametrize("M,B,T", KCONV_CASES)
def test_large_kernel_conv_against_float64(M, B, T):
    import fastdiff_amd
    slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    print(f"\nM={M} B={B} T={T}: slots {slots}, forward / dW ranges and dh slices {splits(M, B, slots)}")
    x, w, bias = _kconv_inputs(M, B, T, M + 1000 * T + B)
    dout = torch.randn(B, M, T, generator=torch.Generator(device="cuda").manual_seed(B * T), device="cuda")
    with launched_kernels() as launched:
        got = _kconv_run(x, w, bias, dout)
    assert LARGE <= launched.keys() and not SMALL & launched.keys(), launched
    _check_kconv(got, _kconv_f64(x, w, bias, dout))
    # one gradient asked for: the same bits as the full backward
    x2 = x.clone().requires_grad_(True)
    fastdiff_amd.kernel_conv1d(x2, w, bias).backward(dout)
    w2 = w.clone().requires_grad_(True)
    fastdiff_amd.kernel_conv1d(x, w2, bias).backward(dout)
    assert torch.equal(x2.grad, got[1]) and torch.equal(w2.grad, got[2])


@pytest.mark.gpu
@pytest.mark.parametrize("layers", [1, 4])
@pytest.mark.parametrize("B,T", [(1, 1), (3, 33), (20, 100), (2, 128)])
def test_frames_kernel_conv_against_float64(B, T, layers):
    """kernel_conv1d_frames: the forward through frames_to_reference(., "forward"), the gradients from frames whose reference-layout
    image is frames_to_reference(dframes, "grad")."""
    from fastdiff_amd import lvc_op
    M = 6144 * layers
    x, w, bias = _kconv_inputs(M, B, T, 7 * M + T)
    dfr = torch.randn(B, layers, T, 6144, generator=torch.Generator(device="cuda").manual_seed(B + T), device="cuda")
    xg, wg, bg = (t.clone().requires_grad_(True) for t in (x, w, bias))
    with launched_kernels() as launched:
        fr = lvc_op.kernel_conv1d_frames(xg, wg, bg)
        fr.backward(dfr)
    assert LARGE <= launched.keys() and not SMALL & launched.keys(), launched
    print(f"\nframes M={M} B={B} T={T}")
    out = lvc_op.frames_to_reference(fr.detach(), "forward").reshape(B, M, T)
    ref = _kconv_f64(x, w, bias, lvc_op.frames_to_reference(dfr, "grad").reshape(B, M, T))
    _check_kconv((out, xg.grad, wg.grad, bg.grad), ref)


def _lvc_inputs(hop, B, T, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, 32, T * hop, generator=g, device="cuda")
    K = torch.randn(B, 32, 64, 3, T, generator=g, device="cuda") / 9.8
    b = torch.randn(B, 64, T, generator=g, device="cuda")
    d = torch.randn(B, 64, T * hop, generator=g, device="cuda")
    return x, K, b, d


@pytest.mark.gpu
@pytest.mark.parametrize("hop,B,T", [(8, 20, 100), (64, 20, 100), (256, 20, 100), (256, 3, 65), (256, 1, 129)])
def test_lvc_operator_at_the_training_shape_against_float64(hop, B, T):
    """T = 65 and 129: one and two frames past the 64-frame tiles of k_lvc_pack / k_lvc_unpack."""
    import fastdiff_amd
    x, K, b, d = _lvc_inputs(hop, B, T, hop * 1000 + T)
    xg, Kg, bg = (t.clone().requires_grad_(True) for t in (x, K, b))
    y = fastdiff_amd.location_variable_convolution(xg, Kg, bg, 1, hop)
    y.backward(d)
    print(f"\nhop {hop} B={B} T={T}")
    for name, got, want in zip(("out", "dx", "dK", "dbias"), (y.detach(), xg.grad, Kg.grad, bg.grad), lvc_ref(x, K, b, d, hop)):
        check(name, got, want, LVC_BAR)


@pytest.mark.gpu
@pytest.mark.parametrize("dx_mode", ["gather", "copy"])
@pytest.mark.parametrize("hop,B,T", [(256, 20, 100), (8, 3, 65)])
def test_lvc_operator_on_frames_against_float64(hop, B, T, dx_mode):
    from fastdiff_amd import lvc_op
    lib, h = lvc_op._handle(torch.device("cuda"))
    x, K, b, d = _lvc_inputs(hop, B, T, hop * 1000 + T + 1)
    fr = lvc_op.reference_to_frames(K[:, None], "forward")[:, 0].clone()
    xg, fg, bg = (t.clone().requires_grad_(True) for t in (x, fr, b))
    assert lib.fd_set_option(h, b"lvc_dx", dx_mode.encode()) == 0
    try:
        y = lvc_op.location_variable_convolution_frames(xg, fg, bg, hop)
        y.backward(d)
        torch.cuda.synchronize()
    finally:
        assert lib.fd_set_option(h, b"lvc_dx", b"gather") == 0
    dK = lvc_op.frames_to_reference(fg.grad[:, None], "grad")[:, 0]
    print(f"\nframes hop {hop} B={B} T={T} lvc_dx={dx_mode}")
    for name, got, want in zip(("out", "dx", "dK", "dbias"), (y.detach(), xg.grad, dK, bg.grad), lvc_ref(x, K, b, d, hop)):
        check(name, got, want, LVC_BAR)


@pytest.mark.gpu
def test_large_kernel_conv_is_bit_reproducible():
    """The partial sums of the ranges and slices are added in a fixed order: two runs give the same bits."""
    M, B, T = 24576, 20, 100
    x, w, bias = _kconv_inputs(M, B, T, 11)
    dout = torch.randn(B, M, T, generator=torch.Generator(device="cuda").manual_seed(12), device="cuda")
    a, b = _kconv_run(x, w, bias, dout), _kconv_run(x, w, bias, dout)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.gpu
def test_calls_of_different_sizes_share_the_kconv_scratch():
    """Every backward below sums its partial results in the handle's one kconv_scratch buffer, grown for the largest call: run one
    after the other, largest first and back, each gives the bits it gave on its own (runs in the reverse order first)."""
    from fastdiff_amd import lvc_op
    gen = torch.Generator(device="cuda").manual_seed(5)

    def rnd(*s):
        return torch.randn(*s, generator=gen, device="cuda")

    big = _kconv_inputs(24576, 20, 128, 21) + (rnd(20, 24576, 128),)
    mid = _kconv_inputs(544, 3, 33, 22) + (rnd(3, 544, 33),)
    side = ([rnd(20, 64, 100) for _ in range(3)], [rnd(256, 64, 3) / 14.0 for _ in range(3)], [rnd(256) for _ in range(3)],
            [rnd(20, 256, 100) for _ in range(3)])
    ic = (rnd(20, 80, 100), rnd(64, 80, 5) / 20.0, rnd(64), rnd(20, 64, 100))

    def run_side():
        xs, ws, bs = ([t.clone().requires_grad_(True) for t in ts] for ts in side[:3])
        outs = lvc_op.kernel_conv1d_side_by_side(xs, ws, bs)
        sum((o * d).sum() for o, d in zip(outs, side[3])).backward()
        return [o.detach() for o in outs] + [t.grad for t in xs + ws + bs]

    def run_ic():
        x, w, b = (t.clone().requires_grad_(True) for t in ic[:3])
        y = lvc_op.input_conv(x, w, b, 0.1)
        y.backward(ic[3])
        return [y.detach(), x.grad, w.grad, b.grad]

    calls = [lambda: _kconv_run(*big), lambda: _kconv_run(*mid), run_side, run_ic]
    alone = [list(c()) for c in reversed(calls)][::-1]
    again = [list(c()) for c in calls] + [list(calls[0]())]
    for i, (got, want) in enumerate(zip(again, alone + alone[:1])):
        assert all(torch.equal(p, q) for p, q in zip(got, want)), i
    _check_kconv(again[-1], _kconv_f64(*big))


@pytest.mark.gpu
def test_in_slope_on_the_large_path():
    """fd_kconv_backward_act with in_slope != 1 at M > 512: dx in front of the activation of the layer below, dx * (h > 0 ? 1 : slope)."""
    from fastdiff_amd import lvc_op
    M, B, T, slope = 544, 3, 33, 0.1
    x, w, bias = _kconv_inputs(M, B, T, 31)
    dout = torch.randn(B, M, T, generator=torch.Generator(device="cuda").manual_seed(32), device="cuda")
    dx = torch.empty_like(x)
    with launched_kernels() as launched:
        lvc_op._call(x.device, "fd_kconv_backward_act", "fd_kconv_backward", x, w, None, dout, B, M, T, 1.0, slope, dx, None, None)
    assert {"kconv_backward_h", "kconv_backward_h_fold"} <= launched.keys() and not SMALL & launched.keys(), launched
    assert bool((x < 0).any()) and bool((x > 0).any())
    ref = _kconv_f64(x, w, bias, dout)[1] * torch.where(x > 0, torch.ones_like(x), torch.full_like(x, slope)).double()
    check("dx", dx, ref, GRAD_BAR)


@pytest.mark.gpu
def test_large_path_refusals():
    import fastdiff_amd
    from fastdiff_amd import lvc_op
    dev = torch.device("cuda")
    x, w, bias = _kconv_inputs(24576, 1, 4, 41)
    with pytest.raises(NotImplementedError, match="512"):                       # the fused activation: M <= 512 only
        fastdiff_amd.kernel_conv1d(x, w, bias, post_slope=0.1)
    y, d, dx = torch.zeros(1, 24576, 4, device="cuda"), torch.zeros(1, 24576, 4, device="cuda"), torch.empty_like(x)
    with pytest.raises(NotImplementedError, match="512"):
        lvc_op._call(dev, "fd_kconv_backward_act", "fd_kconv_backward", x, w, y, d, 1, 24576, 4, 0.1, 1.0, dx, None, None)
    with pytest.raises(NotImplementedError, match="128"):                       # T = 129
        fastdiff_amd.kernel_conv1d(torch.zeros(1, 64, 129, device="cuda"), w, bias)
    # frames: a whole number of 6144-row layers only (check_kconv_frames); buffers sized for M = 6176 all the same
    M, B, T = 6144 + 32, 2, 5
    xf, wf, bf = _kconv_inputs(M, B, T, 42)
    out = torch.empty(B * M * T, device="cuda")
    with pytest.raises(NotImplementedError, match="6144"):
        lvc_op._call(dev, "fd_kconv_forward_frames", "fd_kconv_forward_frames", xf, wf, bf, B, M, T, out)
    dxf, dwf, dbf = torch.empty_like(xf), torch.empty_like(wf), torch.empty_like(bf)
    with pytest.raises(NotImplementedError, match="6144"):
        lvc_op._call(dev, "fd_kconv_backward_frames", "fd_kconv_backward_frames", xf, wf, out, B, M, T, dxf, dwf, dbf)
    torch.cuda.synchronize()
