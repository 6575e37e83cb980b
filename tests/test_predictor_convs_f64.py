"""The KernelPredictor's small convolutions against float64 references that share nothing with the HIP kernels, at their own borders.

Each predictor front end runs an input convolution (Conv1d(80, 64, 5) + LeakyReLU) and six Conv1d(64, 64, 3) + LeakyReLU pairs, and each
predictor has a bias_conv (M = 256); all of them run on the small-M kernels of csrc/fd_kernels_kconv.hip:
    k_kcs_fwd                        wave = (32-row tile wave & 1, column tiles 2 ch, 2 ch + 1 of 32 frames); dead second wave pair at M % 64 = 32
    k_kcs_dw<ALIGNED, ACT>           ALIGNED iff T % 4 = 0; ceil(T / 8) quads, the last element by element; ACT with an item without y
    k_kc_dh<false, ACT> + fold       the mask applied chunk by chunk under the prefetch; in_slope on the way out; taps folded at t = 0, T - 1
    k_kc_dw_sum                      one partial per utterance; 192 and 400 columns; dW = NULL, dbias = NULL; the grid tail
    k_ic_fwd / k_ic_bwd_x / _w       a thread owns 8 frames; the weight gradient walks 4 frames at a time over rows that are zero behind T
    the *_multi launches             up to 8 convolutions side by side
tests/test_lvc_op.py holds them to float64 autograd at T in {1, 5, 7, 37, 50, 100, 128}; here every element of out, dx, dW and dbias is
compared with an explicit float64 evaluation (kconv_ref / conv_taps of the two sibling files) one frame short of, at and one frame past
every 32-frame tile, at every T % 4 and T % 8, with a dead wave pair, with an odd chunk count and at M = 512 (KC_SMALL_M itself), and
-- at batch sizes computed from the device's CU count -- in the masked multi-chunk loop of k_kc_dh that no smaller shape reaches.

The C entry points are called directly (lvc_op._call), so the backward's y is an INPUT of the test: the float32 image of the float64
forward output with +0.0, -0.0, +2^-126 and -2^-126 planted in it, and the reference mask is where(y > 0, 1, post) on exactly that y (for
in_slope: where(h > 0, 1, in_slope) on the given h).  No element's sign depends on the forward under test; saved_output asserts that the
float32 image itself flips no sign.  One weight row with its bias is zero (that row's y is exactly 0), one input frame is zero (h = 0
under in_slope).  Outputs are pre-filled with NaN: an element that no thread writes fails.

Bars: OUT_BAR for outputs, GRAD_BAR for gradients, relative to max(1, max |ref|) per tensor (test_training_kernels_f64.py).  Next to
every HIP distance the test prints the distance of torch's own float32 evaluation of the same expression from float64 (gap32) and the
ratio of the two; the worst ratios are in LABBOOK R37.1."""
import pytest
import torch
import torch.nn.functional as F

from test_training_convs_f64 import _lrelu, _slope, conv_taps, conv_taps_backward
from test_training_kernels_f64 import GRAD_BAR, OUT_BAR, _dh_slices, check, kconv_ref, kconv_ref_backward, launched_kernels, rel_err

T_EDGES = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128)
M_EDGES = (32, 64, 96, 256, 480, 512)      # 32, 96: a dead wave pair; 480: an odd number of 32-row chunks; 512: KC_SMALL_M
IC_T = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 120, 121, 127, 128)
MODES = ((1.0, False, 1.0), (0.1, True, 1.0), (1.0, False, 0.1), (0.1, True, 0.1))      # (post, y given, in_slope)
SIDE_SHAPES = ((64, 3, 33), (96, 2, 5), (256, 2, 65))      # (M, B, T)
# side by side: which items have a y, a dweight, a dbias (item 4 of 8 has neither gradient: both early returns of k_kc_dw_sum)
SIDE_Y = {8: (1, 0, 1, 1, 0, 0, 1, 0), 3: (0, 1, 0)}
SIDE_DW = {8: (1, 1, 0, 1, 0, 1, 1, 0), 3: (1, 0, 1)}
SIDE_DB = {8: (1, 0, 1, 1, 0, 0, 1, 1), 3: (0, 1, 1)}
TINY = 2.0 ** -126                          # the smallest normal float32: no subnormal is planted
PLANTED = (0.0, -0.0, TINY, -TINY)
SMALL_KCONV = {"kconv_forward_small", "kconv_backward_w_small", "kconv_backward_w_sum", "kconv_backward_h", "kconv_backward_h_fold"}
INPUT_CONV = {"input_conv_forward", "input_conv_backward_x", "input_conv_backward_w", "kconv_backward_w_sum"}
NEVER = {"kconv_forward", "kconv_backward_w"}


def kconv_shapes():
    """(M, B, T) of the one-convolution test: every T edge at M = 64 and 96, every M edge at five T, B = 3; B = 1 at T = 1 and 33."""
    shapes = [(M, 3, T) for M in (64, 96) for T in T_EDGES]
    shapes += [(M, 3, T) for M in M_EDGES for T in (1, 5, 33, 100, 128) if (M, 3, T) not in shapes]
    return shapes + [(M, 1, T) for M in M_EDGES for T in (1, 33)]


KCONV_SHAPES = kconv_shapes()
IC_SHAPES = [(B, T) for B in (1, 3) for T in IC_T]


def multi_chunk_batch(M, slots):
    """The smallest B at which dh_slices gives a slice of k_kc_dh more than one 32-row chunk (slots = 2 x CUs)."""
    return next(B for B in range(1, 65536) if _dh_slices(M, B, slots) < M // 32)


# ---- references, in the inputs' type (float64; float32 for the yardstick) ------------------------------------------------------------

def kconv_act_ref(h, W, bias, post):
    return _lrelu(kconv_ref(h, W, bias), post)


def kconv_act_ref_backward(h, W, y, dout, post, in_slope):
    """(dx, dW, dbias): dout masked with where(y > 0, 1, post) on the GIVEN y (None: as it is), dx with where(h > 0, 1, in_slope)."""
    du = dout if y is None else dout * _slope(y.to(dout.dtype), post)
    dx, dW, db = kconv_ref_backward(h, W, du)
    return (dx if in_slope == 1.0 else dx * _slope(h, in_slope)), dW, db


def ic_ref(x, W, bias, post):
    return _lrelu(conv_taps(x, W, bias, 1), post)


def ic_ref_backward(x, W, y, dy, post):
    return conv_taps_backward(x, W, dy * _slope(y.to(dy.dtype), post), 1)


def planted_places(numel):
    return [0, numel // 3, 2 * numel // 3, numel - 1]


def saved_output(y64):
    """The y the backward is given: the float32 image of the float64 output with PLANTED at planted_places.  Before planting the image
    has the sign of the float64 output everywhere (an exact zero stays zero), so outside the planted entries no mask depends on float32."""
    y = y64.float().contiguous()
    assert bool((torch.sign(y).double() == torch.sign(y64)).all()), "the float32 image flips a sign of the float64 output"
    y.view(-1)[planted_places(y.numel())] = torch.tensor(PLANTED, dtype=torch.float32, device=y.device)
    return y


def _zero_frame(x):
    """One input frame exactly zero: the middle frame of the last utterance (with one frame in all: its even channels)."""
    B, _, T = x.shape
    if B * T > 1:
        x[B - 1, :, T // 2] = 0.0
    else:
        x[0, ::2, 0] = 0.0


def kconv_inputs(M, B, T, seed, device="cuda"):
    """x ~ N(0, 1), w / 14, bias, dout, as tests/test_training_kernels_f64.py draws them; row M - 2 of w and bias zero, one frame zero."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(B, 64, T, generator=g, device=device)
    w = torch.randn(M, 64, 3, generator=g, device=device) / 14.0
    bias = torch.randn(M, generator=g, device=device)
    dout = torch.randn(B, M, T, generator=g, device=device)
    w[M - 2] = 0.0
    bias[M - 2] = 0.0
    _zero_frame(x)
    return x, w, bias, dout


def ic_inputs(B, T, seed, device="cuda"):
    """x [B, 80, T] ~ N(0, 1), w [64, 80, 5] / 20, bias, dy; row 62 of w and bias zero, one frame zero."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(B, 80, T, generator=g, device=device)
    w = torch.randn(64, 80, 5, generator=g, device=device) / 20.0
    bias = torch.randn(64, generator=g, device=device)
    dy = torch.randn(B, 64, T, generator=g, device=device)
    w[62] = 0.0
    bias[62] = 0.0
    _zero_frame(x)
    return x, w, bias, dy


def held(kernel, name, where, got, ref64, ref32, bar):
    """Every element of `got` against float64 under `bar`; prints the HIP distance, gap32 and their ratio first."""
    err, gap = rel_err(got, ref64), rel_err(ref32, ref64)
    print(f"  {kernel} {name} [{where}]: hip {err:.2e}  float32 {gap:.2e}  ratio {err / gap if gap > 0 else float('inf'):.2f}")
    check(f"{kernel} {name} [{where}]", got, ref64, bar)


def _f64(*ts):
    return tuple(None if t is None else t.double() for t in ts)


# ---- CPU: the references are what they claim -------------------------------------------------------------------------------------------

def _r64(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("B,T,post", [(2, 7, 0.1), (3, 1, 0.1), (2, 4, 1.0)])
def test_k5_reference_equals_conv1d_and_its_autograd(B, T, post):
    g = torch.Generator().manual_seed(10 * B + T)
    x, w, b, dy = _r64(g, B, 80, T), _r64(g, 64, 80, 5) / 20.0, _r64(g, 64), _r64(g, B, 64, T)
    xa, wa, ba = (t.clone().requires_grad_(True) for t in (x, w, b))
    ya = F.leaky_relu(F.conv1d(xa, wa, ba, padding=2), post)
    ya.backward(dy)
    y = ic_ref(x, w, b, post)
    for got, want in zip((y,) + tuple(ic_ref_backward(x, w, y, dy, post)), (ya.detach(), xa.grad, wa.grad, ba.grad)):
        assert got.shape == want.shape and torch.allclose(got, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("post,with_y,in_slope", MODES)
@pytest.mark.parametrize("B,M,T", [(2, 96, 7), (3, 32, 1)])
def test_masked_and_in_slope_references_equal_autograd(B, M, T, post, with_y, in_slope):
    """h = leaky_relu(z, in_slope) below, y = leaky_relu(conv1d(h), post) above: dx of the reference is autograd's dz (h > 0 iff z > 0)."""
    g = torch.Generator().manual_seed(100 * B + T)
    z, w, b, dout = _r64(g, B, 64, T), _r64(g, M, 64, 3) / 14.0, _r64(g, M), _r64(g, B, M, T)
    z[0, 3, 0] = 0.0
    za, wa, ba = (t.clone().requires_grad_(True) for t in (z, w, b))
    ha = F.leaky_relu(za, in_slope)
    ya = F.leaky_relu(F.conv1d(ha, wa, ba, padding=1), post)
    ya.backward(dout)
    h = ha.detach()
    y = kconv_act_ref(h, w, b, post)
    assert torch.allclose(y, ya.detach(), rtol=0, atol=1e-12)
    for got, want in zip(kconv_act_ref_backward(h, w, y if with_y else None, dout, post, in_slope), (za.grad, wa.grad, ba.grad)):
        assert got.shape == want.shape and torch.allclose(got, want, rtol=0, atol=1e-12)


def test_saved_output_plants_the_four_values_and_refuses_a_flipped_sign():
    x, w, b, _ = (t.double() for t in kconv_inputs(96, 3, 33, 5, "cpu"))
    y64 = kconv_act_ref(x, w, b, 0.1)
    y = saved_output(y64)
    flat, places = y.view(-1), planted_places(y.numel())
    assert flat[places].tolist() == [0.0, 0.0, TINY, -TINY] and bool(torch.signbit(flat[places[1]])) and not bool(torch.signbit(flat[places[0]]))
    assert TINY > 0 and float(torch.tensor(TINY, dtype=torch.float32)) == TINY and TINY >= torch.finfo(torch.float32).tiny
    rest = torch.ones(y.numel(), dtype=torch.bool)
    rest[places] = False
    assert torch.equal(flat[rest], y64.float().view(-1)[rest]) and bool((y64[:, 94] == 0).all()) and bool((y[:, 94] == 0).all())
    mask = _slope(y.double(), 0.1).view(-1)      # the reference mask on the planted entries: slope, slope, 1, slope
    assert mask[places].tolist() == [0.1, 0.1, 1.0, 0.1]
    bad = y64.clone()
    bad[1, 2, 3] = 1e-60                          # positive in float64, zero in float32
    with pytest.raises(AssertionError, match="flips a sign"):
        saved_output(bad)


# ---- CPU: the tables reach what they are chosen for -------------------------------------------------------------------------------------

def test_the_shape_tables_reach_the_edges_they_are_chosen_for():
    assert {T % 4 for T in T_EDGES} == {0, 1, 2, 3} and {T % 8 for T in T_EDGES} >= {0, 1, 7}
    assert set(T_EDGES) >= {T for T in range(1, 129) if T % 32 in (31, 0, 1)}
    assert {M % 64 for M in M_EDGES} == {0, 32} and max(M_EDGES) == 512 and (480 // 32) % 2 == 1
    assert {T for _, _, T in KCONV_SHAPES} == set(T_EDGES) | {100}
    for M in (64, 96):
        assert {T for m, B, T in KCONV_SHAPES if m == M and B == 3} == set(T_EDGES) | {100}
    for T in (1, 5, 33, 100, 128):
        assert {M for M, B, t in KCONV_SHAPES if t == T and B == 3} == set(M_EDGES)
    assert {(M, T) for M, B, T in KCONV_SHAPES if B == 1} == {(M, T) for M in M_EDGES for T in (1, 33)}
    assert len(KCONV_SHAPES) == len(set(KCONV_SHAPES)) == 38 + 30 - 8 + 12 and all(B <= 3 for _, B, _ in KCONV_SHAPES)
    # the input convolution: a thread's 8 frames one short of, at and past full; the 4-frame walk of k_ic_bwd_w at every T % 4
    assert {T % 8 for T in IC_T} >= {0, 1, 7} and {T % 4 for T in IC_T} == {0, 1, 2, 3} and max(IC_T) == 128
    for n in (8, 3):
        assert len(SIDE_Y[n]) == len(SIDE_DW[n]) == len(SIDE_DB[n]) == n
        assert 0 < sum(SIDE_Y[n]) < n and 0 < sum(SIDE_DW[n]) < n and 0 < sum(SIDE_DB[n]) < n
    assert (SIDE_DW[8][4], SIDE_DB[8][4]) == (0, 0)
    assert {M % 64 for M, _, _ in SIDE_SHAPES} == {0, 32} and {T % 4 for _, _, T in SIDE_SHAPES} == {1}


def test_slice_counts_of_the_multi_chunk_rows():
    """On 512 slots (256 CUs, two workgroups each) a slice of k_kc_dh first holds two chunks at (M = 512, B = 33) and three at (M = 480,
    B = 69); every shape of the one-convolution test and of the side-by-side test has one chunk per slice."""
    assert multi_chunk_batch(512, 512) == 33 and _dh_slices(512, 33, 512) == 8 and _dh_slices(512, 32, 512) == 16
    assert multi_chunk_batch(480, 512) == 69 and _dh_slices(480, 69, 512) == 5 and _dh_slices(480, 68, 512) == 15
    for M, B, T in KCONV_SHAPES + [s for s in SIDE_SHAPES]:
        assert _dh_slices(M, B, 512) == M // 32, (M, B, T)
    for cus in (64, 80, 104, 228, 304):          # other devices: the batch stays well inside what the entry points accept
        for M in (512, 480):
            assert multi_chunk_batch(M, 2 * cus) <= 128


@pytest.mark.parametrize("which", ["out", "dx", "dW", "dW_ic"])
def test_the_bars_reject_one_element_just_beyond_them(which):
    """The float32 image of a float64 reference passes; one element moved by 1.01 x the bar fails and by 0.5 x passes -- at frame T - 1,
    frame 32, row M - 1, row 32, utterance B - 1, dW[M - 1, 63, 2] and the input convolution's dW[63, 79, 4]."""
    M, B, T = 96, 3, 65
    if which == "dW_ic":
        x, w, b, dy = (t.double() for t in ic_inputs(B, T, 3, "cpu"))
        ref, bar = ic_ref_backward(x, w, saved_output(ic_ref(x, w, b, 0.1)), dy, 0.1)[1], GRAD_BAR
        places = [(63, 79, 4), (0, 0, 0)]
        assert tuple(ref.shape) == (64, 80, 5)
    else:
        x, w, b, dout = (t.double() for t in kconv_inputs(M, B, T, 4, "cpu"))
        y64 = kconv_act_ref(x, w, b, 0.1)
        dx, dW, _ = kconv_act_ref_backward(x, w, saved_output(y64), dout, 0.1, 0.1)
        ref, bar = {"out": (y64, OUT_BAR), "dx": (dx, GRAD_BAR), "dW": (dW, GRAD_BAR)}[which]
        places = {"out": [(0, 5, T - 1), (1, 7, 32), (0, M - 1, 3), (1, 32, 10), (B - 1, 50, 40)],
                  "dx": [(0, 5, T - 1), (1, 63, 32), (B - 1, 0, 0)],
                  "dW": [(M - 1, 63, 2), (32, 0, 0)]}[which]
    check(which, ref.float(), ref, bar)
    step = 1.01 * bar * max(1.0, float(ref.abs().max()))
    for idx in places:
        for sign in (1.0, -1.0):
            bad = ref.clone()
            bad[idx] += sign * step
            with pytest.raises(AssertionError):
                check(which, bad, ref, bar)
        half = ref.clone()
        half[idx] += 0.5 * step
        check(which, half, ref, bar)
    unwritten = ref.clone()
    unwritten[places[0]] = float("nan")           # an element no thread wrote (the outputs are pre-filled with NaN)
    with pytest.raises(AssertionError):
        check(which, unwritten, ref, bar)


# ---- GPU: how the entry points are driven ----------------------------------------------------------------------------------------------

def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)


def _call(fn, label, *args):
    from fastdiff_amd import lvc_op
    lvc_op._call(torch.device("cuda"), fn, label, *args)


def kconv_forward(x, w, bias, post):
    B, _, T = x.shape
    out = _nan(B, w.shape[0], T)
    _call("fd_kconv_forward_act", "fd_kconv_forward", x, w, bias, B, w.shape[0], T, post, out)
    return out


def kconv_backward(x, w, y, dout, post, in_slope, want=("dx", "dW", "db")):
    """fd_kconv_backward_act for the gradients named in `want`: (dx, dW, db), None where not asked for."""
    B, M, T = dout.shape
    dx = _nan(B, 64, T) if "dx" in want else None
    dW = _nan(M, 64, 3) if "dW" in want else None
    db = _nan(M) if "db" in want else None
    _call("fd_kconv_backward_act", "fd_kconv_backward", x, w, y, dout, B, M, T, post, in_slope, dx, dW, db)
    return dx, dW, db


def ic_forward(x, w, bias, post):
    B, _, T = x.shape
    out = _nan(B, 64, T)
    _call("fd_input_conv_forward", "fd_input_conv_forward", x, w, bias, B, T, post, out)
    return out


def ic_backward(x, w, y, dy, post, want=("dx", "dW", "db")):
    B, _, T = x.shape
    dx = _nan(B, 80, T) if "dx" in want else None
    dW = _nan(64, 80, 5) if "dW" in want else None
    db = _nan(64) if "db" in want else None
    _call("fd_input_conv_backward", "fd_input_conv_backward", x, w, y, dy, B, T, post, dx, dW, db)
    return dx, dW, db


def _slots():
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


# ---- GPU: one small convolution ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("M,B,T", KCONV_SHAPES, ids=[f"M{M}-B{B}-T{T}" for M, B, T in KCONV_SHAPES])
def test_small_kernel_conv_against_float64(M, B, T):
    """out, dx, dW and dbias of fd_kconv_forward_act / fd_kconv_backward_act in the four (post, y, in_slope) modes, every element; then
    each gradient asked for alone: the same bits."""
    x, w, bias, dout = kconv_inputs(M, B, T, M + 1000 * T + B)
    x64, w64, b64, d64 = _f64(x, w, bias, dout)
    print(f"\nM={M} B={B} T={T}: {_dh_slices(M, B, _slots())} dh slices of {M // 32} chunks")
    forward = {}
    for post in (1.0, 0.1):
        with launched_kernels() as launched:
            out = kconv_forward(x, w, bias, post)
        assert launched.keys() == {"kconv_forward_small"}, launched
        ref = kconv_act_ref(x64, w64, b64, post)
        held("k_kcs_fwd", "out", f"M={M} B={B} T={T} post={post}", out, ref, kconv_act_ref(x, w, bias, post), OUT_BAR)
        assert bool((out[:, M - 2] == 0).all()) and bool((ref[:, M - 2] == 0).all())          # the zero row: exactly 0
        forward[post] = ref
    for post, with_y, in_slope in MODES:
        where = f"M={M} B={B} T={T} post={post} y={'given' if with_y else 'none'} in_slope={in_slope}"
        y = saved_output(forward[post]) if with_y else None
        with launched_kernels() as launched:
            got = kconv_backward(x, w, y, dout, post, in_slope)
        assert launched.keys() == SMALL_KCONV - {"kconv_forward_small"} and not NEVER & launched.keys(), launched
        ref = kconv_act_ref_backward(x64, w64, y, d64, post, in_slope)
        yard = kconv_act_ref_backward(x, w, y, dout, post, in_slope)
        for kernel, name, g_, r_, y_ in zip(("k_kc_dh", "k_kcs_dw", "k_kcs_dw"), ("dx", "dW", "dbias"), got, ref, yard):
            held(kernel, name, where, g_, r_, y_, GRAD_BAR)
        for i, only in enumerate(("dx", "dW", "db")):
            alone = kconv_backward(x, w, y, dout, post, in_slope, want=(only,))
            assert [a is not None for a in alone] == [j == i for j in range(3)] and torch.equal(alone[i], got[i]), (where, only)


# ---- GPU: the masked multi-chunk loop of k_kc_dh ---------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("T", [5, 33])
@pytest.mark.parametrize("M", [512, 480])
def test_masked_multi_chunk_dh_against_float64(M, T):
    """The smallest B at which a slice of k_kc_dh<false, true> holds more than one 32-row chunk on this device (33 and 69 on 256 CUs):
    the mask of chunk n + 1 is loaded under the matrix work of chunk n.  The entry point accepts any B up to 65535, so B is the
    computed one, not a neighbour."""
    slots = _slots()
    B = multi_chunk_batch(M, slots)
    nks = _dh_slices(M, B, slots)
    print(f"\nM={M} T={T}: slots {slots}, B={B}: {nks} slices of {M // nks} rows")
    assert nks < M // 32 and M // nks > 32 and (M // nks) % 32 == 0
    x, w, bias, dout = kconv_inputs(M, B, T, M + 7 * T)
    x64, w64, b64, d64 = _f64(x, w, bias, dout)
    y = saved_output(kconv_act_ref(x64, w64, b64, 0.1))
    with launched_kernels() as launched:
        dx, dW, db = kconv_backward(x, w, y, dout, 0.1, 0.1, want=("dx",))
    assert launched.keys() == {"kconv_backward_h", "kconv_backward_h_fold"} and dW is None and db is None, launched
    ref = kconv_act_ref_backward(x64, w64, y, d64, 0.1, 0.1)[0]
    held("k_kc_dh multi-chunk", "dx", f"M={M} B={B} T={T} post=0.1 y=given in_slope=0.1", dx, ref,
         kconv_act_ref_backward(x, w, y, dout, 0.1, 0.1)[0], GRAD_BAR)


# ---- GPU: side by side -------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 3])
@pytest.mark.parametrize("M,B,T", SIDE_SHAPES)
def test_small_kernel_convs_side_by_side_against_float64(M, B, T, n):
    """fd_kconv_forward_act_multi, fd_kconv_backward_x_multi and fd_kconv_backward_w_multi on n convolutions, some items without y,
    without dweight or without dbias: every item against float64, and bit-equal to the same convolution called alone."""
    post, in_slope = 0.1, 0.1
    items = [kconv_inputs(M, B, T, 10007 * (i + 1) + M + T) for i in range(n)]
    xs, ws, bs, ds = (list(t) for t in zip(*items))
    print(f"\nside by side n={n} M={M} B={B} T={T}")
    outs = [_nan(B, M, T) for _ in range(n)]
    with launched_kernels() as launched:
        _call("fd_kconv_forward_act_multi", "fd_kconv_forward_act_multi", n, xs, ws, bs, B, M, T, post, outs)
    assert launched == {"kconv_forward_small": 1}, launched
    ys = []
    for i in range(n):
        ref = kconv_act_ref(*_f64(xs[i], ws[i], bs[i]), post)
        held("k_kcs_fwd multi", "out", f"n={n} item {i} M={M} B={B} T={T}", outs[i], ref, kconv_act_ref(xs[i], ws[i], bs[i], post), OUT_BAR)
        assert torch.equal(outs[i], kconv_forward(xs[i], ws[i], bs[i], post)), i
        ys.append(saved_output(ref) if SIDE_Y[n][i] else None)
    dxs = [_nan(B, 64, T) for _ in range(n)]
    dws = [_nan(M, 64, 3) if SIDE_DW[n][i] else None for i in range(n)]
    dbs = [_nan(M) if SIDE_DB[n][i] else None for i in range(n)]
    with launched_kernels() as launched:
        _call("fd_kconv_backward_x_multi", "fd_kconv_backward_x_multi", n, xs, ws, ys, ds, B, M, T, post, in_slope, dxs)
        _call("fd_kconv_backward_w_multi", "fd_kconv_backward_w_multi", n, xs, ds, ys, B, M, T, post, dws, dbs)
    assert launched == {"kconv_backward_h": 1, "kconv_backward_h_fold": 1, "kconv_backward_w_small": 1, "kconv_backward_w_sum": 1}, launched
    for i in range(n):
        where = f"n={n} item {i} M={M} B={B} T={T} y={'given' if ys[i] is not None else 'none'}"
        post_i = post if ys[i] is not None else 1.0      # alone, an item without y is the plain convolution
        ref = kconv_act_ref_backward(*_f64(xs[i], ws[i]), ys[i], ds[i].double(), post, in_slope)
        yard = kconv_act_ref_backward(xs[i], ws[i], ys[i], ds[i], post, in_slope)
        alone = kconv_backward(xs[i], ws[i], ys[i], ds[i], post_i, in_slope, want=("dx",))[:1] + \
            kconv_backward(xs[i], ws[i], ys[i], ds[i], post_i, 1.0, want=("dW", "db"))[1:]
        for kernel, name, g_, r_, y_, a_ in zip(("k_kc_dh multi", "k_kcs_dw multi", "k_kcs_dw multi"), ("dx", "dW", "dbias"),
                                                (dxs[i], dws[i], dbs[i]), ref, yard, alone):
            if g_ is not None:
                held(kernel, name, where, g_, r_, y_, GRAD_BAR)
                assert torch.equal(g_, a_), (where, name)


# ---- GPU: the input convolution ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("B,T", IC_SHAPES, ids=[f"B{B}-T{T}" for B, T in IC_SHAPES])
def test_input_conv_against_float64(B, T):
    """out, dx, dW [64, 80, 5] and db of fd_input_conv_forward / fd_input_conv_backward with and without the activation, every element;
    then each gradient asked for alone: the same bits."""
    x, w, bias, dy = ic_inputs(B, T, 31 * T + B)
    x64, w64, b64, d64 = _f64(x, w, bias, dy)
    print(f"\ninput conv B={B} T={T}")
    for post in (0.1, 1.0):
        where = f"B={B} T={T} post={post}"
        ref_out = ic_ref(x64, w64, b64, post)
        y = saved_output(ref_out)
        with launched_kernels() as launched:
            out = ic_forward(x, w, bias, post)
            got = ic_backward(x, w, y, dy, post)
        assert launched == dict.fromkeys(INPUT_CONV, 1), launched
        held("k_ic_fwd", "out", where, out, ref_out, ic_ref(x, w, bias, post), OUT_BAR)
        assert bool((out[:, 62] == 0).all())
        ref, yard = ic_ref_backward(x64, w64, y, d64, post), ic_ref_backward(x, w, y, dy, post)
        for kernel, name, g_, r_, y_ in zip(("k_ic_bwd_x", "k_ic_bwd_w", "k_ic_bwd_w"), ("dx", "dW", "db"), got, ref, yard):
            held(kernel, name, where, g_, r_, y_, GRAD_BAR)
        for i, only in enumerate(("dx", "dW", "db")):
            alone = ic_backward(x, w, y, dy, post, want=(only,))
            assert [a is not None for a in alone] == [j == i for j in range(3)] and torch.equal(alone[i], got[i]), (where, only)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [9, 65])
def test_input_convs_side_by_side_against_float64(T):
    """fd_input_conv_forward_multi / fd_input_conv_backward_multi on 8 convolutions (some items without dweight or dbias): every item
    against float64, and bit-equal to the one-convolution entry points."""
    n, B, post = 8, 3, 0.1
    items = [ic_inputs(B, T, 7919 * (i + 1) + T) for i in range(n)]
    xs, ws, bs, ds = (list(t) for t in zip(*items))
    print(f"\ninput conv side by side n={n} B={B} T={T}")
    outs = [_nan(B, 64, T) for _ in range(n)]
    refs = [ic_ref(*_f64(xs[i], ws[i], bs[i]), post) for i in range(n)]
    ys = [saved_output(r) for r in refs]
    dxs = [_nan(B, 80, T) for _ in range(n)]
    dws = [_nan(64, 80, 5) if SIDE_DW[n][i] else None for i in range(n)]
    dbs = [_nan(64) if SIDE_DB[n][i] else None for i in range(n)]
    with launched_kernels() as launched:
        _call("fd_input_conv_forward_multi", "fd_input_conv_forward_multi", n, xs, ws, bs, B, T, post, outs)
        _call("fd_input_conv_backward_multi", "fd_input_conv_backward_multi", n, xs, ws, ys, ds, B, T, post, dxs, dws, dbs)
    assert launched == dict.fromkeys(INPUT_CONV, 1), launched
    for i in range(n):
        where = f"n={n} item {i} B={B} T={T}"
        held("k_ic_fwd multi", "out", where, outs[i], refs[i], ic_ref(xs[i], ws[i], bs[i], post), OUT_BAR)
        assert torch.equal(outs[i], ic_forward(xs[i], ws[i], bs[i], post)), i
        ref, yard = ic_ref_backward(*_f64(xs[i], ws[i]), ys[i], ds[i].double(), post), ic_ref_backward(xs[i], ws[i], ys[i], ds[i], post)
        alone = ic_backward(xs[i], ws[i], ys[i], ds[i], post)
        for kernel, name, g_, r_, y_, a_ in zip(("k_ic_bwd_x multi", "k_ic_bwd_w multi", "k_ic_bwd_w multi"), ("dx", "dW", "db"),
                                                (dxs[i], dws[i], dbs[i]), ref, yard, alone):
            if g_ is not None:
                held(kernel, name, where, g_, r_, y_, GRAD_BAR)
                assert torch.equal(g_, a_), (where, name)
