"""The hand-written training convolutions of csrc/fd_kernels_cconv.hip against float64 references that share nothing with them.

Three operators run these kernels 21 + 2 + 3 times in each direction of every training step:
    fastdiff_amd.conv32    k_cconv_fwd / k_cconv_bwd<DIL>                       the small Conv1d(32, 32, 3) of the denoiser
    lvc_op.conv7           k_c7_first_fwd / k_c7_final_fwd / k_c7_bwd<MODE>     first_audio_conv and final_conv
    lvc_op.upsample        k_ct_fwd / k_ct_bwd<R>                               leaky_relu + ConvTranspose1d(32, 32, 2 r, stride r)
and k_cconv_reduce, which adds up the per-workgroup partials of all three backward passes.  tests/test_lvc_op.py compares them with
torch's autograd; here every element of every output and gradient is compared with an explicit tap-by-tap float64 evaluation, at the
shapes where the code takes another path: every wave and 32-column tile of the forward (256 / 64 / 32 columns) and the backward (128 /
32) one quad short of, at and past its border; utterances shorter than the halo lying side by side; the partial counts at which
k_cconv_reduce's eight slices are empty, hold one element or leave a tail; and shapes built from the device's CU count at which a
persistent workgroup takes a second and a third tile.

Bars: OUT_BAR for outputs, GRAD_BAR for gradients, relative to max(1, max |ref|) per tensor (test_training_kernels_f64.py).  Next to
every HIP distance the test prints the distance of torch's own float32 evaluation of the same expression from float64.

The output activation of conv32 (post != 1): k_cconv_bwd takes the mask from the sign of the saved y.  Where float64's pre-activation
u is within rounding of zero a correct float32 forward may hold either sign, so there the reference backward takes the sign HIP's y
holds (the forward check bounds y there) and everywhere else float64's.  "Within rounding": |u64| <= GUARD * S_u with S_u = |bias| +
sum |W| |a|, the same float64 reference run on absolute values, and GUARD = 100 x 2^-24 -- the worst case of a chain of 96 fused
multiply-adds on the bias plus the roundings of x + skip and of the input activation.  S_u = 0 (a planted row with W = 0 and bias =
0) means every term is exactly zero in every precision: u = 0, decided, and the mask is the slope.  At most 2^-12 of a case's
elements may be undecided; a CPU test asserts that from float64 alone for every case."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_training_kernels_f64 import GRAD_BAR, OUT_BAR, launched_kernels

GUARD = 100.0 * 2.0 ** -24
UNDECIDED_CAP = 2.0 ** -12
DILATIONS = (1, 2, 3, 4, 9, 27)
CUS = 256                                     # an MI355X; the GPU tests rebuild the persistent shapes from the device's own count


def _cdiv(a, b):
    return -(-a // b)


# ---- references: one einsum per tap, in the inputs' type (float64; float32 for the yardstick) ---------------------------------------

def _lrelu(v, s):
    return torch.where(v > 0, v, v * s)


def _slope(v, s):
    """torch's leaky_relu gradient: 1 where v > 0, the slope elsewhere (at 0 and -0 as well)."""
    return torch.where(v > 0, torch.ones_like(v), torch.full_like(v, s))


def conv_taps(a, W, bias, d):
    """u[b, o, t] = bias[o] + sum_k sum_i W[o, i, k] a[b, i, t + (k - c) d], c = (K - 1) / 2, zero outside [0, L)."""
    K, L = W.shape[2], a.shape[2]
    c = (K - 1) // 2
    ap = F.pad(a, (c * d, c * d))
    u = bias[None, :, None].expand(a.shape[0], W.shape[0], L).clone()
    for k in range(K):
        u += torch.einsum("oi,bit->bot", W[:, :, k], ap[:, :, k * d:k * d + L])
    return u


def conv_taps_backward(a, W, du, d):
    """(da, dW, dbias) of conv_taps for the output gradient du."""
    K, L = W.shape[2], a.shape[2]
    c = (K - 1) // 2
    ap, dup = F.pad(a, (c * d, c * d)), F.pad(du, (c * d, c * d))
    dW = torch.stack([torch.einsum("bot,bit->oi", du, ap[:, :, k * d:k * d + L]) for k in range(K)], dim=2)
    da = torch.zeros_like(a)
    for k in range(K):      # da[t] = sum_k W[:, :, k]^T du[t - (k - c) d]
        s = (2 * c - k) * d
        da += torch.einsum("oi,bot->bit", W[:, :, k], dup[:, :, s:s + L])
    return da, dW, du.sum((0, 2))


def conv32_ref_forward(x, skip, W, bias, d, pre, post):
    """(xs, u, y, S_u): xs = x + skip, a = leaky_relu(xs, pre), u = bias + W * a, y = post(u); S_u = the same on absolute values."""
    xs = x if skip is None else x + skip
    a = _lrelu(xs, pre)
    u = conv_taps(a, W, bias, d)
    return xs, u, (u if post == 1.0 else _lrelu(u, post)), conv_taps(a.abs(), W.abs(), bias.abs(), d)


def conv32_ref_backward(xs, W, d, pre, gy, gxs, post_mask):
    """(dxs, dW, dbias): du = gy * post_mask, dxs = gxs + pre'(xs) * (W^T * du); x and skip both receive dxs."""
    du = gy if post_mask is None else gy * post_mask
    da, dW, db = conv_taps_backward(_lrelu(xs, pre), W, du, d)
    dxs = da * _slope(xs, pre)
    return (dxs if gxs is None else dxs + gxs), dW, db


def undecided(u, S):
    """The elements whose sign a correct float32 forward need not share with float64 (module docstring)."""
    return (u.abs() <= GUARD * S) & (S > 0)


def post_mask(u, S, post, y_seen):
    """post'(u) with float64's sign, and the sign of y_seen (the forward under test) at the undecided elements; None for post = 1."""
    if post == 1.0:
        return None, 0
    und = undecided(u, S)
    sign = torch.where(und, y_seen.to(u.dtype), u)
    return _slope(sign, post), int(und.sum())


def conv7_ref(x, W, bias, dy):
    """(y, dx, dW, dbias) of conv1d(x, W, bias, padding=3), taps written out."""
    return (conv_taps(x, W, bias, 1),) + conv_taps_backward(x, W, dy, 1)


def upsample_ref(x, W, bias, dy, r):
    """(y, dx, dW, dbias) of conv_transpose1d(leaky_relu(x, 0.2), W [i, o, 2 r], bias, stride r, padding r / 2): tap k of input
    position j lands on column j r + k - r / 2, i.e. on slot (j, k) of the output padded by r / 2 and folded to [Lin + 1, r] for
    k < r and on slot (j + 1, k - r) for k >= r."""
    B, C, Lin = x.shape
    a = _lrelu(x, 0.2)
    lo = torch.einsum("iok,bij->bojk", W[:, :, :r], a)
    hi = torch.einsum("iok,bij->bojk", W[:, :, r:], a)
    full = F.pad(lo, (0, 0, 0, 1)) + F.pad(hi, (0, 0, 1, 0))                      # [B, O, Lin + 1, r]
    y = full.reshape(B, W.shape[1], (Lin + 1) * r)[:, :, r // 2:r // 2 + Lin * r] + bias[None, :, None]
    dfull = F.pad(dy, (r // 2, r // 2)).reshape(B, W.shape[1], Lin + 1, r)
    dlo, dhi = dfull[:, :, :Lin], dfull[:, :, 1:]
    dW = torch.cat([torch.einsum("bojk,bij->iok", dlo, a), torch.einsum("bojk,bij->iok", dhi, a)], dim=2)
    da = torch.einsum("iok,bojk->bij", W[:, :, :r], dlo) + torch.einsum("iok,bojk->bij", W[:, :, r:], dhi)
    return y, da * _slope(x, 0.2), dW, dy.sum((0, 2))


# ---- the launchers' grids and k_cconv_reduce's slicing (fd_kernels_cconv.hip), restated to name what a shape reaches ------------------

def conv32_geometry(B, L, cus=CUS):
    """cconv_backward: 128-column tiles, grid = min(ntiles, 2 x CUs); the forward has 256-column workgroups of four 64-column waves."""
    tiles = _cdiv(L, 128)
    rem = L - (tiles - 1) * 128                                                # columns of an utterance's last backward tile
    return {"tile": 128, "tiles_per_row": tiles, "ntiles": B * tiles, "grid": min(B * tiles, 2 * cus), "live_waves": _cdiv(rem, 32),
            "last_wave_columns": rem - 32 * (_cdiv(rem, 32) - 1)}


def conv7_geometry(B, L, cus=CUS):
    """conv7_backward: 256-column tiles, grid = min(ntiles, 4 x CUs); k_c7_first_fwd covers 1024 columns per workgroup."""
    tiles = _cdiv(L, 256)
    return {"tile": 256, "tiles_per_row": tiles, "ntiles": B * tiles, "grid": min(B * tiles, 4 * cus), "first_fwd_blocks": _cdiv(L, 1024)}


def upsample_geometry(B, Lin, r, cus=CUS):
    """convt_backward: tiles of Q = 256 / r input positions in NT = Q / 32 sub-tiles of 32, grid = min(ntiles, CUs)."""
    Q = 256 // r
    tiles = _cdiv(Lin, Q)
    rem = Lin - (tiles - 1) * Q
    return {"tile": Q, "tiles_per_row": tiles, "ntiles": B * tiles, "grid": min(B * tiles, cus), "live_subtiles": _cdiv(rem, 32),
            "last_subtile_positions": rem - 32 * (_cdiv(rem, 32) - 1)}


def tiles_per_workgroup(geo):
    """(most, fewest) tiles a workgroup of the persistent loop `for (tile = blockIdx.x; tile < ntiles; tile += gridDim.x)` takes."""
    return _cdiv(geo["ntiles"], geo["grid"]), geo["ntiles"] // geo["grid"]


def reduce_slices(nparts):
    """k_cconv_reduce: eight slices of ceil(nparts / 8) partials; per slice (rounds of the 4-way unrolled loop, tail elements)."""
    per = _cdiv(nparts, 8)
    out = []
    for q in range(8):
        n = max(0, min(nparts, q * per + per) - q * per)
        out.append((n // 4, n % 4))
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------

WAVE_BORDER_LENGTHS = [32 * k + e for k in range(1, 9) for e in (-4, 0, 4)]        # 28, 32, 36, ..., 252, 256, 260
SHORT = [(3, 4, 27), (3, 24, 27), (3, 28, 27), (3, 8, 9), (3, 12, 9)]
CONV32_PARTIALS = {896: 7, 1024: 8, 1028: 9, 3588: 29, 4100: 33}


def conv32_cases(cus=CUS):
    """[(name, B, L, dilation, skip, post)]"""
    cases = []
    for i, L in enumerate(WAVE_BORDER_LENGTHS):
        skip = i % 2 == 0
        cases.append((f"wave-L{L}", 2, L, DILATIONS[i % 6], skip, 0.2 if skip else 1.0))
    cases += [(f"short-L{L}-d{d}", B, L, d, True, 0.2) for B, L, d in SHORT]
    cases += [(f"partials-{n}", 1, L, DILATIONS[j], True, 0.2) for j, (L, n) in enumerate(CONV32_PARTIALS.items())]
    two = (_cdiv(2 * cus + 3, 5) - 1) * 128 + 36                                   # 13092 at 256 CUs: 515 tiles on 512 workgroups
    three = (_cdiv(4 * cus + 1, 5) - 1) * 128 + 100                                # 26212: 1025 tiles = 2 x 512 + 1
    cases += [("persistent-d1", 5, two, 1, True, 0.2), ("persistent-d27", 5, two, 27, True, 0.2), ("persistent-three-d4", 5, three, 4, True, 0.2)]
    return cases


CONV7_LENGTHS = [(2, L) for L in (252, 256, 260, 1020, 1024, 1028, 2052)] + [(3, 4), (3, 8)] + [(1, 1792), (1, 2052)]


def conv7_cases(cus=CUS):
    """[(name, which, B, L)]"""
    persistent = (_cdiv(4 * cus + 3, 3) - 1) * 256 + 4                             # 87556 at 256 CUs: 1029 tiles on 1024 workgroups
    return [(f"{'first' if which == 0 else 'final'}-{B}x{L}", which, B, L) for which in (0, 1) for B, L in CONV7_LENGTHS] + \
        [(f"{'first' if which == 0 else 'final'}-persistent", which, 3, persistent) for which in (0, 1)]


UPSAMPLE_R8 = [(2, n) for n in (31, 32, 33, 63, 64, 65, 95)] + [(3, 1), (3, 2)]
UPSAMPLE_R4 = [(2, n) for n in (31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129)] + [(3, 1), (3, 2)]


def upsample_cases(cus=CUS):
    """[(name, B, Lin, r)]"""
    cases = [(f"r8-{B}x{n}", B, n, 8) for B, n in UPSAMPLE_R8] + [(f"r4-{B}x{n}", B, n, 4) for B, n in UPSAMPLE_R4]
    for r in (8, 4):
        Q = 256 // r
        cases += [(f"r{r}-partials-7", 1, 7 * Q, r), (f"r{r}-partials-9", 1, 8 * Q + 1, r)]
    tpr = _cdiv(cus + 3, 3)                                                        # 87 at 256 CUs: 261 tiles on 256 workgroups
    return cases + [("r8-persistent", 3, (tpr - 1) * 32 + 1, 8), ("r4-persistent", 3, (tpr - 1) * 64 + 33, 4)]


CONV32_CASES, CONV7_CASES, UPSAMPLE_CASES = conv32_cases(), conv7_cases(), upsample_cases()


# ---- inputs (the recipes of tests/test_lvc_op.py, on a CPU generator: the CPU tests see the tensors the GPU tests run) ---------------

def conv32_inputs(B, L, d, skip, post):
    g = torch.Generator().manual_seed(1000003 * d + 16 * L + B)
    x = torch.randn(B, 32, L, generator=g)
    sk = torch.randn(B, 32, L, generator=g) if skip else None
    x[0, 0, :4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30])                         # the input activation's kink
    if skip:
        sk[0, 0, :4] = 0.0
    w = torch.randn(32, 32, 3, generator=g) / 9.8
    bias = torch.randn(32, generator=g)
    if post != 1.0:                                                                # u = 0 exactly in channel 0: the mask is the slope
        w[0] = 0.0
        bias[0] = 0.0
    gy, gxs = torch.randn(B, 32, L, generator=g), (torch.randn(B, 32, L, generator=g) if skip else None)
    return x, sk, w, bias, gy, gxs


def conv7_inputs(which, B, L):
    """x, W, bias and the output gradient dy.  The bias gradient of final_conv is ONE number, the sum of B L zero-mean draws: typically
    sqrt(B L) in size, but a draw can cancel to almost nothing, and then the bar relative to max(1, |ref|) asks for 3e-6 absolute of
    float32 partial sums of size sqrt(B L) whose own rounding is 2^-24 sqrt(B L) each -- a tree of them ends about 2e-7 sqrt(B L) from
    float64 whatever the order (measured on the first draw of (1, 2052): |ref| = 1.25 where sqrt(B L) = 45, HIP 9.4e-6 = 2.1e-7
    sqrt(B L) from it, i.e. 7.5e-6 relative; torch's own float32 sum 60 times its usual distance as well).  So a draw of dy is taken
    only if, in float64 alone, max |db_ref| >= sqrt(B L) / 4: four times what the format needs for the bar (|ref| >= sqrt(B L) /
    15); otherwise the next seed is drawn.  test_conv7_bias_gradients_are_conditioned pins it."""
    cin, cout = (1, 32) if which == 0 else (32, 1)
    for attempt in range(16):
        g = torch.Generator().manual_seed(10 * L + which + 100003 * B + 7919 * attempt)
        x, w, bias = torch.randn(B, cin, L, generator=g), torch.randn(cout, cin, 7, generator=g) / 3.0, torch.randn(cout, generator=g)
        dy = torch.randn(B, cout, L, generator=g)
        if float(dy.double().sum((0, 2)).abs().max()) >= math.sqrt(B * L) / 4:
            return x, w, bias, dy
    raise AssertionError((which, B, L))


def upsample_inputs(B, Lin, r):
    g = torch.Generator().manual_seed(100 * Lin + r + 100003 * B)
    x = torch.randn(B, 32, Lin, generator=g)
    n = min(4, Lin)
    x[0, 0, :n] = torch.tensor([0.0, -0.0, 1e-30, -1e-30])[:n]                     # the activation's kink
    return x, torch.randn(32, 32, 2 * r, generator=g) / 8.0, torch.randn(32, generator=g), torch.randn(B, 32, Lin * r, generator=g)


# ---- the comparison -----------------------------------------------------------------------------------------------------------------

def distance(got, want):
    """max |got - want| over every element relative to max(1, max |want|), in float64."""
    want = want.double()
    return float((got.double().to(want.device) - want).abs().max()) / max(1.0, float(want.abs().max()))


def compare(op, name, got, want, bar, geo=None, unit=1, yardstick=None):
    """Every element of `got` against the float64 `want`; the failure names the place.  Signals [B, C, columns]: utterance, channel,
    column, the column's distance to the nearest 32-column border (in positions of `unit` columns for the up-sampler's output) and
    to the end of the utterance.  Sums over tiles (dW, db): the index, the partial count and the tiles per workgroup of `geo`."""
    assert tuple(got.shape) == tuple(want.shape), (op, name, tuple(got.shape), tuple(want.shape))
    want = want.double()
    diff = (got.double().to(want.device) - want).abs()
    scale = max(1.0, float(want.abs().max()))
    err = float(diff.max()) / scale
    print(f"  {op} {name}: hip {err:.2e}" + (f"  float32 {yardstick:.2e}" if yardstick is not None else "") + f"  (bar {bar:.0e})")
    if err < bar:
        return err
    idx = [int(i) for i in torch.unravel_index(diff.argmax(), diff.shape)]
    where = f"{op} {name}: {err:.3e} >= {bar:.1e} (|d| = {float(diff.max()):.3e}, max|ref| = {scale:.3e}) at {tuple(idx)}"
    if want.dim() == 3 and name not in ("dW", "db"):
        b, ch, col = idx
        pos, n = col // unit, want.shape[2] // unit
        where += (f": utterance {b}, channel {ch}, column {col}" + (f" (position {pos})" if unit > 1 else "") +
                  f", {min(pos % 32, 32 - pos % 32)} past / before the nearest 32-column border (offset {pos % 32} in its tile), {n - 1 - pos} before the end of the utterance")
    else:
        where += ": " + {1: "element {}", 3: "weight [{}, {}], tap {}"}[want.dim()].format(*idx)
    if geo is not None:
        most, fewest = tiles_per_workgroup(geo)
        where += (f"; {geo['grid']} partials, {geo['ntiles']} tiles of {geo['tile']}: {fewest} to {most} tiles per workgroup, "
                  f"reduce slices (rounds of 4, tail) {reduce_slices(geo['grid'])}")
    raise AssertionError(where)


# ---- CPU: the references are what they claim ------------------------------------------------------------------------------------------

def _r64(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("B,L,d,skip,post", [(2, 40, 3, True, 0.2), (3, 12, 27, False, 1.0)])
def test_conv32_reference_equals_conv1d_and_its_autograd(B, L, d, skip, post):
    g = torch.Generator().manual_seed(L + d)
    x, w, bias, gy = _r64(g, B, 32, L), _r64(g, 32, 32, 3) / 9.8, _r64(g, 32), _r64(g, B, 32, L)
    sk, gxs = (_r64(g, B, 32, L), _r64(g, B, 32, L)) if skip else (None, None)
    x[0, 0, :4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30], dtype=torch.float64)
    if skip:
        sk[0, 0, :4] = 0.0
    xa, wa, ba = (t.clone().requires_grad_(True) for t in (x, w, bias))
    sa = sk.clone().requires_grad_(True) if skip else None
    xsa = xa + sa if skip else xa
    ya = F.conv1d(F.leaky_relu(xsa, 0.2), wa, ba, padding=d, dilation=d)
    if post != 1.0:
        ya = F.leaky_relu(ya, post)
    ((ya * gy).sum() + ((xsa * gxs).sum() if skip else 0.0)).backward()
    xs, u, y, S = conv32_ref_forward(x, sk, w, bias, d, 0.2, post)
    assert not bool(undecided(u, S).any())
    mask, _ = post_mask(u, S, post, y)
    dxs, dW, db = conv32_ref_backward(xs, w, d, 0.2, gy, gxs, mask)
    assert torch.equal(xs, xsa.detach()) and bool((S >= u.abs()).all())
    for got, want in ((y, ya.detach()), (dxs, xa.grad), (dW, wa.grad), (db, ba.grad)) + (((dxs, sa.grad),) if skip else ()):
        assert got.shape == want.shape and torch.allclose(got, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("which,B,L", [(0, 2, 12), (1, 3, 4)])
def test_conv7_reference_equals_conv1d_and_its_autograd(which, B, L):
    g = torch.Generator().manual_seed(L + which)
    cin, cout = (1, 32) if which == 0 else (32, 1)
    x, w, bias, dy = _r64(g, B, cin, L), _r64(g, cout, cin, 7) / 3.0, _r64(g, cout), _r64(g, B, cout, L)
    xa, wa, ba = (t.clone().requires_grad_(True) for t in (x, w, bias))
    ya = F.conv1d(xa, wa, ba, padding=3)
    ya.backward(dy)
    for got, want in zip(conv7_ref(x, w, bias, dy), (ya.detach(), xa.grad, wa.grad, ba.grad)):
        assert got.shape == want.shape and torch.allclose(got, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("B,Lin,r", [(2, 5, 8), (3, 1, 4)])
def test_upsample_reference_equals_conv_transpose1d_and_its_autograd(B, Lin, r):
    g = torch.Generator().manual_seed(Lin + r)
    x, w, bias, dy = _r64(g, B, 32, Lin), _r64(g, 32, 32, 2 * r) / 8.0, _r64(g, 32), _r64(g, B, 32, Lin * r)
    x[0, 0, 0] = 0.0
    xa, wa, ba = (t.clone().requires_grad_(True) for t in (x, w, bias))
    ya = F.conv_transpose1d(F.leaky_relu(xa, 0.2), wa, ba, stride=r, padding=r // 2)
    ya.backward(dy)
    for got, want in zip(upsample_ref(x, w, bias, dy, r), (ya.detach(), xa.grad, wa.grad, ba.grad)):
        assert got.shape == want.shape and torch.allclose(got, want, rtol=0, atol=1e-12)


# ---- CPU: every case reaches what it is listed for, at 256 CUs ------------------------------------------------------------------------

def test_reduce_slicing_at_the_listed_partial_counts():
    assert reduce_slices(7) == [(0, 1)] * 7 + [(0, 0)]                            # one empty slice
    assert reduce_slices(8) == [(0, 1)] * 8
    assert reduce_slices(9) == [(0, 2)] * 4 + [(0, 1)] + [(0, 0)] * 3             # three empty slices behind a one-element slice
    assert reduce_slices(29) == [(1, 0)] * 7 + [(0, 1)]                           # the unrolled loop, then a one-element last slice
    assert reduce_slices(33) == [(1, 1)] * 6 + [(0, 3)] + [(0, 0)]                # the unrolled loop plus its tail
    assert reduce_slices(512) == [(16, 0)] * 8 and reduce_slices(1024) == [(32, 0)] * 8 and reduce_slices(256) == [(8, 0)] * 8


def test_conv32_cases_reach_the_borders_they_are_chosen_for():
    cases = {c[0]: c[1:] for c in CONV32_CASES}
    assert len(cases) == len(CONV32_CASES) == 24 + 5 + 5 + 3
    wave = [c for c in CONV32_CASES if c[0].startswith("wave")]
    assert [c[2] for c in wave] == [28, 32, 36, 60, 64, 68, 92, 96, 100, 124, 128, 132, 156, 160, 164, 188, 192, 196, 220, 224, 228, 252, 256, 260]
    assert all(c[1] == 2 for c in wave)
    assert {c[3] for c in wave} == set(DILATIONS) and {(c[4], c[5]) for c in wave} == {(True, 0.2), (False, 1.0)}
    # backward: every one of the four waves of a 128-column tile is the last live one with 28, 32 and 4 columns
    reach = {(conv32_geometry(2, c[2])["live_waves"], conv32_geometry(2, c[2])["last_wave_columns"]) for c in wave}
    assert reach == {(w, n) for w in (1, 2, 3, 4) for n in (28, 32, 4)}
    assert {conv32_geometry(2, c[2])["tiles_per_row"] for c in wave} == {1, 2, 3}
    # forward: 256-column workgroups, 64-column waves of two 32-column tiles
    assert {(_cdiv(L, 64), L % 64) for L in (c[2] for c in wave)} >= {(w, m) for w in (1, 2, 3, 4) for m in (28, 32, 36, 60, 0)} | {(5, 4)}
    for name, (B, L, d, skip, post) in cases.items():
        if name.startswith("short"):
            assert B == 3 and L <= (d + 3) // 4 * 4 and skip and post == 0.2       # no longer than the halo, neighbours on both sides
        if name.startswith("partials"):
            geo = conv32_geometry(B, L)
            assert B == 1 and geo["grid"] == geo["ntiles"] == CONV32_PARTIALS[L] == int(name.split("-")[1])
    assert sorted(CONV32_PARTIALS.values()) == [7, 8, 9, 29, 33]
    for name in ("persistent-d1", "persistent-d27"):
        B, L, d, skip, post = cases[name]
        geo = conv32_geometry(B, L)
        assert (B, L) == (5, 13092) and (geo["ntiles"], geo["grid"], geo["tiles_per_row"]) == (515, 512, 103)
        assert tiles_per_workgroup(geo) == (2, 1) and (0 // 103, 512 // 103) == (0, 4)      # workgroup 0: utterances 0 and 4
        assert (geo["live_waves"], geo["last_wave_columns"]) == (2, 4)
    B, L, d, skip, post = cases["persistent-three-d4"]
    geo = conv32_geometry(B, L)
    assert (B, L, d) == (5, 26212, 4) and geo["ntiles"] == 2 * geo["grid"] + 1 == 1025 and tiles_per_workgroup(geo) == (3, 2)
    assert {cases[n][2] for n in ("persistent-d1", "persistent-d27")} == {1, 27}
    for cus in (64, 80, 104, 228, 304):                                            # other devices: still more tiles than workgroups
        for name, B, L, d, skip, post in conv32_cases(cus)[-3:]:
            geo = conv32_geometry(B, L, cus)
            assert L % 4 == 0 and geo["ntiles"] > (2 if "three" in name else 1) * geo["grid"], (cus, name)


def test_conv7_cases_reach_the_borders_they_are_chosen_for():
    assert len(CONV7_CASES) == 2 * (7 + 2 + 2 + 1) and {c[1] for c in CONV7_CASES} == {0, 1}
    for which in (0, 1):
        mine = {c[0]: c[2:] for c in CONV7_CASES if c[1] == which}
        shapes = set(mine.values())
        assert {(2, L) for L in (252, 256, 260, 1020, 1024, 1028, 2052)} | {(3, 4), (3, 8), (1, 1792), (1, 2052)} <= shapes
        assert conv7_geometry(1, 1792)["grid"] == 7 and conv7_geometry(1, 2052)["grid"] == 9
        assert [conv7_geometry(2, L)["first_fwd_blocks"] for L in (1020, 1024, 1028, 2052)] == [1, 1, 2, 3]
        assert [conv7_geometry(2, L)["tiles_per_row"] for L in (252, 256, 260)] == [1, 1, 2]
        B, L = mine[("first" if which == 0 else "final") + "-persistent"]
        geo = conv7_geometry(B, L)
        assert (B, L) == (3, 87556) and (geo["ntiles"], geo["grid"]) == (1029, 1024) and tiles_per_workgroup(geo) == (2, 1)
    for cus in (64, 80, 104, 228, 304):
        name, which, B, L = conv7_cases(cus)[-1]
        assert L % 4 == 0 and conv7_geometry(B, L, cus)["ntiles"] > conv7_geometry(B, L, cus)["grid"], cus


def test_upsample_cases_reach_the_borders_they_are_chosen_for():
    assert len(UPSAMPLE_CASES) == 9 + 14 + 4 + 2
    for r, Q in ((8, 32), (4, 64)):
        mine = {c[0]: c[1:3] for c in UPSAMPLE_CASES if c[3] == r}
        ragged = {(g["live_subtiles"], g["last_subtile_positions"]) for g in (upsample_geometry(B, n, r) for B, n in mine.values() if B == 2)}
        if r == 8:      # one sub-tile of 32 positions: Q - 1, Q, Q + 1, and the same one and two tiles further
            assert ragged == {(1, 31), (1, 32), (1, 1)}
        else:           # two sub-tiles: each one position short of, at and past full
            assert ragged == {(1, 31), (1, 32), (2, 1), (2, 31), (2, 32), (1, 1)}
        assert {(3, 1), (3, 2)} <= set(mine.values())
        assert upsample_geometry(*mine[f"r{r}-partials-7"], r)["grid"] == 7 and mine[f"r{r}-partials-7"] == (1, 7 * Q)
        assert upsample_geometry(*mine[f"r{r}-partials-9"], r)["grid"] == 9 and mine[f"r{r}-partials-9"] == (1, 8 * Q + 1)
        B, Lin = mine[f"r{r}-persistent"]
        geo = upsample_geometry(B, Lin, r)
        assert (B, Lin) == (3, 86 * Q + (1 if r == 8 else 33)) and (geo["ntiles"], geo["grid"]) == (261, 256)
        assert tiles_per_workgroup(geo) == (2, 1) and (geo["live_subtiles"], geo["last_subtile_positions"]) == ((1, 1) if r == 8 else (2, 1))
    for cus in (64, 80, 104, 228, 304):
        for name, B, Lin, r in upsample_cases(cus)[-2:]:
            assert upsample_geometry(B, Lin, r, cus)["ntiles"] > upsample_geometry(B, Lin, r, cus)["grid"], (cus, name)


@pytest.mark.parametrize("name,which,B,L", CONV7_CASES, ids=[c[0] for c in CONV7_CASES])
def test_conv7_bias_gradients_are_conditioned(name, which, B, L):
    """From float64 alone: the largest bias gradient of every conv7 case is at least sqrt(B L) / 4 (conv7_inputs)."""
    dy = conv7_inputs(which, B, L)[3].double()
    assert float(dy.sum((0, 2)).abs().max()) >= math.sqrt(B * L) / 4 and tuple(dy.shape) == (B, 32 if which == 0 else 1, L)


@pytest.mark.parametrize("name,B,L,d,skip,post", CONV32_CASES, ids=[c[0] for c in CONV32_CASES])
def test_undecided_share_of_every_conv32_case_is_under_the_cap(name, B, L, d, skip, post):
    """From float64 alone: at most 2^-12 of a case's pre-activations lie within GUARD * S_u of zero.  Measured with these inputs (the
    GPU run counts the same elements): none in 29 of the 37 cases, one element at L = 220 and at L = 228 (7.1e-5 of the case, the
    largest share: a third of the cap), 1.3e-5 .. 3.0e-5 at partial counts 9, 29, 33 and the persistent shapes (72 elements at most)."""
    x, sk, w, bias, _, _ = conv32_inputs(B, L, d, skip, post)
    _, u, _, S = conv32_ref_forward(x.double(), None if sk is None else sk.double(), w.double(), bias.double(), d, 0.2, post)
    n = int(undecided(u, S).sum()) if post != 1.0 else 0
    print(f"\n{name}: {n} of {u.numel()} undecided ({n / u.numel():.1e})")
    assert n <= UNDECIDED_CAP * u.numel(), (name, n, u.numel())
    if post != 1.0:
        assert bool((u[:, 0] == 0).all()) and not bool(undecided(u, S)[:, 0].any())      # the planted row: exactly zero, decided


@pytest.mark.parametrize("which", ["y", "dxs", "dW"])
def test_the_helper_rejects_one_element_just_beyond_the_bar(which):
    """The float32 image of the float64 reference passes; one element moved by 1.01 x its bar fails and by 0.5 x passes -- at the last
    column of an utterance, the first column of a tile (backward 128, forward 256) and a weight-gradient element of the last tap."""
    B, L, d = 2, 260, 3
    x, sk, w, bias, gy, gxs = (t.double() for t in conv32_inputs(B, L, d, True, 0.2))
    xs, u, y, S = conv32_ref_forward(x, sk, w, bias, d, 0.2, 0.2)
    dxs, dW, _ = conv32_ref_backward(xs, w, d, 0.2, gy, gxs, post_mask(u, S, 0.2, y)[0])
    ref, bar = {"y": (y, OUT_BAR), "dxs": (dxs, GRAD_BAR), "dW": (dW, GRAD_BAR)}[which]
    places = {"y": [(0, 5, L - 1), (1, 31, L - 1), (1, 7, 256)], "dxs": [(0, 5, L - 1), (1, 0, 128), (0, 31, 256)],
              "dW": [(31, 31, 2), (0, 0, 2), (17, 3, 2)]}[which]
    geo = conv32_geometry(B, L)
    compare("conv32", which, ref.float(), ref, bar, geo)
    step = 1.01 * bar * max(1.0, float(ref.abs().max()))
    for idx in places:
        for sign in (1.0, -1.0):
            bad = ref.clone()
            bad[idx] += sign * step
            with pytest.raises(AssertionError) as e:
                compare("conv32", which, bad, ref, bar, geo)
            msg = str(e.value)
            assert str(idx) in msg and "conv32 " + which in msg
            if which == "dW":
                assert "tap 2" in msg and "6 partials" in msg and "1 to 1 tiles per workgroup" in msg
            else:
                assert f"utterance {idx[0]}, channel {idx[1]}, column {idx[2]}" in msg
                assert f"{L - 1 - idx[2]} before the end of the utterance" in msg and f"offset {idx[2] % 32} in its tile" in msg
        half = ref.clone()
        half[idx] += 0.5 * step
        compare("conv32", which, half, ref, bar, geo)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


def _f64(*ts):
    return tuple(None if t is None else t.double() for t in ts)


def _conv32_run(x, sk, w, bias, d, post, gy, gxs, need_x=True):
    """One forward and backward of fastdiff_amd.conv32: (xs, y, dx, dskip, dW, db)."""
    import fastdiff_amd
    xg, sg = x.clone().requires_grad_(need_x), (None if sk is None else sk.clone().requires_grad_(need_x))
    wg, bg = w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    out = fastdiff_amd.conv32(xg, wg, bg, d, skip=sg, post_slope=post)
    xs, y = out if sk is not None else (None, out)
    loss = (y * gy).sum()
    if sk is not None and need_x:
        loss = loss + (xs * gxs).sum()
    loss.backward()
    return (None if xs is None else xs.detach()), y.detach(), xg.grad, (None if sg is None else sg.grad), wg.grad, bg.grad


def _persistent(name, geo):
    if "persistent" in name:
        most, _ = tiles_per_workgroup(geo)
        assert geo["ntiles"] > geo["grid"] and most >= (3 if "three" in name else 2), (name, geo)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CONV32_CASES)), ids=[c[0] for c in CONV32_CASES])
def test_conv32_against_float64(i):
    """xs, y, dx (= dskip), dW and db of fastdiff_amd.conv32 against the explicit float64 reference, every element.  No bar was moved
    by the yardstick rule: dW and db stay under GRAD_BAR at the persistent shapes."""
    cus = _cus()
    name, B, L, d, skip, post = conv32_cases(cus)[i]
    geo = conv32_geometry(B, L, cus)
    print(f"\nconv32 {name}: B={B} L={L} dilation {d} skip {skip} post {post}; {geo}")
    _persistent(name, geo)
    x, sk, w, bias, gy, gxs = _dev(*conv32_inputs(B, L, d, skip, post))
    with launched_kernels() as launched:
        xs, y, dx, dsk, dW, db = _conv32_run(x, sk, w, bias, d, post, gy, gxs)
    assert {"cconv_fwd", "cconv_bwd", "cconv_reduce"} <= launched.keys(), launched
    if skip:
        assert torch.equal(xs, x + sk) and torch.equal(dx, dsk)                    # bit for bit; x and skip receive the same gradient
    x64, s64, w64, b64, gy64, gxs64 = _f64(x, sk, w, bias, gy, gxs)
    xs64, u64, y64, S64 = conv32_ref_forward(x64, s64, w64, b64, d, 0.2, post)
    y32 = conv32_ref_forward(x, sk, w, bias, d, 0.2, post)[2]
    compare("conv32", "y", y, y64, OUT_BAR, yardstick=distance(y32, y64))
    mask, n_und = post_mask(u64, S64, post, y)
    print(f"  undecided: {n_und} of {u64.numel()} ({n_und / u64.numel():.1e})")
    assert n_und <= UNDECIDED_CAP * u64.numel()
    ref = conv32_ref_backward(xs64, w64, d, 0.2, gy64, gxs64, mask)
    yard = conv32_ref_backward(x + sk if skip else x, w, d, 0.2, gy, gxs, None if mask is None else mask.float())
    for tname, got, want, y32_, g in zip(("dx", "dW", "db"), (dx, dW, db), ref, yard, (None, geo, geo)):
        compare("conv32", tname, got, want, GRAD_BAR, g, yardstick=distance(y32_, want))
    again = _conv32_run(x, sk, w, bias, d, post, gy, gxs)
    assert all(p is None or torch.equal(p, q) for p, q in zip(again, (xs, y, dx, dsk, dW, db)))
    # weights only (dxs == nullptr in k_cconv_bwd): the same bits of dW and db
    only = _conv32_run(x, sk, w, bias, d, post, gy, gxs, need_x=False)
    assert only[2] is None and torch.equal(only[4], dW) and torch.equal(only[5], db)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CONV7_CASES)), ids=[c[0] for c in CONV7_CASES])
def test_conv7_against_float64(i):
    """y, dx, dW and db of lvc_op.conv7 (first_audio_conv and final_conv) against the explicit float64 reference, every element.  No bar
    was moved by the yardstick rule."""
    from fastdiff_amd.lvc_op import conv7, conv7_supported
    cus = _cus()
    name, which, B, L = conv7_cases(cus)[i]
    geo = conv7_geometry(B, L, cus)
    print(f"\nconv7 {name}: B={B} L={L}; {geo}")
    _persistent(name, geo)
    x, w, bias, dy = _dev(*conv7_inputs(which, B, L))

    def run(need_x=True):
        xg, wg, bg = x.clone().requires_grad_(need_x), w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        assert conv7_supported(xg, wg)
        y = conv7(xg, wg, bg)
        y.backward(dy)
        return y.detach(), xg.grad, wg.grad, bg.grad

    with launched_kernels() as launched:
        got = run()
    end = "first" if which == 0 else "final"
    assert {f"conv7_{end}_fwd", f"conv7_{end}_bwd", "cconv_reduce"} <= launched.keys(), launched
    ref, yard = conv7_ref(*_f64(x, w, bias, dy)), conv7_ref(x, w, bias, dy)
    for tname, g_, r_, y_, bar, geo_ in zip(("y", "dx", "dW", "db"), got, ref, yard, (OUT_BAR,) + (GRAD_BAR,) * 3, (None, None, geo, geo)):
        compare(f"conv7[{end}]", tname, g_, r_, bar, geo_, yardstick=distance(y_, r_))
    assert all(torch.equal(p, q) for p, q in zip(run(), got))
    only = run(need_x=False)                                                       # the training case: the audio needs no gradient
    assert only[1] is None and torch.equal(only[2], got[2]) and torch.equal(only[3], got[3])


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(UPSAMPLE_CASES)), ids=[c[0] for c in UPSAMPLE_CASES])
def test_upsample_against_float64(i):
    """y, dx, dW and db of lvc_op.upsample against the explicit float64 reference, every element.  No bar was moved by the yardstick
    rule."""
    from fastdiff_amd.lvc_op import upsample
    cus = _cus()
    name, B, Lin, r = upsample_cases(cus)[i]
    geo = upsample_geometry(B, Lin, r, cus)
    print(f"\nupsample {name}: B={B} Lin={Lin} r={r}; {geo}")
    _persistent(name, geo)
    x, w, bias, dy = _dev(*upsample_inputs(B, Lin, r))

    def run():
        xg, wg, bg = (t.clone().requires_grad_(True) for t in (x, w, bias))
        y = upsample(xg, wg, bg, r)
        y.backward(dy)
        return y.detach(), xg.grad, wg.grad, bg.grad

    with launched_kernels() as launched:
        got = run()
    assert {"convt_train_fwd", "convt_train_bwd", "cconv_reduce"} <= launched.keys(), launched
    ref, yard = upsample_ref(*_f64(x, w, bias, dy), r), upsample_ref(x, w, bias, dy, r)
    for tname, g_, r_, y_, bar, geo_, unit in zip(("y", "dx", "dW", "db"), got, ref, yard, (OUT_BAR,) + (GRAD_BAR,) * 3, (None, None, geo, geo),
                                                  (r, 1, 1, 1)):
        compare(f"upsample[r={r}]", tname, g_, r_, bar, geo_, unit=unit, yardstick=distance(y_, r_))
    assert all(torch.equal(p, q) for p, q in zip(run(), got))
